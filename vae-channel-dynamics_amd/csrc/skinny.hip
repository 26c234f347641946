// Convolutions with a <= 4-channel side (conv_in: 3 input channels; conv_out: 3 output channels; the 4-channel latent
// convs) on the VALU.  On the MFMA tiles those sides are padded to 32 and 7/8 of the matrix work multiplies zeros; at
// 256x256 the five launches cost 6.7 ms.  They are HBM-bound by nature (one 128-channel tensor is read or written
// once: 0.1-0.2 ms at the full rate), so here one lane owns one channel of the WIDE side and keeps its 9 x (<=4)
// weights / accumulators in registers, and the few values of the NARROW side that a pixel's 9 taps need are staged per
// 128-pixel tile in LDS ([128 px][9 taps][4], 18 KB) and read back as broadcast ds_read_b128.  Wide-side global
// accesses are 512-byte rows per pixel; every load goes through a buffer descriptor (out of range = 0).
//   conv_smallk : y[px][n]      = bias[n] + sum_{tap,s} S[src(px,tap)][s] * W[n][tap][s]      (rows form, K <= 4)
//   wgrad_smallk: out[..]       = sum_px V[px][lane] * S[src(px,tap)][s]                      (N <= 4 or M <= 4)
//   conv_smalln : y[px][s]      = bias[s] + sum_{tap,c} XF(x)[px+tap][c] * W[s][tap][c]       (<= 4 outputs; end of file)
// The WIDE side may be stored as bf16 (bf16 mode keeps the 128-channel activations / gradients as bf16): out_bf16 for
// conv_smallk's output, y_bf16 / x_bf16 for wgrad_smallk's V, a_bf16 for conv_smalln's input; the narrow side, the weights
// and the arithmetic are fp32.
// wgrad_smallk's one-lane-per-channel loop is bound by issue, not by bytes (36 FMAs and nine LDS broadcasts per pixel: 0.52 and
// 0.65 ms for the two full-resolution launches, whose 537 MB stream in 0.1 ms): a 3x3 layer with a wide side of >= 64 channels
// runs on the matrix pipe instead, exact fp32 products (v_mfma_f32_16x16x4_f32; the padded 48 x 128 product is 0.08 ms of matrix
// time per launch, inside the memory time, so no operand split), behind a grid-uniform branch of the same kernel
// (wgrad_smallk_mfma below; -DVAE_THIN_F32_MFMA=0 builds the VALU bodies alone).  conv_smallk and conv_smalln keep their VALU bodies.
// The tile shapes, the tile range of a split, the per-element transform, the slab protocol of the weight gradient and the host
// predicates are in thin_common.h, shared with the matrix-pipe kernels of the same launches (conv_thin_bf16.hip,
// wgrad_thin_bf16.hip).
#include "thin_common.h"
#include "launchers.h"

// 0: the VALU bodies alone (the A/B arm of tools/thin_f32_ab.py: make thin_f32_valu)
#ifndef VAE_THIN_F32_MFMA
#define VAE_THIN_F32_MFMA 1
#endif

namespace {

using thin::TP;
using thin::TAPS_MAX;
constexpr int NT = 256;   // 2 pixel streams x 128 channel lanes

// stage S[src(row, tap)][0..3] for the TP rows of tile `m0` (row = linear pixel of the row grid of `g`), straight into LDS.
// (Spelt out, not thin::gather4: this gather also serves 1x1 layers, and through the shared function -- whole, or only its
// pixel mapping -- the two kernels below moved: wgrad_smallk_kernel<false,*> one scalar spill fewer (20 / 24 / 24 for
// 21 / 25 / 25), wgrad_smallk_kernel<true,0> 77 VGPRs for 79.)
__device__ __forceinline__ void stage_small(const vae_conv_geom& g, const float* __restrict__ S, int Cs_small, int K, int m0,
                                            int mrows, f32x4* __restrict__ sI) {
  const int hw = g.Ho * g.Wo;
  const size_t sbytes = (size_t)g.B * g.Hs * g.Ws * Cs_small * 4u;
  const auto rsS = VAE_BUF_RSRC(S, sbytes < BUF_MAX ? sbytes : BUF_MAX);
  for (int e = threadIdx.x; e < TP * g.taps; e += NT) {
    const int row = e / g.taps, tap = e - row * g.taps;
    const int m = m0 + row;
    const int b = m / hw, rem = m - b * hw;
    const int y = rem / g.Wo, x = rem - y * g.Wo;
    const int kh = (g.taps == 9) ? tap / 3 : 0, kw = (g.taps == 9) ? tap - kh * 3 : 0;
    int sy = 0, sx = 0;
    const bool ok = (m < mrows) && src_pixel(g, y, x, kh, kw, sy, sx);
    const unsigned base = ok ? (unsigned)(((b * g.Hs + sy) * g.Ws + sx) * Cs_small) * 4u : BUF_OOB;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < K) v[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsS, ok ? base + 4u * s : BUF_OOB, 0, 0));
    sI[e] = v;
  }
}

__global__ __launch_bounds__(NT) void conv_smallk_kernel(vae_igemm_args p) {
  __shared__ f32x4 sI[TP * TAPS_MAX];
  const vae_conv_geom g = p.g;
  const int tid = threadIdx.x, lane = tid & 127, half = tid >> 7;
  const int m0 = blockIdx.x * TP;
  const int n = blockIdx.y * 128 + lane;
  const bool nok = n < p.N;
  stage_small(g, p.A, g.Cs, p.K, m0, p.M, sI);

  float w[TAPS_MAX][4];
#pragma unroll
  for (int t = 0; t < TAPS_MAX; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      w[t][s] = (nok && t < g.taps && s < p.K) ? p.W[(int64_t)n * p.sn + (int64_t)t * p.st + (int64_t)s * p.sk] : 0.f;
  const float bv = (p.bias && nok) ? p.bias[n] : 0.f;
  const bool cbf = p.out_bf16 != 0;
  const size_t obytes = (size_t)p.M * p.ldc * (cbf ? 2u : 4u);
  const auto rsC = VAE_BUF_RSRC(p.C, obytes);
  __syncthreads();

  float tsum = 0.f;
#pragma unroll 4
  for (int i = 0; i < TP / 2; ++i) {
    const int row = half + 2 * i;
    float acc = bv;
#pragma unroll
    for (int t = 0; t < TAPS_MAX; ++t) {
      if (t < g.taps) {  // uniform
        const f32x4 v = sI[row * g.taps + t];  // same address in every lane: broadcast read
#pragma unroll
        for (int s = 0; s < 4; ++s) acc += v[s] * w[t][s];
      }
    }
    const int m = m0 + row;
    const bool ok = nok && m < p.M;
    buf_store1_elem(rsC, cbf, ok ? m * p.ldc + n : -1, acc);
    const float stored = cbf ? (float)(__bf16)acc : acc;  // the tracker describes the tensor as stored
    tsum += ok ? fabsf(stored) : 0.f;
  }
  if (p.track) {  // uniform: per-channel sum of |y| over this 128-row tile (same partial layout as the MFMA kernels)
    __syncthreads();
    float* red = reinterpret_cast<float*>(sI);
    red[tid] = tsum;
    __syncthreads();
    if (half == 0 && nok) p.track[(int64_t)blockIdx.x * p.N + n] = red[lane] + red[128 + lane];
  }
}

#if VAE_THIN_F32_MFMA
// The 3x3 weight gradient with a wide side of >= 64 channels on the matrix pipe (v_mfma_f32_16x16x4_f32: exact fp32 products):
//     out[(tap, s)][n] = sum_q T[q][(tap, s)] * V[q][n]        q = pixel (the contraction), n = wide channel
// T = the im2col of the narrow tensor, gathered per 128-pixel tile into LDS planes [(tap, s)][pixel] (36 rows; SMALL_X: row 36
// = ones, so row 36 of the product is the bias gradient; padded to 48 = three 16-row blocks), A operand = one ds_read_b128 per
// row block and 16 pixels.  V goes from global memory straight into the B operand: a lane loads the 2 channels cq, cq + 1 of
// pixel 16 h + 4 g + j (g = lane / 16; h, j = the k-step of a 32-pixel chunk) as one 8-byte load (128 contiguous bytes per
// pixel and wave) and gives channel cq + e to the MFMAs of column block e -- the columns of a block are channels 2 apart, which
// only relabels the output.  Wave w = the 32 channels 32 w .. 32 w + 31 over all the pixels (24 accumulator registers, no
// reduction across waves: every sum runs in pixel order); V is prefetched one chunk ahead across tile boundaries, T one tile
// ahead in registers; 4 workgroups per CU (128 registers), so the 1024 workgroups of a full-resolution launch are one round.
constexpr int WM_LDT = TP + 4;                                  // floats per row of T: b128 reads of 16 rows conflict-free
constexpr int WM_ROWS = 48;
constexpr int WM_ITEMS = (TP * TAPS_MAX + NT - 1) / NT;         // (pixel, tap) gathers per thread and tile: 5
constexpr int WG_SI = WM_ROWS * WM_LDT / 4;                     // (the sums of dY, 4 x 256 floats, reuse it at the end)
static_assert(WG_SI >= TP * TAPS_MAX + 32 && WG_SI >= NT, "LDS of wgrad_smallk_kernel");

// 3x3, a wide side of >= 64 channels read as pairs: even, its rows and its base 8-byte (bf16: 4-byte) aligned; with a fused
// GroupNorm, tiles that lie inside one image (one scale / shift pair per lane and tile).  1x1 layers, the 4 -> 4 latent convs
// and every other operand keep the VALU body.
template <bool SMALL_X, int XF>
__device__ __forceinline__ bool wgrad_mfma_serves(const vae_wgrad_args& p, const vae_conv_geom& gs) {
  const int wide = SMALL_X ? p.M : p.N, ldv = SMALL_X ? p.ldy : p.g.Cs;
  const bool vbf = (SMALL_X ? p.y_bf16 : p.x_bf16) != 0;
  const uintptr_t v = reinterpret_cast<uintptr_t>(SMALL_X ? p.dY : p.X);
  return gs.taps == TAPS_MAX && wide >= 64 && wide % 2 == 0 && ldv % 2 == 0 && (v & (vbf ? 3u : 7u)) == 0 &&
         (XF == VAE_XF_NONE || (gs.Ho * gs.Wo) % TP == 0);
}

template <bool SMALL_X, int XF>
__device__ __forceinline__ void wgrad_smallk_mfma(const vae_wgrad_args& p, const vae_conv_geom& gs, int ntiles, float* __restrict__ sT) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lg = lane >> 4;
  const int split = blockIdx.x;
  const int wide = SMALL_X ? p.M : p.N, narrow = SMALL_X ? p.N : p.M;
  const int cq = blockIdx.y * 128 + wave * 32 + lc * 2;  // this lane's two wide channels
  const float* __restrict__ V = SMALL_X ? p.dY : p.X;
  const float* __restrict__ S = SMALL_X ? p.X : p.dY;
  const int ldv = SMALL_X ? p.ldy : p.g.Cs, lds_ = SMALL_X ? p.g.Cs : p.ldy;
  const int npixv = gs.B * gs.Ho * gs.Wo, hwv = gs.Ho * gs.Wo;
  const bool vbf = (SMALL_X ? p.y_bf16 : p.x_bf16) != 0;
  const unsigned esV = vbf ? 2u : 4u;
  const size_t vbytes = (size_t)npixv * ldv * esV;
  const auto rsV = VAE_BUF_RSRC(V, vbytes < BUF_MAX ? vbytes : BUF_MAX);
  const auto rsS = thin::narrow_rsrc(S, gs, lds_);

  // rows 36 .. 47 of T never change: zeros, and (SMALL_X) row 36 = ones
  for (int i = tid; i < (WM_ROWS - 36) * WM_LDT; i += NT) sT[36 * WM_LDT + i] = (SMALL_X && i < WM_LDT) ? 1.f : 0.f;

  f32x4 acc[3][2];  // [row block][column block]: rows (tap = 4 mb + lg, s = r), column = channel cq + e
#pragma unroll
  for (int mb = 0; mb < 3; ++mb)
#pragma unroll
    for (int e = 0; e < 2; ++e) acc[mb][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 ssum = {0.f, 0.f, 0.f, 0.f};  // !SMALL_X: this thread's share of sum_q dY[q][s]
  float sc[2] = {0.f, 0.f}, sh[2] = {0.f, 0.f};
  int xb = -1;

  // this lane's eight pixels mb_ + 16 h + j of a chunk, as stored (an fp32 pair, or 2 bf16 in .x); a pixel past the grid or a
  // channel pair past the wide side is not requested (zeros)
  auto load_v = [&](uint2 (&rv)[8], int mb_) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int m = mb_ + 16 * (k >> 2) + (k & 3);
      const int eoff = neg_unless(m < npixv && cq < wide, m * ldv + cq);
      // one instruction for both storages (a bf16 pair brings the next pair along, unused), converted where it is consumed
      rv[k] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rsV, eoff >= 0 ? (unsigned)eoff * esV : BUF_OOB, 0, 0));
    }
  };
  // T: a thread gathers pixel `trow` of the tile at the taps 2 i + thalf (wave-uniform; consecutive lanes write consecutive LDS words)
  const int trow = tid & (TP - 1), thalf = __builtin_amdgcn_readfirstlane(tid >> 7);
  f32x4 rt[WM_ITEMS];
  auto load_t = [&](int tile, bool valid) {
    int m = tile * TP + trow;
    asm volatile("" : "+v"(m));  // (the same for the gathers)
#pragma unroll
    for (int i = 0; i < WM_ITEMS; ++i) {
      const int tap = 2 * i + thalf;
      rt[i] = thin::gather4(gs, rsS, lds_, narrow, hwv, m, tap, valid && tap < TAPS_MAX && m < npixv);
    }
  };
  auto store_t = [&]() {
#pragma unroll
    for (int i = 0; i < WM_ITEMS; ++i) {
      const int tap = 2 * i + thalf;
      if (tap < TAPS_MAX) {
#pragma unroll
        for (int s = 0; s < 4; ++s) sT[(tap * 4 + s) * WM_LDT + trow] = rt[i][s];  // (s >= narrow: zeros)
        if (!SMALL_X && tap == TAPS_MAX / 2) ssum += rt[i];  // centre tap: dY at this pixel itself
      }
    }
  };
  // the 32 pixels of chunk c (pixels 32 c + 16 h + 4 g + j of the tile)
  auto chunk = [&](const uint2 (&rv)[8], int c) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 fa[3];
#pragma unroll
      for (int mb = 0; mb < 3; ++mb) fa[mb] = *reinterpret_cast<const f32x4*>(&sT[(mb * 16 + lc) * WM_LDT + c * 32 + h * 16 + 4 * lg]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 r = rv[h * 4 + j];
        float v[2];
        v[0] = __builtin_bit_cast(float, vbf ? r.x << 16 : r.x);
        v[1] = __builtin_bit_cast(float, vbf ? r.x & 0xffff0000u : r.y);
        if (XF != VAE_XF_NONE) {  // (whole tiles: no pixel of the wide tensor is padding)
#pragma unroll
          for (int e = 0; e < 2; ++e) v[e] = thin::xform1<XF>(v[e], sc[e], sh[e], cq + e < wide);
        }
#pragma unroll
        for (int mb = 0; mb < 3; ++mb)
#pragma unroll
          for (int e = 0; e < 2; ++e) acc[mb][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[mb][j], v[e], acc[mb][e], 0, 0, 0);
      }
    }
  };

  const thin::TileRange tr = thin::tile_range(split, thin::tiles_per_part(ntiles, p.nsplit), ntiles);
  const int pofs = 4 * lg;  // this lane's first pixel of a tile's chunk 0
  uint2 rva[8], rvb[8];
  if (tr.beg < tr.end) {
    load_t(tr.beg, true);
    load_v(rva, tr.beg * TP + pofs);
  }
  for (int tile = tr.beg; tile < tr.end; ++tile) {
    int mb0 = tile * TP + pofs;
    asm volatile("" : "+v"(mb0));  // (else hipcc keeps one induction register per load of the tile: 32 of them)
    const bool more = tile + 1 < tr.end;
    __syncthreads();  // the previous tile's reads of sT are done (first time round: the constant rows are in place)
    store_t();
    __syncthreads();
    load_t(tile + 1, more);  // in flight under the MFMAs below
    if (XF != VAE_XF_NONE) {
      const int b = (tile * TP) / hwv;  // uniform: a tile lies inside one image (wgrad_mfma_serves)
      if (b != xb) {
        xb = b;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          sc[e] = (cq + e < wide) ? p.scale[(int64_t)b * p.g.Cs + cq + e] : 0.f;
          sh[e] = (cq + e < wide) ? p.shift[(int64_t)b * p.g.Cs + cq + e] : 0.f;
        }
      }
    }
    load_v(rvb, mb0 + 32);
    chunk(rva, 0);
    load_v(rva, mb0 + 64);
    chunk(rvb, 1);
    load_v(rvb, mb0 + 96);
    chunk(rva, 2);
    load_v(rva, more ? mb0 + TP : npixv);
    chunk(rvb, 3);
  }

  // slab of this split: lane (lc, lg) holds rows (tap = 4 mb + lg, s = r) of channels cq, cq + 1
  const thin::Slab sl = thin::slab_of(p, split, TAPS_MAX);
#pragma unroll
  for (int mb = 0; mb < 3; ++mb)
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = mb * 4 + lg, ch = cq + e;
        if (ch < wide) {
          if (t < TAPS_MAX && r < narrow) thin::slab_store<SMALL_X>(sl, ch, t, r, acc[mb][e][r]);
          if (SMALL_X && mb == 2 && r == 0 && lg == 1 && p.bias_partial) thin::bias_partial_row(p, split)[ch] = acc[mb][e][r];  // row 36
        }
      }
  if (!SMALL_X && p.bias_partial && blockIdx.y == 0) {  // sums of dY: 256 threads' shares, fixed order
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) sT[s * NT + tid] = ssum[s];
    __syncthreads();
    if (tid < p.M) {
      float t = 0.f;
      for (int i = 0; i < NT; ++i) t += sT[tid * NT + i];
      thin::bias_partial_row(p, split)[tid] = t;
    }
  }
}
#define WG_BOUNDS __launch_bounds__(NT, 4)  // 128 registers: the 1024 workgroups of a full-resolution launch in one round
#else
constexpr int WG_SI = TP * TAPS_MAX + 32;
#define WG_BOUNDS __launch_bounds__(NT)
#endif

// SMALL_X: the narrow side is X (N <= 4): V = dY over output pixels, S = X gathered with g, out[m = lane][tap][s]
// else   : the narrow side is dY (M <= 4): V = XF(X) over INPUT pixels, S = dY gathered with the transposed geometry
//          (the output pixel whose tap lands on this input pixel), out[s][tap][n = lane]
template <bool SMALL_X, int XF>
__global__ WG_BOUNDS void wgrad_smallk_kernel(vae_wgrad_args p, vae_conv_geom gs, int ntiles) {
  __shared__ f32x4 sI[WG_SI];  // VALU body: [128 px][9 taps] + 128 floats for the bias sums of the final reduction
#if VAE_THIN_F32_MFMA
  if (wgrad_mfma_serves<SMALL_X, XF>(p, gs)) {  // uniform over the grid
    wgrad_smallk_mfma<SMALL_X, XF>(p, gs, ntiles, reinterpret_cast<float*>(sI));
    return;
  }
#endif
  const int tid = threadIdx.x, lane = tid & 127, half = tid >> 7;
  const int split = blockIdx.x;
  const int ch = blockIdx.y * 128 + lane;            // channel of the wide side
  const int wide = SMALL_X ? p.M : p.N, narrow = SMALL_X ? p.N : p.M;
  const bool chok = ch < wide;
  const float* __restrict__ V = SMALL_X ? p.dY : p.X;
  const float* __restrict__ S = SMALL_X ? p.X : p.dY;
  const int ldv = SMALL_X ? p.ldy : p.g.Cs, lds_ = SMALL_X ? p.g.Cs : p.ldy;
  const int npixv = gs.B * gs.Ho * gs.Wo;            // pixels of V (= row grid of gs)
  const int hwv = gs.Ho * gs.Wo;
  const bool vbf = (SMALL_X ? p.y_bf16 : p.x_bf16) != 0;  // storage of the wide operand
  const size_t vbytes = (size_t)npixv * ldv * (vbf ? 2u : 4u);
  const auto rsV = VAE_BUF_RSRC(V, vbytes < BUF_MAX ? vbytes : BUF_MAX);

  float acc[TAPS_MAX][4];
#pragma unroll
  for (int t = 0; t < TAPS_MAX; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[t][s] = 0.f;
  float vsum = 0.f;                                  // SMALL_X: bias gradient of this lane's channel
  f32x4 ssum = {0.f, 0.f, 0.f, 0.f};                 // !SMALL_X: bias gradient = centre-tap sums of dY (same in every lane)
  int xb = -1;
  float xsc = 1.f, xsh = 0.f;

  const thin::TileRange tr = thin::tile_range(split, thin::tiles_per_part(ntiles, p.nsplit), ntiles);
  for (int tile = tr.beg; tile < tr.end; ++tile) {
    const int m0 = tile * TP;
    __syncthreads();  // the previous tile's reads of sI are done
    stage_small(gs, S, lds_, narrow, m0, npixv, sI);
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < TP / 2; ++i) {
      const int row = half + 2 * i;
      const int m = m0 + row;
      const bool ok = chok && m < npixv;
      float v = buf_load1_elem(rsV, vbf, ok ? m * ldv + ch : -1);
      if (XF != VAE_XF_NONE) {
        const int b = min(m, npixv - 1) / hwv;  // uniform per row
        if (b != xb) {
          xb = b;
          xsc = chok ? p.scale[(int64_t)b * p.g.Cs + ch] : 0.f;
          xsh = chok ? p.shift[(int64_t)b * p.g.Cs + ch] : 0.f;
        }
        v = thin::xform1<XF>(v, xsc, xsh, ok);
      }
      if (SMALL_X) vsum += v;
#pragma unroll
      for (int t = 0; t < TAPS_MAX; ++t) {
        if (t < gs.taps) {  // uniform
          const f32x4 sv = sI[row * gs.taps + t];
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[t][s] += v * sv[s];
          if (!SMALL_X && t == gs.taps / 2) ssum += sv;  // centre tap: the output pixel at this input pixel
        }
      }
    }
  }

  // the two pixel streams of a lane are added in a fixed order, then the slab is written
  __syncthreads();
  float* red = reinterpret_cast<float*>(sI);  // [128][36] + 4
  if (half == 1) {
#pragma unroll
    for (int t = 0; t < TAPS_MAX; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) red[lane * 36 + t * 4 + s] = acc[t][s];
    if (SMALL_X) red[128 * 36 + lane] = vsum;
    else if (lane == 0) {
#pragma unroll
      for (int s = 0; s < 4; ++s) red[128 * 36 + s] = ssum[s];
    }
  }
  __syncthreads();
  if (half == 0) {
    const thin::Slab sl = thin::slab_of(p, split, gs.taps);
    if (chok) {
#pragma unroll
      for (int t = 0; t < TAPS_MAX; ++t)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (t < gs.taps && s < narrow) thin::slab_store<SMALL_X>(sl, ch, t, s, acc[t][s] + red[lane * 36 + t * 4 + s]);
    }
    if (p.bias_partial) {
      if (SMALL_X) {  // every channel block owns its channels' sums of dY
        if (chok) thin::bias_partial_row(p, split)[ch] = vsum + red[128 * 36 + lane];
      } else if (blockIdx.y == 0 && lane < p.M) {
        thin::bias_partial_row(p, split)[lane] = ssum[lane] + red[128 * 36 + lane];
      }
    }
  }
}

}  // namespace

bool conv_smallk_eligible(const vae_igemm_args& a) {
  const vae_conv_geom& g = a.g;
  return a.K <= 4 && a.batch == 1 && a.xf == VAE_XF_NONE && a.res == nullptr && a.alpha == 1.0f && g.taps <= TAPS_MAX &&
         g.mode != VAE_MODE_DGRAD_S2 && thin::desc_fits((size_t)a.M * a.ldc, 4u) && thin::narrow_fits(g);
}
int launch_conv_smallk(const vae_igemm_args& a, hipStream_t st) {
  dim3 grid((unsigned)((a.M + TP - 1) / TP), (unsigned)((a.N + 127) / 128));
  hipLaunchKernelGGL(conv_smallk_kernel, grid, dim3(NT), 0, st, a);
  return 0;
}

int wgrad_smallk_kind(const vae_wgrad_args& a) { return thin::wgrad_kind(a); }
int wgrad_smallk_tiles(const vae_wgrad_args& a) { return thin::wgrad_tiles(a); }

int launch_wgrad_smallk(const vae_wgrad_args& a, hipStream_t st) {
  const int kind = thin::wgrad_kind(a), ntiles = thin::wgrad_tiles(a);
  const vae_conv_geom gs = thin::wgrad_geom(a, kind);
  const dim3 grid = thin::wgrad_grid(a, kind);
  if (kind == 1) hipLaunchKernelGGL((wgrad_smallk_kernel<true, VAE_XF_NONE>), grid, dim3(NT), 0, st, a, gs, ntiles);
  else dispatch_xf_or_silu(a.xf, [&](auto xf) { hipLaunchKernelGGL((wgrad_smallk_kernel<false, decltype(xf)::value>), grid, dim3(NT), 0, st, a, gs, ntiles); });
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// conv_smalln: 3x3 stride-1 'same' convolution with <= 4 OUTPUT channels (decoder.conv_out: 128 -> 3), optionally
// with GroupNorm(+SiLU) fused on the input.  One lane owns one output pixel of a 4x32-pixel tile and walks the
// 9 x C input values of its window: activations come from an LDS halo (the staging applies the transform once per
// halo element), weights are wave-uniform and are read through the scalar cache into SGPRs (v_fma with an SGPR
// operand), so the VALU does nothing but the 9*C*N useful FMAs per pixel.
// ---------------------------------------------------------------------------------------------------------
namespace {

constexpr int NTH = thin::TH, NTW = thin::TW, NHW = thin::HW, NHP = thin::HP;  // 4x32 tile, 204 halo pixels
constexpr int NBK = 32, NLD = NBK + 4, NNT = 128;
constexpr int NHQ = NHP * (NBK / 4), NHI = (NHQ + NNT - 1) / NNT;       // 1632 float4 slots, 13 per thread

template <int XF>
__global__ __launch_bounds__(NNT) void conv_smalln_kernel(vae_igemm_args p, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) float sH[NHP * NLD];
  const vae_conv_geom g = p.g;
  const int tid = threadIdx.x;
  const thin::Tile tl = thin::decode(blockIdx.x, tiles_x, tiles_y);
  const int b = tl.b, y0 = tl.y0, x0 = tl.x0;
  const int pr = tid >> 5, px = tid & 31;  // this lane's pixel of the tile
  const bool abf = p.a_bf16 != 0;
  const unsigned esA = abf ? 2u : 4u;
  const auto rsA = VAE_BUF_RSRC(reinterpret_cast<const char*>(p.A) + (int64_t)b * g.Hs * g.Ws * g.Cs * esA, (size_t)g.Hs * g.Ws * g.Cs * esA);
  const float* __restrict__ W = p.W;

  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int hk4 = tid & 7;  // the thread's 4 channels are the same for all of its halo slots
  uint4 rh[NHI];  // as loaded (fp32 quad or 4 bf16): converted when the halo is stored
  int hmask = 0;
  f32x4 rsc = {0.f, 0.f, 0.f, 0.f}, rsh = {0.f, 0.f, 0.f, 0.f};
  auto load_halo = [&](int c0) {
    hmask = 0;
    const int c = c0 + hk4 * 4;
    if (XF != VAE_XF_NONE) {
      const int cs = min(c, p.K - 4);
      rsc = *reinterpret_cast<const f32x4*>(p.scale + (int64_t)b * g.Cs + cs);
      rsh = *reinterpret_cast<const f32x4*>(p.shift + (int64_t)b * g.Cs + cs);
    }
#pragma unroll
    for (int i = 0; i < NHI; ++i) {
      const int q = tid + NNT * i;
      const int pp = q >> 3;
      const int ir = pp / NHW, jc = pp - ir * NHW;
      const int hy = y0 - 1 + ir, hx = x0 - 1 + jc;
      const bool ok = (q < NHQ) && ((unsigned)hy < (unsigned)g.Hs) && ((unsigned)hx < (unsigned)g.Ws) && (c < p.K);
      rh[i] = buf_load4_raw(rsA, esA, ok ? ((hy * g.Ws + hx) * g.Cs + c) : -1);
      hmask |= (ok ? 1 : 0) << i;
    }
  };
  auto store_halo = [&]() {
#pragma unroll
    for (int i = 0; i < NHI; ++i) {
      const int q = tid + NNT * i;
      if (q < NHQ) {
        f32x4 v = raw4_to_f32(rh[i], abf);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = thin::xform1<XF>(v[e], rsc[e], rsh[e], (hmask >> i) & 1);  // padding stays zero after the transform
        *reinterpret_cast<f32x4*>(&sH[(q >> 3) * NLD + hk4 * 4]) = v;
      }
    }
  };

  const int kchunks = (p.K + NBK - 1) / NBK;
  load_halo(0);
  for (int cch = 0; cch < kchunks; ++cch) {
    const int c0 = cch * NBK;
    __syncthreads();  // every lane has left the previous chunk's halo
    store_halo();
    __syncthreads();
    if (cch + 1 < kchunks) load_halo(c0 + NBK);  // in flight during this chunk's FMAs
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap - kh * 3;
      const float* hrow = &sH[((pr + kh) * NHW + px + kw) * NLD];
#pragma unroll
      for (int q = 0; q < NBK / 4; ++q) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(hrow + q * 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if (s < p.N) {  // uniform
            // wave-uniform address: the compiler reads these through the scalar cache
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(W + (int64_t)s * p.sn + (int64_t)tap * p.st + c0 + q * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[s] = __builtin_fmaf(a[e], w4[e], acc[s]);
          }
        }
      }
    }
  }

  const int oy = y0 + pr, ox = x0 + px;
  const auto rsC = VAE_BUF_RSRC(p.C + (int64_t)b * g.Ho * g.Wo * p.ldc, (size_t)g.Ho * g.Wo * p.ldc * 4u);
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < p.N) {
      const float v = acc[s] + (p.bias ? p.bias[s] : 0.f);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsC,
                                            (oy < g.Ho && ox < g.Wo) ? (unsigned)((oy * g.Wo + ox) * p.ldc + s) * 4u : BUF_OOB, 0, 0);
    }
}

}  // namespace

bool conv_smalln_eligible(const vae_igemm_args& a) {
  const vae_conv_geom& g = a.g;
  return a.N <= 4 && a.K >= NBK && a.K % NBK == 0 && a.sn % 4 == 0 && a.st % 4 == 0 && aligned16(a.W) && a.batch == 1 && a.res == nullptr && a.track == nullptr && a.alpha == 1.0f &&
         a.A16 == nullptr && thin::fwd_same_3x3(g) && g.Wo % NTW == 0 && g.Ho % NTH == 0 && a.sk == 1 && g.Cs % 4 == 0 && aligned16(a.A) &&
         (a.xf == VAE_XF_NONE || (aligned16(a.scale) && aligned16(a.shift))) &&
         thin::desc_fits(thin::image_elems(g), 4u) && thin::desc_fits((size_t)g.Ho * g.Wo * a.ldc, 4u);
}
int launch_conv_smalln(const vae_igemm_args& a, hipStream_t st) {
  int tx, ty;
  const dim3 grid = thin::tile_grid(a.g, tx, ty);
  dispatch_xf_or_silu(a.xf, [&](auto xf) { hipLaunchKernelGGL((conv_smalln_kernel<decltype(xf)::value>), grid, dim3(NNT), 0, st, a, tx, ty); });
  return 0;
}
