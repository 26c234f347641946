// fp32 forward and dgrad of an Upsample2D block's convolution, conv3x3(nearest_upsample_2x(x)), as a Winograd-type minimal
// filtering scheme with 9 multiplications per LOW-resolution pixel and channel pair (direct: 36; the four 2x2 phase
// convolutions of round 1: 16).  Two loops, chosen at build time (VAE_UPW_X3): split-bf16 products on v_mfma_f32_32x32x16_bf16,
// 16 channels per step, both operands arriving as ready bf16 planes (the default; described in front of that kernel below), or
// exact fp32 products on v_mfma_f32_32x32x2_f32, 8 channels per step (-DVAE_UPW_X3=0, make upw_x3_off; the "Kernel" paragraph
// below describes it; transforms, tile mapping, seating of the ninth position and the epilogue are the same in both).
//
// Forward.  The 2x2 outputs of low-resolution pixel (i, j) see, through F(2x2, 3x3), the 4x4 patch of the upsampled image with
// origin (2i-1, 2j-1): its rows are x[i-1], x[i], x[i], x[i+1] -- rows (and columns) repeat in pairs, so row 2 of B^T d
// vanishes and only the 3 x 3 transform-domain positions {0, 1, 3}^2 carry anything.  With the factor 2 of position 1 folded
// into the weights nothing is halved at all:
//     Y = A'^T [ sum_ci (G' g G'^T) (.) (L d3 L^T) ] A'     d3: 3x3 low-resolution patch (origin (i-1, j-1)), g: 3x3 kernel
//     L = [1 -1 0; 0 1 0; 0 1 -1]     G' = [1 0 0; 1 1 1; 0 0 1]     A'^T = [1 1 0; 0 1 -1]
// (row 0 of the result: g0 (x[i-1] - x[i]) + (g0+g1+g2) x[i] = g0 x[i-1] + (g1+g2) x[i]: the phase kernel of an even output row).
// Dgrad (mode VAE_MODE_UP2X_DGRAD): the gradient wrt the low-resolution x is the 2x2 sum-pool of the 3x3 dgrad of the
// high-resolution dY; the pool folds into the output transform (sum of the rows of A^T = [1 2 0 -1]) and again only positions
// {0, 1, 3}^2 are needed:
//     dx = s^T [ sum_co (G' g~ G'^T) (.) (Bt3 d4 Bt3^T) ] s    d4: 4x4 patch of dY (origin (2i-1, 2j-1)), g~: rotated kernel
//     Bt3 = [1 0 -1 0; 0 1 1 0; 0 1 0 -1]     s = [1 1 -1]
// Neither the upsampled tensor nor the high-resolution input gradient ever exists.
//
// Kernel: the scheme of conv3_wino.hip (transformed weights U = G' g G'^T rebuilt from the live weights per launch, layout
// [K/8][9][N][8]; chunk of 8 channels per step; the chunk's halo staged once, the V image [9][32 tiles][8] double buffered in
// LDS; U fragments from L2 straight into registers one step ahead; accumulators through LDS in the epilogue), sharing with it
// by name (wino_common.h) tile_of_workgroup / xcd_spatial, the U layout (u_gather, u_out, u_frag, u_bytes), spill_acc and the
// eligibility preamble.  Workgroup = 8 waves = 32 low-resolution pixels (4 x 8) x 64 channels: wave w owns position w (both
// 32-channel blocks) and the NINTH position is split by channel block over two waves on different SIMDs (waves 0, 1 in even
// workgroups, 2, 3 in odd ones: wave k of a workgroup runs on SIMD k % 4), so a workgroup loads the SIMDs 20 20 16 16 MFMAs per
// step and two co-resident workgroups 36 each.  (A first version with one position per wave and 9 waves put three waves of
// every workgroup on SIMD 0: 0.46 of the matrix peak.)
//
// Non-finite operands under the split build (the policy of the flat kernels' F32X3, igemm.hip): Inf and NaN stay non-finite
// (the hi plane carries them, the residual planes become NaN), and a finite value in the top 2^-8 of the fp32 range, which
// rounds to Inf in bf16, behaves like Inf.  Every output whose window contains such a value is non-finite; no other is.
#include "wino_common.h"
#include <type_traits>
#include <algorithm>

// VAE_UPW_PRIO 1 (default): in the dgrad instantiation waves 4..7 (the second-dispatched wave of every SIMD, which multiplies first
// and stages behind it) run the loop at s_setprio 1.  Measured per instantiation and wave half (tools/wino_seat_ab.py,
// profiles/wino4_seat_measured.json): the dgrad 1.4-1.8 % faster, the forward 0.5-1.0 % slower with it, waves 0..3 no difference.
// Re-measured with four channel blocks per workgroup (profiles/upw_wide_measured.json): the dgrad up to 2 % faster, the forward
// 0.4-2.7 % slower with it.
#ifndef VAE_UPW_PRIO
#define VAE_UPW_PRIO 1
#endif
// U images up to this many bytes put the channel blocks of a spatial tile on one XCD (wino::xcd_spatial): of the step's layers the
// 256-channel one (2.4 MB as fp32, 3.5 MB as planes).  Re-measured with four channel blocks per workgroup: 16 MB (the four channel
// tiles of a 512-channel spatial tile on one XCD) 1.8-2.7 % slower at 512 -> 512, 64^2; 2 MB within 0.7 % everywhere.
#ifndef VAE_UPW_XCD_LIMIT
#define VAE_UPW_XCD_LIMIT (4 << 20)
#endif
#ifndef VAE_UPW_X3
#define VAE_UPW_X3 1  // 1: split-bf16 products from bf16 planes of U and V, 16 channels per step; 0: exact fp32 products, 8 channels per step (make upw_x3_off)
#endif
// 32-channel blocks per workgroup of the split loop, per instantiation: 4 (32 tiles x 128 output channels, one workgroup per CU) or 2
// (32 x 64, two per CU: the loop as it was; make upw_nb2).  The V transform, its split and the V / halo LDS traffic are work per
// (tile, input channel) that every channel tile of a spatial tile repeats; four blocks halve the repeats for the same matrix work
// and the same bits.  Measured per launch 0.92-0.98 (forward) and 0.89-0.92 (dgrad) of two blocks (profiles/upw_wide_measured.json).
#ifndef VAE_UPW_NB_FWD
#define VAE_UPW_NB_FWD 4
#endif
#ifndef VAE_UPW_NB_DG
#define VAE_UPW_NB_DG 4
#endif
#if VAE_UPW_X3
#include "bf16_frag.h"
#endif

namespace {

constexpr int UTH = 4, UTW = 8;            // low-resolution pixels (= Winograd tiles) per workgroup tile
constexpr int UTL = UTH * UTW;             // 32
static_assert(UTL == wino::TILES, "spill_acc");
constexpr int NPOS = 9;
constexpr int UNT = 512;                   // 8 waves
constexpr int UNB = 2;                     // 32-channel blocks per workgroup
constexpr int UHF = (UTH + 2) * (UTW + 2); // forward halo pixels (6 x 10)
constexpr int UHD = (2 * UTH + 2) * (2 * UTW + 2);  // dgrad halo pixels (10 x 18)
constexpr int UMLD = 33;                   // epilogue image row (floats)
constexpr int USM = NPOS * UTL * UMLD;     // epilogue image, overlays the V / halo buffers

#if !VAE_UPW_X3  // ---- exact fp32 products: 8 channels per step ----
constexpr int UBK = 8;                     // channels per step
constexpr int USV = NPOS * UTL * UBK;      // floats per V buffer (9216 B)
constexpr int USH = UHD * UBK;             // floats per halo buffer (sized for the dgrad)
constexpr int UP_LDS = (USM > 2 * USV + 2 * USH ? USM : 2 * USV + 2 * USH) * 4;  // 38016 B

// U[pos = a*3+b][n][k] = (G' g G'^T)[a][b] for g = W[n][.][.][k] (forward: N = Cout, K = Cin) or g = rot180(W[k][.][.][n]) (dgrad:
// N = Cin, K = Cout); G' = [1 0 0; 1 1 1; 0 0 1]; layout [K/8][9][N][8]
__global__ __launch_bounds__(256) void upwino_weights_kernel(const float* __restrict__ W, int N, int K, int dgrad, int64_t sn, int64_t sk, int64_t st,
                                                             float* __restrict__ U) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * K) return;
  const int k = (int)(i % K), n = (int)(i / K);
  float g[3][3];
  wino::u_gather(W, n, k, dgrad, sn, sk, st, g);
  float t[3][3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    t[0][b] = g[0][b];
    t[1][b] = (g[0][b] + g[2][b]) + g[1][b];
    t[2][b] = g[2][b];
  }
  float* o = wino::u_out<NPOS>(U, N, n, k);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wino::u_at(o, N, a * 3 + 0) = t[a][0];
    wino::u_at(o, N, a * 3 + 1) = (t[a][0] + t[a][2]) + t[a][1];
    wino::u_at(o, N, a * 3 + 2) = t[a][2];
  }
}

template <bool DG>
__global__ __launch_bounds__(UNT, 4) void conv3_upwino_kernel(vae_igemm_args p, const float* __restrict__ U, int tiles_x, int tiles_y, int xcd_sp) {
  constexpr int WBN = 32 * UNB;           // output channels per workgroup
  constexpr int HW_ = DG ? 2 * UTW + 2 : UTW + 2;  // halo width in pixels
  constexpr int HP = DG ? UHD : UHF;      // halo pixels
  __shared__ __attribute__((aligned(16))) float wsm[UP_LDS / 4];
  float* const sV = wsm;            // [2][USV]
  float* const sH = wsm + 2 * USV;  // [2][USH]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // wave = position 0..7 of the 3 x 3 transform domain
  // position 8: channel block 0 on wave xw0, block 1 on wave xw0 + 1
  const int xw0 = (blockIdx.x & 1) * 2;
  const bool extra = wave == xw0 || wave == xw0 + 1;  // uniform per wave
  const int xnb = wave - xw0;
  const int lr = lane & 31, lh = lane >> 5;
  const vae_conv_geom g = p.g;
  const int tilesN = (p.N + WBN - 1) / WBN;
  const wino::TileId wg = wino::tile_of_workgroup(blockIdx.x, tilesN, tiles_x, tiles_y, xcd_sp);
  const int b = wg.b;
  const int y0 = wg.ty * UTH, x0 = wg.tx * UTW, n0 = wg.tn * WBN;  // low-resolution origin of the tile
  const int nsteps = p.K / UBK;

  // ---- halo role: pixel hp of the chunk's halo, channel quad hq: loaded once per chunk, stored to sH two steps ahead ----
  const bool hrole = tid < 2 * HP;
  const int hp = tid >> 1, hq = tid & 1;
  const int hy = (DG ? 2 * y0 : y0) - 1 + hp / HW_, hx = (DG ? 2 * x0 : x0) - 1 + hp % HW_;
  const bool hin = hrole && ((unsigned)hy < (unsigned)g.Hs) && ((unsigned)hx < (unsigned)g.Ws);
  const auto rsA = VAE_BUF_RSRC(p.A + (int64_t)b * g.Hs * g.Ws * g.Cs, (size_t)g.Hs * g.Ws * g.Cs * 4u);
  const unsigned hbase = hin ? (unsigned)(((hy * g.Ws + hx) * g.Cs + hq * 4) * 4) : BUF_OOB;
  f32x4 rh = {0.f, 0.f, 0.f, 0.f};
  auto load_halo_into = [&](int step, f32x4& h) {
    const bool ok = hin && step < nsteps;
    h = VAE_BUF_LOAD4(rsA, ok ? hbase + (unsigned)(step * UBK * 4) : BUF_OOB);
  };
  auto store_halo_from = [&](float* dst, const f32x4& h) {
    if (hrole) *reinterpret_cast<f32x4*>(&dst[hp * UBK + hq * 4]) = h;
  };

  // ---- V role (threads 0..255): tile vt, channel vc of the chunk ----
  const bool vrole = tid < 256;
  const int vt = (tid >> 3) & 31, vc = tid & 7;
  const int vorg = DG ? ((2 * (vt >> 3)) * HW_ + 2 * (vt & 7)) * UBK + vc : ((vt >> 3) * HW_ + (vt & 7)) * UBK + vc;
  auto write_v = [&](const float* sHc, float* dst) {
    if (!vrole) return;
    float r[3][DG ? 4 : 3];
    if (!DG) {  // L d3 L^T
      float d[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) d[i][j] = sHc[vorg + (i * HW_ + j) * UBK];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        r[0][j] = d[0][j] - d[1][j];
        r[1][j] = d[1][j];
        r[2][j] = d[1][j] - d[2][j];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        dst[((a * 3 + 0) * UTL + vt) * UBK + vc] = r[a][0] - r[a][1];
        dst[((a * 3 + 1) * UTL + vt) * UBK + vc] = r[a][1];
        dst[((a * 3 + 2) * UTL + vt) * UBK + vc] = r[a][1] - r[a][2];
      }
    } else {    // Bt3 d4 Bt3^T
      float d[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) d[i][j] = sHc[vorg + (i * HW_ + j) * UBK];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[0][j] = d[0][j] - d[2][j];
        r[1][j] = d[1][j] + d[2][j];
        r[2][j] = d[1][j] - d[3][j];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        dst[((a * 3 + 0) * UTL + vt) * UBK + vc] = r[a][0] - r[a][2];
        dst[((a * 3 + 1) * UTL + vt) * UBK + vc] = r[a][1] + r[a][2];
        dst[((a * 3 + 2) * UTL + vt) * UBK + vc] = r[a][1] - r[a][3];
      }
    }
  };

  // ---- U fragments of this wave's position: [step][pos][n0 + 32 nb + lr][4 lh .. 4 lh + 3], L2 -> registers one step ahead ----
  const auto rsU = VAE_BUF_RSRC(U, wino::u_bytes(nsteps, NPOS, p.N));
  unsigned bvo[UNB];
#pragma unroll
  for (int q = 0; q < UNB; ++q) bvo[q] = (n0 + q * 32 + lr < p.N) ? wino::u_frag(n0 + q * 32 + lr, lh) : BUF_OOB;
  const unsigned bpos = wino::u_pos_bytes(p.N);
  const unsigned bvx = extra ? bvo[xnb & 1] : BUF_OOB;  // the ninth position's block (waves without one request nothing)
  // ONE register set, refilled behind the MFMAs that consume it (conv3_wino.hip); every step issues the same UNB + 1 requests
  // in code every wave runs (beyond the last chunk the last one again, never used; waves without a ninth-position block request
  // out of range)
  f32x4 bq[UNB + 1];
  auto load_b1 = [&](int step, int i) {
    const int st = min(step, nsteps - 1);
    const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)(st * NPOS + (i < UNB ? wave : 8)) * bpos);
    bq[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsU, i < UNB ? bvo[i < UNB ? i : 0] : bvx, so, 0));
  };

  f32x16 acc[UNB], accx;
#pragma unroll
  for (int nb = 0; nb < UNB; ++nb)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[nb][e] = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) accx[e] = 0.f;

  // prologue: halo(0), halo(1) in LDS, V(0) from halo(0); halo(2) and the U fragments of step 0 in registers
#pragma unroll
  for (int i = 0; i <= UNB; ++i) load_b1(0, i);
  {
    f32x4 h0, h1;
    load_halo_into(0, h0);
    load_halo_into(1, h1);
    load_halo_into(2, rh);
    store_halo_from(sH, h0);
    store_halo_from(sH + USH, h1);
  }
  __syncthreads();
  write_v(sH, sV);
  __syncthreads();
  auto multiply = [&](const float* cV, int s) {  // step s; requests step s+1's fragments as it goes
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(&cV[(wave * UTL + lr) * UBK + 4 * lh]);
    f32x4 ax = a4;
    if (extra) ax = *reinterpret_cast<const f32x4*>(&cV[(8 * UTL + lr) * UBK + 4 * lh]);
#pragma unroll
    for (int nb = 0; nb < UNB; ++nb) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], bq[nb][e], acc[nb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      load_b1(s + 1, nb);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (extra) {
#pragma unroll
      for (int e = 0; e < 4; ++e) accx = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[e], bq[UNB][e], accx, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    load_b1(s + 1, UNB);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stage_next = [&](int s, int par) {
    if (s + 1 < nsteps) write_v(sH + (par ^ 1) * USH, sV + (par ^ 1) * USV);  // V(s+1): nobody reads that buffer now
    store_halo_from(sH + par * USH, rh);                                       // halo(s+2)
    load_halo_into(s + 3, rh);
  };
  // waves 0..3 (which own the V transform) stage first, waves 4..7 multiply first: two copies of the loop, so that the order of
  // the memory requests is fixed inside each and hipcc's wait counts are exact (conv3_wino.hip)
  auto step = [&](int s, int par, auto first_c) {
    const float* cV = sV + par * USV;
    if (decltype(first_c)::value) {
      stage_next(s, par);
      __builtin_amdgcn_sched_barrier(0);
      multiply(cV, s);
    } else {
      multiply(cV, s);
      __builtin_amdgcn_sched_barrier(0);
      stage_next(s, par);
    }
    __syncthreads();
  };
  auto run = [&](auto first_c) {
    int s = 0;
    for (; s + 1 < nsteps; s += 2) {
      step(s, 0, first_c);
      step(s + 1, 1, first_c);
    }
    if (s < nsteps) step(s, 0, first_c);
  };
#if VAE_UPW_PRIO  // one static s_setprio around the loop; a scalar condition: the instruction ignores EXEC
  if (DG && __builtin_amdgcn_readfirstlane(tid) >= 256) __builtin_amdgcn_s_setprio(1);
#endif
  if (wave < 4) run(std::true_type{});  // uniform per wave
  else run(std::false_type{});
#if VAE_UPW_PRIO
  if (DG) __builtin_amdgcn_s_setprio(0);
#endif

  // ---- epilogue: per 32-channel block, M through LDS, then the output transform ----
  float* const sM = wsm;  // [9][32 tiles][UMLD], over the V / halo buffers (the last step's barrier has passed)
  const size_t obytes = (size_t)g.Ho * g.Wo * p.ldc * 4u;
  const auto rsC = VAE_BUF_RSRC(p.C + (int64_t)b * g.Ho * g.Wo * p.ldc, obytes);
#pragma unroll
  for (int nb = 0; nb < UNB; ++nb) {
    if (nb > 0) __syncthreads();  // the previous block's reads are done
    wino::spill_acc(sM, wave, UMLD, acc[nb], lr, lh);
    if (wave == xw0 + nb) wino::spill_acc(sM, 8, UMLD, accx, lr, lh);  // the ninth position's block nb
    __syncthreads();
    {
#pragma unroll
      for (int rnd = 0; rnd < 2; ++rnd) {
        const int co = tid & 31, tile = (tid >> 5) + 16 * rnd;
        const int col = n0 + nb * 32 + co;
        float m[9];
#pragma unroll
        for (int pos = 0; pos < 9; ++pos) m[pos] = sM[(pos * UTL + tile) * UMLD + co];
        const int oy = y0 + (tile >> 3), ox = x0 + (tile & 7);  // low-resolution pixel of the tile
        if (!DG) {
          const float bv = (p.bias && col < p.N) ? p.bias[col] : 0.f;
          float h[2][3];  // A'^T M
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            h[0][j] = m[0 * 3 + j] + m[1 * 3 + j];
            h[1][j] = m[1 * 3 + j] - m[2 * 3 + j];
          }
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const float yv[2] = {h[a][0] + h[a][1], h[a][1] - h[a][2]};
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
              const int py = 2 * oy + a, px = 2 * ox + bb;
              const unsigned off = (col < p.N && py < g.Ho && px < g.Wo) ? (unsigned)(((py * g.Wo + px) * p.ldc + col) * 4) : BUF_OOB;
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv[bb] + bv), rsC, off, 0, 0);
            }
          }
        } else {
          // s^T M s with s = [1 1 -1]
          const float h0 = (m[0] + m[3]) - m[6], h1 = (m[1] + m[4]) - m[7], h2 = (m[2] + m[5]) - m[8];
          const float v = (h0 + h1) - h2;
          const unsigned off = (col < p.N && oy < g.Ho && ox < g.Wo) ? (unsigned)(((oy * g.Wo + ox) * p.ldc + col) * 4) : BUF_OOB;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsC, off, 0, 0);
        }
      }
    }
  }
}

#else  // ---- VAE_UPW_X3: split-bf16 products, 16 channels per step ----
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 rate; a product formed as the six plane products of mma_x3_term (bf16_frag.h) on
// v_mfma_f32_32x32x16_bf16 keeps the matrix pipe busy 2.67x shorter (12 MFMAs of 32 cycles per wave and 16 channels, 18 on the waves
// with a ninth-position block, against 16 / 24 of 64 cycles).  Both operands arrive as ready planes, so the loop itself splits nothing:
//   * V: the V-role threads (0..255: tile, channel PAIR of the 16-channel chunk) transform in fp32 exactly as the exact loop does,
//     split once (split3_pair) and write three plane images [plane][9][32 tiles][16] bf16 into LDS: one split per value, shared by
//     the workgroup's 64 output channels.  A row is 32 bytes; its two 16-byte halves are swapped in rows with (tile >> 3) & 1 set,
//     which makes the A fragment one conflict-free ds_read_b128 per plane (the 16-lane groups of that instruction otherwise meet
//     rows 12-15 and 20-23 on the same banks).
//   * U: upwino_weights_kernel writes [ceil(K/16)][9][3 planes][N][16] bf16 (vae_wino_weight_bytes: 6 bytes per value); lane (r, h)
//     reads n = r, k = 8h .. 8h+7 of a plane with one 16-byte load, L2 -> registers one step ahead, as in the exact loop.
//   * K % 16 == 8: channels >= K of the last chunk are zero planes in U AND zero in V (the halo loads of that channel octet are
//     masked: with Cs > K the memory behind channel K holds anything, and 0 x NaN is NaN).
// Halo staging (two f32x4 per staging thread and chunk), the two copies of the loop, one barrier per step, the seating of the
// ninth position and the epilogue are the exact loop's with two channel blocks per workgroup (upw_nb<DG>() == 2).  LDS: two V
// buffers 55,296 B + two halo buffers (forward 7,680 B, dgrad 23,040 B): two workgroups per CU in both instantiations.
// Four channel blocks (upw_nb<DG>() == 4, the default): a wave multiplies the A planes of its position against four blocks of U
// planes, each set re-requested behind the six MFMAs that consumed it (24 MFMAs per wave and step; 80 accumulator and 60 U-plane
// registers, 188 / 190 in all, no scratch); the ninth position's four blocks sit on waves 4..7, one per SIMD (30 MFMAs there, 54
// per SIMD); one workgroup per CU by registers, same LDS; the epilogue goes through the one image four times.
constexpr int XBK = 16;                    // channels per step
constexpr int XPL = NPOS * UTL * XBK;      // bf16 per V plane (9216 B)
constexpr int XSV = 3 * XPL;               // bf16 per V buffer (27,648 B)
template <bool DG>
constexpr int upw_nb() {
  return DG ? VAE_UPW_NB_DG : VAE_UPW_NB_FWD;
}
static_assert((upw_nb<false>() == 2 || upw_nb<false>() == 4) && (upw_nb<true>() == 2 || upw_nb<true>() == 4), "VAE_UPW_NB_*: 2 or 4");
template <bool DG>
constexpr int upw_lds_bytes() {
  constexpr int used = 2 * XSV * 2 + 2 * (DG ? UHD : UHF) * XBK * 4;
  return used > USM * 4 ? used : USM * 4;
}
extern __shared__ __attribute__((aligned(16))) float upw_lds[];

__host__ __device__ __forceinline__ int upw_chunks(int K) { return (K + XBK - 1) / XBK; }
// bytes of one plane of one position of one chunk ([N][16] bf16), and of the whole image
__host__ __device__ __forceinline__ unsigned upw_plane_bytes(int N) { return (unsigned)N * (XBK * 2u); }
__host__ __device__ __forceinline__ size_t upw_u_bytes(int K, int N) { return (size_t)upw_chunks(K) * NPOS * 3 * upw_plane_bytes(N); }

// (G' g G'^T) of the 3x3 kernel g, G' = [1 0 0; 1 1 1; 0 0 1]: o[a * 3 + b]
__device__ __forceinline__ void upw_u_transform(const float (&g)[3][3], float (&o)[9]) {
  float t[3][3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    t[0][b] = g[0][b];
    t[1][b] = (g[0][b] + g[2][b]) + g[1][b];
    t[2][b] = g[2][b];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a * 3 + 0] = t[a][0];
    o[a * 3 + 1] = (t[a][0] + t[a][2]) + t[a][1];
    o[a * 3 + 2] = t[a][2];
  }
}

// U planes of (n, k), k < roundup16(K): split3 of (G' g G'^T)[a][b] (g as in the exact build), zero planes for k >= K
__global__ __launch_bounds__(256) void upwino_weights_kernel(const float* __restrict__ W, int N, int K, int dgrad, int64_t sn, int64_t sk, int64_t st,
                                                             u16* __restrict__ U) {
  const int K16 = upw_chunks(K) * XBK;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * K16) return;
  const int k = (int)(i % K16), n = (int)(i / K16);
  float u[9];
  if (k < K) {
    float g[3][3];
    wino::u_gather(W, n, k, dgrad, sn, sk, st, g);
    upw_u_transform(g, u);
  } else {
#pragma unroll
    for (int pos = 0; pos < 9; ++pos) u[pos] = 0.f;
  }
  u16* o = U + ((int64_t)(k >> 4) * NPOS * 3 * N + n) * XBK + (k & 15);
#pragma unroll
  for (int pos = 0; pos < 9; ++pos) {
    unsigned hi, mid, lo;
    split3_pair(u[pos], 0.f, hi, mid, lo);
    o[(int64_t)(pos * 3 + 0) * N * XBK] = (u16)hi;
    o[(int64_t)(pos * 3 + 1) * N * XBK] = (u16)mid;
    o[(int64_t)(pos * 3 + 2) * N * XBK] = (u16)lo;
  }
}

template <bool DG>
__global__ __launch_bounds__(UNT, upw_nb<DG>() > 2 ? 2 : 4) void conv3_upwino_kernel(vae_igemm_args p, const u16* __restrict__ U, int tiles_x, int tiles_y, int xcd_sp) {
  constexpr int NB = upw_nb<DG>();        // 32-channel blocks per workgroup
  constexpr bool WIDE = NB > 2;           // the ninth position's NB blocks on waves 4 .. 4 + NB - 1, blocks at or beyond N skipped
  constexpr int WBN = 32 * NB;            // output channels per workgroup
  constexpr int HW_ = DG ? 2 * UTW + 2 : UTW + 2;  // halo width in pixels
  constexpr int HP = DG ? UHD : UHF;      // halo pixels
  constexpr int XSH = HP * XBK;           // floats per halo buffer
  u16* const sV = reinterpret_cast<u16*>(upw_lds);                 // [2][3 planes][9][32 tiles][16]
  float* const sH = upw_lds + XSV;                                 // [2][XSH], behind the 2 XSV bf16 of sV

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // wave = position 0..7 of the 3 x 3 transform domain
  const int lr = lane & 31, lh = lane >> 5;
  const vae_conv_geom g = p.g;
  const int tilesN = (p.N + WBN - 1) / WBN;
  const wino::TileId wg = wino::tile_of_workgroup(blockIdx.x, tilesN, tiles_x, tiles_y, xcd_sp);
  const int b = wg.b;
  const int y0 = wg.ty * UTH, x0 = wg.tx * UTW, n0 = wg.tn * WBN;  // low-resolution origin of the tile
  const int nsteps = upw_chunks(p.K);
  // blocks of this channel tile that reach below N (uniform per workgroup).  A block wholly at or beyond N gets no MFMAs and no
  // epilogue pass, and its U requests are out of range in every lane; the ragged block is masked lane by lane (BUF_OOB)
  const int nlive = WIDE ? min(NB, (p.N - n0 + 31) >> 5) : NB;
  // position 8: channel block q on wave xw0 + q.  Two blocks: waves 0, 1 in even workgroups, 2, 3 in odd ones (two co-resident
  // workgroups then load the SIMDs alike).  Four blocks, one workgroup per CU: waves 4..7, one per SIMD, which multiply first
  // and own no V transform
  const int xw0 = WIDE ? 4 : (blockIdx.x & 1) * 2;
  const int xnb = wave - xw0;
  const bool extra = WIDE ? (wave >= 4 && xnb < nlive) : (wave == xw0 || wave == xw0 + 1);  // uniform per wave

  // ---- halo role: pixel hp of the chunk's halo, channel octet hq: loaded once per chunk, stored to sH two steps ahead.  An octet
  // at or beyond K is not loaded (zeros): K is a multiple of 8, so this is the whole K tail ----
  const bool hrole = tid < 2 * HP;
  const int hp = tid >> 1, hq = tid & 1;
  const int hy = (DG ? 2 * y0 : y0) - 1 + hp / HW_, hx = (DG ? 2 * x0 : x0) - 1 + hp % HW_;
  const bool hin = hrole && ((unsigned)hy < (unsigned)g.Hs) && ((unsigned)hx < (unsigned)g.Ws);
  const auto rsA = VAE_BUF_RSRC(p.A + (int64_t)b * g.Hs * g.Ws * g.Cs, (size_t)g.Hs * g.Ws * g.Cs * 4u);
  const unsigned hbase = hin ? (unsigned)(((hy * g.Ws + hx) * g.Cs + hq * 8) * 4) : BUF_OOB;
  f32x4 rh[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  auto load_halo_into = [&](int step, f32x4 (&h)[2]) {
    const bool ok = hin && step * XBK + hq * 8 < p.K;
    h[0] = VAE_BUF_LOAD4(rsA, ok ? hbase + (unsigned)(step * XBK * 4) : BUF_OOB);
    h[1] = VAE_BUF_LOAD4(rsA, ok ? hbase + (unsigned)(step * XBK * 4 + 16) : BUF_OOB);
  };
  auto store_halo_from = [&](float* dst, const f32x4 (&h)[2]) {
    if (hrole) {
      *reinterpret_cast<f32x4*>(&dst[hp * XBK + hq * 8]) = h[0];
      *reinterpret_cast<f32x4*>(&dst[hp * XBK + hq * 8 + 4]) = h[1];
    }
  };

  // ---- V role (threads 0..255): tile vt, channels 2 vc, 2 vc + 1 of the chunk; a plane row holds its k octets swapped when
  // (tile >> 3) & 1 ----
  const bool vrole = tid < 256;
  const int vt = (tid >> 3) & 31, vc = tid & 7;
  const int vorg = DG ? ((2 * (vt >> 3)) * HW_ + 2 * (vt & 7)) * XBK + 2 * vc : ((vt >> 3) * HW_ + (vt & 7)) * XBK + 2 * vc;
  const int vdst = vt * XBK + (((vc >> 2) ^ ((vt >> 3) & 1)) * 8) + (vc & 3) * 2;  // inside one position of one plane
  auto write_v = [&](const float* sHc, u16* dst) __attribute__((always_inline)) {
    if (!vrole) return;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    constexpr int NJ = DG ? 4 : 3;
    // one row of the transform domain at a time, written before the next is read: the whole patch of both channels would not
    // fit beside the accumulators and the U planes (the rows' sums and differences are the exact loop's)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      // forward, L d3: d0 - d1, d1, d1 - d2;  dgrad, Bt3 d4: d0 - d2, d1 + d2, d1 - d3
      const int ia = DG ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 1), ib = DG ? (a == 2 ? 3 : 2) : (a == 0 ? 1 : 2);
      float r[NJ][2];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const f32x2 x = *reinterpret_cast<const f32x2*>(&sHc[vorg + (ia * HW_ + j) * XBK]);
        if (!DG && a == 1) {
          r[j][0] = x[0];
          r[j][1] = x[1];
        } else {
          const f32x2 y = *reinterpret_cast<const f32x2*>(&sHc[vorg + (ib * HW_ + j) * XBK]);
          const bool add = DG && a == 1;
          r[j][0] = add ? x[0] + y[0] : x[0] - y[0];
          r[j][1] = add ? x[1] + y[1] : x[1] - y[1];
        }
      }
      float o[3][2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (!DG) {  // (.) L^T
          o[0][c] = r[0][c] - r[1][c];
          o[1][c] = r[1][c];
          o[2][c] = r[1][c] - r[2][c];
        } else {    // (.) Bt3^T
          o[0][c] = r[0][c] - r[2][c];
          o[1][c] = r[1][c] + r[2][c];
          o[2][c] = r[1][c] - r[NJ - 1][c];
        }
      }
#pragma unroll
      for (int bb = 0; bb < 3; ++bb) {
        const int pos = a * 3 + bb;
        unsigned hi, mid, lo;
        split3_pair(o[bb][0], o[bb][1], hi, mid, lo);
        *reinterpret_cast<unsigned*>(&dst[0 * XPL + pos * UTL * XBK + vdst]) = hi;
        *reinterpret_cast<unsigned*>(&dst[1 * XPL + pos * UTL * XBK + vdst]) = mid;
        *reinterpret_cast<unsigned*>(&dst[2 * XPL + pos * UTL * XBK + vdst]) = lo;
      }
    }
  };

  // ---- U planes of this wave's position: [step][pos][plane][n0 + 32 nb + lr][8 lh .. 8 lh + 7], L2 -> registers one step ahead ----
  const auto rsU = VAE_BUF_RSRC(U, upw_u_bytes(p.K, p.N));
  unsigned bvo[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) bvo[q] = (n0 + q * 32 + lr < p.N) ? (unsigned)(((n0 + q * 32 + lr) * XBK + lh * 8) * 2) : BUF_OOB;
  const unsigned bpl = upw_plane_bytes(p.N);
  // the ninth position's block (waves without one request nothing).  (Written out for four blocks: a lambda shared with the line
  // above moved hipcc's register allocation of the two-block build away from the measured one)
  const unsigned bvw = (n0 + xnb * 32 + lr < p.N) ? (unsigned)(((n0 + xnb * 32 + lr) * XBK + lh * 8) * 2) : BUF_OOB;
  const unsigned bvx = extra ? (WIDE ? bvw : bvo[xnb & 1]) : BUF_OOB;
  // ONE register set, refilled behind the MFMAs that consume it (conv3_wino.hip); every step issues the same 3 (NB + 1) requests
  // in code every wave runs (beyond the last chunk the last one again, never used; waves without a ninth-position block request
  // out of range)
  bf16x8 bq[NB + 1][3];
  auto load_b3 = [&](int step, int i) __attribute__((always_inline)) {
    const int st = min(step, nsteps - 1);
    const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)((st * NPOS + (i < NB ? wave : 8)) * 3) * bpl);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
      bq[i][pl] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsU, i < NB ? bvo[i < NB ? i : 0] : bvx, so + (unsigned)pl * bpl, 0));
  };

  f32x16 acc[NB], accx;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[nb][e] = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) accx[e] = 0.f;

  // prologue: halo(0), halo(1) in LDS, V(0) from halo(0); halo(2) and the U planes of step 0 in registers
#pragma unroll
  for (int i = 0; i <= NB; ++i) load_b3(0, i);
  {
    f32x4 h0[2], h1[2];
    load_halo_into(0, h0);
    load_halo_into(1, h1);
    load_halo_into(2, rh);
    store_halo_from(sH, h0);
    store_halo_from(sH + XSH, h1);
  }
  __syncthreads();
  write_v(sH, sV);
  __syncthreads();
  const int afrag = lr * XBK + ((lh ^ ((lr >> 3) & 1)) * 8);  // this lane's 8 k of tile lr inside one position of one plane
  auto multiply = [&](const u16* cV, int s) __attribute__((always_inline)) {  // step s; requests step s+1's planes as it goes
    bf16x8 a[3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) a[pl] = frag_direct(&cV[pl * XPL + wave * UTL * XBK + afrag]);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (!WIDE || nb < nlive) {  // uniform per workgroup
#pragma unroll
        for (int t = 0; t < 6; ++t) acc[nb] = mma_x3_term(t, a, bq[nb], acc[nb]);
      }
      __builtin_amdgcn_sched_barrier(0);
      load_b3(s + 1, nb);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (extra) {  // the ninth position's A planes into the set the main blocks are done with
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) a[pl] = frag_direct(&cV[pl * XPL + 8 * UTL * XBK + afrag]);
#pragma unroll
      for (int t = 0; t < 6; ++t) accx = mma_x3_term(t, a, bq[NB], accx);
    }
    __builtin_amdgcn_sched_barrier(0);
    load_b3(s + 1, NB);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto stage_next = [&](int s, int par) __attribute__((always_inline)) {
    store_halo_from(sH + par * XSH, rh);                                       // halo(s+2) (first: its registers are free during the transform)
    if (s + 1 < nsteps) write_v(sH + (par ^ 1) * XSH, sV + (par ^ 1) * XSV);  // V(s+1): nobody reads that buffer now
    load_halo_into(s + 3, rh);
  };
  // waves 0..3 (which own the V transform) stage first, waves 4..7 multiply first: two copies of the loop, so that the order of
  // the memory requests is fixed inside each and hipcc's wait counts are exact (conv3_wino.hip)
  auto step = [&](int s, int par, auto first_c) __attribute__((always_inline)) {
    const u16* cV = sV + par * XSV;
    if (decltype(first_c)::value) {
      stage_next(s, par);
      __builtin_amdgcn_sched_barrier(0);
      multiply(cV, s);
    } else {
      multiply(cV, s);
      __builtin_amdgcn_sched_barrier(0);
      stage_next(s, par);
    }
    __syncthreads();
  };
  auto run = [&](auto first_c) __attribute__((always_inline)) {
    int s = 0;
    for (; s + 1 < nsteps; s += 2) {
      step(s, 0, first_c);
      step(s + 1, 1, first_c);
    }
    if (s < nsteps) step(s, 0, first_c);
  };
#if VAE_UPW_PRIO  // one static s_setprio around the loop; a scalar condition: the instruction ignores EXEC
  if (DG && __builtin_amdgcn_readfirstlane(tid) >= 256) __builtin_amdgcn_s_setprio(1);
#endif
  if (wave < 4) run(std::true_type{});  // uniform per wave
  else run(std::false_type{});
#if VAE_UPW_PRIO
  if (DG) __builtin_amdgcn_s_setprio(0);
#endif

  // ---- epilogue: per 32-channel block, M through LDS, then the output transform ----
  // (the exact loop's text, kept apart: shared through a function, the exact build's registers moved away from the parent's)
  float* const sM = upw_lds;  // [9][32 tiles][UMLD], over the V / halo buffers (the last step's barrier has passed)
  const size_t obytes = (size_t)g.Ho * g.Wo * p.ldc * 4u;
  const auto rsC = VAE_BUF_RSRC(p.C + (int64_t)b * g.Ho * g.Wo * p.ldc, obytes);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (WIDE && nb >= nlive) break;  // uniform per workgroup
    if (nb > 0) __syncthreads();  // the previous block's reads are done
    wino::spill_acc(sM, wave, UMLD, acc[nb], lr, lh);
    if (wave == xw0 + nb) wino::spill_acc(sM, 8, UMLD, accx, lr, lh);  // the ninth position's block nb
    __syncthreads();
    {
#pragma unroll
      for (int rnd = 0; rnd < 2; ++rnd) {
        const int co = tid & 31, tile = (tid >> 5) + 16 * rnd;
        const int col = n0 + nb * 32 + co;
        float m[9];
#pragma unroll
        for (int pos = 0; pos < 9; ++pos) m[pos] = sM[(pos * UTL + tile) * UMLD + co];
        const int oy = y0 + (tile >> 3), ox = x0 + (tile & 7);  // low-resolution pixel of the tile
        if (!DG) {
          const float bv = (p.bias && col < p.N) ? p.bias[col] : 0.f;
          float h[2][3];  // A'^T M
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            h[0][j] = m[0 * 3 + j] + m[1 * 3 + j];
            h[1][j] = m[1 * 3 + j] - m[2 * 3 + j];
          }
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const float yv[2] = {h[a][0] + h[a][1], h[a][1] - h[a][2]};
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
              const int py = 2 * oy + a, px = 2 * ox + bb;
              const unsigned off = (col < p.N && py < g.Ho && px < g.Wo) ? (unsigned)(((py * g.Wo + px) * p.ldc + col) * 4) : BUF_OOB;
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv[bb] + bv), rsC, off, 0, 0);
            }
          }
        } else {
          // s^T M s with s = [1 1 -1]
          const float h0 = (m[0] + m[3]) - m[6], h1 = (m[1] + m[4]) - m[7], h2 = (m[2] + m[5]) - m[8];
          const float v = (h0 + h1) - h2;
          const unsigned off = (col < p.N && oy < g.Ho && ox < g.Wo) ? (unsigned)(((oy * g.Wo + ox) * p.ldc + col) * 4) : BUF_OOB;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsC, off, 0, 0);
        }
      }
    }
  }
}
#endif  // VAE_UPW_X3

}  // namespace

// forward (mode UP2X: source = the low-resolution x, row grid = the high-resolution output) or dgrad (mode UP2X_DGRAD: source =
// the high-resolution dY, row grid = the low-resolution input gradient) of conv3x3(nearest_upsample_2x(x)) in fp32
bool conv3_upwino_eligible(const vae_igemm_args& a) {
  const vae_conv_geom& g = a.g;
  if (!wino::conv_eligible_common(a, NPOS) || a.xf != VAE_XF_NONE) return false;
  if (a.track != nullptr || a.res != nullptr || a.gstat != nullptr || a.a_bf16 || a.res_bf16) return false;
  int Hl, Wl;  // low-resolution size
  if (g.mode == VAE_MODE_UP2X) {
    if (g.Ho != 2 * g.Hs || g.Wo != 2 * g.Ws || a.sk != 1) return false;
    Hl = g.Hs; Wl = g.Ws;
  } else if (g.mode == VAE_MODE_UP2X_DGRAD) {
    if (g.Hs != 2 * g.Ho || g.Ws != 2 * g.Wo || a.sn != 1 || a.bias != nullptr) return false;
    Hl = g.Ho; Wl = g.Wo;
  } else {
    return false;
  }
  if (Hl % UTH != 0 || Wl % UTW != 0 || a.K % 8 != 0 || a.K < 64 || a.K > 1024 || a.N < 32 || a.N % 4 != 0 || g.Cs < a.K) return false;
#if VAE_UPW_X3
  if (upw_u_bytes(a.K, a.N) >= BUF_MAX) return false;  // (N beyond 77,000: the plane image through one descriptor)
#endif
  return true;
}

// bytes of the image launch_upwino_weights writes and launch_conv3_upwino reads
int64_t conv3_upwino_weight_bytes(const vae_igemm_args& a) {
#if VAE_UPW_X3
  return (int64_t)upw_u_bytes(a.K, a.N);  // 6 * 9 * N * roundup16(K)
#else
  return (int64_t)wino::u_bytes(a.K / UBK, NPOS, a.N);
#endif
}

int launch_upwino_weights(const vae_igemm_args& a, float* U, hipStream_t st) {
#if VAE_UPW_X3
  const int64_t n = (int64_t)a.N * upw_chunks(a.K) * XBK;
  hipLaunchKernelGGL(upwino_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.W, a.N, a.K, a.g.mode == VAE_MODE_UP2X_DGRAD ? 1 : 0,
                     a.sn, a.sk, a.st, reinterpret_cast<u16*>(U));
  return 0;
#else
  return wino::launch_weights(upwino_weights_kernel, a, a.g.mode == VAE_MODE_UP2X_DGRAD, U, st);
#endif
}

int launch_conv3_upwino(const vae_igemm_args& a, const float* U, hipStream_t st) {
  const vae_conv_geom& g = a.g;
  const bool dg = g.mode == VAE_MODE_UP2X_DGRAD;
  const int Hl = dg ? g.Ho : g.Hs, Wl = dg ? g.Wo : g.Ws;
  const int tx = Wl / UTW, ty = Hl / UTH;
#if VAE_UPW_X3
  const int wbn = 32 * (dg ? upw_nb<true>() : upw_nb<false>());  // output channels per workgroup
#else
  const int wbn = 32 * UNB;
#endif
  const int tilesN = (a.N + wbn - 1) / wbn;
  const int64_t nt = (int64_t)tilesN * tx * ty * g.B;
  if (nt > 0x7fffffffLL) return VAE_EINVAL;
  constexpr size_t xcd_u = (size_t)VAE_UPW_XCD_LIMIT;
  const int xcd_sp = wino::xcd_spatial(tilesN, (size_t)conv3_upwino_weight_bytes(a), xcd_u, (int64_t)tx * ty * g.B);
#if VAE_UPW_X3  // (the dgrad's 78,336 B are more than 64 KB of dynamic LDS: reserved once per instantiation and device)
  const u16* Up = reinterpret_cast<const u16*>(U);
  if (dg) {
    VAE_RESERVE_LDS(conv3_upwino_kernel<true>, upw_lds_bytes<true>(), "conv3_upwino");
    hipLaunchKernelGGL((conv3_upwino_kernel<true>), dim3((unsigned)nt), dim3(UNT), upw_lds_bytes<true>(), st, a, Up, tx, ty, xcd_sp);
  } else {
    VAE_RESERVE_LDS(conv3_upwino_kernel<false>, upw_lds_bytes<false>(), "conv3_upwino");
    hipLaunchKernelGGL((conv3_upwino_kernel<false>), dim3((unsigned)nt), dim3(UNT), upw_lds_bytes<false>(), st, a, Up, tx, ty, xcd_sp);
  }
#else
  if (dg) hipLaunchKernelGGL((conv3_upwino_kernel<true>), dim3((unsigned)nt), dim3(UNT), 0, st, a, U, tx, ty, xcd_sp);
  else hipLaunchKernelGGL((conv3_upwino_kernel<false>), dim3((unsigned)nt), dim3(UNT), 0, st, a, U, tx, ty, xcd_sp);
#endif
  return 0;
}
