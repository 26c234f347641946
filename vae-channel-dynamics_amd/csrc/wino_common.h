// What the five fp32 Winograd files (conv3_wino.hip, conv3_wino4.hip, conv3_upwino.hip, wgrad3_wino.hip, wgrad3_upwino.hip) agree
// on, once: the workgroup id rules, the layout of the transformed-weight image U, the accumulator spill, the GroupNorm
// epilogues, the split-K slab and the eligibility preambles.  Device and host inlines only; the main loops, their staging roles
// and LDS layouts are measured to the cycle and stay in their files.
// The FORM of some helpers is load-bearing: conv3_wino4_kernel sits at 168 registers with 16 scalar spills, and hipcc's register
// allocation and wait counts there moved with rewrites that mean the same (tools/isa_counts.py on both listings).  Rejected:
// u_bytes as K * POS * N * 4 (one scalar register more in conv3_wino_kernel<0,2>); gnb_x_rsrc taking the argument block and
// testing gnb_ws itself, gnb_load_x selecting the offset before the bf16 branch (scalar spills 13-17, +1..16 waits); gstat_merge
// storing the result itself, its output address then computed in front of the loop (+16 waits); u_at as pos * (N * 8) (two scalar
// registers more in wino4_weights_kernel); the block loop of slab_store at the call site (+1..3 waits).
#pragma once
#include "common.h"
#include "launchers.h"

namespace wino {

// ---------------------------------------------------------------------------------------
// A. the three convolution kernels
// ---------------------------------------------------------------------------------------

// Workgroup id -> (channel block tn, spatial tile tx, ty, image b).  Consecutive ids go round-robin over the 8 XCDs (one L2
// each).  With tn fastest an XCD sees one channel block's slice of U (what fits its L2) but every XCD pulls the whole input:
// Cout/64-fold L2 fills.  When the whole U image is small (xcd_sp, decided by xcd_spatial below: 128 and 256 channels) the
// channel blocks of a spatial tile get ids congruent mod 8 instead, so one L2 fetches that tile's halo once.  Measured on
// conv3_wino_kernel (rocprofv3 FETCH_SIZE/WRITE_SIZE, bytes per launch averaged over the step's 96 launches): tn fastest
// everywhere 1351 MB, this rule 1142 MB, spatial-major everywhere (512 channels too: the U slices then cycle through L2)
// 1207 MB; same speed in all three.
struct TileId {
  int tn, tx, ty, b;
};
__device__ __forceinline__ TileId tile_of_workgroup(int t, int tilesN, int tiles_x, int tiles_y, int xcd_sp) {
  TileId r;
  if (xcd_sp) {
    r.tn = (t >> 3) % tilesN;
    t = ((t >> 3) / tilesN) * 8 + (t & 7);
  } else {
    r.tn = t % tilesN;
    t /= tilesN;
  }
  r.tx = t % tiles_x; t /= tiles_x;
  r.ty = t % tiles_y;
  r.b = t / tiles_y;
  return r;
}
// host: U images up to `limit` bytes (a per-kernel constant: the lowest measured traffic) put the channel blocks of a tile on
// one XCD
inline int xcd_spatial(int tilesN, size_t u_bytes, size_t limit, int64_t spatial_tiles) {
  return (tilesN > 1 && u_bytes <= limit && spatial_tiles % 8 == 0) ? 1 : 0;
}

// The transformed-weight image U: [K/8][POS][N][8] floats (POS = 16, 36 or 9 positions of the transform domain), so the B
// fragment of (channel chunk, position, 32-channel block) is 16 contiguous bytes per lane, 1 KB per wave.
// bytes per position of a chunk, and of the image of `chunks` = K / 8 chunks
__host__ __device__ __forceinline__ unsigned u_pos_bytes(int N) { return (unsigned)N * 32u; }
__host__ __device__ __forceinline__ size_t u_bytes(int chunks, int POS, int N) { return (size_t)chunks * POS * u_pos_bytes(N); }
// the 3x3 kernel of (n, k): g = W[n][.][.][k] (forward, N = Cout, K = Cin) or rot180(W[k][.][.][n]) (dgrad, N = Cin, K = Cout:
// the caller's strides sn, sk are already swapped)
__device__ __forceinline__ void u_gather(const float* __restrict__ W, int n, int k, int dgrad, int64_t sn, int64_t sk, int64_t st, float (&g)[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int tap = dgrad ? (2 - a) * 3 + (2 - b) : a * 3 + b;
      g[a][b] = W[(int64_t)n * sn + (int64_t)k * sk + (int64_t)tap * st];
    }
}
// where (n, k) of position 0 lives (o), and of position pos
template <int POS>
__device__ __forceinline__ float* u_out(float* __restrict__ U, int N, int n, int k) {
  return U + ((int64_t)(k >> 3) * POS * N + n) * 8 + (k & 7);
}
__device__ __forceinline__ float& u_at(float* o, int N, int pos) { return o[(int64_t)pos * N * 8]; }
// per-lane byte offset of the fragment of channel n (k quad lh of the chunk) inside one position
__device__ __forceinline__ unsigned u_frag(int n, int lh) { return (unsigned)((n * 8 + lh * 4) * 4); }
// host: one launch shape for the three weight-transform kernels (256 threads, one (n, k) pair each)
template <typename Kernel>
inline int launch_weights(Kernel kernel, const vae_igemm_args& a, bool dgrad, float* U, hipStream_t st) {
  const int64_t n = (int64_t)a.N * a.K;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.W, a.N, a.K, dgrad ? 1 : 0, a.sn, a.sk, a.st, U);
  return 0;
}

constexpr int TILES = 32;  // Winograd tiles per workgroup of all three kernels (the M side of one 32x32 MFMA)
// Accumulator -> LDS: the 32x32 MFMA result of position pos (lane (lr, lh), element e = tile (e & 3) + 8 (e >> 2) + 4 lh,
// channel lr) into the epilogue image [POS][32 tiles][LD]
__device__ __forceinline__ void spill_acc(float* sM, int pos, int LD, const f32x16& acc, int lr, int lh) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int tile = (e & 3) + 8 * (e >> 2) + 4 * lh;
    sM[(pos * TILES + tile) * LD + lr] = acc[e];
  }
}

// chunk (= workgroup tile) of image b in the `gstat` / `gnb_ws` workspaces
__device__ __forceinline__ int64_t chunk_of_tile(int b, int tiles_x, int tiles_y, int ty, int tx) {
  return (int64_t)b * (tiles_x * tiles_y) + ty * tiles_x + tx;
}

// ---- GroupNorm-backward epilogue (dgrad launches, vaehip.h gnb_*): the first pass of the GroupNorm backward over the gradient
// the kernel has just computed.  x is the GroupNorm input at the thread's output positions, stored fp32 or bf16 ----
// descriptor of `pixels` pixels (ldc channels each) of x from pixel `pixel0` on
__device__ __forceinline__ auto gnb_x_rsrc(const void* x, bool bf16, int64_t pixel0, int64_t pixels, int ldc) {
  const unsigned xes = bf16 ? 2u : 4u;
  return VAE_BUF_RSRC(reinterpret_cast<const char*>(x) + pixel0 * ldc * xes, (size_t)pixels * ldc * xes);
}
// voff + soff: the byte offset of the OUTPUT element (fp32); OOB: voff may be BUF_OOB (partial channel blocks)
template <bool OOB, typename Rsrc>
__device__ __forceinline__ float gnb_load_x(Rsrc rsX, bool bf16, unsigned voff, unsigned soff) {
  if (bf16) {
    const unsigned vh = (OOB && voff == BUF_OOB) ? BUF_OOB : voff >> 1;
    return __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsX, vh, soff >> 1, 0) << 16);
  }
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsX, voff, soff, 0));
}
struct GnbCoef {
  float mu = 0.f, rs = 0.f, ga = 0.f, be = 0.f;
};
__device__ __forceinline__ GnbCoef gnb_coef(const vae_igemm_args& p, int b, int col) {
  const int grp = col / (p.N / p.gnb_groups);
  return GnbCoef{p.gnb_mean[b * p.gnb_groups + grp], p.gnb_rstd[b * p.gnb_groups + grp], p.gnb_gamma[col], p.gnb_beta[col]};
}
// one element: the same arithmetic per element as gn_bwd_partial_kernel (norm.hip); bs1 = sum dz, bs2 = sum dz * xhat
__device__ __forceinline__ void gnb_accumulate(const GnbCoef& c, int silu, float x, float v, float& bs1, float& bs2) {
  const float xh = (x - c.mu) * c.rs;
  float du = v;
  if (silu) du *= silu_grad_f(xh * c.ga + c.be);
  bs1 += du;
  bs2 += du * xh;
}
// redb: [SLOTS][32 channels][2]; slot = tid >> 5 of the thread, channel = tid & 31
__device__ __forceinline__ void gnb_slot_store(float* redb, int tid, float bs1, float bs2) {
  redb[((tid >> 5) * 32 + (tid & 31)) * 2] = bs1;
  redb[((tid >> 5) * 32 + (tid & 31)) * 2 + 1] = bs2;
}
// the SLOTS partial sums of channel c of the block, fixed order -> o[0..1] (the channel's entry of the chunk in gnb_ws)
template <int SLOTS>
__device__ __forceinline__ void gnb_reduce(const float* redb, int c, float* o) {
  float a1 = redb[c * 2], a2 = redb[c * 2 + 1];
#pragma unroll
  for (int w = 1; w < SLOTS; ++w) {
    a1 += redb[(w * 32 + c) * 2];
    a2 += redb[(w * 32 + c) * 2 + 1];
  }
  o[0] = a1;
  o[1] = a2;
}

// ---- GroupNorm moment epilogue: centred moments of the block's groups (cpg channels each, ng = 32 / cpg groups).  A lane
// arrives with the shifted sums of its nlane outputs of one channel (how s2 is accumulated is each kernel's own choice); the
// wave's groups go to red [WAVES][ng][2], then thread grp merges the waves in fixed order (wave w holds nw(w) outputs per group:
// whole numbers far below 2^24, so the running count is exact) ----
__device__ __forceinline__ void gstat_wave_store(float* red, int wave, int cpg, int lr, int lh, float pv, float s1, float s2, float nlane) {
  const int ng = 32 / cpg;
  const MeanM2 a = mm2_wave_group(mm2_from_shifted(pv, s1, s2, nlane), cpg, nlane);
  if (lh == 0 && (lr & (cpg - 1)) == 0) {
    red[(wave * ng + lr / cpg) * 2] = a.m;
    red[(wave * ng + lr / cpg) * 2 + 1] = a.M2;
  }
}
template <int WAVES, typename Count>
__device__ __forceinline__ MeanM2 gstat_merge(const float* red, int ng, int grp, Count nw) {
  MeanM2 a{red[grp * 2], red[grp * 2 + 1]};
  float na = nw(0);
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    const float n = nw(w);
    a = mm2_merge(a, na, MeanM2{red[(w * ng + grp) * 2], red[(w * ng + grp) * 2 + 1]}, n);
    na += n;
  }
  return a;
}

// ---------------------------------------------------------------------------------------
// B. the two weight-gradient kernels: 32 ci x 128 co per workgroup, split-K over unit ranges, slab [split][POS][Cin][Cout]
// ---------------------------------------------------------------------------------------

// Workgroup id -> (tile, split).  Hardware deals consecutive ids round-robin over the 8 XCDs (one L2 each); the tiles of one
// split walk through the SAME pixels (every ci block re-reads the dY strip, every co block the X halo), so they are given
// ids congruent mod 8: one L2 (or, SMALL_SPLITS: with 2 or 4 splits, 8 / nsplit of them) fetches a split's rows once.
struct SplitTile {
  int tile, split;
};
template <bool SMALL_SPLITS>
__device__ __forceinline__ SplitTile split_tile_of_workgroup(int L, int ns, int ntile) {
  SplitTile r;
  if (ns % 8 == 0) {
    const int j = L >> 3;
    r.tile = j % ntile;
    r.split = (j / ntile) * 8 + (L & 7);
  } else if (SMALL_SPLITS && (ns == 2 || ns == 4) && ntile % (8 / ns) == 0) {
    r.split = (L & 7) % ns;
    r.tile = (L >> 3) * (8 / ns) + (L & 7) / ns;
  } else {
    r.tile = L % ntile;
    r.split = L / ntile;
  }
  return r;
}
// the split's units [ubeg, ubeg + nu) of nunits (a split beyond the range has nu = 0 and writes its zero slab)
struct UnitRange {
  int64_t ubeg;
  int nu;
};
__device__ __forceinline__ UnitRange unit_range(int64_t nunits, int nsplit, int split) {
  const int64_t per = (nunits + nsplit - 1) / nsplit;
  const int64_t ubeg = split * per, uend = min(nunits, ubeg + per);
  return UnitRange{ubeg, (int)max((int64_t)0, uend - ubeg)};
}
// the 32 ci x 32 co accumulators of position pos, co blocks nb0 .. nb0 + NB - 1 of the tile, into the split's slab O; lanes along
// co (128-byte rows).  (The block loop lives here: around a call hipcc orders the stores differently and adds a wait.)
template <int NB>
__device__ __forceinline__ void slab_store(float* __restrict__ O, int pos, int N, int M, int n0, int m0, int nb0, const f32x16* acc, int lr, int lh) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int ci = n0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      O[((int64_t)pos * N + ci) * M + m0 + (nb0 + nb) * 32 + lr] = acc[nb][e];
    }
}
// bias gradient: the thread's sums of its channel quad -> over the 16 columns of the strip (lanes xx = 0..15) -> o[at .. at + 3]
__device__ __forceinline__ void bias_tail(const f32x4& bsum, int xx, float* o, int64_t at) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float s = bsum[e];
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) s += __shfl_xor(s, d, 64);
    if (xx == 0) o[at + e] = s;
  }
}

// ---------------------------------------------------------------------------------------
// C. host: what every kernel of the family asks of its arguments (each file adds its own conditions)
// ---------------------------------------------------------------------------------------
inline bool conv_eligible_common(const vae_igemm_args& a, int POS) {
  const vae_conv_geom& g = a.g;
  if (a.prec != VAE_PREC_F32 || a.A16 != nullptr || a.batch != 1 || a.alpha != 1.0f) return false;
  if (g.taps != 9 || g.stride != 1 || g.pad_t != 1 || g.pad_l != 1) return false;
  if (a.tapmask != 0 || a.a_step > 1 || a.c_step > 1 || a.out_bf16) return false;
  if (!aligned16(a.A) || !aligned16(a.C)) return false;
  if ((size_t)g.Hs * g.Ws * g.Cs * 4u >= BUF_MAX || (size_t)g.Ho * g.Wo * a.ldc * 4u >= BUF_MAX) return false;
  return a.K % 8 == 0 && u_bytes(a.K / 8, POS, a.N) < BUF_MAX;
}
inline bool wgrad_eligible_common(const vae_wgrad_args& a, int ci_tile, int co_tile) {
  const vae_conv_geom& g = a.g;
  if (a.prec != VAE_PREC_F32 || a.X16 != nullptr || a.dY16 != nullptr || a.dY == nullptr || a.batch != 1 || a.alpha != 1.0f) return false;
  if (g.taps != 9 || g.stride != 1 || g.pad_t != 1 || g.pad_l != 1 || a.tapmask != 0 || a.y_step > 1) return false;
  if (a.N % ci_tile != 0 || a.M % co_tile != 0 || g.Cs % 4 != 0 || a.ldy % 4 != 0) return false;
  if (!aligned16(a.X) || !aligned16(a.dY)) return false;
  return (size_t)g.B * g.Hs * g.Ws * g.Cs * 4u < BUF_MAX && (size_t)g.B * g.Ho * g.Wo * a.ldy * 4u < BUF_MAX;
}
// chunks per image of the statistics epilogue of a kernel with th x tw-pixel tiles (0 = not available for these arguments)
inline int gstat_chunks(const vae_igemm_args& a, int th, int tw) {
  const vae_conv_geom& g = a.g;
  if (a.gstat_groups <= 0 || a.N % a.gstat_groups != 0 || g.mode == VAE_MODE_DGRAD) return 0;
  const int cpg = a.N / a.gstat_groups;
  if (cpg != 4 && cpg != 8 && cpg != 16) return 0;
  return (g.Wo / tw) * (g.Ho / th);
}
// chunks per image of the GroupNorm-backward epilogue (0 = not available for these arguments): full tiles of a dgrad launch
// whose output has the GroupNorm input's shape
inline int gnb_chunks(const vae_igemm_args& a, int th, int tw) {
  const vae_conv_geom& g = a.g;
  if (g.mode != VAE_MODE_DGRAD || a.gnb_x == nullptr || a.gnb_groups <= 0 || a.N % a.gnb_groups != 0 || a.ldc != a.N) return 0;
  if (a.res != nullptr || a.bias != nullptr || a.out_bf16) return 0;
  if ((size_t)g.Ho * g.Wo * a.ldc * 4u >= BUF_MAX) return 0;
  return (g.Wo / tw) * (g.Ho / th);
}

}  // namespace wino
