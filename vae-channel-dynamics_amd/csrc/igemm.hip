// Implicit-GEMM convolution / GEMM family on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate).
//
// Three operand forms cover every contraction of the SDXL-VAE train step:
//   rows   (A rows = pixels gathered through the conv geometry)
//     - weight tile k-contiguous : conv/linear forward, Q.K^T, dO.V^T
//     - weight tile n-contiguous : conv/linear dgrad, P.V, dS.K
//   wgrad  (contraction over pixels; both tiles k-major) : conv/linear wgrad, P^T.dO, dS^T.Q
//
// Tiling: 64*WM*WN threads (8 waves for the 128x128 tile, 4 for the skinny ones), BK = 32, wave tile =
// (BM/WM) x (BN/WN) built from 32x32 MFMA tiles.  LDS tiles are padded so every ds_read_b128 fragment read is
// bank-conflict free (row stride 36 dwords: 36*i mod 64 hits 16 distinct 16-B slots
// for the 16 rows of a b128 lane group).  Global loads of step s+1 are issued before
// the MFMA block of step s and written to LDS after it (register-staged prefetch);
// GroupNorm+SiLU is applied to the A operand in that write pass, so the normalised
// activation never exists in HBM.
#include "common.h"
#include <algorithm>
#include <stdlib.h>

#include "launchers.h"

namespace {

constexpr int BK = 32;
__device__ __forceinline__ int b_lo_of(int m0, int hw) { return m0 / hw; }

// ---------------------------------------------------------------------------------------
// rows kernel.  Pipeline: LDS is double buffered; the global loads of K-step s+2 are issued and
// the registers of step s+1 are transformed + written to the other LDS stage in the MIDDLE of
// step s's MFMA block, so one workgroup barrier per K-step suffices and the VALU/LDS-write work
// sits in the shadow of MFMAs already issued.  The GroupNorm scale/shift rows the tile needs are
// staged in LDS once per workgroup (they used to be 8 dependent global loads per thread per step).
// ---------------------------------------------------------------------------------------

template <int BM, int BN, int WM, int WN, bool BKM, bool VEC, int XF>
__global__ __launch_bounds__(64 * WM * WN) void igemm_rows_kernel(vae_igemm_args p) {
  constexpr int NT = 64 * WM * WN;  // 4 waves (skinny tiles) or 8 waves (128x128: 4 waves/SIMD at 2 workgroups/CU)
  constexpr int NL = NT;
  constexpr int RP = NT / 8;        // tile rows covered by one pass of the float4 loaders
  constexpr int LDA = BK + 4;
  constexpr int LDB = BKM ? (BN + 4) : (BK + 4);
  constexpr int SA = BM * LDA;
  constexpr int SB = BKM ? BK * LDB : BN * LDB;
  constexpr int STAGE = SA + SB;
  constexpr int SS = (XF != VAE_XF_NONE) ? 2 * SS_HALF : 0;
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NI = TN / 32;
  constexpr int AR = BM / RP;                       // A rows per thread
  constexpr int BR = BKM ? (BK / (NL / (BN / 4))) : (BN / RP);
  static_assert(AR >= 1 && BR >= 1 && TM % 32 == 0 && TN % 32 == 0, "tile/wave layout");
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE + SS];
  float* sS = smem + 2 * STAGE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lt = tid;
  const int wm = wave / WN, wn = wave % WN;
  const int tilesN = (p.N + BN - 1) / BN;
  const int tm = blockIdx.x / tilesN, tn = blockIdx.x % tilesN;
  const int m0 = tm * BM, n0 = tn * BN;
  const int z = blockIdx.z;
  const vae_conv_geom g = p.g;
  const SrcMap smap = make_srcmap(g);
  const float* __restrict__ A = p.A + (int64_t)z * p.sAb;
  const float* __restrict__ W = p.W + (int64_t)z * p.sWb;
  const int hw = g.Ho * g.Wo;

  // stride-2 dgrad, parity-class-major rows: the tile's class fixes the taps it meets
  const bool s2c = (g.mode == VAE_MODE_DGRAD_S2);
  const int hh = g.Ho >> 1, wh = g.Wo >> 1;
  const int cls_rows = s2c ? p.M >> 2 : 1;
  const int cls = s2c ? m0 / cls_rows : 0;
  const int cpy = cls >> 1, cpx = cls & 1;
  const int nkw = s2c ? (cpx ? 1 : 2) : 3;
  const int ntaps = s2c ? (cpy ? 1 : 2) * nkw : g.taps;
  auto row_pixel = [&](int m, int& b, int& y, int& x) {  // GEMM row -> (image, y, x) of the row grid
    if (s2c) {
      const int r = m - cls * cls_rows;
      b = r / (hh * wh);
      const int rem = r - b * (hh * wh);
      const int i = rem / wh;
      y = 2 * i + cpy;
      x = 2 * (rem - i * wh) + cpx;
    } else {
      b = m / hw;
      const int rem = m - b * hw;
      y = rem / g.Wo;
      x = rem - y * g.Wo;
    }
  };

  // vectorised instantiations read both operands through buffer descriptors (common.h): out-of-range offsets read
  // zeros, so no select sits on a loaded value.  The activation descriptor starts at the first image this tile's
  // rows touch (the host checked that the images one tile can span fit 32-bit offsets).
  const int b_base = s2c ? (m0 - cls * cls_rows) / (hh * wh) : b_lo_of(m0, hw);
  const size_t img = (size_t)g.Hs * g.Ws * g.Cs;
  const size_t abytes = (size_t)(g.B - b_base) * img * 4u, wbytes = (size_t)(BKM ? (int64_t)p.K * p.sk : (int64_t)p.N * p.sn) * 4u;
  const auto rsA = VAE_BUF_RSRC(A + (int64_t)b_base * img, abytes < BUF_MAX ? abytes : BUF_MAX);
  const auto rsW = VAE_BUF_RSRC(W, wbytes < BUF_MAX ? wbytes : BUF_MAX);

  // per-thread A rows
  const int k4 = lt & 7, r0 = lt >> 3;
  int rb[AR], ry[AR], rx[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    int m = m0 + r0 + RP * i;
    if (m < p.M) {
      row_pixel(m, rb[i], ry[i], rx[i]);
    } else {
      rb[i] = -1; ry[i] = 0; rx[i] = 0;
    }
  }

  // scale/shift table for the batches this tile touches
  // (the host checks with vae_xf_fusable_rows that the rows of one tile never need more than SS_HALF entries)
  const int b_lo = m0 / hw;
  if (XF != VAE_XF_NONE) {
    const int b_hi = (min(p.M, m0 + BM) - 1) / hw;
    const int nent = min((b_hi - b_lo + 1) * p.K, SS_HALF);
    for (int i = tid; i < nent; i += NT) {
      const int j = i / p.K, c = i - j * p.K;
      sS[i] = p.scale[(int64_t)(b_lo + j) * g.Cs + c];
      sS[SS_HALF + i] = p.shift[(int64_t)(b_lo + j) * g.Cs + c];
    }
  }

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int kchunks = (p.K + BK - 1) / BK;
  const int steps = ntaps * kchunks;

  f32x4 ra[AR], rbw[BR];
  int a_b[AR];  // batch index of the loaded row (for scale/shift), -1 = padding
  int reg_c0 = 0;

  auto load_regs = [&](int s) {
    const int ord = s / kchunks;  // ordinal of the tap among the taps this tile meets
    const int c0 = (s - ord * kchunks) * BK;
    reg_c0 = c0;
    int kh, kw;
    if (s2c) {
      const int a = ord / nkw;
      kh = cpy ? 1 : 2 * a;
      kw = cpx ? 1 : 2 * (ord - a * nkw);
    } else {
      kh = (g.taps == 9) ? ord / 3 : 0;
      kw = (g.taps == 9) ? ord - kh * 3 : 0;
    }
    const int tap = kh * 3 + kw;
    const int c = c0 + k4 * 4;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int sy = 0, sx = 0;
      const bool ok = src_pixel(smap, ry[i], rx[i], kh, kw, sy, sx) && (rb[i] >= 0);
      if (VEC) {
        ra[i] = VAE_BUF_LOAD4(rsA, oob_unless(ok && c < p.K, ((unsigned)(((rb[i] - b_base) * g.Hs + sy) * g.Ws + sx) * (unsigned)g.Cs + (unsigned)c) * 4u));
      } else {
        ra[i] = load4s(A + (((int64_t)rb[i] * g.Hs + sy) * g.Ws + sx) * g.Cs + c, ok, c, p.K);
      }
      a_b[i] = ok ? rb[i] : -1;
    }
    if (!BKM) {
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        const int n = n0 + r0 + RP * i;
        if (VEC) rbw[i] = VAE_BUF_LOAD4(rsW, oob_unless(n < p.N && c < p.K, ((unsigned)n * (unsigned)p.sn + (unsigned)tap * (unsigned)p.st + (unsigned)c) * 4u));
        else rbw[i] = load4s(W + (int64_t)n * p.sn + (int64_t)tap * p.st + c, n < p.N, c, p.K);
      }
    } else {
      constexpr int NQ = BN / 4, KR = NL / NQ;
      const int n4 = lt % NQ, kq = lt / NQ;
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        const int k = c0 + kq + KR * i;
        const int n = n0 + n4 * 4;
        if (VEC) rbw[i] = VAE_BUF_LOAD4(rsW, oob_unless(k < p.K && n < p.N, ((unsigned)k * (unsigned)p.sk + (unsigned)tap * (unsigned)p.st + (unsigned)n) * 4u));
        else rbw[i] = load4s(W + (int64_t)k * p.sk + (int64_t)tap * p.st + n, k < p.K, n, p.N);
      }
    }
  };

  auto store_lds = [&](float* sA, float* sB) {
    const int c = reg_c0 + k4 * 4;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      f32x4 v = ra[i];
      if (XF != VAE_XF_NONE) {
        const bool ok = (a_b[i] >= 0) && (c < p.K);
        const int o = ok ? (a_b[i] - b_lo) * p.K + c : 0;
        v = xform4_tab<XF>(v, sS + o, sS + SS_HALF + o, ok);
      }
      *reinterpret_cast<f32x4*>(&sA[(r0 + RP * i) * LDA + k4 * 4]) = v;
    }
    if (!BKM) {
#pragma unroll
      for (int i = 0; i < BR; ++i) *reinterpret_cast<f32x4*>(&sB[(r0 + RP * i) * LDB + k4 * 4]) = rbw[i];
    } else {
      constexpr int NQ = BN / 4, KR = NL / NQ;
      const int n4 = lt % NQ, kq = lt / NQ;
#pragma unroll
      for (int i = 0; i < BR; ++i) *reinterpret_cast<f32x4*>(&sB[(kq + KR * i) * LDB + n4 * 4]) = rbw[i];
    }
  };

  const int lr = lane & 31, lh = lane >> 5;
  // fragments of k-group kk+1 are requested before the MFMAs of kk are issued (pinned with sched_barrier)
  f32x4 fa[2][MI], fb[2][NI];
  auto fetch = [&](const float* sA, const float* sB, int kk, f32x4* a, f32x4* b) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      a[mi] = *reinterpret_cast<const f32x4*>(&sA[(wm * TM + mi * 32 + lr) * LDA + kk * 8 + lh * 4]);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      if (!BKM) {
        b[ni] = *reinterpret_cast<const f32x4*>(&sB[(wn * TN + ni * 32 + lr) * LDB + kk * 8 + lh * 4]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) b[ni][j] = sB[(kk * 8 + lh * 4 + j) * LDB + wn * TN + ni * 32 + lr];
      }
    }
  };
  auto compute = [&](const float* sA, const float* sB, int kk) {  // fragments of kk already requested
    if (kk + 1 < BK / 8) fetch(sA, sB, kk + 1, fa[(kk + 1) & 1], fb[(kk + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk & 1][mi][j], fb[kk & 1][ni][j], acc[mi][ni], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };

  load_regs(0);
  __syncthreads();  // scale/shift table visible
  store_lds(smem, smem + SA);
  if (steps > 1) load_regs(1);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const float* cA = smem + (s & 1) * STAGE;
    const float* cB = cA + SA;
    fetch(cA, cB, 0, fa[0], fb[0]);
    compute(cA, cB, 0);
    compute(cA, cB, 1);
    if (s + 1 < steps) {  // staged in the shadow of the MFMAs already issued
      float* nA = smem + ((s + 1) & 1) * STAGE;
      store_lds(nA, nA + SA);
      if (s + 2 < steps) load_regs(s + 2);
    }
    compute(cA, cB, 2);
    compute(cA, cB, 3);
    __syncthreads();
  }

  // ---------------- epilogue ----------------
  // outputs and the residual through buffer descriptors (common.h): a row / column outside the matrix is an
  // out-of-range offset (load reads 0, store is dropped): no branch per element, residual loads issued back to back
  float* __restrict__ C = p.C + (int64_t)z * p.sCb;
  const size_t obytes = (size_t)p.M * p.ldc * 4u;
  const auto rsC = VAE_BUF_RSRC(C, obytes);
  const auto rsR = VAE_BUF_RSRC(p.res ? p.res + (int64_t)z * p.sCb : C, obytes);
  float tsum[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) tsum[ni] = 0.f;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int col = n0 + wn * TN + ni * 32 + lr;
    const bool colok = col < p.N;
    const float bv = (p.bias && colok) ? p.bias[col] : 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned off[16];
      float rv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * TM + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        unsigned orow = (unsigned)row;
        if (s2c) {  // class-major row -> pixel-major output row
          int b, y, x;
          row_pixel(row < p.M ? row : m0, b, y, x);
          orow = (unsigned)((b * g.Ho + y) * g.Wo + x);
        }
        off[r] = (colok && row < p.M) ? (orow * (unsigned)p.ldc + (unsigned)col) * 4u : BUF_OOB;
        rv[r] = 0.f;
      }
      if (p.res) {  // uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsR, off[r], 0, 0));
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = p.alpha * acc[mi][ni][r] + bv + rv[r];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsC, off[r], 0, 0);
        tsum[ni] += (off[r] != BUF_OOB) ? fabsf(v) : 0.f;
      }
    }
  }
  if (p.track && z == 0) {
    float* red = smem;  // [WM][BN]; the last loop barrier already separated it from the MFMA reads
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float s2 = tsum[ni] + __shfl_xor(tsum[ni], 32, 64);
      if (lh == 0) red[wm * BN + wn * TN + ni * 32 + lr] = s2;
    }
    __syncthreads();
    if (tid < BN) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WM; ++w) t += red[w * BN + tid];
      if (n0 + tid < p.N) p.track[(int64_t)tm * p.N + n0 + tid] = t;
    }
  }
}

// ---------------------------------------------------------------------------------------
// wgrad kernel: out[m][tap][n] = sum_pix dY[pix][m] * XF(X[src(pix,tap)][n])
// Same double-buffered one-barrier pipeline.  The bias gradient (column sums of dY) is folded in:
// workgroups with tn == 0 and tap == 0 add up the dY tiles they stage anyway.
// ---------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, bool VEC, int XF>
__global__ __launch_bounds__(64 * WM * WN) void wgrad_kernel(vae_wgrad_args p) {
  constexpr int NT = 64 * WM * WN;
  constexpr int NL = NT;
  constexpr int LDA = BM + 4, LDB = BN + 4;
  constexpr int SA = BK * LDA, SB = BK * LDB;
  constexpr int STAGE = SA + SB;
  constexpr int SS = (XF != VAE_XF_NONE) ? 2 * SS_HALF : 0;
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NI = TN / 32;
  constexpr int AQ = BM / 4, AKR = NL / AQ, AI = BK / AKR;  // dY tile: AQ float4 per row
  constexpr int BQ = BN / 4, BKR = NL / BQ, BI = BK / BKR;
  static_assert(AI >= 1 && BI >= 1 && TM % 32 == 0 && TN % 32 == 0, "tile/wave layout");
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE + SS];
  float* sS = smem + 2 * STAGE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lt = tid;
  const int wm = wave / WN, wn = wave % WN;
  const int tilesN = (p.N + BN - 1) / BN;
  const int tm = blockIdx.x / tilesN, tn = blockIdx.x % tilesN;
  const int m0 = tm * BM, n0 = tn * BN;
  const int tap = blockIdx.y / p.nsplit, split = blockIdx.y % p.nsplit;
  const int z = blockIdx.z;
  const vae_conv_geom g = p.g;
  const SrcMap smap = make_srcmap(g);
  const int kh = (g.taps == 9) ? tap / 3 : 0, kw = (g.taps == 9) ? tap - kh * 3 : 0;
  const float* __restrict__ dY = p.dY + (int64_t)z * p.sYb;
  const float* __restrict__ X = p.X + (int64_t)z * p.sXb;

  int chunk = (p.npix + p.nsplit - 1) / p.nsplit;
  chunk = ((chunk + BK - 1) / BK) * BK;
  const int pbeg = split * chunk;
  const int pend = min(p.npix, pbeg + chunk);
  const int steps = (pend > pbeg) ? (pend - pbeg + BK - 1) / BK : 0;
  const int hw = g.Ho * g.Wo;
  const bool do_bias = (p.bias_partial != nullptr) && tn == 0 && tap == 0 && z == 0;

  // (the host checks with vae_xf_fusable_wgrad that one split never spans more than SS_HALF/BN batch items)
  const int b_lo = pbeg / hw;
  if (XF != VAE_XF_NONE && steps > 0) {
    const int nb = (pend - 1) / hw - b_lo + 1;
    const int ncol = min(BN, p.N - n0);
    const int nent = min(nb * BN, SS_HALF);
    for (int i = tid; i < nent; i += NT) {
      const int j = i / BN, c = i - j * BN;
      const bool ok = c < ncol;
      sS[i] = ok ? p.scale[(int64_t)(b_lo + j) * g.Cs + n0 + c] : 0.f;
      sS[SS_HALF + i] = ok ? p.shift[(int64_t)(b_lo + j) * g.Cs + n0 + c] : 0.f;
    }
  }

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  // buffer descriptors (vectorised instantiations): dY from this split's first pixel, X from its first image
  const size_t img = (size_t)g.Hs * g.Ws * g.Cs;
  const size_t ybytes = (size_t)(steps > 0 ? pend - pbeg : 0) * p.ldy * 4u, xbytes = (size_t)(g.B - b_lo) * img * 4u;
  const auto rsY = VAE_BUF_RSRC(dY + (int64_t)pbeg * p.ldy, ybytes < BUF_MAX ? ybytes : BUF_MAX);
  const auto rsX = VAE_BUF_RSRC(X + (int64_t)b_lo * img, xbytes < BUF_MAX ? xbytes : BUF_MAX);

  const int a4 = lt % AQ, akq = lt / AQ;
  const int b4 = lt % BQ, bkq = lt / BQ;
  f32x4 ra[AI], rx[BI];
  int xb[BI];
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};

  auto load_regs = [&](int s) {
    const int pb = pbeg + s * BK;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int pix = pb + akq + AKR * i;
      const int c = m0 + a4 * 4;
      if (VEC) ra[i] = VAE_BUF_LOAD4(rsY, oob_unless(pix < pend && c < p.M, ((unsigned)(pix - pbeg) * (unsigned)p.ldy + (unsigned)c) * 4u));
      else ra[i] = load4s(dY + (int64_t)pix * p.ldy + c, pix < pend, c, p.M);
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const int pix = pb + bkq + BKR * i;
      const int c = n0 + b4 * 4;
      const int b = pix / hw, rem = pix - b * hw;
      const int y = rem / g.Wo, x = rem - y * g.Wo;
      int sy = 0, sx = 0;
      const bool ok = src_pixel(smap, y, x, kh, kw, sy, sx) && (pix < pend);
      if (VEC) rx[i] = VAE_BUF_LOAD4(rsX, oob_unless(ok && c < p.N, ((unsigned)(((b - b_lo) * g.Hs + sy) * g.Ws + sx) * (unsigned)g.Cs + (unsigned)c) * 4u));
      else rx[i] = load4s(X + (((int64_t)b * g.Hs + sy) * g.Ws + sx) * g.Cs + c, ok, c, p.N);
      xb[i] = ok ? b : -1;
    }
  };
  auto store_lds = [&](float* sA, float* sB) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      *reinterpret_cast<f32x4*>(&sA[(akq + AKR * i) * LDA + a4 * 4]) = ra[i];
      if (do_bias) bsum += ra[i];
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      f32x4 v = rx[i];
      if (XF != VAE_XF_NONE) {
        const bool ok = xb[i] >= 0;
        const int o = ok ? (xb[i] - b_lo) * BN + b4 * 4 : 0;
        v = xform4_tab<XF>(v, sS + o, sS + SS_HALF + o, ok);
      }
      *reinterpret_cast<f32x4*>(&sB[(bkq + BKR * i) * LDB + b4 * 4]) = v;
    }
  };

  const int lr = lane & 31, lh = lane >> 5;
  f32x4 fa[2][MI], fb[2][NI];
  auto fetch = [&](const float* sA, const float* sB, int kk, f32x4* a, f32x4* b) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kk * 8 + lh * 4 + j;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi][j] = sA[k * LDA + wm * TM + mi * 32 + lr];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b[ni][j] = sB[k * LDB + wn * TN + ni * 32 + lr];
    }
  };
  auto compute = [&](const float* sA, const float* sB, int kk) {  // fragments of kk already requested
    if (kk + 1 < BK / 8) fetch(sA, sB, kk + 1, fa[(kk + 1) & 1], fb[(kk + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk & 1][mi][j], fb[kk & 1][ni][j], acc[mi][ni], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };

  if (steps > 0) {
    load_regs(0);
    __syncthreads();  // scale/shift table visible
    store_lds(smem, smem + SA);
    if (steps > 1) load_regs(1);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
      const float* cA = smem + (s & 1) * STAGE;
      const float* cB = cA + SA;
      fetch(cA, cB, 0, fa[0], fb[0]);
      compute(cA, cB, 0);
      compute(cA, cB, 1);
      if (s + 1 < steps) {
        float* nA = smem + ((s + 1) & 1) * STAGE;
        store_lds(nA, nA + SA);
        if (s + 2 < steps) load_regs(s + 2);
      }
      compute(cA, cB, 2);
      compute(cA, cB, 3);
      __syncthreads();
    }
  }

  const int64_t ld = (int64_t)g.taps * p.N;
  float* __restrict__ O = (p.nsplit == 1 ? p.out : p.partial + (int64_t)split * p.M * ld) + (int64_t)z * p.sOb;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int col = n0 + wn * TN + ni * 32 + lr;
    if (col >= p.N) continue;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * TM + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < p.M) O[(int64_t)row * ld + (int64_t)tap * p.N + col] = p.alpha * acc[mi][ni][r];
      }
  }
  if (do_bias) {  // uniform per workgroup
    f32x4* red = reinterpret_cast<f32x4*>(smem);  // [AKR][AQ]
    red[akq * AQ + a4] = bsum;
    __syncthreads();
    if (tid < AQ) {
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < AKR; ++r) t += red[r * AQ + tid];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + tid * 4 + e;
        if (m < p.M) p.bias_partial[(int64_t)split * p.M + m] = t[e];
      }
    }
  }
}

// out[i] = sum_k partial[k][i], fixed association (reproducible).  16-byte loads, 8 independent loads in flight per
// thread; KP threads share a column quad and split the k range (a 128-channel layer has 128 splits of only 147 K elements:
// one thread per element leaves too few bytes in flight to fill HBM), combined through LDS in k order.
// A second, small reduction (the bias gradient: [nsplit][n2]) rides in the same launch: workgroups main_blocks.. do it.
template <int KP>
__global__ __launch_bounds__(256) void reduce_splits_kernel(const float* __restrict__ partial, int nsplit, int64_t n, float* __restrict__ out,
                                                            int main_blocks, const float* __restrict__ partial2, int n2, float* __restrict__ out2) {
  constexpr int COLS = 256 / KP;
  __shared__ f32x4 red[KP > 1 ? 256 : 1];
  if ((int)blockIdx.x >= main_blocks) {  // uniform per workgroup
    const int i = ((int)blockIdx.x - main_blocks) * 256 + threadIdx.x;
    if (i < n2) {
      float s2 = 0.f;
      for (int k = 0; k < nsplit; ++k) s2 += partial2[(int64_t)k * n2 + i];
      out2[i] = s2;
    }
    return;
  }
  const int col = threadIdx.x % COLS, kp = threadIdx.x / COLS;
  const int64_t n4 = n >> 2;
  const int per = (nsplit + KP - 1) / KP;
  const int k0 = kp * per, k1 = min(nsplit, k0 + per);
  auto column = [&](int64_t i) {  // sum of splits [k0, k1) of column quad i
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    const f32x4* p = reinterpret_cast<const f32x4*>(partial) + i;
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
      f32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p[(int64_t)(k + j) * n4];
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; k < k1; ++k) s += p[(int64_t)k * n4];
    return s;
  };
  if (KP == 1) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)main_blocks * 256) reinterpret_cast<f32x4*>(out)[i] = column(i);
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * COLS + col;  // one workgroup per COLS column quads (no loop: the barrier below is uniform)
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i < n4) s = column(i);
  red[threadIdx.x] = s;
  __syncthreads();
  if (kp == 0 && i < n4) {
#pragma unroll
    for (int j = 1; j < KP; ++j) s += red[j * COLS + col];
    reinterpret_cast<f32x4*>(out)[i] = s;
  }
}
__global__ void reduce_splits_scalar_kernel(const float* __restrict__ partial, int nsplit, int64_t n, float* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += partial[(int64_t)k * n + i];
    out[i] = s;
  }
}

template <int BM, int BN, int WM, int WN, bool BKM, bool VEC>
int launch_rows_xf(const vae_igemm_args& a, dim3 grid, hipStream_t st) {
  if (BKM) {
    if (a.xf != VAE_XF_NONE) { vae_set_error("igemm_rows: xf unsupported with n-contiguous weights"); return VAE_EINVAL; }
    hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, BKM, VEC, VAE_XF_NONE>), grid, dim3(64 * WM * WN), 0, st, a);
    return 0;
  }
  switch (a.xf) {
    case VAE_XF_NONE: hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, false, VEC, VAE_XF_NONE>), grid, dim3(64 * WM * WN), 0, st, a); break;
    case VAE_XF_AFFINE: hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, false, VEC, VAE_XF_AFFINE>), grid, dim3(64 * WM * WN), 0, st, a); break;
    case VAE_XF_AFFINE_SILU: hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, false, VEC, VAE_XF_AFFINE_SILU>), grid, dim3(64 * WM * WN), 0, st, a); break;
    default: vae_set_error("igemm_rows: bad xf %d", a.xf); return VAE_EINVAL;
  }
  return 0;
}

template <int BM, int BN, int WM, int WN>
int launch_rows(const vae_igemm_args& a, bool bkm, bool vec, hipStream_t st) {
  dim3 grid((unsigned)(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN)), 1, (unsigned)a.batch);
  if (bkm) return vec ? launch_rows_xf<BM, BN, WM, WN, true, true>(a, grid, st) : launch_rows_xf<BM, BN, WM, WN, true, false>(a, grid, st);
  return vec ? launch_rows_xf<BM, BN, WM, WN, false, true>(a, grid, st) : launch_rows_xf<BM, BN, WM, WN, false, false>(a, grid, st);
}

template <int BM, int BN, int WM, int WN, bool VEC>
int launch_wgrad_xf(const vae_wgrad_args& a, dim3 grid, hipStream_t st) {
  switch (a.xf) {
    case VAE_XF_NONE: hipLaunchKernelGGL((wgrad_kernel<BM, BN, WM, WN, VEC, VAE_XF_NONE>), grid, dim3(64 * WM * WN), 0, st, a); break;
    case VAE_XF_AFFINE: hipLaunchKernelGGL((wgrad_kernel<BM, BN, WM, WN, VEC, VAE_XF_AFFINE>), grid, dim3(64 * WM * WN), 0, st, a); break;
    case VAE_XF_AFFINE_SILU: hipLaunchKernelGGL((wgrad_kernel<BM, BN, WM, WN, VEC, VAE_XF_AFFINE_SILU>), grid, dim3(64 * WM * WN), 0, st, a); break;
    default: vae_set_error("wgrad: bad xf %d", a.xf); return VAE_EINVAL;
  }
  return 0;
}
template <int BM, int BN, int WM, int WN>
int launch_wgrad(const vae_wgrad_args& a, bool vec, hipStream_t st) {
  dim3 grid((unsigned)(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN)), (unsigned)(a.g.taps * a.nsplit), (unsigned)a.batch);
  return vec ? launch_wgrad_xf<BM, BN, WM, WN, true>(a, grid, st) : launch_wgrad_xf<BM, BN, WM, WN, false>(a, grid, st);
}

}  // namespace

int launch_rows_f32(const vae_igemm_args& a, bool bkm, bool vec, hipStream_t st) {
  return (a.N <= 32) ? launch_rows<128, 32, 4, 1>(a, bkm, vec, st) : launch_rows<128, 128, 4, 2>(a, bkm, vec, st);
}
int launch_wgrad_f32(const vae_wgrad_args& a, bool vec, hipStream_t st) {
  if (a.M <= 32) return launch_wgrad<32, 128, 1, 4>(a, vec, st);
  if (a.N <= 32) return launch_wgrad<128, 32, 4, 1>(a, vec, st);
  return launch_wgrad<128, 128, 4, 2>(a, vec, st);
}

static int reduce_splits_impl(const float* partial, int32_t nsplit, int64_t n, float* out, const float* partial2, int32_t n2, float* out2,
                              hipStream_t st) {
  const int extra = partial2 ? (n2 + 255) / 256 : 0;
  if (n % 4 == 0 && aligned16(partial) && aligned16(out)) {
    const int64_t n4 = n / 4;
    if (nsplit >= 32) {  // few elements, many splits: 4 threads per column quad
      const int64_t blocks = (n4 + 63) / 64;
      VAE_CHECK(blocks + extra < (1ll << 31), "reduce_splits: too many elements");
      hipLaunchKernelGGL(reduce_splits_kernel<4>, dim3((unsigned)(blocks + extra)), dim3(256), 0, st, partial, nsplit, n, out, (int)blocks, partial2, n2, out2);
    } else {
      const int64_t blocks = std::min<int64_t>((n4 + 255) / 256, 8192);
      hipLaunchKernelGGL(reduce_splits_kernel<1>, dim3((unsigned)(blocks + extra)), dim3(256), 0, st, partial, nsplit, n, out, (int)blocks, partial2, n2, out2);
    }
  } else {
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(reduce_splits_scalar_kernel, dim3(blocks), dim3(256), 0, st, partial, nsplit, n, out);
    if (partial2) hipLaunchKernelGGL(reduce_splits_scalar_kernel, dim3(extra), dim3(256), 0, st, partial2, nsplit, (int64_t)n2, out2);
  }
  return 0;
}
extern "C" int vae_reduce_splits(const float* partial, int32_t nsplit, int64_t n, float* out, void* stream) {
  VAE_CHECK(partial && out && nsplit > 0 && n > 0, "reduce_splits: bad args");
  if (int rc = reduce_splits_impl(partial, nsplit, n, out, nullptr, 0, nullptr, (hipStream_t)stream)) return rc;
  VAE_LAUNCH_CHECK("reduce_splits");
  return VAE_OK;
}
extern "C" int vae_reduce_splits2(const float* partial, int32_t nsplit, int64_t n, float* out, const float* partial2, int32_t n2, float* out2,
                                  void* stream) {
  VAE_CHECK(partial && out && partial2 && out2 && nsplit > 0 && n > 0 && n2 > 0, "reduce_splits2: bad args");
  if (int rc = reduce_splits_impl(partial, nsplit, n, out, partial2, n2, out2, (hipStream_t)stream)) return rc;
  VAE_LAUNCH_CHECK("reduce_splits2");
  return VAE_OK;
}
extern "C" int vae_wgrad_wino_reduce(const float* slab, int32_t nsplit, int32_t npos, int32_t Cin, int32_t Cout, float* scratch, float* dW,
                                     const float* bias_partial, float* db, void* stream) {
  VAE_CHECK(slab && dW && nsplit > 0 && Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0, "wgrad_wino_reduce: bad args");
  VAE_CHECK(npos == 16 || npos == 9, "wgrad_wino_reduce: npos must be 16 (plain 3x3 layer) or 9 (upsampler convolution)");
  VAE_CHECK((bias_partial == nullptr) == (db == nullptr), "wgrad_wino_reduce: bias_partial and db go together");
  VAE_CHECK(nsplit == 1 || scratch != nullptr, "wgrad_wino_reduce: nsplit > 1 needs the [16*Cin*Cout] scratch buffer");
  hipStream_t st = (hipStream_t)stream;
  if (nsplit > 1) {  // wide fixed-order sum over the splits first (the slab of a 128-channel layer is 64 x 1 MB), then the transform
    if (int rc = reduce_splits_impl(slab, nsplit, (int64_t)npos * Cin * Cout, scratch, bias_partial, bias_partial ? Cout : 0, db, st)) return rc;
    VAE_LAUNCH_CHECK("reduce_splits");
    if (int rc = (npos == 9 ? launch_upwino_wgrad_reduce : launch_wino_wgrad_reduce)(scratch, 1, Cin, Cout, dW, nullptr, nullptr, st)) return rc;
  } else {
    if (int rc = (npos == 9 ? launch_upwino_wgrad_reduce : launch_wino_wgrad_reduce)(slab, 1, Cin, Cout, dW, bias_partial, db, st)) return rc;
  }
  VAE_LAUNCH_CHECK("wino_wgrad_reduce");
  return VAE_OK;
}
