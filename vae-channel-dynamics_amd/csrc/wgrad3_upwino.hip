// fp32 weight gradient of an Upsample2D block's convolution, conv3x3(nearest_upsample_2x(x)), with 9 multiplications per
// LOW-resolution pixel and (ci, co) pair (direct: 36; the four 2x2 phase weight gradients of round 1: 16).  Companion of
// conv3_upwino.hip.  Two loops, chosen at build time (VAE_UPWGRAD_X3): split-bf16 products on v_mfma_f32_32x32x16_bf16, two units per
// step (the default; described in front of its step below), or exact fp32 products on v_mfma_f32_32x32x2_f32, one unit per step
// (-DVAE_UPWGRAD_X3=0, make upwgrad_x3_off; the "Kernel" paragraph describes it; staging roles, operand builders, slab, bias
// partials and reduction are the same in both).
//
// F(3x3, 2x2) on the 2x2 block of dY that belongs to low-resolution pixel (i, j) reads the 4x4 patch of the UPSAMPLED input with
// origin (2i-1, 2j-1), whose rows are x[i-1], x[i], x[i], x[i+1]: row 2 of B^T d vanishes, so only the positions {0, 1, 3}^2 of the
// transform domain carry anything.  With the factor 2 of position 1 moved into G nothing is halved:
//     dW = A''^T [ sum_pixels (G'' dy G''^T) (.) (L d3 L^T) ] A''     d3: 3x3 low-resolution patch of x, dy: 2x2 block of dY
//     L = [1 -1 0; 0 1 0; 0 1 -1]     G'' = [1 0; 1 1; 0 1]     A''^T = [1 1 0; 0 1 0; 0 1 -1]
// (row 0 of dW: dy0 (x[i-1] - x[i]) + (dy0 + dy1) x[i] = dy0 x[i-1] + dy1 x[i]: tap kh = 0 meets x[i-1] from the even output row
// and x[i] from the odd one.)  Per position a GEMM  M_p[ci][co] = sum_pixels V_p[pixel][ci] * D_p[pixel][co].
//
// Kernel: the scheme of wgrad3_wino.hip, sharing with it by name (wino_common.h) split_tile_of_workgroup (without the rule for
// 2 and 4 splits), unit_range, slab_store, bias_tail and the eligibility preamble -- a unit = 8 low-resolution pixels of one
// row (a 2 x 16 strip of dY); per unit the 3 x 10-pixel halo of x and the strip of dY go to LDS untransformed, transposed to
// [row][channel][x]; a wave builds its MFMA operands while reading them; split-K slabs [split][9][Cin][Cout];
// wgrad_wino_reduce_kernel<9> (igemm.hip, one body for both schemes) sums the slabs in fixed order, applies A''^T . A'' and
// writes OHWI.  Workgroup = 8 waves = 32 ci x 128 co x 9 positions: wave w owns position w (all four 32-channel blocks of co),
// and the NINTH position is split by channel block over waves 0..3 -- one per SIMD (wave k of a workgroup runs on SIMD k % 4),
// so every SIMD carries 36 MFMAs per step.  (A first version with one position per wave and 9 waves put three waves of every
// workgroup on SIMD 0: 0.51 of the matrix peak.)  One workgroup per CU at 158 registers (a 128-register build spilled 27, with
// scratch reloads inside the loop); two staging register sets, the next-but-one unit requested behind the first channel block's
// MFMAs.  The split loop: 168 registers, 100,352 B of dynamic LDS (two stages per pair, double buffered), no scratch.
#include "wino_common.h"
#include <algorithm>
#include <type_traits>

#ifndef VAE_UPWGRAD_X3
#define VAE_UPWGRAD_X3 1  // 1: split-bf16 products, two units per step; 0: exact fp32 products, one unit per step (make upwgrad_x3_off)
#endif
#if VAE_UPWGRAD_X3
#include "bf16_frag.h"
#endif
// VAE_UPWGRAD_PRIO 1 (default): waves 4..7 (the second-dispatched wave of every SIMD, which loses the issue arbitration to its partner)
// run the split loop at s_setprio 1, as in wgrad3_wino.hip: 3.1-3.5 % faster on the step's three layers (profiles/upw_tiles_measured.json)
#ifndef VAE_UPWGRAD_PRIO
#define VAE_UPWGRAD_PRIO 1
#endif

namespace {

constexpr int GCI = 32, GCO = 128, NPOS = 9, GNT = 512, GNB = GCO / 32;
constexpr int XSX = 12;                 // x pitch of a staged halo row (floats): 10 columns + padding (16-byte reads at 0 / 4 / 8)
constexpr int XSY = 20;                 // x pitch of a staged dY row: 16 columns + padding
constexpr int SXF = 3 * GCI * XSX;      // halo stage: [3 rows][32 ci][XSX]
constexpr int SYF = 2 * GCO * XSY;      // dY stage:   [2 rows][128 co][XSY]
constexpr int GSTAGE = SXF + SYF;       // 6272 floats (25088 B)
#if VAE_UPWGRAD_X3
constexpr int GPAIR = 2 * GSTAGE;                     // the two stages of a pair of units
constexpr int GLDS = 2 * GPAIR * (int)sizeof(float);  // double buffered: 100352 B
extern __shared__ __attribute__((aligned(16))) float upwgrad_lds[];
#endif

__global__ __launch_bounds__(GNT, 2) void wgrad3_upwino_kernel(vae_wgrad_args p, int strips, int64_t nunits) {
#if VAE_UPWGRAD_X3
  float* const smem = upwgrad_lds;
#else
  __shared__ __attribute__((aligned(16))) float smem[2 * GSTAGE];
#endif

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // wave = position (pr, pc) 0..7; position 8: block `wave` on waves 0..3
  const int lr = lane & 31, lh = lane >> 5;
  const vae_conv_geom g = p.g;  // Hs x Ws: the low-resolution x; Ho x Wo = 2 Hs x 2 Ws: dY
  const int tilesN = p.N / GCI, ntile = tilesN * (p.M / GCO);
  const wino::SplitTile wg = wino::split_tile_of_workgroup<false>(blockIdx.x, p.nsplit, ntile);  // (2 or 4 splits: tile fastest)
  const int tile = wg.tile, split = wg.split;
  const int tm = tile / tilesN, tn = tile % tilesN;
  const int m0 = tm * GCO, n0 = tn * GCI;
  const wino::UnitRange ur = wino::unit_range(nunits, p.nsplit, split);
  const int64_t ubeg = ur.ubeg;
  const int nu = ur.nu;
  const int upi = g.Hs * strips;  // units per image
  const bool do_bias = (p.bias_partial != nullptr) && tn == 0;

  // ---- staging roles.  dY strip (all 512 threads): column xx, channel quad yq, both rows.  x halo (threads 0..239): row xr,
  // column xc of the 3 x 10 halo, channel quad xq (fastest: 16-byte neighbours in memory) ----
  const int xx = tid & 15, yq = tid >> 4;
  const bool xrole = tid < 240;
  const int xq = tid & 7, xc = (tid >> 3) % 10, xr = tid / 80;
  const auto rsX = VAE_BUF_RSRC(p.X, (size_t)g.B * g.Hs * g.Ws * g.Cs * 4u);
  const auto rsY = VAE_BUF_RSRC(p.dY, (size_t)g.B * g.Ho * g.Wo * p.ldy * 4u);
  // TWO sets of staging registers (the kernel runs at a 256-register budget): unit k+2 is requested during step k, behind its
  // first block's MFMAs, and stored at the end of step k+1 -- two steps (~3 us) of lead; with one set requested at the start
  // of a step and stored at its end the store sat on the HBM round trip
  struct Stg {
    f32x4 rx, ry[2];
  };
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  Stg s0{z4, {z4, z4}}, s1{z4, {z4, z4}};
  f32x4 bsum = z4;
  // the unit the next load_unit call requests (calls go through ubeg, ubeg+1, ...: counters instead of divisions per step)
  int ub = (int)(ubeg / upi), urow = (int)((ubeg - (int64_t)ub * upi) / strips), ustrip = (int)((ubeg - (int64_t)ub * upi) % strips);
  const unsigned rowY = (unsigned)g.Wo * p.ldy * 4u;
  auto load_unit = [&](int k, Stg& r) {  // requests for unit ubeg + k (beyond the range: nothing is read, zeros)
    const bool ok = k < nu;
    const int b = ub, i = urow, x0 = ustrip * 8;
    if (++ustrip == strips) {
      ustrip = 0;
      if (++urow == g.Hs) {
        urow = 0;
        ++ub;
      }
    }
    const int hy = i - 1 + xr, hx = x0 - 1 + xc;
    const bool xin = ok && xrole && ((unsigned)hy < (unsigned)g.Hs) && ((unsigned)hx < (unsigned)g.Ws);
    r.rx = VAE_BUF_LOAD4(rsX, xin ? (unsigned)(((b * g.Hs + hy) * g.Ws + hx) * g.Cs + n0 + 4 * xq) * 4u : BUF_OOB);  // (unsigned before the * 4: descriptors reach 4 GiB)
    const unsigned baseY = (unsigned)((b * g.Ho + 2 * i) * g.Wo + 2 * x0 + xx) * (unsigned)p.ldy * 4u + (unsigned)(m0 + 4 * yq) * 4u;
#pragma unroll
    for (int a = 0; a < 2; ++a) r.ry[a] = VAE_BUF_LOAD4(rsY, ok ? baseY + a * rowY : BUF_OOB);
  };
  auto store_unit = [&](float* st, const Stg& r) {
    float* sx = st;
    float* sy = st + SXF;
    if (xrole) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sx[(xr * GCI + 4 * xq + e) * XSX + xc] = r.rx[e];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sy[(a * GCO + 4 * yq + e) * XSY + xx] = r.ry[a][e];
      if (do_bias) bsum += r.ry[a];
    }
  };

  f32x16 acc[GNB], accx;  // accx: position 8, channel block `wave` (waves 0..3)
#pragma unroll
  for (int nb = 0; nb < GNB; ++nb)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[nb][e] = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) accx[e] = 0.f;

#if VAE_UPWGRAD_X3
  // One set of staging registers per unit of a pair (s0: the first): a wave stores pair kp+1 during step kp and requests pair kp+2
  // right behind the stores, into the same registers: a whole step in flight.  The units are stored in ascending order, dY row 0
  // before row 1: the order of the bias sums is the exact loop's (units beyond the range add zeros)
  auto stage_pair = [&](float* st, int kp) __attribute__((always_inline)) {
    store_unit(st, s0);
    store_unit(st + GSTAGE, s1);
    load_unit(2 * kp + 2, s0);
    load_unit(2 * kp + 3, s1);
  };
  load_unit(0, s0);
  load_unit(1, s1);
  stage_pair(smem, 0);  // pair 0 to LDS, pair 1 requested
  __syncthreads();
#else
  load_unit(0, s0);
  store_unit(smem, s0);
  load_unit(1, s1);
  __syncthreads();
#endif

  // operand builders for position (pr, pc).  V fragment: lane (ci = lr, half lh) takes tiles 4 lh + e: halo columns 4 lh .. 4 lh + 5
  // of the rows the position combines (rows 0, 1, 2 of the halo = x[i-1], x[i], x[i+1]: pr 0: r0 - r1, 1: r1, 2: r1 - r2).
  // D fragment of channel block nb: tiles 4 lh + e = dY columns 8 lh + 2 e, + 1 (pr 0: dy row 0, 1: row 0 + row 1, 2: row 1).
  auto build_a = [&](auto PR, auto PC, const float* cx, f32x4& a4) {
    constexpr int pr = decltype(PR)::value, pc = decltype(PC)::value;
    constexpr int vr1 = pr == 0 ? 0 : 1, vr2 = pr == 0 ? 1 : 2;
    const int voff1 = (vr1 * GCI + lr) * XSX + 4 * lh, voff2 = (vr2 * GCI + lr) * XSX + 4 * lh;
    float rc[8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const f32x4 u1 = *reinterpret_cast<const f32x4*>(&cx[voff1 + 4 * c]);
      if (pr == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) rc[4 * c + e] = u1[e];
      } else {
        const f32x4 u2 = *reinterpret_cast<const f32x4*>(&cx[voff2 + 4 * c]);
#pragma unroll
        for (int e = 0; e < 4; ++e) rc[4 * c + e] = u1[e] - u2[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a4[e] = pc == 0 ? rc[e] - rc[e + 1] : (pc == 1 ? rc[e + 1] : rc[e + 1] - rc[e + 2]);
  };
  auto build_b = [&](auto PR, auto PC, const float* cy, int nb, f32x4& b4) {
    constexpr int pr = decltype(PR)::value, pc = decltype(PC)::value;
    constexpr int dr1 = pr == 2 ? 1 : 0;
    const int doff = (dr1 * GCO + nb * 32 + lr) * XSY + 8 * lh;
    float rc[8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(&cy[doff + 4 * c]);
      if (pr == 1) {
        const f32x4 d1 = *reinterpret_cast<const f32x4*>(&cy[doff + GCO * XSY + 4 * c]);
#pragma unroll
        for (int e = 0; e < 4; ++e) rc[4 * c + e] = d0[e] + d1[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) rc[4 * c + e] = d0[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) b4[e] = pc == 0 ? rc[2 * e] : (pc == 1 ? rc[2 * e] + rc[2 * e + 1] : rc[2 * e + 1]);
  };
  using I2 = std::integral_constant<int, 2>;

  // The loop body is instantiated per position: straight-line code, no per-step branches.
  auto run = [&](auto PR, auto PC, auto EXTRA) {
    constexpr bool extra = decltype(EXTRA)::value;  // this wave also owns block `wave` of position 8 = (2, 2)
#if VAE_UPWGRAD_X3
    // The K = 16 of v_mfma_f32_32x32x16_bf16 is two units: a split's unit range is walked in pairs (an odd last unit is paired with
    // the zeros load_unit delivers beyond the range), each unit in a stage of its own ([pair parity][unit of the pair][GSTAGE]).
    // A lane half's eight k are the four tiles it takes in the exact loop, of the pair's first unit (k 0..3) and of its second
    // (k 4..7), in the V and in the D operand alike.  build_a / build_b stay in fp32; their results are split in registers (split8)
    // and a product is the six plane products of mma_x3_term, smallest first: 24 (30 on waves 0..3) MFMAs of 32 cycles per wave and
    // pair against 32 (40) of 64 cycles.  Waves 0..3 store the next pair behind their V operands, waves 4..7 in front of their last
    // block: the two waves of a SIMD store at opposite ends of the step (wgrad3_wino.hip).
    auto step = [&](int kp) {
      const float* cst = smem + (kp & 1) * GPAIR;
      float* nst = smem + ((kp + 1) & 1) * GPAIR;
      Bf3 a3, bb;
      {
        f32x4 a0, a1;
        build_a(PR, PC, cst, a0);
        build_a(PR, PC, cst + GSTAGE, a1);
        a3 = split8(a0, a1);
      }
      if (extra) stage_pair(nst, kp + 1);
      __builtin_amdgcn_sched_barrier(0);
      // no scheduling barrier between the blocks: block nb+1's LDS reads and additions may move up between block nb's MFMAs
#pragma unroll
      for (int nb = 0; nb < GNB; ++nb) {
        if (nb == GNB - 1 && !extra) {
          __builtin_amdgcn_sched_barrier(0);
          stage_pair(nst, kp + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 b0, b1;
        build_b(PR, PC, cst + SXF, nb, b0);
        build_b(PR, PC, cst + GSTAGE + SXF, nb, b1);
        bb = split8(b0, b1);
#pragma unroll
        for (int t = 0; t < 6; ++t) acc[nb] = mma_x3_term(t, a3.p, bb.p, acc[nb]);
      }
      if (extra) {
        f32x4 a0, a1, b0, b1;
        build_a(I2{}, I2{}, cst, a0);
        build_a(I2{}, I2{}, cst + GSTAGE, a1);
        build_b(I2{}, I2{}, cst + SXF, wave, b0);
        build_b(I2{}, I2{}, cst + GSTAGE + SXF, wave, b1);
        a3 = split8(a0, a1);
        bb = split8(b0, b1);
#pragma unroll
        for (int t = 0; t < 6; ++t) accx = mma_x3_term(t, a3.p, bb.p, accx);
      }
      __syncthreads();
    };
    const int np = (nu + 1) / 2;  // steps
    for (int kp = 0; kp < np; ++kp) step(kp);
#else
    auto step = [&](int k, const Stg& cur, Stg& nxt) {  // cur: unit k+1 (requested during step k-1); nxt receives unit k+2
      const float* cx = smem + (k & 1) * GSTAGE;
      const float* cy = cx + SXF;
      float* nst = smem + ((k + 1) & 1) * GSTAGE;
      f32x4 a4, bb[2];
      build_a(PR, PC, cx, a4);
      build_b(PR, PC, cy, 0, bb[0]);
#pragma unroll
      for (int nb = 0; nb < GNB; ++nb) {
        __builtin_amdgcn_sched_barrier(0);
        if (nb == 1) {  // the requests for unit k+2 (index counters + 3 loads) behind the first block's MFMAs
          load_unit(k + 2, nxt);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (nb + 1 < GNB) build_b(PR, PC, cy, nb + 1, bb[(nb + 1) & 1]);  // the next block's operands, while this block's MFMAs issue
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], bb[nb & 1][e], acc[nb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (extra) {
        f32x4 ax, bx;
        build_a(I2{}, I2{}, cx, ax);
        build_b(I2{}, I2{}, cy, wave, bx);
#pragma unroll
        for (int e = 0; e < 4; ++e) accx = __builtin_amdgcn_mfma_f32_32x32x2f32(ax[e], bx[e], accx, 0, 0, 0);
      }
      store_unit(nst, cur);
      __syncthreads();
    };
    int k = 0;
    for (; k + 1 < nu; k += 2) {
      step(k, s1, s0);
      step(k + 1, s0, s1);
    }
    if (k < nu) step(k, s1, s0);
#endif
  };
#if VAE_UPWGRAD_X3 && VAE_UPWGRAD_PRIO  // one static s_setprio around the loop; a scalar condition: the instruction ignores EXEC
  if (__builtin_amdgcn_readfirstlane(tid) >= 256) __builtin_amdgcn_s_setprio(1);
#endif
  {
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using T = std::true_type;
    using F_ = std::false_type;
    switch (wave) {  // (wave-uniform: pr = wave / 3, pc = wave % 3; waves 0..3 carry the ninth position's blocks)
      case 0: run(I0{}, I0{}, T{}); break;
      case 1: run(I0{}, I1{}, T{}); break;
      case 2: run(I0{}, I2{}, T{}); break;
      case 3: run(I1{}, I0{}, T{}); break;
      case 4: run(I1{}, I1{}, F_{}); break;
      case 5: run(I1{}, I2{}, F_{}); break;
      case 6: run(I2{}, I0{}, F_{}); break;
      default: run(I2{}, I1{}, F_{}); break;
    }
  }
#if VAE_UPWGRAD_X3 && VAE_UPWGRAD_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif

  // ---- epilogue: slab [split][9 positions][Cin][Cout]; lanes along co (128-byte rows) ----
  float* __restrict__ O = p.partial + (int64_t)split * NPOS * p.N * p.M;
  wino::slab_store<GNB>(O, wave, p.N, p.M, n0, m0, 0, acc, lr, lh);
  if (wave < 4) wino::slab_store<1>(O, 8, p.N, p.M, n0, m0, wave, &accx, lr, lh);
  if (do_bias) wino::bias_tail(bsum, xx, p.bias_partial, (int64_t)split * p.M + m0 + 4 * yq);  // workgroup-uniform
}

}  // namespace

// conv3x3(nearest_upsample_2x(x)) in fp32: geometry mode UP2X (source = the low-resolution x, row grid = dY at twice the size),
// 8 | low-resolution width, 32 | Cin, 128 | Cout
bool wgrad3_upwino_eligible(const vae_wgrad_args& a) {
  const vae_conv_geom& g = a.g;
  if (!wino::wgrad_eligible_common(a, GCI, GCO) || a.x_bf16 || a.y_bf16 || a.xf != VAE_XF_NONE) return false;
  if (g.mode != VAE_MODE_UP2X || g.Ho != 2 * g.Hs || g.Wo != 2 * g.Ws) return false;
  return g.Ws % 8 == 0 && g.Cs >= a.N;
}

int64_t wgrad3_upwino_units(const vae_conv_geom& g) { return (int64_t)g.B * g.Hs * (g.Ws / 8); }

int launch_wgrad3_upwino(const vae_wgrad_args& a, hipStream_t st) {
  const vae_conv_geom& g = a.g;
  const int64_t nunits = wgrad3_upwino_units(g);
  dim3 grid((unsigned)((a.M / GCO) * (a.N / GCI) * a.nsplit), 1, 1);
#if VAE_UPWGRAD_X3  // (more than 64 KB of dynamic LDS: reserved once per device)
  VAE_RESERVE_LDS(wgrad3_upwino_kernel, GLDS, "wgrad3_upwino");
  hipLaunchKernelGGL(wgrad3_upwino_kernel, grid, dim3(GNT), GLDS, st, a, g.Ws / 8, nunits);
#else
  hipLaunchKernelGGL(wgrad3_upwino_kernel, grid, dim3(GNT), 0, st, a, g.Ws / 8, nunits);
#endif
  return 0;
}
