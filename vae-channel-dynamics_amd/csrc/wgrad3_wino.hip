// Winograd F(3x3, 2x2) for the fp32 weight gradient of the 3x3 stride-1 layers: the 3x3 gradient of a (ci, co) pair over a 2x2
// block of output pixels needs 16 multiplications instead of 36 (2.25x fewer MFMA passes); fp32 accumulation over all tiles in
// the transform domain.  Two loops, chosen at build time (VAE_WGRAD_X3): split-bf16 products on v_mfma_f32_32x32x16_bf16, two units
// per step (the default; described in front of that kernel below), or exact fp32 products on v_mfma_f32_32x32x2_f32, one unit per
// step (-DVAE_WGRAD_X3=0; the points below describe it, and staging, operand roles, slab and reduction are the same in both).
//     dW = A^T [ sum_tiles (G dy G^T) (.) (B^T d B) ] A      d: 4x4 patch of XF(X) (origin 2t-1), dy: 2x2 block of dY, dW: 3x3
//     B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]   G = [1 0; .5 .5; .5 -.5; 0 1]   A^T = [1 1 1 0; 0 1 -1 0; 0 1 1 -1]
// Per position p = (i, j) of the 4x4 transform domain this is a GEMM  M_p[ci][co] = sum_tile V_p[tile][ci] * D_p[tile][co].
//   * Workgroup (8 waves) = 32 ci x 128 co x all 16 positions over a range of units; unit = a 2 x 16-pixel strip of the output
//     (8 tiles = the K-step).  Per unit the 4 x 18-pixel halo of X (GroupNorm + SiLU applied once per element) and the 2 x 16 x 128
//     strip of dY go to LDS *untransformed* but transposed to [row][channel][x]: 30 KB per step, double buffered, one barrier.
//   * Wave w owns positions (i = w/2, j = 2(w%2), 2(w%2)+1) and builds its MFMA operands while reading them: lane (channel, half)
//     reads the 12 / 8 contiguous x values its four tiles need from the 2 (or 1) rows that position row i combines
//     (conflict-free 16-byte reads at a row pitch of 20 floats) and forms the row / column combinations in registers
//     (18 additions for the V fragment pair, <= 12 per channel block for D).  No transformed image ever exists in LDS.
//     The halves of G are left out (D' = G' dy G'^T with G' = [1 0; 1 1; 1 -1; 0 1]) and applied as exact power-of-two
//     factors c_i c_j, c = (1, .5, .5, 1), by the reduction.
//   * Split-K over unit ranges: a workgroup writes its 16 x 32 x 128 accumulators into a slab [split][16][Cin][Cout];
//     wgrad_wino_reduce_kernel<16> (igemm.hip, shared with the upsampler scheme) reads the slab once: it sums the splits in
//     fixed order (deterministic), applies the factors and A^T . A and writes OHWI through an LDS transpose; the bias gradient
//     (column sums of dY) rides along as in the direct kernel.
// Numerics: measured against the direct kernel in tests/test_kernels_gpu.py (the transform-domain sums cancel in the output
// transform, so the error is a few 1e-6 of the gradient scale instead of 1e-7; the parity bar is 1e-4).
// Shared with wgrad3_upwino.hip (wino_common.h): workgroup id -> (tile, split), the split's unit range, the slab store, the bias
// tail and the eligibility preamble.
#include "wino_common.h"
#ifndef VAE_ABLATE
#define VAE_ABLATE 0  // diagnostic builds (tools/ablation_builds.sh, wrong results): bit 0 no global loads, 1 no LDS stores, 4 no barrier
#endif
#ifndef VAE_WGRAD_DEFER
#define VAE_WGRAD_DEFER 2  // channel blocks (of 4) whose MFMAs waves 4..7 issue one step late; 0: all eight waves run one program
#endif
#ifndef VAE_WGRAD_PRIO
#define VAE_WGRAD_PRIO 1  // 1: waves 4..7 (the second-dispatched wave of every SIMD, which loses the issue arbitration to its partner) run the loop at s_setprio 1; 0: no priority
#endif
#ifndef VAE_WGRAD_X3
#define VAE_WGRAD_X3 1  // 1: split-bf16 products on v_mfma_f32_32x32x16_bf16, two units per step; 0: exact fp32 products, one unit per step (make wgrad_x3_off)
#endif
#if VAE_WGRAD_X3
#include "bf16_frag.h"
#endif
#include <algorithm>
#include <type_traits>

namespace {

constexpr int GCI = 32, GCO = 128, GNT = 512;
constexpr int XS = 20;                  // x pitch of a staged row (floats): 18 halo / 16 strip columns + padding
constexpr int SXF = 4 * GCI * XS;       // halo stage: [4 rows][32 ci][XS]
constexpr int SYF = 2 * GCO * XS;       // dY stage:   [2 rows][128 co][XS]
constexpr int GSTAGE = SXF + SYF;       // 7680 floats (30720 B)

#if !VAE_WGRAD_X3  // ---- exact fp32 products: one unit (K = 8 tiles) per step ----
template <int XF>
__global__ __launch_bounds__(GNT, 1) void wgrad3_wino_kernel(vae_wgrad_args p, int strips, int64_t nunits) {
  __shared__ __attribute__((aligned(16))) float smem[2 * GSTAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const vae_conv_geom g = p.g;
  const int tilesN = p.N / GCI, ntile = tilesN * (p.M / GCO);
  const wino::SplitTile wg = wino::split_tile_of_workgroup<true>(blockIdx.x, p.nsplit, ntile);  // (with the rule for 2 and 4 splits)
  const int tile = wg.tile, split = wg.split;
  const int tm = tile / tilesN, tn = tile % tilesN;
  const int m0 = tm * GCO, n0 = tn * GCI;
  const wino::UnitRange ur = wino::unit_range(nunits, p.nsplit, split);
  const int64_t ubeg = ur.ubeg;
  const int nu = ur.nu;
  const int upi = (g.Ho / 2) * strips;  // units per image
  const bool do_bias = (p.bias_partial != nullptr) && tn == 0;
#ifdef VAE_WGRAD_TIMING  // debug build (tools/wgrad_timing.py): shader-clock stamps of waves 0 and 4 (the two waves of SIMD 0) of workgroups 0..7 -> p.out,
  // which this kernel otherwise never touches: [workgroup][wave / 4][4 + TSN * 5] uint64 = entry, loop exit, 100 MHz clock at both; per step TS0.. :
  // begin (barrier released), deferred MFMAs issued, operands built (first own MFMA), last MFMA issued, barrier reached
  constexpr int TS0 = 2, TSN = 8;
  const bool tw = (tid & 255) == 0 && blockIdx.x < 8 && p.out != nullptr;
  unsigned long long* const tout = reinterpret_cast<unsigned long long*>(p.out) + (blockIdx.x * 2 + (tid >> 8)) * (4 + TSN * 5);
  unsigned long long tst[5];
  const unsigned long long te0 = __builtin_amdgcn_s_memtime(), tr0 = __builtin_amdgcn_s_memrealtime();
#define GSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); tst[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define GSTAMPS_OUT(k) do { if (tw && (k) >= TS0 && (k) < TS0 + TSN) { _Pragma("unroll") for (int i_ = 0; i_ < 5; ++i_) tout[4 + ((k) - TS0) * 5 + i_] = tst[i_]; } } while (0)
#else
#define GSTAMP(i) do { } while (0)
#define GSTAMPS_OUT(k) do { } while (0)
#endif

  // ---- staging roles.  X halo: thread -> (row xr, channel quad xq, column xx) of the 4 x 16 main block, threads with
  // (tid & 8) == 0 && tid < 128 also one element of the two extra columns (same channel quad: shared GroupNorm rows).
  // Lanes run along x (16) and 4 channel quads: the four 4-byte LDS writes of a loaded float4 are conflict-free ----
  const int xx = tid & 15, xq = (tid >> 4) & 7, xr = tid >> 7;
  const bool xe_role = tid < 128 && (tid & 8) == 0;
  const int ex = 16 + (tid & 1), er = (tid >> 1) & 3;
  // dY strip: thread -> (column xx, channel quad yq) for both rows
  const int yq = tid >> 4;
  const auto rsX = VAE_BUF_RSRC(p.X, (size_t)g.B * g.Hs * g.Ws * g.Cs * 4u);
  const auto rsY = VAE_BUF_RSRC(p.dY, (size_t)g.B * g.Ho * g.Wo * p.ldy * 4u);
  // Two sets of staging registers: the requests for unit k+2 go out at the start of step k (into the set unit k used) and are
  // stored during step k+1, so they have a whole step in flight wherever in the step a wave does its stores.
  struct Stg {
    f32x4 rx, rxe, ry[2];
    int b;  // image of the unit (workgroup-uniform)
    bool xin, xein;
  };
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  Stg s0{z4, z4, {z4, z4}, -1, false, false}, s1 = s0;
  f32x4 bsum = z4;
  // GroupNorm rows of the thread's channel quad for image sc_b: one set, re-read when a stored unit belongs to the next image
  // (a workgroup's unit range crosses few image boundaries; the re-read waits for L2 once per boundary)
  f32x4 rsc = {1.f, 1.f, 1.f, 1.f}, rsh = z4;
  int sc_b = -1;
  // the unit the next load_unit call requests (calls go through ubeg, ubeg+1, ...: counters instead of divisions per step)
  int ub = (int)(ubeg / upi), uty = (int)((ubeg - (int64_t)ub * upi) / strips), ustrip = (int)((ubeg - (int64_t)ub * upi) % strips);
  // Addresses = a workgroup-uniform part (scalar registers) + a per-thread constant; an element is padding when one of the
  // thread's position flags meets the unit's border flag (bit 0: first halo row / top border, 1: last halo row / bottom border,
  // 2: first halo column / left border, 3: last halo column / right border, 4: always / unit beyond the range).
  const unsigned thrX = ((xr * g.Ws + xx) * g.Cs + n0 + 4 * xq) * 4u, thrE = ((er * g.Ws + ex) * g.Cs + n0 + 4 * xq) * 4u;
  const unsigned thrY = (xx * p.ldy + m0 + 4 * yq) * 4u, rowY = (unsigned)g.Wo * p.ldy * 4u;
  const int tfX = (xr == 0 ? 1 : 0) | (xr == 3 ? 2 : 0) | (xx == 0 ? 4 : 0) | 16;
  const int tfE = xe_role ? ((er == 0 ? 1 : 0) | (er == 3 ? 2 : 0) | (ex == 17 ? 8 : 0) | 16) : 31;
  auto load_unit = [&](int k, Stg& r) {  // requests for unit ubeg + k (beyond the range: nothing is read, zeros)
    const bool ok = k < nu;
    const int b = ub, ty = uty, x0 = ustrip * 16;
    if (++ustrip == strips) {
      ustrip = 0;
      if (++uty == g.Ho / 2) {
        uty = 0;
        ++ub;
      }
    }
    r.b = ok ? b : -1;
    const int uf = (ty == 0 ? 1 : 0) | (2 * ty + 2 >= g.Hs ? 2 : 0) | (x0 == 0 ? 4 : 0) | (x0 + 16 >= g.Ws ? 8 : 0) | (ok ? 0 : 16);
    // (the halo origin may lie before the tensor: unsigned arithmetic wraps, the sum with the thread's part is exact)
    const unsigned baseX = (unsigned)((b * g.Hs + 2 * ty - 1) * g.Ws + x0 - 1) * (unsigned)g.Cs * 4u;
    const unsigned baseY = (unsigned)((b * g.Ho + 2 * ty) * g.Wo + x0) * (unsigned)p.ldy * 4u;
    r.xin = (tfX & uf) == 0;
    r.rx = VAE_BUF_LOAD4(rsX, r.xin ? baseX + thrX : BUF_OOB);
    r.xein = (tfE & uf) == 0;
    r.rxe = VAE_BUF_LOAD4(rsX, r.xein ? baseX + thrE : BUF_OOB);
#pragma unroll
    for (int a = 0; a < 2; ++a) r.ry[a] = VAE_BUF_LOAD4(rsY, ok ? baseY + a * rowY + thrY : BUF_OOB);
  };
  auto xform = [&](f32x4 v, bool in) {
    if (XF != VAE_XF_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float u = v[e] * rsc[e] + rsh[e];
        if (XF == VAE_XF_AFFINE_SILU) u = silu_f(u);
        v[e] = in ? u : 0.f;  // padding stays zero AFTER the transform
      }
    }
    return v;
  };
  auto store_unit = [&](float* st, const Stg& r) {
    float* sx = st;
    float* sy = st + SXF;
    if (XF != VAE_XF_NONE && r.b >= 0 && r.b != sc_b) {  // workgroup-uniform
      sc_b = r.b;
      rsc = *reinterpret_cast<const f32x4*>(p.scale + (int64_t)sc_b * g.Cs + n0 + 4 * xq);
      rsh = *reinterpret_cast<const f32x4*>(p.shift + (int64_t)sc_b * g.Cs + n0 + 4 * xq);
    }
    const f32x4 v = xform(r.rx, r.xin);
#pragma unroll
    for (int e = 0; e < 4; ++e) sx[(xr * GCI + 4 * xq + e) * XS + xx] = v[e];
    if (xe_role) {
      const f32x4 ve = xform(r.rxe, r.xein);
#pragma unroll
      for (int e = 0; e < 4; ++e) sx[(er * GCI + 4 * xq + e) * XS + ex] = ve[e];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sy[(a * GCO + 4 * yq + e) * XS + xx] = r.ry[a][e];
      if (do_bias) bsum += r.ry[a];
    }
  };

  // ---- operand roles: wave -> row i of the transform domain and the column pair (2 jh, 2 jh + 1) ----
  const int wi = wave >> 1, jh = wave & 1;
  // V row combination: B^T row i = x[r1] + sg * x[r2]
  const int vr1 = wi == 0 ? 0 : (wi == 2 ? 2 : 1), vr2 = wi == 0 ? 2 : (wi == 1 ? 2 : (wi == 2 ? 1 : 3));
  const int voff1 = (vr1 * GCI + lr) * XS + 8 * lh, voff2 = (vr2 * GCI + lr) * XS + 8 * lh;
  // D' row combination: i = 0: dy row 0, 3: row 1, 1: row0 + row1, 2: row0 - row1
  const int dr1 = wi == 3 ? 1 : 0;

  f32x16 acc[2][4];
#pragma unroll
  for (int pi = 0; pi < 2; ++pi)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[pi][nb][e] = 0.f;

  load_unit(0, s0);
  store_unit(smem, s0);
  load_unit(1, s1);
  __syncthreads();

  // The loop body is instantiated per (two-row D combination?, column pair): straight-line code, no per-step branches.
  auto run = [&](auto WI, auto JH) {
    constexpr int wic = decltype(WI)::value, jhc = decltype(JH)::value;
    constexpr bool two = wic == 1 || wic == 2;  // D' row i combines both dY rows
    constexpr bool vplus = wic == 1;            // sign of the second row in the combinations (V: B^T row i, D': G' row i)
    // The two waves of a SIMD (w and w + 4) run the same program between the same barriers and would build their operands at
    // the same time, the matrix pipe idle in both.  Waves 4..7 (wic >= 2) therefore hold the MFMAs of a step's last `ndef`
    // channel blocks back: the operands (a4 and the bb the step ends with) stay in registers across the barrier and the
    // MFMAs open the NEXT step, in front of its LDS reads, while the partner builds.  Every accumulator still receives the
    // same products in the same order (units ascending, e = 0..3): the sums do not change by a bit.
    constexpr int ndef = wic >= 2 ? VAE_WGRAD_DEFER : 0;
    static_assert(ndef >= 0 && ndef <= 2, "bb holds the operands of two channel blocks");
    f32x4 a4[2], bb[2][2];  // V fragments of the two positions; D' operands of channel blocks nb (bb[nb & 1])
    if (ndef > 0) {  // (the first step's held-back MFMAs add 0 * 0 to accumulators that are +0)
      a4[0] = a4[1] = z4;
      bb[0][0] = bb[0][1] = bb[1][0] = bb[1][1] = z4;
    }
    auto held_back = [&]() {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int nb = 4 - ndef; nb < 4; ++nb)
#pragma unroll
          for (int pi = 0; pi < 2; ++pi) acc[pi][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[pi][e], bb[nb & 1][pi][e], acc[pi][nb], 0, 0, 0);
    };
    auto step = [&](int k, const Stg& cur, Stg& nxt) {  // cur: unit k+1 (requested during step k-1); nxt receives unit k+2
      const float* cx = smem + (k & 1) * GSTAGE;
      const float* cy = cx + SXF;
      float* nst = smem + ((k + 1) & 1) * GSTAGE;
      GSTAMP(0);
      if (ndef > 0) {
        __builtin_amdgcn_sched_barrier(0);
        held_back();
        __builtin_amdgcn_sched_barrier(0);
      }
      GSTAMP(1);
      // D' operands: raw dY rows of channel block nb -> b4 of the two positions.  The operands of block nb+1 are formed and
      // the rows of block nb+2 requested WHILE the MFMAs of block nb issue (interleaved below): the two waves of a SIMD
      // take turns on the matrix pipe and so drift into the same phase -- operand building in a phase of its own would leave
      // the pipe idle in both at once.
      f32x4 rd[2][2];  // [row][x quad]
      auto read_d = [&](int nb, f32x4 (&d)[2][2]) {
        const int doff = (dr1 * GCO + nb * 32 + lr) * XS + 8 * lh;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          d[0][c] = *reinterpret_cast<const f32x4*>(&cy[doff + 4 * c]);
          if (two) d[1][c] = *reinterpret_cast<const f32x4*>(&cy[doff + GCO * XS + 4 * c]);
        }
      };
      auto build_b = [&](const f32x4 (&d)[2][2], f32x4 (&b4)[2]) {
        float rc[8];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) rc[4 * c + e] = !two ? d[0][c][e] : (vplus ? d[0][c][e] + d[1][c][e] : d[0][c][e] - d[1][c][e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (jhc == 0) {
            b4[0][e] = rc[2 * e];
            b4[1][e] = rc[2 * e] + rc[2 * e + 1];
          } else {
            b4[0][e] = rc[2 * e] - rc[2 * e + 1];
            b4[1][e] = rc[2 * e + 1];
          }
        }
      };
      // V fragments of the two positions: 12 x values of the two rows, combined
      {
        f32x4 u1[3], u2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          u1[c] = *reinterpret_cast<const f32x4*>(&cx[voff1 + 4 * c]);
          u2[c] = *reinterpret_cast<const f32x4*>(&cx[voff2 + 4 * c]);
        }
        float rc[12];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) rc[4 * c + e] = vplus ? u1[c][e] + u2[c][e] : u1[c][e] - u2[c][e];
        __builtin_amdgcn_sched_barrier(0);
        read_d(0, rd);  // (after the row combination: its 24 input registers are free again)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (jhc == 0) {
            a4[0][e] = rc[2 * e] - rc[2 * e + 2];
            a4[1][e] = rc[2 * e + 1] + rc[2 * e + 2];
          } else {
            a4[0][e] = rc[2 * e + 2] - rc[2 * e + 1];
            a4[1][e] = rc[2 * e + 1] - rc[2 * e + 3];
          }
        }
        build_b(rd, bb[0]);
        read_d(1, rd);
      }
      if (!(VAE_ABLATE & 2) && wave < 4) store_unit(nst, cur);  // the two waves of a SIMD store at opposite ends of the step
      GSTAMP(2);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        __builtin_amdgcn_sched_barrier(0);
        if (nb == 1) {  // the requests for unit k+2 (index counters + 4 loads) behind the first block's MFMAs, not in front of the
          // step, where both waves of a SIMD build operands and the matrix pipe has nothing to do (2.1-2.7 % of the kernel)
          if (!(VAE_ABLATE & 1)) load_unit(k + 2, nxt);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (nb == 3 && wave >= 4) {  // (waves 4..7: the LDS stores of unit k+1 behind the third block's MFMAs, not between the last MFMA and the barrier)
          if (!(VAE_ABLATE & 2)) store_unit(nst, cur);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (nb < 3) build_b(rd, bb[(nb + 1) & 1]);  // block nb+1's operands, during the first half of this block's MFMAs
        if (nb < 2) read_d(nb + 2, rd);             // block nb+2's rows into the same registers, during the second half
        if (nb < 4 - ndef) {  // (a held-back block: its operands are built here, its MFMAs open the next step)
#pragma unroll
          for (int pi = 0; pi < 2; ++pi)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[pi][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[pi][e], bb[nb & 1][pi][e], acc[pi][nb], 0, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);  // VALU
          }
          __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // DS read
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (nb == 3 - ndef) GSTAMP(3);
      }
      GSTAMP(4);
      GSTAMPS_OUT(k);
      if (!(VAE_ABLATE & 16)) __syncthreads();
    };
    int k = 0;
    for (; k + 1 < nu; k += 2) {
      step(k, s1, s0);
      step(k + 1, s0, s1);
    }
    if (k < nu) step(k, s1, s0);
    if (ndef > 0 && nu > 0) held_back();  // the last step's (a split without units has none and writes its zero slab)
  };
#if VAE_WGRAD_PRIO  // one static s_setprio around the loop, no flips inside; a scalar condition: the instruction ignores EXEC
  if (__builtin_amdgcn_readfirstlane(tid) >= 256) __builtin_amdgcn_s_setprio(1);
#endif
  {
    using J0 = std::integral_constant<int, 0>;
    using J1 = std::integral_constant<int, 1>;
    switch (wave) {  // (wave-uniform: wi = wave / 2, jh = wave % 2)
      case 0: run(std::integral_constant<int, 0>{}, J0{}); break;
      case 1: run(std::integral_constant<int, 0>{}, J1{}); break;
      case 2: run(std::integral_constant<int, 1>{}, J0{}); break;
      case 3: run(std::integral_constant<int, 1>{}, J1{}); break;
      case 4: run(std::integral_constant<int, 2>{}, J0{}); break;
      case 5: run(std::integral_constant<int, 2>{}, J1{}); break;
      case 6: run(std::integral_constant<int, 3>{}, J0{}); break;
      default: run(std::integral_constant<int, 3>{}, J1{}); break;
    }
  }
#if VAE_WGRAD_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif

#ifdef VAE_WGRAD_TIMING
  if (tw) {
    tout[0] = te0;
    tout[1] = __builtin_amdgcn_s_memtime();
    tout[2] = tr0;
    tout[3] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  // ---- epilogue: slab [split][16 positions][Cin][Cout]; lanes along co (128-byte rows) ----
  float* __restrict__ O = p.partial + (int64_t)split * 16 * p.N * p.M;
  wino::slab_store<4>(O, wi * 4 + 2 * jh, p.N, p.M, n0, m0, 0, acc[0], lr, lh);  // the wave's two positions
  wino::slab_store<4>(O, wi * 4 + 2 * jh + 1, p.N, p.M, n0, m0, 0, acc[1], lr, lh);
  if (do_bias) wino::bias_tail(bsum, xx, p.bias_partial, (int64_t)split * p.M + m0 + 4 * yq);  // workgroup-uniform
}

#else  // ---- split-bf16 products: two units (K = 16 tiles) per step ----
// The K = 16 of v_mfma_f32_32x32x16_bf16 is two units: a split's unit range is walked in pairs (an odd last unit is paired with
// the zeros load_unit delivers beyond the range).  Both units are staged as in the exact loop, each in a stage of its own
// ([pair parity][unit of the pair][GSTAGE], 120 KB of dynamic LDS), and every LDS access is the exact loop's at a uniform offset:
// the bank-conflict freedom of the [row][channel][x] image carries over unchanged.  A lane half's eight k are the four tiles
// it takes in the exact loop, of the pair's first unit (k 0..3) and of its second (k 4..7), in the V and in the D' operand alike.
// The transforms stay in fp32; their results are split into three bf16 planes in registers (split3, bf16_frag.h) and a product is
// the six plane products of mma_x3_term, smallest first, into the fp32 accumulator: 48 MFMAs of 32 cycles per wave and pair
// against 64 of 64 cycles.  The split is vector work (about 5.5 instructions per value, 80 values per lane and pair: 650 vector
// instructions per wave and step beside the 48 MFMAs), and vector issue, not the matrix pipe, now bounds the loop: a step of two
// units takes 7800-7900 cycles against 2 x 5300-5430 of the exact loop.
constexpr int GPAIR = 2 * GSTAGE;                  // the two stages of a pair of units
constexpr int GLDS = 2 * GPAIR * (int)sizeof(float);  // double buffered: 122880 B
extern __shared__ __attribute__((aligned(16))) float wgrad_lds[];

template <int XF>
__global__ __launch_bounds__(GNT, 1) void wgrad3_wino_kernel(vae_wgrad_args p, int strips, int64_t nunits) {
  float* const smem = wgrad_lds;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const vae_conv_geom g = p.g;
  const int tilesN = p.N / GCI, ntile = tilesN * (p.M / GCO);
  const wino::SplitTile wg = wino::split_tile_of_workgroup<true>(blockIdx.x, p.nsplit, ntile);  // (with the rule for 2 and 4 splits)
  const int tile = wg.tile, split = wg.split;
  const int tm = tile / tilesN, tn = tile % tilesN;
  const int m0 = tm * GCO, n0 = tn * GCI;
  const wino::UnitRange ur = wino::unit_range(nunits, p.nsplit, split);
  const int64_t ubeg = ur.ubeg;
  const int nu = ur.nu;
  const int upi = (g.Ho / 2) * strips;  // units per image
  const bool do_bias = (p.bias_partial != nullptr) && tn == 0;
#ifdef VAE_WGRAD_TIMING  // debug build (tools/wgrad_timing.py): shader-clock stamps of waves 0 and 4 (the two waves of SIMD 0) of workgroups 0..7 -> p.out,
  // which this kernel otherwise never touches: [workgroup][wave / 4][4 + TSN * 5] uint64 = entry, loop exit, 100 MHz clock at both; per step (a pair
  // of units) TS0.. : begin (barrier released), the same again (the exact loop's deferred MFMAs), first block's operands built (first own MFMA), last MFMA issued, barrier reached
  constexpr int TS0 = 2, TSN = 8;
  const bool tw = (tid & 255) == 0 && blockIdx.x < 8 && p.out != nullptr;
  unsigned long long* const tout = reinterpret_cast<unsigned long long*>(p.out) + (blockIdx.x * 2 + (tid >> 8)) * (4 + TSN * 5);
  unsigned long long tst[5];
  const unsigned long long te0 = __builtin_amdgcn_s_memtime(), tr0 = __builtin_amdgcn_s_memrealtime();
#define GSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); tst[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define GSTAMPS_OUT(k) do { if (tw && (k) >= TS0 && (k) < TS0 + TSN) { _Pragma("unroll") for (int i_ = 0; i_ < 5; ++i_) tout[4 + ((k) - TS0) * 5 + i_] = tst[i_]; } } while (0)
#else
#define GSTAMP(i) do { } while (0)
#define GSTAMPS_OUT(k) do { } while (0)
#endif

  // ---- staging roles, per unit as in the exact loop.  X halo: thread -> (row xr, channel quad xq, column xx) of the 4 x 16 main
  // block, threads with (tid & 8) == 0 && tid < 128 also one element of the two extra columns (same channel quad: shared
  // GroupNorm rows).  Lanes run along x (16) and 4 channel quads: the four 4-byte LDS writes of a loaded float4 are conflict-free ----
  const int xx = tid & 15, xq = (tid >> 4) & 7, xr = tid >> 7;
  const bool xe_role = tid < 128 && (tid & 8) == 0;
  const int ex = 16 + (tid & 1), er = (tid >> 1) & 3;
  // dY strip: thread -> (column xx, channel quad yq) for both rows
  const int yq = tid >> 4;
  const auto rsX = VAE_BUF_RSRC(p.X, (size_t)g.B * g.Hs * g.Ws * g.Cs * 4u);
  const auto rsY = VAE_BUF_RSRC(p.dY, (size_t)g.B * g.Ho * g.Wo * p.ldy * 4u);
  const auto rsS = VAE_BUF_RSRC(p.scale, (size_t)g.B * g.Cs * 4u);  // GroupNorm rows [B][Cs] (XF != none only)
  const auto rsH = VAE_BUF_RSRC(p.shift, (size_t)g.B * g.Cs * 4u);
  // One set of staging registers per unit of a pair: a wave stores pair k+1 during step k and requests pair k+2 right behind
  // the stores, into the same registers, so the requests have a whole step in flight wherever in the step the wave stores.
  struct Stg {
    f32x4 rx, rxe, ry[2];
    int b, uf;  // image and border flags of the unit (workgroup-uniform: scalar registers)
  };
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  Stg s0{z4, z4, {z4, z4}, -1, 16}, s1 = s0;
  f32x4 bsum = z4;
  // GroupNorm rows of the thread's channel quad for image sc_b: one set, re-read when a stored unit belongs to the next image.
  // The units are stored in ascending order, so a pair whose units lie in two images re-reads the rows between its two stores.
  f32x4 rsc = {1.f, 1.f, 1.f, 1.f}, rsh = z4;
  int sc_b = -1;
  // the unit the next load_unit call requests (calls go through ubeg, ubeg+1, ...: counters instead of divisions per step)
  int ub = (int)(ubeg / upi), uty = (int)((ubeg - (int64_t)ub * upi) / strips), ustrip = (int)((ubeg - (int64_t)ub * upi) % strips);
  // Addresses = a workgroup-uniform part (scalar registers) + a per-thread constant; an element is padding when one of the
  // thread's position flags meets the unit's border flag (bit 0: first halo row / top border, 1: last halo row / bottom border,
  // 2: first halo column / left border, 3: last halo column / right border, 4: always / unit beyond the range).
  const unsigned thrX = ((xr * g.Ws + xx) * g.Cs + n0 + 4 * xq) * 4u, thrE = ((er * g.Ws + ex) * g.Cs + n0 + 4 * xq) * 4u;
  const unsigned thrY = (xx * p.ldy + m0 + 4 * yq) * 4u, rowY = (unsigned)g.Wo * p.ldy * 4u;
  const int tfX = (xr == 0 ? 1 : 0) | (xr == 3 ? 2 : 0) | (xx == 0 ? 4 : 0) | 16;
  const int tfE = xe_role ? ((er == 0 ? 1 : 0) | (er == 3 ? 2 : 0) | (ex == 17 ? 8 : 0) | 16) : 31;
  auto load_unit = [&](int k, Stg& r) __attribute__((always_inline)) {  // requests for unit ubeg + k (beyond the range: nothing is read, zeros)
    const bool ok = k < nu;
    const int b = ub, ty = uty, x0 = ustrip * 16;
    if (++ustrip == strips) {
      ustrip = 0;
      if (++uty == g.Ho / 2) {
        uty = 0;
        ++ub;
      }
    }
    r.b = ok ? b : -1;
    const int uf = (ty == 0 ? 1 : 0) | (2 * ty + 2 >= g.Hs ? 2 : 0) | (x0 == 0 ? 4 : 0) | (x0 + 16 >= g.Ws ? 8 : 0) | (ok ? 0 : 16);
    // (the halo origin may lie before the tensor: unsigned arithmetic wraps, the sum with the thread's part is exact)
    const unsigned baseX = (unsigned)((b * g.Hs + 2 * ty - 1) * g.Ws + x0 - 1) * (unsigned)g.Cs * 4u;
    const unsigned baseY = (unsigned)((b * g.Ho + 2 * ty) * g.Wo + x0) * (unsigned)p.ldy * 4u;
    r.uf = uf;  // (the stores ask the flags again: two lane masks per unit would stay live for a step)
    r.rx = VAE_BUF_LOAD4(rsX, (tfX & uf) == 0 ? baseX + thrX : BUF_OOB);
    r.rxe = VAE_BUF_LOAD4(rsX, (tfE & uf) == 0 ? baseX + thrE : BUF_OOB);
#pragma unroll
    for (int a = 0; a < 2; ++a) r.ry[a] = VAE_BUF_LOAD4(rsY, ok ? baseY + a * rowY + thrY : BUF_OOB);
  };
  auto xform = [&](f32x4 v, bool in) {
    if (XF != VAE_XF_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float u = v[e] * rsc[e] + rsh[e];
        if (XF == VAE_XF_AFFINE_SILU) u = silu_f(u);
        v[e] = in ? u : 0.f;  // padding stays zero AFTER the transform
      }
    }
    return v;
  };
  auto store_unit = [&](float* st, const Stg& r) __attribute__((always_inline)) {
    float* sx = st;
    float* sy = st + SXF;
    if (XF != VAE_XF_NONE && r.b >= 0 && r.b != sc_b) {  // workgroup-uniform
      sc_b = r.b;
      const unsigned at = (unsigned)(sc_b * g.Cs + n0 + 4 * xq) * 4u;  // (through descriptors: no per-thread pointers live across the loop)
      rsc = VAE_BUF_LOAD4(rsS, at);
      rsh = VAE_BUF_LOAD4(rsH, at);
    }
    const f32x4 v = xform(r.rx, (tfX & r.uf) == 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) sx[(xr * GCI + 4 * xq + e) * XS + xx] = v[e];
    if (xe_role) {
      const f32x4 ve = xform(r.rxe, (tfE & r.uf) == 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) sx[(er * GCI + 4 * xq + e) * XS + ex] = ve[e];
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sy[(a * GCO + 4 * yq + e) * XS + xx] = r.ry[a][e];
      if (do_bias) bsum += r.ry[a];
    }
  };
  // pair kp -> its two stages, then the requests for pair kp + 1 (inlined at every call: a call would pass the captures through scratch)
  auto stage_pair = [&](float* st, int kp) __attribute__((always_inline)) {
    if (!(VAE_ABLATE & 2)) {
      store_unit(st, s0);
      store_unit(st + GSTAGE, s1);
    }
    if (!(VAE_ABLATE & 1)) {
      load_unit(2 * kp + 2, s0);
      load_unit(2 * kp + 3, s1);
    }
  };

  // ---- operand roles: wave -> row i of the transform domain and the column pair (2 jh, 2 jh + 1) ----
  const int wi = wave >> 1, jh = wave & 1;
  // V row combination: B^T row i = x[r1] + sg * x[r2]
  const int vr1 = wi == 0 ? 0 : (wi == 2 ? 2 : 1), vr2 = wi == 0 ? 2 : (wi == 1 ? 2 : (wi == 2 ? 1 : 3));
  const int voff1 = (vr1 * GCI + lr) * XS + 8 * lh, voff2 = (vr2 * GCI + lr) * XS + 8 * lh;
  // D' row combination: i = 0: dy row 0, 3: row 1, 1: row0 + row1, 2: row0 - row1
  const int dr1 = wi == 3 ? 1 : 0;

  f32x16 acc[2][4];
#pragma unroll
  for (int pi = 0; pi < 2; ++pi)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[pi][nb][e] = 0.f;

  load_unit(0, s0);
  load_unit(1, s1);
  stage_pair(smem, 0);  // pair 0 to LDS, pair 1 requested
  __syncthreads();
  const int np = (nu + 1) / 2;  // steps

  // The loop body is instantiated per (two-row D combination?, column pair): straight-line code, no per-step branches.
  auto run = [&](auto WI, auto JH) {
    constexpr int wic = decltype(WI)::value, jhc = decltype(JH)::value;
    constexpr bool two = wic == 1 || wic == 2;  // D' row i combines both dY rows
    constexpr bool vplus = wic == 1;            // sign of the second row in the combinations (V: B^T row i, D': G' row i)
    // All eight waves run one program.  Holding waves 4..7's last block back by a step (the exact loop's stagger) measured
    // 0-1.4 % SLOWER here: the loop is bound by vector issue, not by the matrix pipe (profiles/wgrad_x3_measured.json).
    Bf3 a3[2], bb[2];  // V operands of the two positions; D' operands of the channel block at hand
    auto mma = [&](auto NB) {  // block nb: 12 MFMAs, the two accumulators alternate
      constexpr int nb = decltype(NB)::value;
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) acc[pi][nb] = mma_x3_term(t, a3[pi].p, bb[pi].p, acc[pi][nb]);
    };
    auto step = [&](int kp) {
      const float* cst = smem + (kp & 1) * GPAIR;
      float* nst = smem + ((kp + 1) & 1) * GPAIR;
      GSTAMP(0);
      GSTAMP(1);  // (no held-back MFMAs in this loop: tools/wgrad_timing.py reads a `held` segment of zero)
      // V operands of the two positions: per unit 12 x values of the two rows, combined; then the split
      {
        f32x4 af[2][2];  // [unit][position]
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float* cx = cst + u * GSTAGE;
          f32x4 u1[3], u2[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            u1[c] = *reinterpret_cast<const f32x4*>(&cx[voff1 + 4 * c]);
            u2[c] = *reinterpret_cast<const f32x4*>(&cx[voff2 + 4 * c]);
          }
          float rc[12];
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) rc[4 * c + e] = vplus ? u1[c][e] + u2[c][e] : u1[c][e] - u2[c][e];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (jhc == 0) {
              af[u][0][e] = rc[2 * e] - rc[2 * e + 2];
              af[u][1][e] = rc[2 * e + 1] + rc[2 * e + 2];
            } else {
              af[u][0][e] = rc[2 * e + 2] - rc[2 * e + 1];
              af[u][1][e] = rc[2 * e + 1] - rc[2 * e + 3];
            }
          }
        }
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) a3[pi] = split8(af[0][pi], af[1][pi]);
      }
      if (wic < 2) stage_pair(nst, kp + 1);  // the two waves of a SIMD store at opposite ends of the step
      __builtin_amdgcn_sched_barrier(0);
      // D' operands of channel block nb: per unit the raw dY rows -> the fp32 values of the two positions; then the split.
      // No scheduling barrier between the blocks: block nb+1's LDS reads and additions may move up between block nb's MFMAs.
      auto block = [&](auto NB) {
        constexpr int nb = decltype(NB)::value;
        if (nb == 3 && wic >= 2) {  // (waves 4..7: the LDS stores of pair kp+1 in front of the last block, not between the last MFMA and the barrier)
          __builtin_amdgcn_sched_barrier(0);
          stage_pair(nst, kp + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 bf[2][2];  // [unit][position]
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float* cy = cst + u * GSTAGE + SXF;
          const int doff = (dr1 * GCO + nb * 32 + lr) * XS + 8 * lh;
          f32x4 d[2][2];  // [row][x quad]
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            d[0][c] = *reinterpret_cast<const f32x4*>(&cy[doff + 4 * c]);
            if (two) d[1][c] = *reinterpret_cast<const f32x4*>(&cy[doff + GCO * XS + 4 * c]);
          }
          float rc[8];
#pragma unroll
          for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) rc[4 * c + e] = !two ? d[0][c][e] : (vplus ? d[0][c][e] + d[1][c][e] : d[0][c][e] - d[1][c][e]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (jhc == 0) {
              bf[u][0][e] = rc[2 * e];
              bf[u][1][e] = rc[2 * e] + rc[2 * e + 1];
            } else {
              bf[u][0][e] = rc[2 * e] - rc[2 * e + 1];
              bf[u][1][e] = rc[2 * e + 1];
            }
          }
        }
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) bb[pi] = split8(bf[0][pi], bf[1][pi]);
        if (nb == 0) GSTAMP(2);
        mma(NB);
        if (nb == 3) GSTAMP(3);
      };
      block(std::integral_constant<int, 0>{});
      block(std::integral_constant<int, 1>{});
      block(std::integral_constant<int, 2>{});
      block(std::integral_constant<int, 3>{});
      GSTAMP(4);
      GSTAMPS_OUT(kp);
      if (!(VAE_ABLATE & 16)) __syncthreads();
    };
    for (int kp = 0; kp < np; ++kp) step(kp);
  };
#if VAE_WGRAD_PRIO  // one static s_setprio around the loop, no flips inside; a scalar condition: the instruction ignores EXEC
  if (__builtin_amdgcn_readfirstlane(tid) >= 256) __builtin_amdgcn_s_setprio(1);
#endif
  {
    using J0 = std::integral_constant<int, 0>;
    using J1 = std::integral_constant<int, 1>;
    switch (wave) {  // (wave-uniform: wi = wave / 2, jh = wave % 2)
      case 0: run(std::integral_constant<int, 0>{}, J0{}); break;
      case 1: run(std::integral_constant<int, 0>{}, J1{}); break;
      case 2: run(std::integral_constant<int, 1>{}, J0{}); break;
      case 3: run(std::integral_constant<int, 1>{}, J1{}); break;
      case 4: run(std::integral_constant<int, 2>{}, J0{}); break;
      case 5: run(std::integral_constant<int, 2>{}, J1{}); break;
      case 6: run(std::integral_constant<int, 3>{}, J0{}); break;
      default: run(std::integral_constant<int, 3>{}, J1{}); break;
    }
  }
#if VAE_WGRAD_PRIO
  __builtin_amdgcn_s_setprio(0);
#endif

#ifdef VAE_WGRAD_TIMING
  if (tw) {
    tout[0] = te0;
    tout[1] = __builtin_amdgcn_s_memtime();
    tout[2] = tr0;
    tout[3] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  // ---- epilogue: slab [split][16 positions][Cin][Cout]; lanes along co (128-byte rows) ----
  float* __restrict__ O = p.partial + (int64_t)split * 16 * p.N * p.M;
  wino::slab_store<4>(O, wi * 4 + 2 * jh, p.N, p.M, n0, m0, 0, acc[0], lr, lh);  // the wave's two positions
  wino::slab_store<4>(O, wi * 4 + 2 * jh + 1, p.N, p.M, n0, m0, 0, acc[1], lr, lh);
  if (do_bias) wino::bias_tail(bsum, xx, p.bias_partial, (int64_t)split * p.M + m0 + 4 * yq);  // workgroup-uniform
}
#endif  // VAE_WGRAD_X3

}  // namespace

// plain 3x3 stride-1 pad-1 layer in fp32 with 16-pixel strips, 32 | Cin, 128 | Cout
bool wgrad3_wino_eligible(const vae_wgrad_args& a) {
  const vae_conv_geom& g = a.g;
  if (!wino::wgrad_eligible_common(a, GCI, GCO) || g.mode != VAE_MODE_FWD || g.Ho != g.Hs || g.Wo != g.Ws) return false;
  return g.Ho % 2 == 0 && g.Wo % 16 == 0;
}

int64_t wgrad3_wino_units(const vae_conv_geom& g) { return (int64_t)g.B * (g.Ho / 2) * (g.Wo / 16); }

int launch_wgrad3_wino(const vae_wgrad_args& a, hipStream_t st) {
  const vae_conv_geom& g = a.g;
  const int64_t nunits = wgrad3_wino_units(g);
  dim3 grid((unsigned)((a.M / GCO) * (a.N / GCI) * a.nsplit), 1, 1);
  const int strips = g.Wo / 16;
#if VAE_WGRAD_X3  // (more than 64 KB of dynamic LDS: reserved once per instantiation and device)
  int rc = 0;
  dispatch_xf_or_silu(a.xf, [&](auto xf) {
    constexpr int XF = decltype(xf)::value;
    rc = [&]() -> int { VAE_RESERVE_LDS(wgrad3_wino_kernel<XF>, GLDS, "wgrad3_wino"); return 0; }();
    if (rc == 0) hipLaunchKernelGGL(wgrad3_wino_kernel<XF>, grid, dim3(GNT), GLDS, st, a, strips, nunits);
  });
  return rc;
#else
  dispatch_xf_or_silu(a.xf, [&](auto xf) { hipLaunchKernelGGL(wgrad3_wino_kernel<decltype(xf)::value>, grid, dim3(GNT), 0, st, a, strips, nunits); });
  return 0;
#endif
}
