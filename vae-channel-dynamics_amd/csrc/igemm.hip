// Flat implicit-GEMM convolution / GEMM family: the kernels behind every geometry no specialised kernel serves (stride-2
// convolutions and their parity-class dgrad, 1x1, tiny and ragged maps, attention linears and batched GEMMs, skinny layers).
//
// Three operand forms cover every contraction of the SDXL-VAE train step:
//   rows   (A rows = pixels gathered through the conv geometry; A tile [BM rows][BK k], k-contiguous)
//     - weight tile k-contiguous ([BN][BK])              : conv/linear forward, Q.K^T, dO.V^T
//     - weight tile n-contiguous ([BK][BN], BKM = true)  : conv/linear dgrad, P.V, dS.K
//   wgrad  (contraction over pixels; both tiles pixel-major, [BK px][BM] and [BK px][BN]) : conv/linear wgrad, P^T.dO, dS^T.Q
//
// There is ONE rows body and ONE wgrad body.  Each is instantiated under three arithmetic policies:
//   F32  (VAE_PREC_F32): exact fp32 products, fp32 accumulate, on v_mfma_f32_32x32x2_f32.  Serves any shape: the unvectorised
//         instantiations (VEC = false) load element by element.  Also the vectorised 4-wave skinny tiles (128 x 32, 32 x 128).
//   F32X3 (VAE_PREC_F32, VEC = true, the 8-wave 128 x 128 tile): fp32 operands and results, but NOT exact fp32 products: every
//         operand value is split into three bf16 planes while staged in LDS and a product is six bf16 plane products on
//         v_mfma_f32_32x32x16_bf16, fp32 accumulate (<= 2^-25 of |a b| per product; the matrix pipe is busy 2.67 x shorter than
//         with the fp32 MFMA).  A finite operand in the top 2^-8 of the fp32 range rounds to Inf in its first plane; Inf / NaN
//         stay non-finite (see the policy).  -DVAE_FLAT_X3=0 puts these instantiations back on F32 (the A/B arm: the bits of
//         exact fp32 products).
//   BF16 (VAE_PREC_BF16): operands rounded to bf16 while staged in LDS, products on v_mfma_f32_32x32x16_bf16, fp32 accumulate.
//         Every activation operand is stored as fp32 or as bf16, per tensor (a_bf16 / out_bf16 / res_bf16, x_bf16 / y_bf16:
//         wave-uniform switches on the load / store instructions; the weights W are always the fp32 master copy).  Only the
//         vectorised shapes (16-B aligned, channel counts % 4 == 0) exist; the rest stays on the F32 kernels.
// A policy holds what really differs (LDS element, K step, paddings, staging conversion, fragment reads, the MFMA block, the
// epilogue's element access); the bodies ask it for a type, a constant or a small function and never which policy it is.
//
// Tiling: 64*WM*WN threads (8 waves for the 128x128 tile, 4 for the skinny ones), wave tile = (BM/WM) x (BN/WN) built from
// 32x32 MFMA tiles.  Global loads of step s+2 are issued, and the registers of step s+1 written to the other LDS stage, in
// the middle of step s's MFMA block (register-staged prefetch); GroupNorm+SiLU is applied to the activation operand in that
// write pass, so the normalised activation never exists in HBM.
#include "bf16_frag.h"
#include <algorithm>
#include <stdlib.h>
#include <type_traits>

#include "launchers.h"

namespace {

// ---------------------------------------------------------------------------------------
// arithmetic policies
// ---------------------------------------------------------------------------------------
// a lane's coordinates in the fragment reads.  lr / lh: row (or column) and k half of the MFMA operand layout;
// trq / trp / trh: row, column quad and column half this lane addresses in a 16-lane group's transposing read (bf16_frag.h)
struct LanePos {
  int lr, lh, trq, trp, trh;
};
__device__ __forceinline__ LanePos lane_pos(int lane) { return LanePos{lane & 31, lane >> 5, (lane & 15) >> 2, lane & 3, (lane >> 4) & 1}; }

struct F32 {
  typedef float elem;    // LDS element
  typedef f32x4 raw4;    // what a 16-byte operand load lands in
  typedef f32x4 frag;    // this lane half's 4 consecutive k of a k-group: element j feeds MFMA j (k = 2, one per lane half)
  typedef unsigned off_t;  // epilogue element handle: byte offset, BUF_OOB = outside the matrix
  static constexpr int BK_ROWS = 32, BK_WGRAD = 32;  // K step (channels / pixels)
  static constexpr int KG = 8;                       // k per k-group
  // LDS row paddings (elements).  Row stride 36 dwords: 36*i mod 64 hits 16 distinct 16-B slots for the 16 rows of a b128
  // lane group, so every ds_read_b128 fragment read is bank-conflict free; the transposing (dword) reads of the [k][col]
  // tiles take the same 4.
  static constexpr int PAD_K = 4, PAD_T = 4;
  static constexpr bool SETPRIO = true;  // s_setprio brackets the MFMA block
  static constexpr bool PAIR16 = false;
  // An operand tile is PLANES images of the tile in LDS, a plane stride apart (the stride is the body's: one tile); the staging
  // and fragment functions take that stride.  One plane here.  LDS_DYNAMIC: the stages are the kernel's dynamic LDS, which the
  // launcher sizes (rows_lds_elems / wgrad_lds_elems) and reserves (VAE_RESERVE_LDS); else a static array of the body.
  static constexpr int PLANES = 1;
  static constexpr bool LDS_DYNAMIC = false;
  static constexpr bool flag(int32_t) { return false; }  // operands and results are fp32: no storage switch exists

  static __device__ __forceinline__ raw4 load4(__amdgpu_buffer_rsrc_t rs, unsigned, bool ok, int row, int ld, int c) {
    return VAE_BUF_LOAD4(rs, oob_unless(ok, ((unsigned)row * (unsigned)ld + (unsigned)c) * 4u));
  }
  static __device__ __forceinline__ f32x4 to_f32(raw4 r, bool) { return r; }
  static __device__ __forceinline__ void put4(elem* d, f32x4 v, int) { *reinterpret_cast<f32x4*>(d) = v; }
  static __device__ __forceinline__ void put4_stored(elem* d, raw4, f32x4 v, bool, int) { put4(d, v, 0); }
  // 4 consecutive k at p (one ds_read_b128)
  static __device__ __forceinline__ frag frag_k(const elem* p, int) { return *reinterpret_cast<const f32x4*>(p); }
  // the same 4 k of k-group kg from a [k][col] tile: this lane's column of the 32 from col0
  static __device__ __forceinline__ frag frag_t(const elem* tile, int ld, int kg, LanePos l, int col0, int) {
    frag v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = tile[(kg * 8 + l.lh * 4 + j) * ld + col0 + l.lr];
    return v;
  }
  // both operands from [k][col] tiles (wgrad), MI / NI fragments from columns colA / colB on.  The a and b reads alternate
  // per k row: the compiler's pairing of the dword reads, and with it the register count, follows the source order.
  template <int MI, int NI>
  static __device__ __forceinline__ void frags_tt(frag* a, frag* b, const elem* sA, int ldA, int colA, const elem* sB, int ldB, int colB, int kg, LanePos l,
                                                  int, int) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kg * 8 + l.lh * 4 + j;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi][j] = sA[k * ldA + colA + mi * 32 + l.lr];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b[ni][j] = sB[k * ldB + colB + ni * 32 + l.lr];
    }
  }
  template <int MI, int NI>
  static __device__ __forceinline__ void mma(f32x16 (&acc)[MI][NI], const frag* a, const frag* b) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi][j], b[ni][j], acc[mi][ni], 0, 0, 0);
  }
  static __device__ __forceinline__ off_t out_off(bool ok, int orow, int ldc, int col) {
    return ok ? ((unsigned)orow * (unsigned)ldc + (unsigned)col) * 4u : BUF_OOB;
  }
  static __device__ __forceinline__ bool inside(off_t o) { return o != BUF_OOB; }
  static __device__ __forceinline__ float load1(__amdgpu_buffer_rsrc_t rs, bool, off_t o) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, o, 0, 0));
  }
  static __device__ __forceinline__ void store1(__amdgpu_buffer_rsrc_t rs, bool, off_t o, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, o, 0, 0);
  }
};

struct BF16 {
  typedef u16 elem;
  typedef uint4 raw4;    // as loaded (fp32 quad, or 4 bf16 in the low half): converted at the LDS write
  typedef bf16x8 frag;   // 8 k per lane half: one MFMA of k = 16 per k-group
  typedef int off_t;     // epilogue element handle: element offset (C and res may differ in storage), -1 = outside the matrix
  static constexpr int BK_ROWS = 64, BK_WGRAD = 32;
  static constexpr int KG = 16;
  // k-contiguous rows: 144 B row stride, conflict-free ds_read_b128.  [k][col] rows: 64 B mod 256 B row strides put the four
  // rows of a transposing read's block in different bank ranges (bf16_frag.h).
  static constexpr int PAD_K = 8, PAD_T = 32;
  static constexpr bool SETPRIO = false;
  static constexpr bool PAIR16 = true;  // the rows epilogue has the paired 4-byte bf16 store
  static constexpr int PLANES = 1;
  static constexpr bool LDS_DYNAMIC = false;
  static __device__ __forceinline__ bool flag(int32_t v) { return v != 0; }  // storage of an operand / result (uniform)

  static __device__ __forceinline__ raw4 load4(__amdgpu_buffer_rsrc_t rs, unsigned esize, bool ok, int row, int ld, int c) {
    return buf_load4_raw(rs, esize, neg_unless(ok, row * ld + c));
  }
  static __device__ __forceinline__ f32x4 to_f32(raw4 r, bool bf) { return raw4_to_f32(r, bf); }
  static __device__ __forceinline__ void put4(elem* d, f32x4 v, int) { *reinterpret_cast<uint2*>(d) = pack4(v); }
  // an operand that is staged untransformed and already stored as bf16 goes to LDS as loaded
  static __device__ __forceinline__ void put4_stored(elem* d, raw4 r, f32x4 v, bool bf, int) {
    *reinterpret_cast<uint2*>(d) = bf ? uint2{r.x, r.y} : pack4(v);
  }
  static __device__ __forceinline__ frag frag_k(const elem* p, int) { return frag_direct(p); }
  static __device__ __forceinline__ frag frag_t(const elem* tile, int ld, int kg, LanePos l, int col0, int) {
    return frag_tr(tile + (kg * 16 + l.lh * 8 + l.trq) * ld + col0 + l.trh * 16 + l.trp * 4, ld);
  }
  template <int MI, int NI>
  static __device__ __forceinline__ void frags_tt(frag* a, frag* b, const elem* sA, int ldA, int colA, const elem* sB, int ldB, int colB, int kg, LanePos l,
                                                  int, int) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) a[mi] = frag_t(sA, ldA, kg, l, colA + mi * 32, 0);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) b[ni] = frag_t(sB, ldB, kg, l, colB + ni * 32, 0);
  }
  template <int MI, int NI>
  static __device__ __forceinline__ void mma(f32x16 (&acc)[MI][NI], const frag* a, const frag* b) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  }
  static __device__ __forceinline__ off_t out_off(bool ok, int orow, int ldc, int col) { return ok ? orow * ldc + col : -1; }
  static __device__ __forceinline__ bool inside(off_t o) { return o >= 0; }
  static __device__ __forceinline__ float load1(__amdgpu_buffer_rsrc_t rs, bool bf, off_t o) { return buf_load1_elem(rs, bf, o); }
  static __device__ __forceinline__ void store1(__amdgpu_buffer_rsrc_t rs, bool bf, off_t o, float v) { buf_store1_elem(rs, bf, o, v); }

  // bf16 output with an even column count (and a bf16 residual or none): adjacent lanes hold adjacent columns of the same 16
  // rows; they swap every other register, so a lane stores BOTH columns of its pair for 8 rows -- 4-byte stores and 4-byte
  // residual loads instead of 2-byte ones (the 2-byte form cost the flat kernels 20 % when bf16 storage came in)
  static __device__ __forceinline__ bool pair16(const vae_igemm_args& p, bool cbf, bool rbf, const char* C) {
    return cbf && (p.N % 2 == 0) && (p.ldc % 2 == 0) && (p.res == nullptr || rbf) && p.track == nullptr && ((reinterpret_cast<uintptr_t>(C) & 3u) == 0);
  }
  // one 32-column block of a wave tile whose rows start at trow0 (lane half lh); row_pixel: the stride-2 dgrad's (s2c) row mapping
  template <int MI, int NI, class RowPixel>
  static __device__ __forceinline__ void store_pairs(const vae_igemm_args& p, const f32x16 (&acc)[MI][NI], int ni, __amdgpu_buffer_rsrc_t rsC,
                                                     __amdgpu_buffer_rsrc_t rsR, int col, bool colok, int m0, int trow0, int lh, bool s2c,
                                                     RowPixel row_pixel) {
    const bool odd = col & 1;
    const float b0 = (p.bias && colok) ? p.bias[col & ~1] : 0.f, b1 = (p.bias && colok) ? p.bias[col | 1] : 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      unsigned o16[8], rr[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = 2 * j + (odd ? 1 : 0);
        const int row = trow0 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        int orow = row;
        if (s2c) {
          int b, y, x;
          row_pixel(row < p.M ? row : m0, b, y, x);
          orow = (b * p.g.Ho + y) * p.g.Wo + x;
        }
        o16[j] = (colok && row < p.M) ? (unsigned)(orow * p.ldc + (col & ~1)) * 2u : BUF_OOB;
        rr[j] = 0u;
      }
      if (p.res) {  // uniform
#pragma unroll
        for (int j = 0; j < 8; ++j) rr[j] = __builtin_amdgcn_raw_buffer_load_b32(rsR, o16[j], 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a0 = p.alpha * acc[mi][ni][2 * j], a1 = p.alpha * acc[mi][ni][2 * j + 1];
        const float recv = lane_xor1(odd ? a0 : a1);
        typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
        bf16x2_t h;
        h[0] = (__bf16)((odd ? recv : a0) + b0 + __builtin_bit_cast(float, rr[j] << 16));
        h[1] = (__bf16)((odd ? a1 : recv) + b1 + __builtin_bit_cast(float, rr[j] & 0xffff0000u));
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h), rsC, o16[j], 0, 0);
      }
    }
  }
};

// F32X3: fp32 operands and results, products on the bf16 matrix pipe: each operand value a is staged as three bf16 planes
//   hi = bf16(a), mid = bf16(a - hi), lo = bf16((a - hi) - mid)      (round to nearest even; both subtractions are exact in fp32)
// so that hi + mid + lo = a up to 2^-26 |a|, and a.b is the sum of the six bf16 products that are not below 2^-24 |a.b|, added
// into the fp32 accumulator smallest first.  Everything outside LDS (loads, descriptors, transform, epilogue) is F32's; the LDS
// image and the fragment reads are BF16's, once per plane.  K step: at 32 the three planes of both 128-row tiles, double buffered,
// are 120 KB, one 8-wave workgroup per CU, and the kernels gained 1.3 x over exact fp32; at 16 (one k-group per step and barrier)
// they are 72 KB, TWO workgroups per CU as under F32, and the gain is 1.5 x (tools/flat_x3_ab.py, profiles/flat_x3_measured.json).
// The stages are dynamic LDS (62-78 KB by instantiation).  8-wave tiles only (F32For): a 4-wave loader pass covers 32 k.
// Non-finite and extreme operands: Inf and NaN stay non-finite (Inf - Inf makes the lower planes NaN, so a product that exact
// fp32 gives as Inf may come out NaN); a finite value in the top 2^-8 of the fp32 range rounds to Inf in the hi plane and then
// behaves like Inf; mid / lo planes that fall below the bf16 normal range may flush to zero, hi carries the value.
#ifndef VAE_FLAT_X3
#define VAE_FLAT_X3 1
#endif
struct F32X3 : F32 {
  typedef u16 elem;
  struct frag { bf16x8 p[3]; };  // 8 k per lane half of every plane
  static constexpr int BK_ROWS = 16, BK_WGRAD = 16;  // one k-group per step
  static constexpr int KG = 16;
  // k-contiguous rows: 48 B row stride, 3 i mod 16: distinct 16-B slots for the 16 rows of a b128 lane group, conflict-free
  // ds_read_b128.  [k][col] rows as BF16.
  static constexpr int PAD_K = 8, PAD_T = 32;
  static constexpr bool SETPRIO = false;
  static constexpr int PLANES = 3;
  static constexpr bool LDS_DYNAMIC = true;

  static __device__ __forceinline__ void put4(elem* d, f32x4 v, int ps) {
    uint2 hi, mid, lo;
    split3(v, hi, mid, lo);  // (bf16_frag.h)
    *reinterpret_cast<uint2*>(d) = hi;
    *reinterpret_cast<uint2*>(d + ps) = mid;
    *reinterpret_cast<uint2*>(d + 2 * ps) = lo;
  }
  static __device__ __forceinline__ void put4_stored(elem* d, raw4, f32x4 v, bool, int ps) { put4(d, v, ps); }
  static __device__ __forceinline__ frag frag_k(const elem* p, int ps) {
    frag f;
#pragma unroll
    for (int q = 0; q < 3; ++q) f.p[q] = BF16::frag_k(p + q * ps, 0);
    return f;
  }
  static __device__ __forceinline__ frag frag_t(const elem* tile, int ld, int kg, LanePos l, int col0, int ps) {
    frag f;
#pragma unroll
    for (int q = 0; q < 3; ++q) f.p[q] = BF16::frag_t(tile + q * ps, ld, kg, l, col0, 0);
    return f;
  }
  template <int MI, int NI>
  static __device__ __forceinline__ void frags_tt(frag* a, frag* b, const elem* sA, int ldA, int colA, const elem* sB, int ldB, int colB, int kg, LanePos l,
                                                  int psA, int psB) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) a[mi] = frag_t(sA, ldA, kg, l, colA + mi * 32, psA);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) b[ni] = frag_t(sB, ldB, kg, l, colB + ni * 32, psB);
  }
  // term by term over the wave tile (the accumulators alternate), smallest terms first (mma_x3_term, bf16_frag.h)
  template <int MI, int NI>
  static __device__ __forceinline__ void mma(f32x16 (&acc)[MI][NI], const frag* a, const frag* b) {
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = mma_x3_term(t, a[mi].p, b[ni].p, acc[mi][ni]);
  }
};

// the policy of the fp32 instantiations: F32X3 for the vectorised 8-wave tile (128 x 128).  The 4-wave skinny tiles (128 x 32,
// 32 x 128) keep exact fp32 products: measured under F32X3 they were no faster (rows 1.01-1.04 x the time) or slower (the weight
// gradient behind a fused GroupNorm 1.32 x): profiles/flat_x3_measured.json.  VAE_FLAT_X3 = 0: exact fp32 products everywhere
// (the A/B arm)
template <bool VEC, int WAVES>
using F32For = std::conditional_t<VEC && WAVES == 8 && (VAE_FLAT_X3 != 0), F32X3, F32>;

// LDS elements of a body: two stages of PLANES x (A tile + B tile), and the GroupNorm scale / shift table behind them
template <class P, int BM, int BN, bool BKM, int XF>
constexpr int rows_lds_elems() {
  constexpr int BK = P::BK_ROWS;
  return 2 * P::PLANES * (BM * (BK + P::PAD_K) + (BKM ? BK * (BN + P::PAD_T) : BN * (BK + P::PAD_K))) +
         ((XF != VAE_XF_NONE) ? 2 * SS_HALF * (4 / (int)sizeof(typename P::elem)) : 0);
}
template <class P, int BM, int BN, int XF>
constexpr int wgrad_lds_elems() {
  return 2 * P::PLANES * P::BK_WGRAD * (BM + P::PAD_T + BN + P::PAD_T) + ((XF != VAE_XF_NONE) ? 2 * SS_HALF * (4 / (int)sizeof(typename P::elem)) : 0);
}
// the stages' storage: static, or the kernel's dynamic LDS where the policy says so (the launcher passes *_lds_elems)
extern __shared__ __attribute__((aligned(16))) unsigned char lds_dynamic[];

template <int MI, int NI>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MI][NI]) {
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
}

// ---------------------------------------------------------------------------------------
// rows body.  Pipeline: LDS is double buffered; the global loads of K-step s+2 are issued and the registers of step s+1 are
// transformed + written to the other LDS stage in the MIDDLE of step s's MFMA block, so one workgroup barrier per K-step
// suffices and the VALU/LDS-write work sits in the shadow of MFMAs already issued.  A step is NKG = 1, 2 or 4 k-groups.  The
// GroupNorm scale/shift rows the tile needs are staged in LDS once per workgroup (they used to be 8 dependent global loads
// per thread per step).
// (The pipeline driver -- compute and the step loop -- is written out in both bodies: behind a shared function hipcc's
// register allocation moved by 2..5 VGPRs in most instantiations and one bf16 rows kernel lost a wave of occupancy.)
// ---------------------------------------------------------------------------------------
template <class P, int BM, int BN, int WM, int WN, bool BKM, bool VEC, int XF>
__device__ __forceinline__ void rows_body(const vae_igemm_args& p) {
  typedef typename P::elem elem;
  constexpr int BK = P::BK_ROWS;
  constexpr int NT = 64 * WM * WN;  // 4 waves (skinny tiles) or 8 waves (128x128: 4 waves/SIMD at 2 workgroups/CU)
  constexpr int KQ = BK / 4;        // float4 per k-contiguous tile row
  constexpr int RP = NT / KQ;       // tile rows covered by one pass of the float4 loaders
  constexpr int LDA = BK + P::PAD_K;
  constexpr int LDB = BKM ? (BN + P::PAD_T) : (BK + P::PAD_K);
  constexpr int SA = BM * LDA;
  constexpr int SB = BKM ? BK * LDB : BN * LDB;
  constexpr int PL = P::PLANES;   // planes of a tile, SA / SB apart
  constexpr int STAGE = PL * (SA + SB);  // elements
  constexpr int SS = (XF != VAE_XF_NONE) ? 2 * SS_HALF * (4 / (int)sizeof(elem)) : 0;
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NI = TN / 32;
  constexpr int AR = BM / RP;  // A rows per thread
  constexpr int NQ = BN / 4, KR = NT / NQ;  // n-contiguous weight tile: NQ float4 per k row, KR k rows per pass
  constexpr int BR = BKM ? (BK / KR) : (BN / RP);
  static_assert(AR >= 1 && BR >= 1 && TM % 32 == 0 && TN % 32 == 0 && (BK / P::KG == 1 || BK / P::KG == 2 || BK / P::KG == 4), "tile/wave layout");
  static_assert(2 * STAGE + SS == rows_lds_elems<P, BM, BN, BKM, XF>(), "the launcher reserves what the body lays out");
  __shared__ __attribute__((aligned(16))) elem smem_static[P::LDS_DYNAMIC ? 1 : 2 * STAGE + SS];
  elem* const smem = P::LDS_DYNAMIC ? reinterpret_cast<elem*>(lds_dynamic) : smem_static;
  float* sS = reinterpret_cast<float*>(smem + 2 * STAGE);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const LanePos lp = lane_pos(lane);
  const int lr = lp.lr, lh = lp.lh;
  const int tilesN = (p.N + BN - 1) / BN;
  const int tm = blockIdx.x / tilesN, tn = blockIdx.x % tilesN;
  const int m0 = tm * BM, n0 = tn * BN;
  const int z = blockIdx.z;
  const vae_conv_geom g = p.g;
  const SrcMap smap = make_srcmap(g);
  const bool abf = P::flag(p.a_bf16), cbf = P::flag(p.out_bf16), rbf = P::flag(p.res_bf16);  // storage of A / C / res
  const unsigned esA = abf ? 2u : 4u;
  const char* __restrict__ A = reinterpret_cast<const char*>(p.A) + (int64_t)z * p.sAb * esA;
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
  const int b_base = s2c ? (m0 - cls * cls_rows) / (hh * wh) : m0 / hw;
  const size_t img = (size_t)g.Hs * g.Ws * g.Cs;
  const size_t abytes = (size_t)(g.B - b_base) * img * esA, wbytes = (size_t)(BKM ? (int64_t)p.K * p.sk : (int64_t)p.N * p.sn) * 4u;
  const auto rsA = VAE_BUF_RSRC(A + (int64_t)b_base * img * esA, abytes < BUF_MAX ? abytes : BUF_MAX);
  const auto rsW = VAE_BUF_RSRC(W, wbytes < BUF_MAX ? wbytes : BUF_MAX);

  // per-thread A rows
  const int k4 = tid % KQ, r0 = tid / KQ;
  const int n4 = tid % NQ, kq = tid / NQ;  // n-contiguous weight tile
  int rb[AR], ry[AR], rx[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int m = m0 + r0 + RP * i;
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
  zero_acc(acc);

  const int kchunks = (p.K + BK - 1) / BK;
  const int steps = ntaps * kchunks;

  typename P::raw4 ra[AR];
  f32x4 rw[BR];
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
      if constexpr (VEC) ra[i] = P::load4(rsA, esA, ok && c < p.K, ((rb[i] - b_base) * g.Hs + sy) * g.Ws + sx, g.Cs, c);
      else ra[i] = load4s(p.A + (int64_t)z * p.sAb + (((int64_t)rb[i] * g.Hs + sy) * g.Ws + sx) * g.Cs + c, ok, c, p.K);
      a_b[i] = ok ? rb[i] : -1;
    }
    if (!BKM) {
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        const int n = n0 + r0 + RP * i;
        if constexpr (VEC) rw[i] = VAE_BUF_LOAD4(rsW, oob_unless(n < p.N && c < p.K, ((unsigned)n * (unsigned)p.sn + (unsigned)tap * (unsigned)p.st + (unsigned)c) * 4u));
        else rw[i] = load4s(W + (int64_t)n * p.sn + (int64_t)tap * p.st + c, n < p.N, c, p.K);
      }
    } else {
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        const int k = c0 + kq + KR * i;
        const int n = n0 + n4 * 4;
        if constexpr (VEC) rw[i] = VAE_BUF_LOAD4(rsW, oob_unless(k < p.K && n < p.N, ((unsigned)k * (unsigned)p.sk + (unsigned)tap * (unsigned)p.st + (unsigned)n) * 4u));
        else rw[i] = load4s(W + (int64_t)k * p.sk + (int64_t)tap * p.st + n, k < p.K, n, p.N);
      }
    }
  };
  auto store_lds = [&](elem* sA, elem* sB) {
    const int c = reg_c0 + k4 * 4;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      f32x4 v = P::to_f32(ra[i], abf);
      if (XF != VAE_XF_NONE) {
        const bool ok = (a_b[i] >= 0) && (c < p.K);
        const int o = ok ? (a_b[i] - b_lo) * p.K + c : 0;
        v = xform4_tab<XF>(v, sS + o, sS + SS_HALF + o, ok);
      }
      P::put4(&sA[(r0 + RP * i) * LDA + k4 * 4], v, SA);
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      if (!BKM) P::put4(&sB[(r0 + RP * i) * LDB + k4 * 4], rw[i], SB);
      else P::put4(&sB[(kq + KR * i) * LDB + n4 * 4], rw[i], SB);
    }
  };
  // fragments of k-group kg+1 are requested before the MFMAs of kg are issued (pinned with sched_barrier)
  typename P::frag fa[2][MI], fb[2][NI];
  auto fetch = [&](const elem* sA, const elem* sB, int kg, typename P::frag* a, typename P::frag* b) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) a[mi] = P::frag_k(&sA[(wm * TM + mi * 32 + lr) * LDA + kg * P::KG + lh * (P::KG / 2)], SA);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      if (!BKM) b[ni] = P::frag_k(&sB[(wn * TN + ni * 32 + lr) * LDB + kg * P::KG + lh * (P::KG / 2)], SB);
      else b[ni] = P::frag_t(sB, LDB, kg, lp, wn * TN + ni * 32, SB);
    }
  };
  constexpr int NKG = BK / P::KG;
  auto compute = [&](const elem* sA, const elem* sB, int kg) {  // fragments of kg already requested
    if (kg + 1 < NKG) fetch(sA, sB, kg + 1, fa[(kg + 1) & 1], fb[(kg + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    if (P::SETPRIO) __builtin_amdgcn_s_setprio(1);
    P::mma(acc, fa[kg & 1], fb[kg & 1]);
    if (P::SETPRIO) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  load_regs(0);
  __syncthreads();  // scale/shift table visible
  store_lds(smem, smem + PL * SA);
  if (steps > 1) load_regs(1);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const elem* cA = smem + (s & 1) * STAGE;
    const elem* cB = cA + PL * SA;
    fetch(cA, cB, 0, fa[0], fb[0]);
    if (NKG > 1) compute(cA, cB, 0);  // (a step of one k-group: its fragments are requested, then the staging, then its MFMAs)
    if (NKG == 4) compute(cA, cB, 1);
    if (s + 1 < steps) {  // staged in the shadow of the MFMAs already issued
      elem* nA = smem + ((s + 1) & 1) * STAGE;
      store_lds(nA, nA + PL * SA);
      if (s + 2 < steps) load_regs(s + 2);
    }
    compute(cA, cB, NKG / 2);
    if (NKG == 4) compute(cA, cB, 3);
    __syncthreads();
  }

  // ---------------- epilogue ----------------
  // outputs and the residual through buffer descriptors (common.h): a row / column outside the matrix is an
  // out-of-range offset (load reads 0, store is dropped): no branch per element, residual loads issued back to back
  const unsigned esC = cbf ? 2u : 4u, esR = rbf ? 2u : 4u;
  char* __restrict__ C = reinterpret_cast<char*>(p.C) + (int64_t)z * p.sCb * esC;
  const auto rsC = VAE_BUF_RSRC(C, (size_t)p.M * p.ldc * esC);
  const auto rsR = VAE_BUF_RSRC(p.res ? reinterpret_cast<const char*>(p.res) + (int64_t)z * p.sCb * esR : C, (size_t)p.M * p.ldc * (p.res ? esR : esC));
  float tsum[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) tsum[ni] = 0.f;
  bool pair16 = false;
  if constexpr (P::PAIR16) pair16 = P::pair16(p, cbf, rbf, C);
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int col = n0 + wn * TN + ni * 32 + lr;
    const bool colok = col < p.N;
    const float bv = (p.bias && colok) ? p.bias[col] : 0.f;
    if constexpr (P::PAIR16) {
      if (pair16) {  // uniform
        P::store_pairs(p, acc, ni, rsC, rsR, col, colok, m0, m0 + wm * TM, lh, s2c, row_pixel);
        continue;
      }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      typename P::off_t off[16];
      float rv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * TM + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        int orow = row;
        if (s2c) {  // class-major row -> pixel-major output row
          int b, y, x;
          row_pixel(row < p.M ? row : m0, b, y, x);
          orow = (b * g.Ho + y) * g.Wo + x;
        }
        off[r] = P::out_off(colok && row < p.M, orow, p.ldc, col);
        rv[r] = 0.f;
      }
      if (p.res) {  // uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = P::load1(rsR, rbf, off[r]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = p.alpha * acc[mi][ni][r] + bv + rv[r];
        P::store1(rsC, cbf, off[r], v);
        tsum[ni] += P::inside(off[r]) ? fabsf(v) : 0.f;
      }
    }
  }
  if (p.track && z == 0) {
    float* red = reinterpret_cast<float*>(smem);  // [WM][BN]; the last loop barrier already separated it from the MFMA reads
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const float s2 = tsum[ni] + __shfl_xor(tsum[ni], 32, 64);
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
// wgrad body: out[m][tap][n] = sum_pix dY[pix][m] * XF(X[src(pix,tap)][n]).  Both tiles pixel-major, both fragments through
// the transposing read; the same double-buffered one-barrier pipeline.  The bias gradient (column sums of dY) is folded in:
// workgroups with tn == 0 and tap == 0 add up the dY tiles they stage anyway.
// ---------------------------------------------------------------------------------------
template <class P, int BM, int BN, int WM, int WN, bool VEC, int XF>
__device__ __forceinline__ void wgrad_body(const vae_wgrad_args& p) {
  typedef typename P::elem elem;
  constexpr int BK = P::BK_WGRAD;  // pixels per step
  constexpr int NT = 64 * WM * WN;
  constexpr int LDA = BM + P::PAD_T, LDB = BN + P::PAD_T;
  constexpr int SA = BK * LDA, SB = BK * LDB;
  constexpr int PL = P::PLANES;
  constexpr int STAGE = PL * (SA + SB);
  constexpr int SS = (XF != VAE_XF_NONE) ? 2 * SS_HALF * (4 / (int)sizeof(elem)) : 0;
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NI = TN / 32;
  constexpr int AQ = BM / 4, AKR = NT / AQ, AI = BK / AKR;  // dY tile: AQ float4 per row
  constexpr int BQ = BN / 4, BKR = NT / BQ, BI = BK / BKR;
  static_assert(AI >= 1 && BI >= 1 && TM % 32 == 0 && TN % 32 == 0 && (BK / P::KG == 1 || BK / P::KG == 2 || BK / P::KG == 4), "tile/wave layout");
  static_assert(2 * STAGE + SS == wgrad_lds_elems<P, BM, BN, XF>(), "the launcher reserves what the body lays out");
  __shared__ __attribute__((aligned(16))) elem smem_static[P::LDS_DYNAMIC ? 1 : 2 * STAGE + SS];
  elem* const smem = P::LDS_DYNAMIC ? reinterpret_cast<elem*>(lds_dynamic) : smem_static;
  float* sS = reinterpret_cast<float*>(smem + 2 * STAGE);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const LanePos lp = lane_pos(lane);
  const int lr = lp.lr, lh = lp.lh;
  const int tilesN = (p.N + BN - 1) / BN;
  const int tm = blockIdx.x / tilesN, tn = blockIdx.x % tilesN;
  const int m0 = tm * BM, n0 = tn * BN;
  const int tap = blockIdx.y / p.nsplit, split = blockIdx.y % p.nsplit;
  const int z = blockIdx.z;
  const vae_conv_geom g = p.g;
  const SrcMap smap = make_srcmap(g);
  const int kh = (g.taps == 9) ? tap / 3 : 0, kw = (g.taps == 9) ? tap - kh * 3 : 0;
  const bool ybf = P::flag(p.y_bf16), xbf = P::flag(p.x_bf16);  // storage of dY / X
  const unsigned esY = ybf ? 2u : 4u, esX = xbf ? 2u : 4u;
  const char* __restrict__ dY = reinterpret_cast<const char*>(p.dY) + (int64_t)z * p.sYb * esY;
  const char* __restrict__ X = reinterpret_cast<const char*>(p.X) + (int64_t)z * p.sXb * esX;

  int chunk = (p.npix + p.nsplit - 1) / p.nsplit;
  chunk = ((chunk + 31) / 32) * 32;  // to 32 pixels under every policy: the host's table-fit check (vae_xf_fusable_wgrad) assumes it
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
  zero_acc(acc);

  // buffer descriptors (vectorised instantiations): dY from this split's first pixel, X from its first image
  const size_t img = (size_t)g.Hs * g.Ws * g.Cs;
  const size_t ybytes = (size_t)(steps > 0 ? pend - pbeg : 0) * p.ldy * esY, xbytes = (size_t)(g.B - b_lo) * img * esX;
  const auto rsY = VAE_BUF_RSRC(dY + (int64_t)pbeg * p.ldy * esY, ybytes < BUF_MAX ? ybytes : BUF_MAX);
  const auto rsX = VAE_BUF_RSRC(X + (int64_t)b_lo * img * esX, xbytes < BUF_MAX ? xbytes : BUF_MAX);

  const int a4 = tid % AQ, akq = tid / AQ;
  const int b4 = tid % BQ, bkq = tid / BQ;
  typename P::raw4 ra[AI], rx[BI];
  int xb[BI];
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};

  auto load_regs = [&](int s) {
    const int pb = pbeg + s * BK;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int pix = pb + akq + AKR * i;
      const int c = m0 + a4 * 4;
      if constexpr (VEC) ra[i] = P::load4(rsY, esY, pix < pend && c < p.M, pix - pbeg, p.ldy, c);
      else ra[i] = load4s(p.dY + (int64_t)z * p.sYb + (int64_t)pix * p.ldy + c, pix < pend, c, p.M);
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      const int pix = pb + bkq + BKR * i;
      const int c = n0 + b4 * 4;
      const int b = pix / hw, rem = pix - b * hw;
      const int y = rem / g.Wo, x = rem - y * g.Wo;
      int sy = 0, sx = 0;
      const bool ok = src_pixel(smap, y, x, kh, kw, sy, sx) && (pix < pend);
      if constexpr (VEC) rx[i] = P::load4(rsX, esX, ok && c < p.N, ((b - b_lo) * g.Hs + sy) * g.Ws + sx, g.Cs, c);
      else rx[i] = load4s(p.X + (int64_t)z * p.sXb + (((int64_t)b * g.Hs + sy) * g.Ws + sx) * g.Cs + c, ok, c, p.N);
      xb[i] = ok ? b : -1;
    }
  };
  auto store_lds = [&](elem* sA, elem* sB) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const f32x4 v = P::to_f32(ra[i], ybf);
      P::put4_stored(&sA[(akq + AKR * i) * LDA + a4 * 4], ra[i], v, ybf, SA);
      if (do_bias) bsum += v;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      f32x4 v = P::to_f32(rx[i], xbf);
      if (XF != VAE_XF_NONE) {
        const bool ok = xb[i] >= 0;
        const int o = ok ? (xb[i] - b_lo) * BN + b4 * 4 : 0;
        v = xform4_tab<XF>(v, sS + o, sS + SS_HALF + o, ok);
      }
      P::put4(&sB[(bkq + BKR * i) * LDB + b4 * 4], v, SB);
    }
  };
  typename P::frag fa[2][MI], fb[2][NI];
  auto fetch = [&](const elem* sA, const elem* sB, int kg, typename P::frag* a, typename P::frag* b) {
    P::template frags_tt<MI, NI>(a, b, sA, LDA, wm * TM, sB, LDB, wn * TN, kg, lp, SA, SB);
  };
  constexpr int NKG = BK / P::KG;
  auto compute = [&](const elem* sA, const elem* sB, int kg) {  // fragments of kg already requested
    if (kg + 1 < NKG) fetch(sA, sB, kg + 1, fa[(kg + 1) & 1], fb[(kg + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    if (P::SETPRIO) __builtin_amdgcn_s_setprio(1);
    P::mma(acc, fa[kg & 1], fb[kg & 1]);
    if (P::SETPRIO) __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  };
  if (steps > 0) {
    load_regs(0);
    __syncthreads();  // scale/shift table visible
    store_lds(smem, smem + PL * SA);
    if (steps > 1) load_regs(1);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
      const elem* cA = smem + (s & 1) * STAGE;
      const elem* cB = cA + PL * SA;
      fetch(cA, cB, 0, fa[0], fb[0]);
      if (NKG > 1) compute(cA, cB, 0);
      if (NKG == 4) compute(cA, cB, 1);
      if (s + 1 < steps) {  // staged in the shadow of the MFMAs already issued
        elem* nA = smem + ((s + 1) & 1) * STAGE;
        store_lds(nA, nA + PL * SA);
        if (s + 2 < steps) load_regs(s + 2);
      }
      compute(cA, cB, NKG / 2);
      if (NKG == 4) compute(cA, cB, 3);
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

// entry points: a body under its policy
template <int BM, int BN, int WM, int WN, bool BKM, bool VEC, int XF>
__global__ __launch_bounds__(64 * WM * WN) void igemm_rows_kernel(vae_igemm_args p) { rows_body<F32For<VEC, WM * WN>, BM, BN, WM, WN, BKM, VEC, XF>(p); }
template <int BM, int BN, int WM, int WN, bool VEC, int XF>
__global__ __launch_bounds__(64 * WM * WN) void wgrad_kernel(vae_wgrad_args p) { wgrad_body<F32For<VEC, WM * WN>, BM, BN, WM, WN, VEC, XF>(p); }
template <int BM, int BN, int WM, int WN, bool BKM, int XF>
__global__ __launch_bounds__(64 * WM * WN) void igemm_rows_bf16_kernel(vae_igemm_args p) { rows_body<BF16, BM, BN, WM, WN, BKM, true, XF>(p); }
template <int BM, int BN, int WM, int WN, int XF>
__global__ __launch_bounds__(64 * WM * WN) void wgrad_bf16_kernel(vae_wgrad_args p) { wgrad_body<BF16, BM, BN, WM, WN, true, XF>(p); }

// out2[i] = sum_k partial2[k][i] for the 256 columns of workgroup `blk` (the bias gradient: few columns, up to 1024 splits), added
// one after the other in ascending k.  Sixteen loads go out before the first of them is added: a loop of one load and one add per
// split waits a full memory latency per split, 1024 times for the <= 4-channel weight gradients.
__device__ __forceinline__ void small_column_sums(const float* __restrict__ partial2, int nsplit, int n2, float* __restrict__ out2, int blk) {
  const int i = blk * 256 + (int)threadIdx.x;
  if (i >= n2) return;
  const float* p = partial2 + i;
  float s = 0.f;
  int k = 0;
  for (; k + 16 <= nsplit; k += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[(int64_t)(k + j) * n2];
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
  }
  for (; k < nsplit; ++k) s += p[(int64_t)k * n2];
  out2[i] = s;
}

// out[i] = sum_k partial[k][i], fixed association (reproducible).  16-byte loads, 8 independent loads in flight per
// thread; KP threads share a column quad and split the k range (a 128-channel layer has 128 splits of only 147 K elements:
// one thread per element leaves too few bytes in flight to fill HBM), combined through LDS in k order.
// A second, small reduction (the bias gradient: [nsplit][n2]) rides in the same launch: workgroups main_blocks.. do it
// (small_column_sums).
template <int KP>
__global__ __launch_bounds__(256) void reduce_splits_kernel(const float* __restrict__ partial, int nsplit, int64_t n, float* __restrict__ out,
                                                            int main_blocks, const float* __restrict__ partial2, int n2, float* __restrict__ out2) {
  constexpr int COLS = 256 / KP;
  __shared__ f32x4 red[KP > 1 ? 256 : 1];
  if ((int)blockIdx.x >= main_blocks) {  // uniform per workgroup
    small_column_sums(partial2, nsplit, n2, out2, (int)blockIdx.x - main_blocks);
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

// Reduction of a Winograd weight-gradient slab [nsplit][NPOS][Cin][Cout] (wgrad3_wino.hip: NPOS = 16, wgrad3_upwino.hip: 9) into
// dW [Cout][3][3][Cin] (OHWI) in one launch: the slab is read once, nothing is staged in global memory.
//     S_p[ci][co] = sum_k slab[k][p][ci][co]
//     NPOS 16:  dW[co][a][b][ci] = sum_{i,j} At[a][i] At[b][j] c_i c_j S_{4i+j}[ci][co]   At = [1 1 1 0; 0 1 -1 0; 0 1 1 -1], c = (1, .5, .5, 1)
//     NPOS  9:  dW[co][a][b][ci] = sum_{i,j} At[a][i] At[b][j]         S_{3i+j}[ci][co]   At = [1 1 0; 0 1 0; 0 1 -1]
// S_p is added in the association of reduce_splits_kernel (which used to form it in a buffer of its own, so dW keeps its bits):
//     nsplit >= 32:  ((g0 + g1) + g2) + g3, g_j = the splits [j per, (j + 1) per), per = ceil(nsplit / 4);   nsplit < 32: one range;
//     a range = rounds of 8 splits, each added to the sum as ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)), then the rest one by one.
// Workgroup = a tile of TCI ci x 32 co = Q column quads (16-byte loads, lanes along co: 128-byte rows) and KP = 256 / Q thread
// groups that share the POSITIONS (group g: positions g, g + KP, ..), so that no sum is split over threads and the parallelism
// costs no change of association: a thread has 8 or 16 loads of one position in flight (rounds), or one load of each of its
// positions (the rest).  The sums meet in LDS, thread group 0 applies the transform to its quad and the tile goes out through an
// LDS transpose with lanes along ci.  The launcher picks the largest tile that still gives 256 workgroups: a 128-channel layer
// (64 splits of 1 MB) runs as 256 workgroups of 2 x 32 with one position per thread, a 512-channel layer (4 splits of 16 MB) as
// 256 workgroups of 32 x 32 with all 16 positions in a thread.
// Workgroups beyond the tiles sum the bias-gradient slab [nsplit][Cout] (small_column_sums).
template <int NPOS, int TCI>
__global__ __launch_bounds__(256) void wgrad_wino_reduce_kernel(const float* __restrict__ slab, int nsplit, int N, int M, float* __restrict__ dW,
                                                                int tiles, const float* __restrict__ bpart, float* __restrict__ db) {
  constexpr int TQ = 8, TCO = 4 * TQ, Q = TCI * TQ, KP = 256 / Q, NP = (NPOS + KP - 1) / KP;
  constexpr int ST0 = KP > 1 ? NPOS * Q * 4 : 0;  // floats of the sums [NPOS][Q] quads; behind them the transposed tile [9][TCO][TCI + 1]
  __shared__ __attribute__((aligned(16))) float smem[ST0 + 9 * TCO * (TCI + 1)];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= tiles) {  // uniform per workgroup
    small_column_sums(bpart, nsplit, M, db, (int)blockIdx.x - tiles);
    return;
  }
  const int tilesM = M / TCO;
  const int c0 = ((int)blockIdx.x / tilesM) * TCI, m0 = ((int)blockIdx.x % tilesM) * TCO;
  const int q = tid % Q, kp = tid / Q;
  const int cq = q % TQ, cl = q / TQ;
  const int64_t pstride4 = ((int64_t)N * M) >> 2, sstride4 = NPOS * pstride4;  // one position / one split, in quads
  const f32x4* src = reinterpret_cast<const f32x4*>(slab + (int64_t)(c0 + cl) * M + m0 + 4 * cq);
  const f32x4* sp[NP];  // this thread's positions kp + j KP (one past the last: position 0 again, read and dropped)
#pragma unroll
  for (int j = 0; j < NP; ++j) sp[j] = src + (kp + j * KP < NPOS ? kp + j * KP : 0) * pstride4;
  auto tree8 = [](const f32x4* v) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); };
  auto range = [&](int k0, int k1, f32x4(&g)[NP]) {  // the splits [k0, k1) of every position of this thread
#pragma unroll
    for (int j = 0; j < NP; ++j) g[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int k = k0;
    if constexpr (NP == 1) {  // two rounds' loads at once
      for (; k + 16 <= k1; k += 16) {
        f32x4 v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = sp[0][(int64_t)(k + i) * sstride4];
        g[0] += tree8(v);
        g[0] += tree8(v + 8);
      }
    }
    for (; k + 8 <= k1; k += 8) {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        f32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = sp[j][(int64_t)(k + i) * sstride4];
        g[j] += tree8(v);
      }
    }
    for (; k < k1; ++k) {
      f32x4 v[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) v[j] = sp[j][(int64_t)k * sstride4];
#pragma unroll
      for (int j = 0; j < NP; ++j) g[j] += v[j];
    }
  };
  f32x4 mine[NP];
  if (nsplit >= 32) {
    const int per = (nsplit + 3) / 4;
    range(0, min(nsplit, per), mine);
    for (int r = 1; r < 4; ++r) {
      f32x4 g[NP];
      range(r * per, min(nsplit, (r + 1) * per), g);
#pragma unroll
      for (int j = 0; j < NP; ++j) mine[j] += g[j];
    }
  } else {
    range(0, nsplit, mine);
  }
  f32x4 acc[NPOS];
  if constexpr (KP > 1) {
    f32x4* red = reinterpret_cast<f32x4*>(smem);  // [NPOS][Q]
#pragma unroll
    for (int j = 0; j < NP; ++j)
      if (kp + j * KP < NPOS) red[(kp + j * KP) * Q + q] = mine[j];
    __syncthreads();
    if (kp == 0) {
#pragma unroll
      for (int p = 0; p < NPOS; ++p) acc[p] = red[p * Q + q];
    }
  } else {
#pragma unroll
    for (int p = 0; p < NPOS; ++p) acc[p] = mine[p];
  }
  float(*sT)[TCO][TCI + 1] = reinterpret_cast<float(*)[TCO][TCI + 1]>(smem + ST0);
  if (kp == 0) {
    f32x4 o[9];
    if constexpr (NPOS == 16) {
      f32x4 h[3][4];  // A^T (c c^T (.) S)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float cj = (j == 1 || j == 2) ? 0.5f : 1.f;
        const f32x4 r0 = acc[0 * 4 + j] * cj, r1 = acc[1 * 4 + j] * (0.5f * cj), r2 = acc[2 * 4 + j] * (0.5f * cj), r3 = acc[3 * 4 + j] * cj;
        h[0][j] = (r0 + r1) + r2;
        h[1][j] = r1 - r2;
        h[2][j] = (r1 + r2) - r3;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        o[a * 3 + 0] = (h[a][0] + h[a][1]) + h[a][2];
        o[a * 3 + 1] = h[a][1] - h[a][2];
        o[a * 3 + 2] = (h[a][1] + h[a][2]) - h[a][3];
      }
    } else {
      f32x4 h[3][3];  // A''^T S
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        h[0][j] = acc[0 * 3 + j] + acc[1 * 3 + j];
        h[1][j] = acc[1 * 3 + j];
        h[2][j] = acc[1 * 3 + j] - acc[2 * 3 + j];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        o[a * 3 + 0] = h[a][0] + h[a][1];
        o[a * 3 + 1] = h[a][1];
        o[a * 3 + 2] = h[a][1] - h[a][2];
      }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) sT[t][4 * cq + e][cl] = o[t][e];
  }
  __syncthreads();
  for (int idx = tid; idx < 9 * TCO * TCI; idx += 256) {  // lanes along ci, then the 9 taps of one co: (9 N)-float rows of dW
    const int c = idx % TCI, r = idx / TCI;
    const int t = r % 9, ml = r / 9;
    dW[((int64_t)(m0 + ml) * 9 + t) * N + c0 + c] = sT[t][ml][c];
  }
}

// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
using std::false_type;  // (int_c and dispatch_xf, THE xf switch: common_host.h)
using std::true_type;

// BF: the bf16 policy (vectorised shapes only: the caller checked, `vec` is not read)
template <bool BF, int BM, int BN, int WM, int WN>
int launch_rows_tile(const vae_igemm_args& a, bool bkm, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN)), 1, (unsigned)a.batch), block(64 * WM * WN);
  auto go = [&](auto bkm_c, auto vec_c) {
    constexpr bool BKM = decltype(bkm_c)::value, VEC = decltype(vec_c)::value;
    int rc = 0;  // of the LDS reservation
    auto launch = [&](auto xf) {
      constexpr int XF = decltype(xf)::value;
      if constexpr (BF) {
        hipLaunchKernelGGL((igemm_rows_bf16_kernel<BM, BN, WM, WN, BKM, XF>), grid, block, 0, st, a);
      } else if constexpr (F32For<VEC, WM * WN>::LDS_DYNAMIC) {
        constexpr int LDS = rows_lds_elems<F32For<VEC, WM * WN>, BM, BN, BKM, XF>() * (int)sizeof(typename F32For<VEC, WM * WN>::elem);
        if (rc == 0) rc = [&]() -> int { VAE_RESERVE_LDS((igemm_rows_kernel<BM, BN, WM, WN, BKM, VEC, XF>), LDS, "igemm_rows"); return 0; }();
        if (rc == 0) hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, BKM, VEC, XF>), grid, block, LDS, st, a);
      } else {
        hipLaunchKernelGGL((igemm_rows_kernel<BM, BN, WM, WN, BKM, VEC, XF>), grid, block, 0, st, a);
      }
    };
    if constexpr (BKM) {  // the n-contiguous weight tile exists untransformed only
      if (a.xf != VAE_XF_NONE) { vae_set_error("igemm_rows: xf unsupported with n-contiguous weights"); return VAE_EINVAL; }
      launch(int_c<VAE_XF_NONE>{});
    } else if (!dispatch_xf(a.xf, launch)) {
      vae_set_error("igemm_rows: bad xf %d", a.xf);
      return VAE_EINVAL;
    }
    return rc;
  };
  if (BF || vec) return bkm ? go(true_type{}, true_type{}) : go(false_type{}, true_type{});
  if constexpr (!BF) return bkm ? go(true_type{}, false_type{}) : go(false_type{}, false_type{});
  return 0;
}
template <bool BF>
int launch_rows(const vae_igemm_args& a, bool bkm, bool vec, hipStream_t st) {
  return (a.N <= 32) ? launch_rows_tile<BF, 128, 32, 4, 1>(a, bkm, vec, st) : launch_rows_tile<BF, 128, 128, 4, 2>(a, bkm, vec, st);
}

template <bool BF, int BM, int BN, int WM, int WN>
int launch_wgrad_tile(const vae_wgrad_args& a, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN)), (unsigned)(a.g.taps * a.nsplit), (unsigned)a.batch), block(64 * WM * WN);
  auto go = [&](auto vec_c) {
    int rc = 0;  // of the LDS reservation
    auto launch = [&](auto xf) {
      constexpr bool VEC = decltype(vec_c)::value;
      constexpr int XF = decltype(xf)::value;
      if constexpr (BF) {
        hipLaunchKernelGGL((wgrad_bf16_kernel<BM, BN, WM, WN, XF>), grid, block, 0, st, a);
      } else if constexpr (F32For<VEC, WM * WN>::LDS_DYNAMIC) {
        constexpr int LDS = wgrad_lds_elems<F32For<VEC, WM * WN>, BM, BN, XF>() * (int)sizeof(typename F32For<VEC, WM * WN>::elem);
        if (rc == 0) rc = [&]() -> int { VAE_RESERVE_LDS((wgrad_kernel<BM, BN, WM, WN, VEC, XF>), LDS, "wgrad"); return 0; }();
        if (rc == 0) hipLaunchKernelGGL((wgrad_kernel<BM, BN, WM, WN, VEC, XF>), grid, block, LDS, st, a);
      } else {
        hipLaunchKernelGGL((wgrad_kernel<BM, BN, WM, WN, VEC, XF>), grid, block, 0, st, a);
      }
    };
    if (dispatch_xf(a.xf, launch)) return rc;
    vae_set_error("wgrad: bad xf %d", a.xf);
    return VAE_EINVAL;
  };
  if (BF || vec) return go(true_type{});
  if constexpr (!BF) return go(false_type{});
  return 0;
}
template <bool BF>
int launch_wgrad(const vae_wgrad_args& a, bool vec, hipStream_t st) {
  if (a.M <= 32) return launch_wgrad_tile<BF, 32, 128, 1, 4>(a, vec, st);
  if (a.N <= 32) return launch_wgrad_tile<BF, 128, 32, 4, 1>(a, vec, st);
  return launch_wgrad_tile<BF, 128, 128, 4, 2>(a, vec, st);
}

}  // namespace

int launch_rows_f32(const vae_igemm_args& a, bool bkm, bool vec, hipStream_t st) { return launch_rows<false>(a, bkm, vec, st); }
int launch_rows_bf16(const vae_igemm_args& a, bool bkm, hipStream_t st) { return launch_rows<true>(a, bkm, true, st); }
int launch_wgrad_f32(const vae_wgrad_args& a, bool vec, hipStream_t st) { return launch_wgrad<false>(a, vec, st); }
int launch_wgrad_bf16(const vae_wgrad_args& a, hipStream_t st) { return launch_wgrad<true>(a, true, st); }

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
  VAE_CHECK(aligned16(slab), "wgrad_wino_reduce: the slab must be 16-byte aligned");
  VAE_CHECK((int64_t)Cin * Cout <= (1ll << 30), "wgrad_wino_reduce: too many channel pairs");
  (void)scratch;  // unused since the reduction reads the slab once (kept in the signature)
  hipStream_t st = (hipStream_t)stream;
  const int extra = bias_partial ? (Cout + 255) / 256 : 0;
  auto launch = [&](auto npos_c, auto tci_c) {
    constexpr int NPOS = decltype(npos_c)::value, TCI = decltype(tci_c)::value;
    const int tiles = (Cin / TCI) * (Cout / 32);
    hipLaunchKernelGGL((wgrad_wino_reduce_kernel<NPOS, TCI>), dim3((unsigned)(tiles + extra)), dim3(256), 0, st, slab, nsplit, Cin, Cout, dW, tiles,
                       bias_partial, db);
  };
  // the largest tile (32, 8 or 2 ci x 32 co: 1, 4 or 16 thread groups over the positions) that leaves 256 workgroups
  const int64_t t32 = (int64_t)(Cin / 32) * (Cout / 32);
  auto pick = [&](auto npos_c) {
    if (t32 >= 256) launch(npos_c, int_c<32>{});
    else if (4 * t32 >= 256) launch(npos_c, int_c<8>{});
    else launch(npos_c, int_c<2>{});
  };
  if (npos == 9) pick(int_c<9>{});
  else pick(int_c<16>{});
  VAE_LAUNCH_CHECK("wgrad_wino_reduce");
  return VAE_OK;
}
