// bf16 operand helpers shared by the bf16-compute kernels (gfx950).
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

// 4 fp32 -> 4 bf16 (round to nearest even, v_cvt_pk_bf16_f32), packed for one ds_write_b64
__device__ __forceinline__ uint2 pack4(f32x4 v) {
  bf16x4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = (__bf16)v[e];
  return __builtin_bit_cast(uint2, h);
}
// 4 bf16 (as loaded: 8 bytes) -> 4 fp32
__device__ __forceinline__ f32x4 unpack4(uint2 r) {
  f32x4 v;
  v[0] = __builtin_bit_cast(float, r.x << 16);
  v[1] = __builtin_bit_cast(float, r.x & 0xffff0000u);
  v[2] = __builtin_bit_cast(float, r.y << 16);
  v[3] = __builtin_bit_cast(float, r.y & 0xffff0000u);
  return v;
}
// Split-bf16 ("x3") operands: an fp32 value a as three bf16 planes
//   hi = bf16(a), mid = bf16(a - hi), lo = bf16((a - hi) - mid)      (round to nearest even; both subtractions are exact in fp32)
// so that hi + mid + lo = a up to 2^-26 |a|.  About 5.5 vector instructions per value.  Used by the flat fp32 kernels (igemm.hip,
// F32X3: planes staged in LDS), by the two Winograd weight gradients (wgrad3_wino.hip, wgrad3_upwino.hip: planes built in registers) and by the upsampler
// convolution (conv3_upwino.hip: V planes staged in LDS, U planes written by its weights kernel).
// (pack4 as two 2-wide conversions: element by element, hipcc converts one pair of the four singly and merges it with a v_perm_b32)
__device__ __forceinline__ uint2 pack4_pairs(f32x4 v) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t a = {v[0], v[1]}, b = {v[2], v[3]};
  return uint2{__builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2_t)), __builtin_bit_cast(unsigned, __builtin_convertvector(b, bf16x2_t))};
}
__device__ __forceinline__ void split3(f32x4 v, uint2& hi, uint2& mid, uint2& lo) {
  hi = pack4_pairs(v);
  const f32x4 h = unpack4(hi);
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = v[e] - h[e];
  mid = pack4_pairs(r);
  const f32x4 m = unpack4(mid);
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = r[e] - m[e];
  lo = pack4_pairs(r);
}
// the same split of two values (one v_cvt_pk_bf16_f32 per plane): planes as bf16 pairs, a in the low half
__device__ __forceinline__ void split3_pair(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const auto pk = [](float x, float y) { const f32x2_t v = {x, y}; return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t)); };
  hi = pk(a, b);
  const float ra = a - __builtin_bit_cast(float, hi << 16), rb = b - __builtin_bit_cast(float, hi & 0xffff0000u);
  mid = pk(ra, rb);
  lo = pk(ra - __builtin_bit_cast(float, mid << 16), rb - __builtin_bit_cast(float, mid & 0xffff0000u));
}
struct Bf3 {
  bf16x8 p[3];  // planes hi, mid, lo of a lane half's eight k
};
// the MFMA operand of eight fp32 values (the two Winograd weight gradients: v0 = the four tiles of a pair's first unit, v1 = of
// its second)
__device__ __forceinline__ Bf3 split8(f32x4 v0, f32x4 v1) {
  uint2 q0[3], q1[3];
  split3(v0, q0[0], q0[1], q0[2]);
  split3(v1, q1[0], q1[1], q1[2]);
  Bf3 f;
#pragma unroll
  for (int i = 0; i < 3; ++i) f.p[i] = __builtin_bit_cast(bf16x8, uint4{q0[i].x, q0[i].y, q1[i].x, q1[i].y});
  return f;
}
// A product a.b of split operands is the sum of the six plane products that are not below 2^-24 |a.b|, added into the fp32
// accumulator smallest first: term t = 0..5 is hi.lo, lo.hi, mid.mid, hi.mid, mid.hi, hi.hi (planes 0 = hi, 1 = mid, 2 = lo)
__device__ __forceinline__ f32x16 mma_x3_term(int t, const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 acc) {
  constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[t]], b[PB[t]], acc, 0, 0, 0);
}
// 4 consecutive elements of an operand stored as fp32 or bf16, through a buffer descriptor whose range is in BYTES of that
// storage.  ONE instruction for both storages -- a 16-byte load at element offset `eoff` (a bf16 operand's load also brings the
// next 4 elements along, unused) -- and the conversion happens where the value is CONSUMED (raw4_to_f32 at the LDS write a
// pipeline step later).  A storage-dependent load instruction plus an immediate conversion had made hipcc wait for every load
// right behind it (the flat kernels lost 20 % when bf16 storage came in).  eoff < 0 = out of range (reads zeros).
__device__ __forceinline__ uint4 buf_load4_raw(__amdgpu_buffer_rsrc_t rs, unsigned esize, int eoff) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, eoff >= 0 ? (unsigned)eoff * esize : BUF_OOB, 0, 0));
}
__device__ __forceinline__ f32x4 raw4_to_f32(uint4 r, bool bf) {
  if (bf) return unpack4(uint2{r.x, r.y});
  return __builtin_bit_cast(f32x4, r);
}
// one element through a descriptor (fp32: 4-byte, bf16: 2-byte access); eoff < 0 = out of range
__device__ __forceinline__ float buf_load1_elem(__amdgpu_buffer_rsrc_t rs, bool bf, int eoff) {
  if (bf) return __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rs, eoff >= 0 ? (unsigned)eoff * 2u : BUF_OOB, 0, 0) << 16);
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, eoff >= 0 ? (unsigned)eoff * 4u : BUF_OOB, 0, 0));
}
__device__ __forceinline__ void buf_store1_elem(__amdgpu_buffer_rsrc_t rs, bool bf, int eoff, float v) {
  if (bf) {
    const __bf16 h = (__bf16)v;
    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, h), rs, eoff >= 0 ? (unsigned)eoff * 2u : BUF_OOB, 0, 0);
  } else {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs, eoff >= 0 ? (unsigned)eoff * 4u : BUF_OOB, 0, 0);
  }
}
// MFMA operand from a k-contiguous image: 8 consecutive k at p (one ds_read_b128)
__device__ __forceinline__ bf16x8 frag_direct(const u16* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p));
}
// MFMA operand from a [k][col] image (k = the contraction index runs down the rows): 8 consecutive k for this
// lane's column through two transposing reads (ds_read_b64_tr_b16).  Within a 16-lane group, lane 4q+pp supplies
// the address of row q, columns 4pp..4pp+3 of a 4x16 block and lane i receives column i (cdna_hip_programming.md
// T10).  `p` = the address this lane supplies for rows k0..k0+3; rows k0+4..k0+7 are `4*ld` elements further.
// Row strides of 64 B mod 256 B (e.g. 160 or 96 bf16) put the four rows of a block in different bank ranges.
__device__ __forceinline__ bf16x8 frag_tr(const u16* p, int ld) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * ld));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}
