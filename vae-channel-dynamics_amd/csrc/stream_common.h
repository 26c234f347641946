// What the streaming kernels share (norm.hip, track.hip, lens.hip, elementwise.hip; image_metrics.hip shares nothing that
// leaves its kernels' compiled figures alone): fp32 / bf16 storage access, the runtime GroupNorm(+SiLU) element transform, the
// pixel-chunk layout, and the per-wave-then-four block reduction (on wave_reduce of common.h).  These kernels promise bitwise
// reproducible results ("per-workgroup partial + fixed-order final pass"), so a reduction here has ONE association order,
// stated at its definition; a caller that needs another order does not use it.
#pragma once
#include <type_traits>
#include "bf16_frag.h"

// ---------------------------------------------------------------------------------------------------------
// storage: a tensor held as fp32 or as bf16 (the upper half of an fp32); `i` indexes quads (load4 / store4) or elements (load1)
// ---------------------------------------------------------------------------------------------------------
template <bool BF>
__device__ __forceinline__ f32x4 load4(const void* base, int64_t i) {
  if (!BF) return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + i * 4);
  return unpack4(*reinterpret_cast<const uint2*>(reinterpret_cast<const u16*>(base) + i * 4));
}
template <bool BF>
__device__ __forceinline__ void store4(void* base, int64_t i, f32x4 v) {
  if (!BF) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(base) + i * 4) = v;
  else *reinterpret_cast<uint2*>(reinterpret_cast<u16*>(base) + i * 4) = pack4(v);
}
__device__ __forceinline__ float load1(const void* base, int64_t i, bool bf) {
  if (bf) return __builtin_bit_cast(float, (unsigned)reinterpret_cast<const u16*>(base)[i] << 16);
  return reinterpret_cast<const float*>(base)[i];
}

// GroupNorm affine (+SiLU) of one element with a runtime xf (VAE_XF_AFFINE or VAE_XF_AFFINE_SILU; the caller skips VAE_XF_NONE).
// (xform1 of thin_common.h and xform4_tab of common.h are the compile-time forms: they also zero padding, and choosing one of
// them from a runtime xf would put a switch where this has a select.)
__device__ __forceinline__ float affine_xf(float v, float sc, float sh, int xf) {
  const float u = v * sc + sh;
  return (xf == VAE_XF_AFFINE_SILU) ? silu_f(u) : u;
}

// ---------------------------------------------------------------------------------------------------------
// layout: 256 threads = PR pixel rows x Q lanes (make_lay: float4 lanes, Q = C / 4); a workgroup owns pixel chunk `chunk` of `nchunk`
// ---------------------------------------------------------------------------------------------------------
struct Lay {
  int Q, PR, cq, pr;
};
__device__ __forceinline__ Lay make_lay_q(int Q) {
  Lay l;
  l.Q = Q;
  l.PR = 256 / l.Q;
  l.cq = threadIdx.x % l.Q;
  l.pr = threadIdx.x / l.Q;
  return l;
}
__device__ __forceinline__ Lay make_lay(int C) { return make_lay_q(C >> 2); }
// pixels [p0, p1) of a chunk; a trailing chunk can start beyond HW: then p1 < p0
struct ChunkRange {
  int p0, p1;
};
__device__ __forceinline__ ChunkRange chunk_span(int HW, int per, int chunk) {
  const int p0 = chunk * per;
  return {p0, min(HW, p0 + per)};
}
__device__ __forceinline__ ChunkRange chunk_range(int HW, int nchunk, int chunk) {
  return chunk_span(HW, (HW + nchunk - 1) / nchunk, chunk);
}

// ---------------------------------------------------------------------------------------------------------
// reductions
// ---------------------------------------------------------------------------------------------------------
// (wave_reduce<Op> of common.h: shuffle offsets 32 -> 1)
// one value per wave of a 256-thread workgroup -> (r0 op r1) op (r2 op r3)
template <class Op, class T>
__device__ __forceinline__ T combine4(const T* r) {
  return Op::f(Op::f(r[0], r[1]), Op::f(r[2], r[3]));
}
// over a 256-thread workgroup: wave_reduce, then combine4 of the four waves' values through red[4]; every thread ends with the result
template <class Op, class T>
__device__ __forceinline__ T block_reduce(T v, T* red /*[4]*/) {
  v = wave_reduce<Op>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return combine4<Op>(red);
}

// The fixed 256-lane LDS trees (track_final_kernel, mom_block and the second tree of moments_channel_kernel, block_sum3 of
// image_metrics.hip) and the "rows dealt to T threads, partials added in order" sums (gn_stats_final_kernel, gn_bwd_final_kernel)
// stay in their kernels: every shared form tried moved the compiled code of a kernel that used it.

// ---------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------
// workgroups of 256 threads for a grid-stride pass over n items
inline int ew_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}
// a runtime flag as a template argument: launch(std::true_type / std::false_type); nest it for several flags
template <class Launch>
void dispatch_bool(bool on, Launch launch) {
  if (on) launch(std::true_type{});
  else launch(std::false_type{});
}
