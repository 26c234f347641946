// What the per-channel statistics kernels share (track.hip's moments, chanhist.hip, chancov.hip, changrad.hip, actreg.hip,
// changroup.hip; wdyn.hip takes absmax_of): the W-channel load, the partial passes' frame -- tile and chunk prologue, the
// one-operand row loop, the row-order LDS fold -- and the host's shape and launch predicates.  Spelled out in their kernels,
// because every shared form tried moved registers or waits of a kernel that used it: the per-lane scale / shift load (all four
// kernels that have one), the row loops of moments_partial_kernel and of changrad_partial_kernel (two operands).  The final
// passes stay in their files: their trees and lane assignments differ on purpose (stream_common.h).
#pragma once
#include "stream_common.h"

// W consecutive channels of one pixel (an element offset, not a quad index: off is a multiple of 4 only where the host chose W = 4)
template <int W, bool XBF>
__device__ __forceinline__ void load_units(const void* base, int64_t off, float (&v)[W]) {
  if constexpr (W == 4) {
    f32x4 q;
    if constexpr (XBF) q = unpack4(*reinterpret_cast<const uint2*>(reinterpret_cast<const u16*>(base) + off));
    else q = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + off);
    v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
  } else {
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = load1(base, off + e, XBF);
  }
}

// max |y| kept as a bit pattern (for |y| the unsigned order of the patterns is the order of the values, NaN above infinity)
__device__ __forceinline__ float absmax_of(unsigned bits) {
  return bits > 0x7f800000u ? __builtin_bit_cast(float, 0x7fc00000u) : __builtin_bit_cast(float, bits);
}

// ---------------------------------------------------------------------------------------------------------
// the partial passes' frame: one workgroup per (pixel chunk = blockIdx.x, image = blockIdx.y, tile of UT channel units =
// blockIdx.z), a unit being W channels; lanes across the tile's units, PR pixel rows down the chunk
// ---------------------------------------------------------------------------------------------------------
struct StatFrame {
  int u0, nut;   // first unit and units of this workgroup's tile
  int PR, pr;    // pixel rows of the workgroup, this thread's (pr >= PR: a thread without work)
  int c0;        // this thread's first channel
  int chunk, b;
  int p0, p1;    // the chunk's pixels; p0 < HW: the host makes every chunk non-empty
};
template <int UT, int W>
__device__ __forceinline__ StatFrame stat_frame(int HW, int C, int nchunk) {
  StatFrame f;
  const int nu = C / W;
  f.u0 = blockIdx.z * UT;
  f.nut = min(UT, nu - f.u0);
  const Lay l = make_lay_q(f.nut);
  f.PR = l.PR, f.pr = l.pr;
  f.c0 = (f.u0 + l.cq) * W;
  f.chunk = blockIdx.x, f.b = blockIdx.y;
  const ChunkRange cr = chunk_range(HW, nchunk, f.chunk);
  f.p0 = cr.p0, f.p1 = cr.p1;
  return f;
}

// THE order of a partial pass (these kernels promise bitwise repeatable results; the loops that stay in their kernels keep it
// too): a thread takes the pixels p0 + pr, p0 + pr + PR, ... of its chunk in ascending order, one take(v) per pixel, whether the
// pixel was loaded in a group of four (four loads in flight per lane) or in the single-row tail; fold_rows then adds the
// workgroup's pixel rows 0 .. PR - 1 in that order.  xb: element offset of (image b, pixel 0, channel c0).  The caller skips
// threads with pr >= PR.  (The functors go by const reference: by value, actreg_partial_kernel<4, .> changed its registers.)
template <int W, bool XBF, class Take>
__device__ __forceinline__ void for_rows(const void* x, int64_t xb, int ld, const StatFrame& f, const Take& take) {
  const int PR = f.PR, p1 = f.p1;
  int pix = f.p0 + f.pr;
  for (; pix + 3 * PR < p1; pix += 4 * PR) {
    float v[4][W];
#pragma unroll
    for (int k = 0; k < 4; ++k) load_units<W, XBF>(x, xb + (int64_t)(pix + k * PR) * ld, v[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) take(v[k]);
  }
  for (; pix < p1; pix += PR) {
    float v[W];
    load_units<W, XBF>(x, xb + (int64_t)pix * ld, v);
    take(v);
  }
}
// thread t < nut (pixel row 0) folds its channel unit over the workgroup's pixel rows: add(i) for the LDS slot i of rows 0 .. PR - 1
template <class Add>
__device__ __forceinline__ void fold_rows(const StatFrame& f, const Add& add) {
  for (int r = 0; r < f.PR; ++r) {
    const int i = r * f.nut + threadIdx.x;
    add(i);
  }
}

// ---------------------------------------------------------------------------------------------------------
// host: what every pass (and size query) of these entry points asks of its arguments; `who` is the entry point's name
// ---------------------------------------------------------------------------------------------------------
inline int stat_check_shape(const char* who, int32_t B, int32_t HW, int32_t C, int32_t nchunk) {
  VAE_CHECK(B > 0 && HW > 0 && C > 0 && nchunk > 0, "%s: bad args (B=%d HW=%d C=%d nchunk=%d)", who, B, HW, C, nchunk);
  VAE_CHECK((int64_t)B * HW < ((int64_t)1 << 31), "%s: B * HW = %lld: 2^31 elements per channel or more", who,
            (long long)((int64_t)B * HW));
  const int per = (HW + nchunk - 1) / nchunk;
  VAE_CHECK(nchunk <= 65535 && B <= 65535 && (int64_t)(nchunk - 1) * per < HW,
            "%s: nchunk=%d for HW=%d leaves an empty chunk (or too many workgroups)", who, nchunk, HW);
  VAE_CHECK((int64_t)B * nchunk < ((int64_t)1 << 31), "%s: B * nchunk = %lld rows", who, (long long)((int64_t)B * nchunk));
  return VAE_OK;
}
// the runtime GroupNorm(+SiLU) transform of an operand with pixel stride ld
inline int stat_check_xf(const char* who, int32_t xf, const float* scale, const float* shift, int32_t ld, int32_t C) {
  VAE_CHECK(ld >= C, "%s: pixel stride ld=%d below C=%d", who, ld, C);
  VAE_CHECK(xf == VAE_XF_NONE || xf == VAE_XF_AFFINE || xf == VAE_XF_AFFINE_SILU, "%s: xf=%d", who, xf);
  VAE_CHECK(xf == VAE_XF_NONE || (scale && shift), "%s: xf needs scale and shift", who);
  return VAE_OK;
}
// four channels per lane where the operand's rows allow a 16 B (fp32) / 8 B (bf16) load, one otherwise
inline bool vec4_ok(const void* p, bool bf16, int C, int ld) {
  return C % 4 == 0 && ld % 4 == 0 && (((uintptr_t)p) & (bf16 ? 7u : 15u)) == 0;
}
