// Per-(sample, channel) sums of y = XF(x) for the ActivityMonitor's GroupNorm group dynamics and per-sample activity metrics
// (monitor.py): S1 = sum y, S2 = sum y^2 and A = sum |y| over the H * W pixels of every (image b, channel c), in one read of an
// NHWC activation: the inputs of vae_moments_partial (fp32 or bf16 storage, any pixel stride ld >= C, the optional runtime
// GroupNorm(+SiLU) transform applied on the fly).  Nothing here reduces over the batch: that is what the metrics are about.
//
// Partial pass: built as actreg_partial_kernel: one workgroup per (pixel chunk, image, tile of 256 channels), lanes across
// channels and pixel rows down the chunk, four pixel rows in flight per lane.  y is evaluated in fp32 (exactly the stored value
// without a transform) and widened; a lane keeps its three sums per channel in FLOAT64: the square of an fp32 value is exact in
// float64, so the only roundings are those of the additions, 2^-53 each.  The group metrics subtract n mu^2 from sum y^2, which
// cancels log2((mu / sigma)^2) bits: at mu = 10^3 sigma that is 20 of float64's 53 and all of fp32's 24.  The pass stays memory
// bound: five float64 instructions per element (one conversion, one exact product, three additions) against 4 (2) bytes read.
// The workgroup's pixel rows are added through LDS in row order, and three doubles per (image, chunk, channel) go to
// ws [B * nchunk][C][3] with plain stores.
//
// Final pass: one thread per (image, channel, sum) adds the nchunk partials of its word in chunk order.  No atomics anywhere,
// no zero-fill: repeated launches are bitwise identical.  A NaN or an infinity reaches the sums of its own (b, c) only.
#include "stream_common.h"

namespace {

constexpr int CG_CT = 256;   // channels of a full tile
constexpr int CG_WORDS = 3;  // sum y, sum y^2, sum |y|

// W consecutive channels of one pixel (as actreg.hip, which keeps its own copy: its compiled code stays as it is)
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

// ws: [B * nchunk][C][CG_WORDS] doubles
template <int W, bool XBF>
__global__ __launch_bounds__(256) void changroup_partial_kernel(const void* __restrict__ x, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, int xf, int HW, int C, int ld,
                                                                int nchunk, double* __restrict__ ws) {
  __shared__ double red[CG_WORDS][W][256];
  constexpr int UT = CG_CT / W;                  // channel units of a full tile
  const int nu = C / W;                          // channel units of W channels
  const int u0 = blockIdx.z * UT;
  const int nut = min(UT, nu - u0);              // units of this workgroup
  const Lay l = make_lay_q(nut);
  const int PR = l.PR, pr = l.pr;                // pixel rows of the workgroup
  const int c0 = (u0 + l.cq) * W;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const ChunkRange cr = chunk_range(HW, nchunk, chunk);  // p0 < HW: the host makes every chunk non-empty
  const int p0 = cr.p0, p1 = cr.p1;
  double s1[W], s2[W], sa[W];
#pragma unroll
  for (int e = 0; e < W; ++e) s1[e] = s2[e] = sa[e] = 0.0;
  if (pr < PR) {
    float sc[W], sh[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      sc[e] = xf != VAE_XF_NONE ? scale[(int64_t)b * ld + c0 + e] : 1.f;
      sh[e] = xf != VAE_XF_NONE ? shift[(int64_t)b * ld + c0 + e] : 0.f;
    }
    const int64_t xb = (int64_t)b * HW * ld + c0;
    auto take = [&](const float (&v)[W]) {
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float y = xf != VAE_XF_NONE ? affine_xf(v[e], sc[e], sh[e], xf) : v[e];
        const double d = (double)y;
        const double q = d * d;  // exact: 48 significant bits at most
        s1[e] += d;
        s2[e] += q;
        sa[e] += __builtin_fabs(d);
      }
    };
    int pix = p0 + pr;
    // four pixel rows in flight per lane, then the same per-element order as the single-row tail
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
#pragma unroll
  for (int e = 0; e < W; ++e) {
    red[0][e][threadIdx.x] = s1[e];
    red[1][e][threadIdx.x] = s2[e];
    red[2][e][threadIdx.x] = sa[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < nut) {  // pr == 0: c0 is this thread's first channel
    const int64_t row = (int64_t)b * nchunk + chunk;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      double t1 = 0.0, t2 = 0.0, ta = 0.0;
      for (int r = 0; r < PR; ++r) {
        const int i = r * nut + threadIdx.x;
        t1 += red[0][e][i];
        t2 += red[1][e][i];
        ta += red[2][e][i];
      }
      double* dst = ws + (row * C + (c0 + e)) * CG_WORDS;
      dst[0] = t1;
      dst[1] = t2;
      dst[2] = ta;
    }
  }
}

// sums [B][C][3] doubles: word w = (c, j) of image b is the sum over the image's chunks, in chunk order
__global__ __launch_bounds__(256) void changroup_final_kernel(const double* __restrict__ ws, int nchunk, int64_t nw /* C * 3 */,
                                                              double* __restrict__ sums) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (w >= nw) return;
  const double* src = ws + (int64_t)b * nchunk * nw + w;
  double acc = 0.0;
  int r = 0;
  // four rows in flight per thread, added in row order as the single-row tail adds them
  for (; r + 3 < nchunk; r += 4) {
    double t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = src[(int64_t)(r + k) * nw];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += t[k];
  }
  for (; r < nchunk; ++r) acc += src[(int64_t)r * nw];
  sums[(int64_t)b * nw + w] = acc;
}

// what both passes (and the size query) ask of a shape
int check_shape(const char* who, int32_t B, int32_t HW, int32_t C, int32_t nchunk) {
  VAE_CHECK(B > 0 && HW > 0 && C > 0 && nchunk > 0, "%s: bad args (B=%d HW=%d C=%d nchunk=%d)", who, B, HW, C, nchunk);
  VAE_CHECK((int64_t)B * HW < ((int64_t)1 << 31), "%s: B * HW = %lld: 2^31 elements per channel or more", who,
            (long long)((int64_t)B * HW));
  const int per = (HW + nchunk - 1) / nchunk;
  VAE_CHECK(nchunk <= 65535 && B <= 65535 && (int64_t)(nchunk - 1) * per < HW,
            "%s: nchunk=%d for HW=%d leaves an empty chunk (or too many workgroups)", who, nchunk, HW);
  VAE_CHECK((int64_t)B * nchunk < ((int64_t)1 << 31), "%s: B * nchunk = %lld rows", who, (long long)((int64_t)B * nchunk));
  return VAE_OK;
}

}  // namespace

extern "C" int vae_changroup_workspace(int32_t B, int32_t HW, int32_t C, int32_t nchunk, int64_t* ndoubles) {
  VAE_CHECK(ndoubles, "changroup_workspace: null args");
  if (int rc = check_shape("changroup_workspace", B, HW, C, nchunk)) return rc;
  *ndoubles = (int64_t)B * nchunk * C * CG_WORDS;
  return VAE_OK;
}

extern "C" int vae_changroup_partial(const void* x, int32_t x_bf16, const float* scale, const float* shift, int32_t xf, int32_t B,
                                     int32_t HW, int32_t C, int32_t ld, int32_t nchunk, double* ws, void* stream) {
  VAE_CHECK(x && ws, "changroup_partial: null args");
  if (int rc = check_shape("changroup_partial", B, HW, C, nchunk)) return rc;
  VAE_CHECK(ld >= C, "changroup_partial: pixel stride ld=%d below C=%d", ld, C);
  VAE_CHECK(xf == VAE_XF_NONE || xf == VAE_XF_AFFINE || xf == VAE_XF_AFFINE_SILU, "changroup_partial: xf=%d", xf);
  VAE_CHECK(xf == VAE_XF_NONE || (scale && shift), "changroup_partial: xf needs scale and shift");
  VAE_CHECK(aligned16(ws), "changroup_partial: unaligned workspace");
  // four channels per lane where the rows allow a 16 B (fp32) / 8 B (bf16) load, one otherwise
  const uintptr_t amask = x_bf16 ? 7u : 15u;
  const bool vec = C % 4 == 0 && ld % 4 == 0 && (((uintptr_t)x) & amask) == 0;
  const int tiles = (C + CG_CT - 1) / CG_CT;  // C / W units in tiles of CG_CT / W
  VAE_CHECK(tiles <= 65535, "changroup_partial: C=%d: too many channel tiles", C);
  const dim3 grid(nchunk, B, tiles);
  hipStream_t s = (hipStream_t)stream;
  dispatch_bool(vec, [&](auto V) {
    dispatch_bool(x_bf16, [&](auto XB) {
      hipLaunchKernelGGL((changroup_partial_kernel<decltype(V)::value ? 4 : 1, decltype(XB)::value>), grid, dim3(256), 0, s, x, scale,
                         shift, xf, HW, C, ld, nchunk, ws);
    });
  });
  VAE_LAUNCH_CHECK("changroup_partial");
  return VAE_OK;
}

extern "C" int vae_changroup_final(const double* ws, int32_t B, int32_t HW, int32_t C, int32_t nchunk, double* sums, void* stream) {
  VAE_CHECK(ws && sums, "changroup_final: null args");
  if (int rc = check_shape("changroup_final", B, HW, C, nchunk)) return rc;
  VAE_CHECK(aligned16(ws), "changroup_final: unaligned workspace");
  const int64_t nw = (int64_t)C * CG_WORDS;
  const int64_t blocks = (nw + 255) / 256;
  VAE_CHECK(blocks <= 0x7fffffff, "changroup_final: C=%d: too many words", C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(changroup_final_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, ws, nchunk, nw, sums);
  VAE_LAUNCH_CHECK("changroup_final");
  return VAE_OK;
}
