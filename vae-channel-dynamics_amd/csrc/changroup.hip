// Per-(sample, channel) sums of y = XF(x) for the ActivityMonitor's GroupNorm group dynamics and per-sample activity metrics
// (monitor.py): S1 = sum y, S2 = sum y^2 and A = sum |y| over the H * W pixels of every (image b, channel c), in one read of an
// NHWC activation: the inputs of vae_moments_partial (fp32 or bf16 storage, any pixel stride ld >= C, the optional runtime
// GroupNorm(+SiLU) transform applied on the fly).  Nothing here reduces over the batch: that is what the metrics are about.
//
// Partial pass: on the frame of chanstat_common.h: one workgroup per (pixel chunk, image, tile of 256 channels), lanes across
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
#include "chanstat_common.h"

namespace {

constexpr int CG_CT = 256;   // channels of a full tile
constexpr int CG_WORDS = 3;  // sum y, sum y^2, sum |y|

// ws: [B * nchunk][C][CG_WORDS] doubles
template <int W, bool XBF>
__global__ __launch_bounds__(256) void changroup_partial_kernel(const void* __restrict__ x, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, int xf, int HW, int C, int ld,
                                                                int nchunk, double* __restrict__ ws) {
  __shared__ double red[CG_WORDS][W][256];
  const StatFrame f = stat_frame<CG_CT / W, W>(HW, C, nchunk);
  const int c0 = f.c0, b = f.b;
  double s1[W], s2[W], sa[W];
#pragma unroll
  for (int e = 0; e < W; ++e) s1[e] = s2[e] = sa[e] = 0.0;
  if (f.pr < f.PR) {
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
    for_rows<W, XBF>(x, xb, ld, f, take);
  }
#pragma unroll
  for (int e = 0; e < W; ++e) {
    red[0][e][threadIdx.x] = s1[e];
    red[1][e][threadIdx.x] = s2[e];
    red[2][e][threadIdx.x] = sa[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < f.nut) {  // pr == 0: c0 is this thread's first channel
    const int64_t row = (int64_t)b * nchunk + f.chunk;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      double t1 = 0.0, t2 = 0.0, ta = 0.0;
      fold_rows(f, [&](int i) {
        t1 += red[0][e][i];
        t2 += red[1][e][i];
        ta += red[2][e][i];
      });
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

}  // namespace

extern "C" int vae_changroup_workspace(int32_t B, int32_t HW, int32_t C, int32_t nchunk, int64_t* ndoubles) {
  VAE_CHECK(ndoubles, "changroup_workspace: null args");
  if (int rc = stat_check_shape("changroup_workspace", B, HW, C, nchunk)) return rc;
  *ndoubles = (int64_t)B * nchunk * C * CG_WORDS;
  return VAE_OK;
}

extern "C" int vae_changroup_partial(const void* x, int32_t x_bf16, const float* scale, const float* shift, int32_t xf, int32_t B,
                                     int32_t HW, int32_t C, int32_t ld, int32_t nchunk, double* ws, void* stream) {
  VAE_CHECK(x && ws, "changroup_partial: null args");
  if (int rc = stat_check_shape("changroup_partial", B, HW, C, nchunk)) return rc;
  if (int rc = stat_check_xf("changroup_partial", xf, scale, shift, ld, C)) return rc;
  VAE_CHECK(aligned16(ws), "changroup_partial: unaligned workspace");
  const bool vec = vec4_ok(x, x_bf16, C, ld);
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
  if (int rc = stat_check_shape("changroup_final", B, HW, C, nchunk)) return rc;
  VAE_CHECK(aligned16(ws), "changroup_final: unaligned workspace");
  const int64_t nw = (int64_t)C * CG_WORDS;
  const int64_t blocks = (nw + 255) / 256;
  VAE_CHECK(blocks <= 0x7fffffff, "changroup_final: C=%d: too many words", C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(changroup_final_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, ws, nchunk, nw, sums);
  VAE_LAUNCH_CHECK("changroup_final");
  return VAE_OK;
}
