// Whole-tensor moments for the ActivityMonitor metrics that are not the fused mean |A| (monitor.py:56-80): per-channel mean |y|,
// the mean and the unbiased std of y = XF(x), for an NHWC activation stored as fp32 or bf16, with an optional GroupNorm(+SiLU)
// transform applied on the fly (no gn_apply) and any pixel stride ld >= C (a channel-prefix view is read in place).
//
// Partial pass: one workgroup per (pixel chunk, image, tile of 256 channel units), lanes across channels as in
// gn_track_partial_kernel.  Each (b, chunk, c) cell leaves sum|y|, sum(y - K), sum((y - K)^2) and K, where the pivot K is y at
// the chunk's first pixel: inside a chunk the shifted sums of all lanes share one pivot and simply add, and nothing of the form
// sum(y^2) - n mean^2 is ever formed in fp32.  Final pass: the cells of each channel are turned into (mean, M2) and merged in fp64
// with Chan's formula (one workgroup per channel), then the channels are merged the same way (one workgroup).  Every reduction is
// a fixed-order loop or LDS tree: no atomics, repeated launches are bitwise identical.
#include "chanstat_common.h"

namespace {

template <int W>
__device__ __forceinline__ void apply_xf(float (&v)[W], const float (&sc)[W], const float (&sh)[W], int xf) {
  if (xf == VAE_XF_NONE) return;
#pragma unroll
  for (int e = 0; e < W; ++e) v[e] = affine_xf(v[e], sc[e], sh[e], xf);
}

// ws: [C][B * nchunk] cells of {sum|y|, sum(y - K), sum((y - K)^2), K}
template <int W, bool XBF>
__global__ __launch_bounds__(256) void moments_partial_kernel(const void* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int xf, int HW, int C, int ld,
                                                              int nchunk, float* __restrict__ ws) {
  __shared__ float red[3][W][256];
  const StatFrame f = stat_frame<256, W>(HW, C, nchunk);  // tiles of 256 units, whatever W
  const int PR = f.PR, c0 = f.c0, b = f.b, p0 = f.p0, p1 = f.p1;
  float sc[W], sh[W];
#pragma unroll
  for (int e = 0; e < W; ++e) {
    sc[e] = xf != VAE_XF_NONE ? scale[(int64_t)b * ld + c0 + e] : 1.f;
    sh[e] = xf != VAE_XF_NONE ? shift[(int64_t)b * ld + c0 + e] : 0.f;
  }
  const int64_t xb = (int64_t)b * HW * ld + c0;
  float K[W];
  load_units<W, XBF>(x, xb + (int64_t)p0 * ld, K);
  apply_xf<W>(K, sc, sh, xf);
  float sa[W], s1[W], s2[W];
#pragma unroll
  for (int e = 0; e < W; ++e) sa[e] = s1[e] = s2[e] = 0.f;
  if (f.pr < PR) {
    int pix = p0 + f.pr;
    // four loads in flight per lane, then the single-pixel tail: the order of for_rows (chanstat_common.h), spelled out here
    for (; pix + 3 * PR < p1; pix += 4 * PR) {
      float v[4][W];
#pragma unroll
      for (int k = 0; k < 4; ++k) load_units<W, XBF>(x, xb + (int64_t)(pix + k * PR) * ld, v[k]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        apply_xf<W>(v[k], sc, sh, xf);
#pragma unroll
        for (int e = 0; e < W; ++e) {
          const float d = v[k][e] - K[e];
          sa[e] += fabsf(v[k][e]);
          s1[e] += d;
          s2[e] += d * d;
        }
      }
    }
    for (; pix < p1; pix += PR) {
      float v[W];
      load_units<W, XBF>(x, xb + (int64_t)pix * ld, v);
      apply_xf<W>(v, sc, sh, xf);
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float d = v[e] - K[e];
        sa[e] += fabsf(v[e]);
        s1[e] += d;
        s2[e] += d * d;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e) {
    red[0][e][threadIdx.x] = sa[e];
    red[1][e][threadIdx.x] = s1[e];
    red[2][e][threadIdx.x] = s2[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < f.nut) {
    const int64_t rows = (int64_t)gridDim.y * nchunk;
    const int64_t row = (int64_t)b * nchunk + f.chunk;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      f32x4 t = {0.f, 0.f, 0.f, K[e]};
      fold_rows(f, [&](int i) {
        t[0] += red[0][e][i];
        t[1] += red[1][e][i];
        t[2] += red[2][e][i];
      });
      store4<false>(ws, (int64_t)(c0 + e) * rows + row, t);
    }
  }
}

struct Mom { double n, m, M2; };
__device__ __forceinline__ Mom mom_merge(Mom a, Mom b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, d = b.m - a.m;
  return Mom{n, a.m + d * (b.n / n), a.M2 + b.M2 + d * d * (a.n * b.n / n)};
}

// fixed LDS tree over 256 lanes; lane 0 ends with the merge of all
__device__ __forceinline__ Mom mom_block(Mom a, double (*red)[256]) {
  red[0][threadIdx.x] = a.n;
  red[1][threadIdx.x] = a.m;
  red[2][threadIdx.x] = a.M2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const Mom r = mom_merge(Mom{red[0][threadIdx.x], red[1][threadIdx.x], red[2][threadIdx.x]},
                              Mom{red[0][threadIdx.x + o], red[1][threadIdx.x + o], red[2][threadIdx.x + o]});
      red[0][threadIdx.x] = r.n;
      red[1][threadIdx.x] = r.m;
      red[2][threadIdx.x] = r.M2;
    }
    __syncthreads();
  }
  return Mom{red[0][0], red[1][0], red[2][0]};
}

// one workgroup per channel: out[c] = mean |y|; chan[c] = (mean, M2) of the channel
__global__ __launch_bounds__(256) void moments_channel_kernel(const float* __restrict__ ws, int B, int HW, int nchunk,
                                                              double* __restrict__ chan, float* __restrict__ out) {
  __shared__ double red[3][256];
  const int c = blockIdx.x;
  const int rows = B * nchunk;
  const int per = (HW + nchunk - 1) / nchunk;
  Mom a{0.0, 0.0, 0.0};
  double sa = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const f32x4 t = load4<false>(ws, (int64_t)c * rows + r);
    const ChunkRange cr = chunk_span(HW, per, r % nchunk);
    const double n = (double)(cr.p1 - cr.p0);
    const double s1 = t[1], dm = s1 / n;
    sa += (double)t[0];
    a = mom_merge(a, Mom{n, (double)t[3] + dm, fmax((double)t[2] - s1 * dm, 0.0)});
  }
  const Mom m = mom_block(a, red);
  // sum |y|: a second tree over the same LDS (the moments of lane 0 are in registers now)
  __syncthreads();
  red[0][threadIdx.x] = sa;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[0][threadIdx.x] += red[0][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[c] = (float)(red[0][0] / ((double)B * (double)HW));
    chan[2 * c] = m.m;
    chan[2 * c + 1] = m.M2;
  }
}

// one workgroup: out[C] = mean, out[C + 1] = unbiased std over all B * HW * C elements (NaN when there is one element, as torch)
__global__ __launch_bounds__(256) void moments_total_kernel(const double* __restrict__ chan, int C, double n_each,
                                                            float* __restrict__ out) {
  __shared__ double red[3][256];
  Mom a{0.0, 0.0, 0.0};
  for (int c = threadIdx.x; c < C; c += 256) a = mom_merge(a, Mom{n_each, chan[2 * c], chan[2 * c + 1]});
  const Mom m = mom_block(a, red);
  if (threadIdx.x == 0) {
    out[C] = (float)m.m;
    out[C + 1] = (float)sqrt(m.M2 / (m.n - 1.0));
  }
}

}  // namespace

extern "C" int vae_moments_partial(const void* x, int32_t x_bf16, const float* scale, const float* shift, int32_t xf, int32_t B,
                                   int32_t HW, int32_t C, int32_t ld, int32_t nchunk, float* ws, void* stream) {
  VAE_CHECK(x && ws && B > 0 && HW > 0 && C > 0 && ld >= C && nchunk > 0, "moments_partial: bad args");
  if (int rc = stat_check_xf("moments_partial", xf, scale, shift, ld, C)) return rc;
  const int per = (HW + nchunk - 1) / nchunk;
  VAE_CHECK(nchunk <= 65535 && B <= 65535 && (int64_t)(nchunk - 1) * per < HW,
            "moments_partial: nchunk=%d for HW=%d leaves an empty chunk (or too many workgroups)", nchunk, HW);
  VAE_CHECK(aligned16(ws), "moments_partial: unaligned workspace");
  const bool vec = vec4_ok(x, x_bf16, C, ld);
  const int W = vec ? 4 : 1;
  const int tiles = (C / W + 255) / 256;
  const dim3 grid(nchunk, B, tiles);
  hipStream_t s = (hipStream_t)stream;
  dispatch_bool(vec, [&](auto V) {
    dispatch_bool(x_bf16, [&](auto XB) {
      hipLaunchKernelGGL((moments_partial_kernel<decltype(V)::value ? 4 : 1, decltype(XB)::value>), grid, dim3(256), 0, s, x, scale, shift, xf, HW,
                         C, ld, nchunk, ws);
    });
  });
  VAE_LAUNCH_CHECK("moments_partial");
  return VAE_OK;
}

extern "C" int vae_moments_final(const float* ws, int32_t B, int32_t HW, int32_t C, int32_t nchunk, double* chan, float* out,
                                 void* stream) {
  VAE_CHECK(ws && chan && out && B > 0 && HW > 0 && C > 0 && nchunk > 0 && (int64_t)B * nchunk <= 0x7fffffff,
            "moments_final: bad args");
  VAE_CHECK(aligned16(ws), "moments_final: unaligned workspace");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(moments_channel_kernel, dim3(C), dim3(256), 0, s, ws, B, HW, nchunk, chan, out);
  VAE_LAUNCH_CHECK("moments_final");
  hipLaunchKernelGGL(moments_total_kernel, dim3(1), dim3(256), 0, s, chan, C, (double)B * (double)HW, out);
  VAE_LAUNCH_CHECK("moments_final");
  return VAE_OK;
}
