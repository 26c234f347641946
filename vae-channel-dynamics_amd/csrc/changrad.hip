// Per-channel gradient metrics of one backward pass for the ActivityMonitor (monitor.py CHANGRAD_METRICS), in one read of the
// pair (a, g): a module's NHWC output a and the gradient g of the loss with respect to it.  Per channel c over the N = B * HW
// pixel rows: mean |g|, max |g| (NaN if the channel holds one), the gain gradient sum_b sum_p a g (dL/ds_c at s_c = 1 for an
// output multiplied by a per-channel gain) and the Taylor saliency (1 / B) sum_b |sum_p a g|.  a and g are each fp32 or bf16,
// each with its own pixel stride ld >= C (a channel-prefix view is read in place).
//
// Partial pass: one workgroup per (pixel chunk, image, tile of 256 channels), lanes across channels and pixel rows down the
// chunk as in moments_partial_kernel; four pixel rows of both streams (eight loads) in flight per lane.  A lane keeps, per
// channel, sum |g| and sum a g in fp32 (the product rounded once: the library is built with -ffp-contract=off) and max |g| as a
// bit pattern (for |g| the unsigned order of the patterns is the order of the values, NaN above infinity).  The workgroup's
// pixel rows are added through LDS in row order, and three words per (channel, image, chunk) go to ws [C][B * nchunk][3] with
// plain stores.
//
// Final pass: one workgroup per channel, float64 throughout.  The 256 threads are IB image lanes x CL chunk lanes (CL the
// largest power of two <= min(256, nchunk)): a chunk lane adds its chunks of an image in order, an LDS tree over the chunk
// lanes gives the image's P[b] = sum a g and its sum |g|; the image lane adds P, |P| and sum |g| over its images in order, and
// a last LDS tree over all threads gives the channel's values.  No atomics anywhere: repeated launches are bitwise identical.
#include "chanstat_common.h"

namespace {

constexpr int CG_CT = 256;  // channels of a full tile
constexpr int CG_WORDS = 3;  // sum |g|, sum a g, max |g| bits

// ws: [C][B * nchunk][CG_WORDS] words
template <int W, bool ABF, bool GBF>
__global__ __launch_bounds__(256) void changrad_partial_kernel(const void* __restrict__ a, const void* __restrict__ g, int HW, int C,
                                                               int lda, int ldg, int nchunk, unsigned* __restrict__ ws) {
  __shared__ float red[2][W][256];
  __shared__ unsigned rmax[W][256];
  const StatFrame f = stat_frame<CG_CT / W, W>(HW, C, nchunk);
  const int c0 = f.c0, b = f.b;
  float sg[W], sp[W];
  unsigned amax[W];
#pragma unroll
  for (int e = 0; e < W; ++e) sg[e] = sp[e] = 0.f, amax[e] = 0u;
  if (f.pr < f.PR) {
    const int64_t ab = (int64_t)b * HW * lda + c0;
    const int64_t gb = (int64_t)b * HW * ldg + c0;
    auto take = [&](const float (&va)[W], const float (&vg)[W]) {
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const unsigned m = __builtin_bit_cast(unsigned, vg[e]) & 0x7fffffffu;
        amax[e] = max(amax[e], m);
        sg[e] += __builtin_bit_cast(float, m);
        const float prod = va[e] * vg[e];
        sp[e] += prod;
      }
    };
    const int PR = f.PR, p1 = f.p1;
    int pix = f.p0 + f.pr;
    // four pixel rows of both streams in flight per lane, then the single-row tail: the order of for_rows (chanstat_common.h)
    for (; pix + 3 * PR < p1; pix += 4 * PR) {
      float va[4][W], vg[4][W];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        load_units<W, ABF>(a, ab + (int64_t)(pix + k * PR) * lda, va[k]);
        load_units<W, GBF>(g, gb + (int64_t)(pix + k * PR) * ldg, vg[k]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) take(va[k], vg[k]);
    }
    for (; pix < p1; pix += PR) {
      float va[W], vg[W];
      load_units<W, ABF>(a, ab + (int64_t)pix * lda, va);
      load_units<W, GBF>(g, gb + (int64_t)pix * ldg, vg);
      take(va, vg);
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e) {
    red[0][e][threadIdx.x] = sg[e];
    red[1][e][threadIdx.x] = sp[e];
    rmax[e][threadIdx.x] = amax[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < f.nut) {  // pr == 0: c0 is this thread's first channel
    const int64_t rows = (int64_t)gridDim.y * nchunk;
    const int64_t row = (int64_t)b * nchunk + f.chunk;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      float tg = 0.f, tp = 0.f;
      unsigned tm = 0u;
      fold_rows(f, [&](int i) {
        tg += red[0][e][i];
        tp += red[1][e][i];
        tm = max(tm, rmax[e][i]);
      });
      unsigned* dst = ws + ((int64_t)(c0 + e) * rows + row) * CG_WORDS;
      dst[0] = __builtin_bit_cast(unsigned, tg);
      dst[1] = __builtin_bit_cast(unsigned, tp);
      dst[2] = tm;
    }
  }
}

// sums [3][C] doubles = mean |g|, gain gradient, saliency; absmax [C]
__global__ __launch_bounds__(256) void changrad_final_kernel(const unsigned* __restrict__ ws, int B, int nchunk, int C, int CL,
                                                             double n, double nb, double* __restrict__ sums,
                                                             float* __restrict__ absmax) {
  __shared__ double sh[3][256];
  __shared__ unsigned shm[256];
  const int c = blockIdx.x, t = threadIdx.x;
  const int IB = 256 / CL;                       // images in flight
  const int ib = t / CL, cj = t % CL;
  const unsigned* src = ws + (int64_t)c * B * nchunk * CG_WORDS;
  double tg = 0.0, tgain = 0.0, tsal = 0.0;      // of the images of this image lane (kept by its chunk lane 0)
  unsigned tm = 0u;
  for (int b0 = 0; b0 < B; b0 += IB) {
    const int b = b0 + ib;
    double g = 0.0, p = 0.0;
    unsigned m = 0u;
    if (b < B) {
      for (int k = cj; k < nchunk; k += CL) {
        const unsigned* w = src + ((int64_t)b * nchunk + k) * CG_WORDS;
        g += (double)__builtin_bit_cast(float, w[0]);
        p += (double)__builtin_bit_cast(float, w[1]);
        m = max(m, w[2]);
      }
    }
    sh[0][t] = g, sh[1][t] = p, shm[t] = m;
    __syncthreads();
    for (int s = CL >> 1; s > 0; s >>= 1) {
      if (cj < s) {
        sh[0][t] += sh[0][t + s];
        sh[1][t] += sh[1][t + s];
        shm[t] = max(shm[t], shm[t + s]);
      }
      __syncthreads();
    }
    if (cj == 0 && b < B) {
      const double P = sh[1][t];
      tg += sh[0][t];
      tgain += P;
      tsal += fabs(P);
      tm = max(tm, shm[t]);
    }
    __syncthreads();
  }
  sh[0][t] = tg, sh[1][t] = tgain, sh[2][t] = tsal, shm[t] = tm;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      sh[0][t] += sh[0][t + s];
      sh[1][t] += sh[1][t + s];
      sh[2][t] += sh[2][t + s];
      shm[t] = max(shm[t], shm[t + s]);
    }
    __syncthreads();
  }
  if (t == 0) {
    sums[c] = sh[0][0] / n;
    sums[(int64_t)C + c] = sh[1][0];
    sums[2 * (int64_t)C + c] = sh[2][0] / nb;
    const unsigned mx = shm[0];
    absmax[c] = absmax_of(mx);
  }
}

}  // namespace

extern "C" int vae_changrad_workspace(int32_t B, int32_t HW, int32_t C, int32_t nchunk, int64_t* nwords) {
  VAE_CHECK(nwords, "changrad_workspace: null args");
  if (int rc = stat_check_shape("changrad_workspace", B, HW, C, nchunk)) return rc;
  *nwords = (int64_t)B * nchunk * C * CG_WORDS;
  return VAE_OK;
}

extern "C" int vae_changrad_partial(const void* a, int32_t a_bf16, int32_t lda, const void* g, int32_t g_bf16, int32_t ldg, int32_t B,
                                    int32_t HW, int32_t C, int32_t nchunk, uint32_t* ws, void* stream) {
  VAE_CHECK(a && g && ws, "changrad_partial: null args");
  if (int rc = stat_check_shape("changrad_partial", B, HW, C, nchunk)) return rc;
  VAE_CHECK(lda >= C && ldg >= C, "changrad_partial: pixel stride lda=%d or ldg=%d below C=%d", lda, ldg, C);
  VAE_CHECK(aligned16(ws), "changrad_partial: unaligned workspace");
  const bool vec = vec4_ok(a, a_bf16, C, lda) && vec4_ok(g, g_bf16, C, ldg);
  const int tiles = (C + CG_CT - 1) / CG_CT;  // C / W units in tiles of CG_CT / W
  VAE_CHECK(tiles <= 65535, "changrad_partial: C=%d: too many channel tiles", C);
  const dim3 grid(nchunk, B, tiles);
  hipStream_t s = (hipStream_t)stream;
  dispatch_bool(vec, [&](auto V) {
    dispatch_bool(a_bf16, [&](auto AB) {
      dispatch_bool(g_bf16, [&](auto GB) {
        hipLaunchKernelGGL((changrad_partial_kernel<decltype(V)::value ? 4 : 1, decltype(AB)::value, decltype(GB)::value>), grid,
                           dim3(256), 0, s, a, g, HW, C, lda, ldg, nchunk, ws);
      });
    });
  });
  VAE_LAUNCH_CHECK("changrad_partial");
  return VAE_OK;
}

extern "C" int vae_changrad_final(const uint32_t* ws, int32_t B, int32_t HW, int32_t C, int32_t nchunk, double* sums, float* absmax,
                                  void* stream) {
  VAE_CHECK(ws && sums && absmax, "changrad_final: null args");
  if (int rc = stat_check_shape("changrad_final", B, HW, C, nchunk)) return rc;
  VAE_CHECK(aligned16(ws), "changrad_final: unaligned workspace");
  int CL = 1;
  while (CL * 2 <= nchunk && CL < 256) CL *= 2;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(changrad_final_kernel, dim3((unsigned)C), dim3(256), 0, s, ws, B, nchunk, C, CL, (double)B * HW,
                     (double)B, sums, absmax);
  VAE_LAUNCH_CHECK("changrad_final");
  return VAE_OK;
}
