// Activation penalties of the fused train step (vaehip/actreg.py): a loss term on a module's NHWC output a of shape [B][HW][C],
// N = B * HW pixel rows, w_c the 0 / 1 channel mask.
//   ceiling (threshold t):  P = weight / (N C) * sum_c w_c sum relu(|a| - t)^2        dP/da = k_c psi(a), psi(a) = a - clamp(a, -t, t)
//   floor   (threshold t):  P = weight / C * sum_c w_c relu(t - m_c)^2, m_c = mean |a| dP/da = k_c psi(a), psi(a) = sign(a), sign(0) = 0
// with k_c = 2 weight w_c grad_scale / (N C) for the ceiling and -2 weight w_c relu(t - m_c) grad_scale / (N C) for the floor.
//
// Statistics, partial pass: one read of a (fp32 or bf16, pixel stride ld >= C: a channel-prefix view is read in place), on the
// frame of chanstat_common.h: one workgroup per (pixel chunk, image, tile of 256 channels), lanes across channels and pixel rows down
// the chunk, four pixel rows in flight per lane.  A lane keeps, per channel, in fp32 the sum of e^2 with e = |a| - t over the
// elements with !(|a| <= t) (e rounded once, the square rounded once: the library is built with -ffp-contract=off) and the sum of
// |a|, and the number of such elements as an exact 32-bit count.  A NaN counts as over the threshold and makes both sums of its
// channel NaN, an infinity makes them infinite; neither reaches another channel.  The workgroup's pixel rows are added through
// LDS in row order, and three words per (channel, image, chunk) go to ws [C][B * nchunk][3] with plain stores.
//
// Statistics, final pass: one workgroup per channel, float64: thread t adds the rows t, t + 256, ... of its channel in order and
// a fixed LDS tree adds the 256 threads.  It writes the three sums, the channel's share of P and k_c.  No atomics anywhere:
// repeated launches are bitwise identical.
//
// Inject: out = g + k_c psi(a), out of place, grid-stride over units of four channels (one where a 16-byte access -- 8-byte for
// bf16 -- is not possible).  fp32 arithmetic: psi rounded once (exact for the floor), the product rounded once, the sum rounded
// once, a bf16 result rounded once more.  An element whose product is zero passes g on as it is, so a zero coefficient (weight
// 0, a masked channel, a floor that is met) and a ceiling nothing exceeds leave g bit for bit wherever a is finite (0 * inf and
// 0 * NaN are NaN: a non-finite a makes its own element NaN whatever the coefficient).
#include "chanstat_common.h"

namespace {

constexpr int AR_CT = 256;    // channels of a full tile
constexpr int AR_WORDS = 3;   // sum e^2, sum |a|, count
constexpr int AR_CEILING = 0, AR_FLOOR = 1;

// ws: [C][B * nchunk][AR_WORDS] words
template <int W, bool ABF>
__global__ __launch_bounds__(256) void actreg_partial_kernel(const void* __restrict__ a, int HW, int C, int lda, int nchunk, float thr,
                                                             unsigned* __restrict__ ws) {
  __shared__ float red[2][W][256];
  __shared__ unsigned rcnt[W][256];
  const StatFrame f = stat_frame<AR_CT / W, W>(HW, C, nchunk);
  const int c0 = f.c0, b = f.b;
  float se[W], sa[W];
  unsigned cnt[W];
#pragma unroll
  for (int e = 0; e < W; ++e) se[e] = sa[e] = 0.f, cnt[e] = 0u;
  if (f.pr < f.PR) {
    const int64_t ab = (int64_t)b * HW * lda + c0;
    auto take = [&](const float (&va)[W]) {
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float m = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, va[e]) & 0x7fffffffu);
        sa[e] += m;
        if (!(m <= thr)) {  // a NaN is over the threshold
          const float ex = m - thr;
          const float sq = ex * ex;
          se[e] += sq;
          cnt[e] += 1u;
        }
      }
    };
    for_rows<W, ABF>(a, ab, lda, f, take);
  }
#pragma unroll
  for (int e = 0; e < W; ++e) {
    red[0][e][threadIdx.x] = se[e];
    red[1][e][threadIdx.x] = sa[e];
    rcnt[e][threadIdx.x] = cnt[e];
  }
  __syncthreads();
  if ((int)threadIdx.x < f.nut) {  // pr == 0: c0 is this thread's first channel
    const int64_t rows = (int64_t)gridDim.y * nchunk;
    const int64_t row = (int64_t)b * nchunk + f.chunk;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      float te = 0.f, ta = 0.f;
      unsigned tc = 0u;
      fold_rows(f, [&](int i) {
        te += red[0][e][i];
        ta += red[1][e][i];
        tc += rcnt[e][i];
      });
      unsigned* dst = ws + ((int64_t)(c0 + e) * rows + row) * AR_WORDS;
      dst[0] = __builtin_bit_cast(unsigned, te);
      dst[1] = __builtin_bit_cast(unsigned, ta);
      dst[2] = tc;
    }
  }
}

// sums [3][C] doubles = sum relu(|a| - t)^2, sum |a|, count over t; pen [C] doubles; coef [C] floats
__global__ __launch_bounds__(256) void actreg_final_kernel(const unsigned* __restrict__ ws, int rows, int C, int kind, double thr,
                                                           double weight, const float* __restrict__ mask, double grad_scale,
                                                           double n, double* __restrict__ sums, double* __restrict__ pen,
                                                           float* __restrict__ coef) {
  __shared__ double sh[3][256];
  const int c = blockIdx.x, t = threadIdx.x;
  const unsigned* src = ws + (int64_t)c * rows * AR_WORDS;
  double te = 0.0, ta = 0.0, tc = 0.0;  // (a count stays exact: below 2^31 in all)
  int r = t;
  // four rows (twelve loads) in flight per thread, added in row order as the single-row tail adds them
  for (; r + 3 * 256 < rows; r += 4 * 256) {
    unsigned w[4][AR_WORDS];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < AR_WORDS; ++j) w[k][j] = src[(int64_t)(r + k * 256) * AR_WORDS + j];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      te += (double)__builtin_bit_cast(float, w[k][0]);
      ta += (double)__builtin_bit_cast(float, w[k][1]);
      tc += (double)w[k][2];
    }
  }
  for (; r < rows; r += 256) {
    const unsigned* w = src + (int64_t)r * AR_WORDS;
    te += (double)__builtin_bit_cast(float, w[0]);
    ta += (double)__builtin_bit_cast(float, w[1]);
    tc += (double)w[2];
  }
  sh[0][t] = te, sh[1][t] = ta, sh[2][t] = tc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      sh[0][t] += sh[0][t + s];
      sh[1][t] += sh[1][t + s];
      sh[2][t] += sh[2][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double S = sh[0][0], A = sh[1][0];
    sums[c] = S;
    sums[(int64_t)C + c] = A;
    sums[2 * (int64_t)C + c] = sh[2][0];
    const double k = weight * (mask ? (double)mask[c] : 1.0);
    double p = 0.0, kc = 0.0;
    if (k != 0.0) {  // weight 0 or a masked channel: exactly zero, whatever the channel holds
      const double nc = n * (double)C;
      if (kind == AR_CEILING) {
        p = k * S / nc;
        kc = 2.0 * k * grad_scale / nc;
      } else {
        const double d = thr - A / n;
        const double r = d <= 0.0 ? 0.0 : d;  // a NaN mean stays NaN
        p = k * r * r / (double)C;
        kc = r == 0.0 ? 0.0 : -2.0 * k * r * grad_scale / nc;
      }
    }
    pen[c] = p;
    coef[c] = (float)kc;
  }
}

template <int KIND>
__device__ __forceinline__ float psi(float a, float thr) {
  if constexpr (KIND == AR_CEILING) return a - fminf(fmaxf(a, -thr), thr);  // a NaN: fmin / fmax give the bound, a - bound is NaN
  else return a > 0.f ? 1.f : (a < 0.f ? -1.f : a);                        // +-0 and NaN as they are
}

// one unit of W channels per thread and trip; unit i = (pixel row i / nu, channel unit i % nu), stepped without a division per trip
template <int KIND, int W, bool ABF, bool GBF>
__global__ __launch_bounds__(256) void actreg_inject_kernel(const void* __restrict__ a, const void* __restrict__ g,
                                                            const float* __restrict__ coef, int64_t rows, int nu, int lda, int ldg,
                                                            float thr, void* __restrict__ out) {
  const int64_t n = rows * nu;
  const int64_t step = (int64_t)gridDim.x * 256;
  const int64_t dpix = step / nu;
  const int dcq = (int)(step - dpix * nu);
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t pix = i / nu;
  int cq = (int)(i - pix * nu);
  const int ldo = nu * W;
  auto load = [&](int64_t p, int c, float (&va)[W], float (&vg)[W], float (&kc)[W]) {
    load_units<W, ABF>(a, p * lda + (int64_t)c * W, va);
    load_units<W, GBF>(g, p * ldg + (int64_t)c * W, vg);
    load_units<W, false>(coef, (int64_t)c * W, kc);
  };
  auto finish = [&](int64_t p, int c, const float (&va)[W], const float (&vg)[W], const float (&kc)[W]) {
    float vo[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float ps = psi<KIND>(va[e], thr);
      const float pr = kc[e] * ps;
      const float s = vg[e] + pr;
      vo[e] = pr == 0.f ? vg[e] : s;
    }
    const int64_t oo = p * ldo + (int64_t)c * W;
    if constexpr (W == 4) {
      store4<GBF>(out, oo >> 2, f32x4{vo[0], vo[1], vo[2], vo[3]});
    } else if constexpr (GBF) {
      const __bf16 h = (__bf16)vo[0];
      reinterpret_cast<u16*>(out)[oo] = __builtin_bit_cast(u16, h);
    } else {
      reinterpret_cast<float*>(out)[oo] = vo[0];
    }
  };
  auto advance = [&](int64_t& p, int& c) {
    p += dpix;
    c += dcq;
    if (c >= nu) c -= nu, p += 1;
  };
  // two units (six loads) in flight per thread, then the single-unit tail
  for (; i + step < n; i += 2 * step) {
    int64_t pix1 = pix;
    int cq1 = cq;
    advance(pix1, cq1);
    float va[2][W], vg[2][W], kc[2][W];
    load(pix, cq, va[0], vg[0], kc[0]);
    load(pix1, cq1, va[1], vg[1], kc[1]);
    finish(pix, cq, va[0], vg[0], kc[0]);
    finish(pix1, cq1, va[1], vg[1], kc[1]);
    pix = pix1, cq = cq1;
    advance(pix, cq);
  }
  if (i < n) {
    float va[W], vg[W], kc[W];
    load(pix, cq, va, vg, kc);
    finish(pix, cq, va, vg, kc);
  }
}

int check_kind(const char* who, int32_t kind, double threshold) {
  VAE_CHECK(kind == AR_CEILING || kind == AR_FLOOR, "%s: kind=%d (0 = ceiling, 1 = floor)", who, kind);
  VAE_CHECK(threshold > 0.0 && threshold <= 3.0e38, "%s: threshold %g is not a finite positive number", who, threshold);
  return VAE_OK;
}

}  // namespace

extern "C" int vae_actreg_workspace(int32_t B, int32_t HW, int32_t C, int32_t nchunk, int64_t* nwords) {
  VAE_CHECK(nwords, "actreg_workspace: null args");
  if (int rc = stat_check_shape("actreg_workspace", B, HW, C, nchunk)) return rc;
  *nwords = (int64_t)B * nchunk * C * AR_WORDS;
  return VAE_OK;
}

extern "C" int vae_actreg_partial(const void* a, int32_t a_bf16, int32_t lda, int32_t B, int32_t HW, int32_t C, int32_t nchunk,
                                  float threshold, uint32_t* ws, void* stream) {
  VAE_CHECK(a && ws, "actreg_partial: null args");
  if (int rc = stat_check_shape("actreg_partial", B, HW, C, nchunk)) return rc;
  VAE_CHECK(threshold > 0.f && threshold <= 3.0e38f, "actreg_partial: threshold %g is not a finite positive number", (double)threshold);
  VAE_CHECK(lda >= C, "actreg_partial: pixel stride lda=%d below C=%d", lda, C);
  VAE_CHECK(aligned16(ws), "actreg_partial: unaligned workspace");
  const bool vec = vec4_ok(a, a_bf16, C, lda);
  const int tiles = (C + AR_CT - 1) / AR_CT;  // C / W units in tiles of AR_CT / W
  VAE_CHECK(tiles <= 65535, "actreg_partial: C=%d: too many channel tiles", C);
  const dim3 grid(nchunk, B, tiles);
  hipStream_t s = (hipStream_t)stream;
  dispatch_bool(vec, [&](auto V) {
    dispatch_bool(a_bf16, [&](auto AB) {
      hipLaunchKernelGGL((actreg_partial_kernel<decltype(V)::value ? 4 : 1, decltype(AB)::value>), grid, dim3(256), 0, s, a, HW, C, lda,
                         nchunk, threshold, ws);
    });
  });
  VAE_LAUNCH_CHECK("actreg_partial");
  return VAE_OK;
}

extern "C" int vae_actreg_final(const uint32_t* ws, int32_t B, int32_t HW, int32_t C, int32_t nchunk, int32_t kind, double threshold,
                                double weight, const float* mask, double grad_scale, double* sums, double* pen, float* coef,
                                void* stream) {
  VAE_CHECK(ws && sums && pen && coef, "actreg_final: null args");
  if (int rc = stat_check_shape("actreg_final", B, HW, C, nchunk)) return rc;
  if (int rc = check_kind("actreg_final", kind, threshold)) return rc;
  VAE_CHECK(weight >= 0.0 && weight <= 1.0e300, "actreg_final: weight %g is not a finite number >= 0", weight);
  VAE_CHECK(grad_scale == grad_scale && grad_scale >= -1.0e300 && grad_scale <= 1.0e300, "actreg_final: grad_scale %g is not finite",
            grad_scale);
  VAE_CHECK(aligned16(ws), "actreg_final: unaligned workspace");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(actreg_final_kernel, dim3((unsigned)C), dim3(256), 0, s, ws, B * nchunk, C, kind, threshold, weight, mask,
                     grad_scale, (double)B * HW, sums, pen, coef);
  VAE_LAUNCH_CHECK("actreg_final");
  return VAE_OK;
}

extern "C" int vae_actreg_inject(const void* a, int32_t a_bf16, int32_t lda, const void* g, int32_t g_bf16, int32_t ldg,
                                 const float* coef, int64_t rows, int32_t C, int32_t kind, float threshold, void* out, void* stream) {
  VAE_CHECK(a && g && coef && out, "actreg_inject: null args");
  VAE_CHECK(rows > 0 && C > 0 && rows < ((int64_t)1 << 31), "actreg_inject: bad args (rows=%lld C=%d)", (long long)rows, C);
  if (int rc = check_kind("actreg_inject", kind, (double)threshold)) return rc;
  VAE_CHECK(lda >= C && ldg >= C, "actreg_inject: pixel stride lda=%d or ldg=%d below C=%d", lda, ldg, C);
  VAE_CHECK(out != a && out != g, "actreg_inject: out of place only");
  // (out is contiguous: its pixel stride is C)
  const bool vec = vec4_ok(a, a_bf16, C, lda) && vec4_ok(g, g_bf16, C, ldg) && vec4_ok(out, g_bf16, C, C) && aligned16(coef);
  const int nu = vec ? C / 4 : C;
  const dim3 grid(ew_blocks(rows * nu));
  hipStream_t s = (hipStream_t)stream;
  dispatch_bool(kind == AR_FLOOR, [&](auto K) {
    dispatch_bool(vec, [&](auto V) {
      dispatch_bool(a_bf16, [&](auto AB) {
        dispatch_bool(g_bf16, [&](auto GB) {
          hipLaunchKernelGGL((actreg_inject_kernel<decltype(K)::value ? AR_FLOOR : AR_CEILING, decltype(V)::value ? 4 : 1,
                                                   decltype(AB)::value, decltype(GB)::value>),
                             grid, dim3(256), 0, s, a, g, coef, rows, nu, lda, ldg, threshold, out);
        });
      });
    });
  });
  VAE_LAUNCH_CHECK("actreg_inject");
  return VAE_OK;
}
