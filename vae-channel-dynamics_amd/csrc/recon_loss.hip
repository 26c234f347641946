// Reconstruction losses of the fused train step beyond plain MSE, with their gradient seeds (vaehip/losses.py):
//   rec = pixel + ssim_weight * (1 - ssim),  drecon = grad_scale * d rec / d recon
// pixel: mean of d^2 (mse), |d| (l1) or the Huber term (|d| <= delta ? d^2 / 2 : delta (|d| - delta / 2)) of d = fp32(recon - target);
// ssim: the mean SSIM index of u(recon) against u(target), u(v) = (v + 1) / 2 NOT clamped (a clamp would zero the gradient
// exactly where the reconstruction has left [-1, 1]), 11 x 11 gaussian window (sigma 1.5), c1 = 0.01^2, c2 = 0.03^2, over the
// (H - 10) x (W - 10) positions whose whole window lies inside the image: the positions of image_metrics.hip.
//
// Four kernels, no atomics, per-workgroup partials in float64 and one fixed-order final pass: repeated launches are bitwise
// identical.  Every offset is 64-bit.
//   pixel_loss_kernel   one read of recon and target: the partial sums of the term (formed in double from the fp32 d) and
//                       drecon = coef * g(d), one fp32 subtraction and one fp32 multiplication; 16-byte accesses when all
//                       three tensors are 16-byte aligned (and a scalar tail), scalar accesses otherwise.
//   ssim_fwd_kernel     image_metrics_partial_kernel's structure (fp32 halo in LDS, widened on read, separable float64 passes):
//                       per workgroup the sum of the index S, and per window position the float64 coefficients
//                         a = dS/d mu_p, b = dS/d E[p^2], c = dS/d E[p t]      (p = u(recon), t = u(target))
//                       float64 because on nearly flat images the three terms of the gradient cancel (fp32 statistics are off
//                       by 5e-4 of the gradient's maximum there).
//   ssim_bwd_kernel     one workgroup per (image, channel, pixel tile): the transposed gaussian over the halo of the three maps
//                       (zero outside the valid positions), then drecon += (float)(f * (G'a + 2 p G'b + t G'c)),
//                       f = -grad_scale * ssim_weight / (2 * positions); every pixel belongs to exactly one workgroup.
//   recon_final_kernel  pixel, SSIM and KL partials -> scalars[3] = {rec, kl, total}, terms[2] = {pixel, ssim}.
#include <math.h>
#include "stream_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// pixel term
// ---------------------------------------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ float pixel_elem(float r, float x, double delta, float deltaf, float coef, double& acc) {
  const float d = r - x;
  const double dd = (double)d, ad = fabs(dd);
  if (KIND == VAE_LOSS_MSE) {
    acc += dd * dd;
    return coef * d;
  }
  const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (KIND == VAE_LOSS_L1) {
    acc += ad;
    return coef * sgn;
  }
  const bool quad = ad <= delta;
  acc += quad ? 0.5 * dd * dd : delta * (ad - 0.5 * delta);
  return coef * (quad ? d : deltaf * sgn);
}

// the first nq quads with 16-byte accesses (nq = n / 4 when every tensor is 16-byte aligned, else 0), the rest one by one
template <int KIND, bool GRAD>
__global__ __launch_bounds__(256) void pixel_loss_kernel(const float* __restrict__ r, const float* __restrict__ x, int64_t n,
                                                         int64_t nq, double delta, float coef, double* __restrict__ partial,
                                                         float* __restrict__ drec) {
  __shared__ double red[4];
  const float deltaf = (float)delta;
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  for (int64_t i = t0; i < nq; i += stride) {
    const f32x4 a = load4<false>(r, i), b = load4<false>(x, i);
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = pixel_elem<KIND>(a[e], b[e], delta, deltaf, coef, acc);
    if (GRAD) store4<false>(drec, i, g);
  }
  for (int64_t j = 4 * nq + t0; j < n; j += stride) {
    const float g = pixel_elem<KIND>(r[j], x[j], delta, deltaf, coef, acc);
    if (GRAD) drec[j] = g;
  }
  acc = block_reduce<OpAdd>(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

inline int pixel_blocks(int64_t n) { return ew_blocks((n + 3) / 4); }

// ---------------------------------------------------------------------------------------------------------
// SSIM
// ---------------------------------------------------------------------------------------------------------
constexpr int RL_K = 11;                 // window taps
constexpr int RL_TH = 22, RL_TW = 32;    // forward: window positions per tile; backward: pixels per tile
constexpr int RL_HH = RL_TH + RL_K - 1;  // 32 halo rows: 8 runs of 4 columns each = one horizontal work item per lane
constexpr int RL_HW = RL_TW + RL_K - 1;  // 42 halo columns
constexpr int RL_LD = 43;                // LDS row pitch of a halo (odd: the 4 rows x 8 runs of a half wave meet distinct banks, fp32 and float64)
constexpr int RL_RH = 4;                 // outputs per lane, horizontal pass
constexpr int RL_RV = 3;                 // outputs per lane, vertical pass (8 lane rows x 3 >= RL_TH)
constexpr int RL_NST = (RL_HH * RL_HW + 255) / 256;  // halo elements per lane
static_assert(RL_HH * (RL_TW / RL_RH) == 256 && (256 / RL_TW) * RL_RV >= RL_TH, "tile shape and workgroup size belong together");

struct RlWindow { double w[RL_K]; };

__device__ __forceinline__ double to_unit_d(float v) { return ((double)v + 1.0) * 0.5; }

// horizontal pass of Q planes: lane = (halo row, run of RL_RH columns); tap(j) is the window weight that meets halo column c0 + j - o
// of output o, val(j, v) fills the Q values at halo column c0 + j
template <int Q, bool FLIP, class Val>
__device__ __forceinline__ void pass_rows(const RlWindow& win, double (*hq)[RL_HH][RL_TW], Val val) {
  const int row = threadIdx.x / (RL_TW / RL_RH), c0 = (threadIdx.x % (RL_TW / RL_RH)) * RL_RH;
  double h[RL_RH][Q];
#pragma unroll
  for (int o = 0; o < RL_RH; ++o)
#pragma unroll
    for (int q = 0; q < Q; ++q) h[o][q] = 0.0;
#pragma unroll
  for (int j = 0; j < RL_RH + RL_K - 1; ++j) {
    double v[Q];
    val(row, c0 + j, v);
#pragma unroll
    for (int o = 0; o < RL_RH; ++o) {
      if (j - o >= 0 && j - o < RL_K) {
        const double w = win.w[FLIP ? RL_K - 1 - (j - o) : j - o];
#pragma unroll
        for (int q = 0; q < Q; ++q) h[o][q] = fma(w, v[q], h[o][q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int o = 0; o < RL_RH; ++o) hq[q][row][c0 + o] = h[o][q];
}

// vertical pass: lane = (column, run of RL_RV rows) -> s[o][q] for tile rows r0 + o (rows >= RL_TH are the caller's to drop)
template <int Q, bool FLIP>
__device__ __forceinline__ void pass_cols(const RlWindow& win, const double (*hq)[RL_HH][RL_TW], double (&s)[RL_RV][Q]) {
  const int col = threadIdx.x % RL_TW, r0 = (threadIdx.x / RL_TW) * RL_RV;
#pragma unroll
  for (int o = 0; o < RL_RV; ++o)
#pragma unroll
    for (int q = 0; q < Q; ++q) s[o][q] = 0.0;
#pragma unroll
  for (int j = 0; j < RL_RV + RL_K - 1; ++j) {
    const int row = min(r0 + j, RL_HH - 1);  // rows past the halo belong to outputs past the tile
    double v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = hq[q][row][col];
#pragma unroll
    for (int o = 0; o < RL_RV; ++o) {
      if (j - o >= 0 && j - o < RL_K) {
        const double w = win.w[FLIP ? RL_K - 1 - (j - o) : j - o];
#pragma unroll
        for (int q = 0; q < Q; ++q) s[o][q] = fma(w, v[q], s[o][q]);
      }
    }
  }
}

// partial [B * C * tiles] = sum of S over the tile's positions; maps [3][B * C][H - 10][W - 10] = a, b, c (null: forward only)
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ pred, int64_t psb, int64_t psc, int64_t psh,
                                                       int64_t psw, const float* __restrict__ target, int64_t tsb, int64_t tsc,
                                                       int64_t tsh, int64_t tsw, int C, int H, int W, int tiles_x, int tiles_y,
                                                       int64_t plane, RlWindow win, double* __restrict__ partial,
                                                       double* __restrict__ maps) {
  __shared__ float sp[RL_HH * RL_LD], st[RL_HH * RL_LD];
  __shared__ double hq[5][RL_HH][RL_TW];  // horizontally filtered p, t, p^2, t^2, p t
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int bc = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int ty = tile / tiles_x, tx = tile % tiles_x;
  const int b = bc / C, c = bc % C;
  const int y0 = ty * RL_TH, x0 = tx * RL_TW;
  const int Hp = H - (RL_K - 1), Wp = W - (RL_K - 1);
  const float* pb = pred + ((int64_t)b * psb + (int64_t)c * psc);
  const float* tb = target + ((int64_t)b * tsb + (int64_t)c * tsc);

  // the halo as given (fp32 is exact for it); elements outside the image feed only positions that are dropped below
  float pv[RL_NST], tv[RL_NST];
#pragma unroll
  for (int k = 0; k < RL_NST; ++k) {
    const int i = tid + k * 256;
    const int y = y0 + i / RL_HW, x = x0 + i % RL_HW;
    const bool in = i < RL_HH * RL_HW && y < H && x < W;
    pv[k] = in ? pb[(int64_t)y * psh + (int64_t)x * psw] : 0.f;
    tv[k] = in ? tb[(int64_t)y * tsh + (int64_t)x * tsw] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < RL_NST; ++k) {
    const int i = tid + k * 256;
    if (i < RL_HH * RL_HW) {
      sp[(i / RL_HW) * RL_LD + i % RL_HW] = pv[k];
      st[(i / RL_HW) * RL_LD + i % RL_HW] = tv[k];
    }
  }
  __syncthreads();
  pass_rows<5, false>(win, hq, [&](int row, int col, double* v) {
    const double p = to_unit_d(sp[row * RL_LD + col]), t = to_unit_d(st[row * RL_LD + col]);
    v[0] = p;
    v[1] = t;
    v[2] = p * p;
    v[3] = t * t;
    v[4] = p * t;
  });
  __syncthreads();
  double s[RL_RV][5];
  pass_cols<5, false>(win, hq, s);
  const int col = tid % RL_TW, r0 = (tid / RL_TW) * RL_RV;
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  double acc = 0.0;
#pragma unroll
  for (int o = 0; o < RL_RV; ++o) {
    const int r = r0 + o;
    if (r < RL_TH && y0 + r < Hp && x0 + col < Wp) {
      const double mp = s[o][0], mt = s[o][1];
      const double spp = s[o][2] - mp * mp, stt = s[o][3] - mt * mt, spt = s[o][4] - mp * mt;
      const double A1 = 2.0 * mp * mt + c1, A2 = 2.0 * spt + c2, B1 = mp * mp + mt * mt + c1, B2 = spp + stt + c2;
      const double inv = 1.0 / (B1 * B2);
      const double S = (A1 * A2) / (B1 * B2);
      acc += S;
      if (maps) {
        double* m = maps + (((int64_t)bc * Hp + (y0 + r)) * Wp + (x0 + col));
        m[0] = (2.0 * mt * A2 - 2.0 * mt * A1) * inv - S * (2.0 * mp / B1 - 2.0 * mp / B2);
        m[plane] = -S / B2;
        m[2 * plane] = 2.0 * A1 * inv;
      }
    }
  }
  acc = block_reduce<OpAdd>(acc, red);
  if (tid == 0) partial[blockIdx.x] = acc;
}

// drec[pixel] += (float)(f * (G'a + 2 p G'b + t G'c)); G' = the transposed gaussian over the valid-position maps
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ pred, int64_t psb, int64_t psc, int64_t psh,
                                                       int64_t psw, const float* __restrict__ target, int64_t tsb, int64_t tsc,
                                                       int64_t tsh, int64_t tsw, const double* __restrict__ maps, int C, int H,
                                                       int W, int tiles_x, int tiles_y, int64_t plane, RlWindow win, double f,
                                                       float* __restrict__ drec, int64_t dsb, int64_t dsc, int64_t dsh,
                                                       int64_t dsw) {
  __shared__ double sm[3][RL_HH * RL_LD];  // a, b, c at positions (y0 - 10 + row, x0 - 10 + column)
  __shared__ double hq[3][RL_HH][RL_TW];
  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int bc = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int ty = tile / tiles_x, tx = tile % tiles_x;
  const int b = bc / C, c = bc % C;
  const int y0 = ty * RL_TH, x0 = tx * RL_TW;
  const int Hp = H - (RL_K - 1), Wp = W - (RL_K - 1);
  const double* mb = maps + (int64_t)bc * Hp * Wp;

  double mv[3][RL_NST];
#pragma unroll
  for (int k = 0; k < RL_NST; ++k) {
    const int i = tid + k * 256;
    const int py = y0 - (RL_K - 1) + i / RL_HW, px = x0 - (RL_K - 1) + i % RL_HW;
    const bool in = i < RL_HH * RL_HW && py >= 0 && py < Hp && px >= 0 && px < Wp;
    const int64_t off = (int64_t)py * Wp + px;
#pragma unroll
    for (int q = 0; q < 3; ++q) mv[q][k] = in ? mb[off + q * plane] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < RL_NST; ++k) {
    const int i = tid + k * 256;
    if (i < RL_HH * RL_HW) {
#pragma unroll
      for (int q = 0; q < 3; ++q) sm[q][(i / RL_HW) * RL_LD + i % RL_HW] = mv[q][k];
    }
  }
  __syncthreads();
  // pixel x0 + o gathers positions x0 + o - k with weight w[k]: halo column o + j carries k = 10 - j
  pass_rows<3, true>(win, hq, [&](int row, int col, double* v) {
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = sm[q][row * RL_LD + col];
  });
  __syncthreads();
  double s[RL_RV][3];
  pass_cols<3, true>(win, hq, s);
  const int col = tid % RL_TW, r0 = (tid / RL_TW) * RL_RV;
#pragma unroll
  for (int o = 0; o < RL_RV; ++o) {
    const int y = y0 + r0 + o, x = x0 + col;
    if (r0 + o < RL_TH && y < H && x < W) {
      const double p = to_unit_d(pred[(int64_t)b * psb + (int64_t)c * psc + (int64_t)y * psh + (int64_t)x * psw]);
      const double t = to_unit_d(target[(int64_t)b * tsb + (int64_t)c * tsc + (int64_t)y * tsh + (int64_t)x * tsw]);
      float* d = drec + ((int64_t)b * dsb + (int64_t)c * dsc + (int64_t)y * dsh + (int64_t)x * dsw);
      *d += (float)(f * (s[o][0] + 2.0 * p * s[o][1] + t * s[o][2]));
    }
  }
}

// one workgroup per image: out[b] = mean of S over the image's C * (H - 10) * (W - 10) positions
__global__ __launch_bounds__(256) void ssim_index_kernel(const double* __restrict__ partial, int cells, double positions,
                                                         double* __restrict__ out) {
  __shared__ double red[4];
  const double* w = partial + (int64_t)blockIdx.x * cells;
  double acc = 0.0;
  for (int i = threadIdx.x; i < cells; i += 256) acc += w[i];
  acc = block_reduce<OpAdd>(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = acc / positions;
}

__global__ __launch_bounds__(256) void recon_final_kernel(const double* __restrict__ pix, int npix, double n,
                                                          const double* __restrict__ ssim, int64_t nssim, double positions,
                                                          double ssim_weight, const float* __restrict__ kl_partial, int nkl,
                                                          double B, double kl_weight, float* __restrict__ scalars,
                                                          float* __restrict__ terms) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < npix; i += 256) s += pix[i];
  s = block_reduce<OpAdd>(s, red);
  double q = 0.0;
  for (int64_t i = threadIdx.x; i < nssim; i += 256) q += ssim[i];
  q = block_reduce<OpAdd>(q, red);
  double k = 0.0;
  for (int i = threadIdx.x; i < nkl; i += 256) k += (double)kl_partial[i];
  k = block_reduce<OpAdd>(k, red);
  if (threadIdx.x == 0) {
    const double pixel = s / n, kl = k / B;
    double rec = pixel, index = NAN;  // no SSIM term: terms[1] says so
    if (ssim) {
      index = q / positions;
      rec = pixel + ssim_weight * (1.0 - index);
    }
    scalars[0] = (float)rec;
    scalars[1] = (float)kl;
    scalars[2] = (float)(rec + kl_weight * kl);
    terms[0] = (float)pixel;
    terms[1] = (float)index;
  }
}

struct RlPlan { int tiles_x, tiles_y; int64_t cells, plane; };  // cells: forward workgroups per image; plane: doubles of one map

// fwd: tiles of window positions; bwd: tiles of pixels
int ssim_plan(const char* who, bool bwd, int32_t B, int32_t C, int32_t H, int32_t W, RlPlan* p) {
  VAE_CHECK(B > 0 && C > 0, "%s: B=%d C=%d (need B >= 1 and C >= 1)", who, B, C);
  VAE_CHECK(H >= RL_K && W >= RL_K, "%s: a %d x %d image is smaller than the %d x %d SSIM window", who, H, W, RL_K, RL_K);
  const int h = bwd ? H : H - (RL_K - 1), w = bwd ? W : W - (RL_K - 1);
  p->tiles_y = (h + RL_TH - 1) / RL_TH;
  p->tiles_x = (w + RL_TW - 1) / RL_TW;
  p->cells = (int64_t)C * p->tiles_y * p->tiles_x;
  p->plane = (int64_t)B * C * (H - (RL_K - 1)) * (W - (RL_K - 1));
  VAE_CHECK(p->cells * B <= 0x7fffffff, "%s: %d x %d x %d x %d needs more than 2^31 - 1 workgroups", who, B, C, H, W);
  return VAE_OK;
}

RlWindow make_window() {  // exp(-(i - 5)^2 / (2 sigma^2)), normalised: the window of evaluate.ssim_per_image
  RlWindow win;
  double sum = 0.0;
  for (int i = 0; i < RL_K; ++i) {
    const double a = ((double)i - (RL_K - 1) / 2.0) / 1.5;
    win.w[i] = exp(-(a * a) / 2.0);
    sum += win.w[i];
  }
  for (int i = 0; i < RL_K; ++i) win.w[i] /= sum;
  return win;
}

inline bool al(const void* p, unsigned mask) { return ((uintptr_t)p & mask) == 0; }

}  // namespace

extern "C" int vae_pixel_loss_blocks(int64_t n) { return n > 0 ? pixel_blocks(n) : VAE_EINVAL; }

extern "C" int vae_pixel_loss(const float* recon, const float* target, int64_t n, int32_t kind, double delta, double grad_scale,
                              double* partial, float* drecon, void* stream) {
  VAE_CHECK(recon && target && partial, "pixel_loss: null args");
  VAE_CHECK(n > 0, "pixel_loss: n=%lld (need n >= 1)", (long long)n);
  VAE_CHECK(kind == VAE_LOSS_MSE || kind == VAE_LOSS_L1 || kind == VAE_LOSS_HUBER, "pixel_loss: unknown kind %d", kind);
  VAE_CHECK(kind != VAE_LOSS_HUBER || (delta > 0.0 && isfinite(delta)), "pixel_loss: huber delta=%g (need a finite delta > 0)", delta);
  VAE_CHECK(isfinite(grad_scale), "pixel_loss: grad_scale=%g", grad_scale);
  VAE_CHECK(al(recon, 3) && al(target, 3) && al(drecon, 3) && al(partial, 7), "pixel_loss: unaligned operand, result or workspace");
  const int64_t nq = al(recon, 15) && al(target, 15) && al(drecon, 15) ? n / 4 : 0;
  const float coef = (float)(grad_scale * (kind == VAE_LOSS_MSE ? 2.0 : 1.0) / (double)n);
  const dim3 grid(pixel_blocks(n));
  auto launch = [&](auto k) {
    dispatch_bool(drecon != nullptr, [&](auto g) {
      hipLaunchKernelGGL((pixel_loss_kernel<decltype(k)::value, decltype(g)::value>), grid, dim3(256), 0, (hipStream_t)stream, recon,
                         target, n, nq, delta, coef, partial, drecon);
    });
  };
  if (kind == VAE_LOSS_MSE) launch(std::integral_constant<int, VAE_LOSS_MSE>{});
  else if (kind == VAE_LOSS_L1) launch(std::integral_constant<int, VAE_LOSS_L1>{});
  else launch(std::integral_constant<int, VAE_LOSS_HUBER>{});
  VAE_LAUNCH_CHECK("pixel_loss");
  return VAE_OK;
}

extern "C" int vae_ssim_tile(int32_t axis) { return axis == 0 ? RL_TH : axis == 1 ? RL_TW : VAE_EINVAL; }

extern "C" int vae_ssim_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int64_t* npartial, int64_t* nmaps) {
  VAE_CHECK(npartial && nmaps, "ssim_workspace: null result pointer");
  RlPlan p;
  if (int rc = ssim_plan("ssim_workspace", false, B, C, H, W, &p)) return rc;
  *npartial = p.cells * B;
  *nmaps = 3 * p.plane;
  return VAE_OK;
}

extern "C" int vae_ssim_fwd(const float* pred, int64_t psb, int64_t psc, int64_t psh, int64_t psw, const float* target, int64_t tsb,
                            int64_t tsc, int64_t tsh, int64_t tsw, int32_t B, int32_t C, int32_t H, int32_t W, double* partial,
                            double* maps, void* stream) {
  VAE_CHECK(pred && target && partial, "ssim_fwd: null args");
  VAE_CHECK(al(pred, 3) && al(target, 3) && al(partial, 7) && al(maps, 7), "ssim_fwd: unaligned operand or workspace");
  RlPlan p;
  if (int rc = ssim_plan("ssim_fwd", false, B, C, H, W, &p)) return rc;
  hipLaunchKernelGGL(ssim_fwd_kernel, dim3((unsigned)(p.cells * B)), dim3(256), 0, (hipStream_t)stream, pred, psb, psc, psh, psw,
                     target, tsb, tsc, tsh, tsw, C, H, W, p.tiles_x, p.tiles_y, p.plane, make_window(), partial, maps);
  VAE_LAUNCH_CHECK("ssim_fwd");
  return VAE_OK;
}

extern "C" int vae_ssim_bwd(const float* pred, int64_t psb, int64_t psc, int64_t psh, int64_t psw, const float* target, int64_t tsb,
                            int64_t tsc, int64_t tsh, int64_t tsw, const double* maps, int32_t B, int32_t C, int32_t H, int32_t W,
                            double scale, float* drecon, int64_t dsb, int64_t dsc, int64_t dsh, int64_t dsw, void* stream) {
  VAE_CHECK(pred && target && maps && drecon, "ssim_bwd: null args");
  VAE_CHECK(al(pred, 3) && al(target, 3) && al(drecon, 3) && al(maps, 7), "ssim_bwd: unaligned operand, result or workspace");
  VAE_CHECK(isfinite(scale), "ssim_bwd: scale=%g", scale);
  RlPlan p;
  if (int rc = ssim_plan("ssim_bwd", true, B, C, H, W, &p)) return rc;
  const double f = -scale * 0.5 / (double)p.plane;
  hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)(p.cells * B)), dim3(256), 0, (hipStream_t)stream, pred, psb, psc, psh, psw,
                     target, tsb, tsc, tsh, tsw, maps, C, H, W, p.tiles_x, p.tiles_y, p.plane, make_window(), f, drecon, dsb, dsc,
                     dsh, dsw);
  VAE_LAUNCH_CHECK("ssim_bwd");
  return VAE_OK;
}

extern "C" int vae_ssim_index(const double* partial, int32_t B, int32_t C, int32_t H, int32_t W, double* out, void* stream) {
  VAE_CHECK(partial && out, "ssim_index: null args");
  VAE_CHECK(al(partial, 7) && al(out, 7), "ssim_index: unaligned workspace or result");
  RlPlan p;
  if (int rc = ssim_plan("ssim_index", false, B, C, H, W, &p)) return rc;
  hipLaunchKernelGGL(ssim_index_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, partial, (int)p.cells,
                     (double)(p.plane / B), out);
  VAE_LAUNCH_CHECK("ssim_index");
  return VAE_OK;
}

extern "C" int vae_recon_loss_final(const double* pixel_partial, int64_t n, const double* ssim_partial, int32_t B, int32_t C,
                                    int32_t H, int32_t W, double ssim_weight, const float* kl_partial, int32_t kl_nblk,
                                    float kl_weight, float* scalars, float* terms, void* stream) {
  VAE_CHECK(pixel_partial && kl_partial && scalars && terms, "recon_loss_final: null args");
  VAE_CHECK(n > 0 && B > 0 && kl_nblk > 0, "recon_loss_final: n=%lld B=%d kl_nblk=%d", (long long)n, B, kl_nblk);
  VAE_CHECK(al(pixel_partial, 7) && al(ssim_partial, 7) && al(kl_partial, 3) && al(scalars, 3) && al(terms, 3),
            "recon_loss_final: unaligned workspace or result");
  VAE_CHECK(ssim_weight >= 0.0 && isfinite(ssim_weight), "recon_loss_final: ssim_weight=%g (need a finite weight >= 0)", ssim_weight);
  RlPlan p = {0, 0, 0, 1};
  if (ssim_partial) {
    if (int rc = ssim_plan("recon_loss_final", false, B, C, H, W, &p)) return rc;
  }
  hipLaunchKernelGGL(recon_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pixel_partial, pixel_blocks(n), (double)n,
                     ssim_partial, p.cells * B, (double)p.plane, ssim_weight, kl_partial, B * kl_nblk, (double)B, (double)kl_weight,
                     scalars, terms);
  VAE_LAUNCH_CHECK("recon_loss_final");
  return VAE_OK;
}
