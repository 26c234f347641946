// Image-quality metrics of a reconstruction against its target (evaluate.py: Average MSE, PSNR, SSIM): per image the sum of
// squared differences of the values as given, the same sum of the [0,1]-mapped values u(x) = clamp((x + 1) / 2, 0, 1), and the
// mean SSIM index of u(pred) against u(target) over the positions whose whole 11 x 11 gaussian window (sigma 1.5) lies inside
// the image -- the positions torchmetrics keeps after its reflect-padded convolution and 5-pixel crop, so no padding exists here
// and nothing outside an image is read.  Both operands are fp32 with four element strides each (NCHW, channels-last, batch
// slices: read in place); every offset is 64-bit.
//
// Partial pass: one workgroup per (image, channel, tile of IM_TH x IM_TW window positions).  The 32 x 42 halo of u(pred) and
// u(target) is staged in LDS as fp32 (the values are exact there); the squared differences are summed while staging, each pixel
// by the one tile that owns it (the last tile row / column also owns the 10 border pixels behind it).  Horizontal 11-tap pass
// over p, t, p^2, t^2, p t in float64 into LDS, vertical pass and the index from LDS.  The window statistics are float64
// because var = E[x^2] - mu^2 in fp32 costs 1e-4 of the index on flat regions (evaluate.ssim_per_image).  Each workgroup leaves
// three doubles; the final pass adds the C * tiles cells of an image in a fixed order.  No atomics: repeated launches are
// bitwise identical.
#include <math.h>
#include "common.h"

namespace {

constexpr int IM_K = 11;                 // window taps
constexpr int IM_TH = 22, IM_TW = 32;    // window positions per tile
constexpr int IM_HH = IM_TH + IM_K - 1;  // 32 halo rows: 8 runs of 4 columns each = one horizontal work item per lane
constexpr int IM_HW = IM_TW + IM_K - 1;  // 42 halo columns
constexpr int IM_LD = 43;                // LDS row pitch of the fp32 halo (odd: the 4 rows x 8 runs of a half wave meet 32 banks)
constexpr int IM_RH = 4;                 // outputs per lane, horizontal pass
constexpr int IM_RV = 3;                 // outputs per lane, vertical pass (8 lane rows x 3 >= IM_TH)
static_assert(IM_HH * (IM_TW / IM_RH) == 256 && (256 / IM_TW) * IM_RV >= IM_TH, "tile shape and workgroup size belong together");

struct ImWindow { double w[IM_K]; };

__device__ __forceinline__ float to_unit_f(float x) { return fminf(fmaxf((x + 1.0f) * 0.5f, 0.0f), 1.0f); }

// fixed LDS tree over 256 lanes for three sums; the result is valid in lane 0
__device__ __forceinline__ void block_sum3(double (&v)[3], double* red) {
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k * 256 + threadIdx.x] = v[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k * 256 + threadIdx.x] += red[k * 256 + threadIdx.x + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = red[k * 256];
}

// ws [B * C][tiles_y * tiles_x][3] = {sum (p - t)^2, sum (u(p) - u(t))^2, sum of the SSIM index} of the cell
__global__ __launch_bounds__(256) void image_metrics_partial_kernel(const float* __restrict__ pred, int64_t psb, int64_t psc,
                                                                    int64_t psh, int64_t psw, const float* __restrict__ target,
                                                                    int64_t tsb, int64_t tsc, int64_t tsh, int64_t tsw, int C, int H,
                                                                    int W, int tiles_x, int tiles_y, ImWindow win,
                                                                    double* __restrict__ ws) {
  __shared__ float sp[IM_HH * IM_LD], st[IM_HH * IM_LD];
  __shared__ double hq[5][IM_HH][IM_TW];  // horizontally filtered p, t, p^2, t^2, p t; afterwards the reduction's scratch
  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int bc = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int ty = tile / tiles_x, tx = tile % tiles_x;
  const int b = bc / C, c = bc % C;
  const int y0 = ty * IM_TH, x0 = tx * IM_TW;
  const int own_h = ty == tiles_y - 1 ? IM_HH : IM_TH;  // pixels whose squared differences this tile adds
  const int own_w = tx == tiles_x - 1 ? IM_HW : IM_TW;
  const float* pb = pred + ((int64_t)b * psb + (int64_t)c * psc);
  const float* tb = target + ((int64_t)b * tsb + (int64_t)c * tsc);

  // the halo: every load of the lane goes out before the first is used (one round trip to memory, not one per element)
  constexpr int NST = (IM_HH * IM_HW + 255) / 256;
  float pv[NST], tv[NST];
#pragma unroll
  for (int k = 0; k < NST; ++k) {
    const int i = tid + k * 256;
    const int y = y0 + i / IM_HW, x = x0 + i % IM_HW;
    const bool in = i < IM_HH * IM_HW && y < H && x < W;
    pv[k] = in ? pb[(int64_t)y * psh + (int64_t)x * psw] : 0.f;
    tv[k] = in ? tb[(int64_t)y * tsh + (int64_t)x * tsw] : 0.f;
  }
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < NST; ++k) {
    const int i = tid + k * 256;
    const int ly = i / IM_HW, lx = i % IM_HW;
    if (i < IM_HH * IM_HW) {
      float up = 0.f, ut = 0.f;
      if (y0 + ly < H && x0 + lx < W) {
        up = to_unit_f(pv[k]);
        ut = to_unit_f(tv[k]);
        if (ly < own_h && lx < own_w) {
          const double dr = (double)pv[k] - (double)tv[k], du = (double)up - (double)ut;
          acc[0] += dr * dr;
          acc[1] += du * du;
        }
      }
      sp[ly * IM_LD + lx] = up;
      st[ly * IM_LD + lx] = ut;
    }
  }
  __syncthreads();

  {  // horizontal pass: lane = (halo row, run of IM_RH columns)
    const int row = tid / (IM_TW / IM_RH), c0 = (tid % (IM_TW / IM_RH)) * IM_RH;
    double h[IM_RH][5];
#pragma unroll
    for (int o = 0; o < IM_RH; ++o)
#pragma unroll
      for (int q = 0; q < 5; ++q) h[o][q] = 0.0;
#pragma unroll
    for (int j = 0; j < IM_RH + IM_K - 1; ++j) {
      const double p = (double)sp[row * IM_LD + c0 + j], t = (double)st[row * IM_LD + c0 + j];
      const double v[5] = {p, t, p * p, t * t, p * t};
#pragma unroll
      for (int o = 0; o < IM_RH; ++o) {
        if (j - o >= 0 && j - o < IM_K) {
#pragma unroll
          for (int q = 0; q < 5; ++q) h[o][q] = fma(win.w[j - o], v[q], h[o][q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int o = 0; o < IM_RH; ++o) hq[q][row][c0 + o] = h[o][q];
  }
  __syncthreads();

  {  // vertical pass and the index: lane = (column, run of IM_RV rows)
    const int col = tid % IM_TW, r0 = (tid / IM_TW) * IM_RV;
    double s[IM_RV][5];
#pragma unroll
    for (int o = 0; o < IM_RV; ++o)
#pragma unroll
      for (int q = 0; q < 5; ++q) s[o][q] = 0.0;
#pragma unroll
    for (int j = 0; j < IM_RV + IM_K - 1; ++j) {
      const int row = min(r0 + j, IM_HH - 1);  // rows past the halo belong to outputs past the tile, which are dropped below
      double v[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) v[q] = hq[q][row][col];
#pragma unroll
      for (int o = 0; o < IM_RV; ++o) {
        if (j - o >= 0 && j - o < IM_K) {
#pragma unroll
          for (int q = 0; q < 5; ++q) s[o][q] = fma(win.w[j - o], v[q], s[o][q]);
        }
      }
    }
    const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
#pragma unroll
    for (int o = 0; o < IM_RV; ++o) {
      const int r = r0 + o;
      if (r < IM_TH && y0 + r < H - (IM_K - 1) && x0 + col < W - (IM_K - 1)) {
        const double mp = s[o][0], mt = s[o][1];
        const double spp = s[o][2] - mp * mp, stt = s[o][3] - mt * mt, spt = s[o][4] - mp * mt;
        acc[2] += ((2.0 * mp * mt + c1) * (2.0 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2));
      }
    }
  }
  __syncthreads();
  block_sum3(acc, &hq[0][0][0]);
  if (tid == 0) {
    double* cell = ws + (int64_t)blockIdx.x * 3;
    cell[0] = acc[0];
    cell[1] = acc[1];
    cell[2] = acc[2];
  }
}

// one workgroup per image: out[b] = {sse_raw, sse_unit, mean SSIM} from the image's `cells` consecutive workspace cells
__global__ __launch_bounds__(256) void image_metrics_final_kernel(const double* __restrict__ ws, int cells, double positions,
                                                                  double* __restrict__ out) {
  __shared__ double red[3 * 256];
  const double* w = ws + (int64_t)blockIdx.x * cells * 3;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < cells; i += 256) {
    acc[0] += w[(int64_t)i * 3];
    acc[1] += w[(int64_t)i * 3 + 1];
    acc[2] += w[(int64_t)i * 3 + 2];
  }
  block_sum3(acc, red);
  if (threadIdx.x == 0) {
    out[blockIdx.x * 3] = acc[0];
    out[blockIdx.x * 3 + 1] = acc[1];
    out[blockIdx.x * 3 + 2] = acc[2] / positions;
  }
}

struct ImPlan { int tiles_x, tiles_y; int64_t cells; };  // cells: per image

int image_metrics_plan(const char* who, int32_t B, int32_t C, int32_t H, int32_t W, ImPlan* p) {
  VAE_CHECK(B > 0 && C > 0, "%s: B=%d C=%d (need B >= 1 and C >= 1)", who, B, C);
  VAE_CHECK(H >= IM_K && W >= IM_K, "%s: a %d x %d image is smaller than the %d x %d SSIM window", who, H, W, IM_K, IM_K);
  p->tiles_y = (H - (IM_K - 1) + IM_TH - 1) / IM_TH;
  p->tiles_x = (W - (IM_K - 1) + IM_TW - 1) / IM_TW;
  p->cells = (int64_t)C * p->tiles_y * p->tiles_x;
  VAE_CHECK(p->cells * B <= 0x7fffffff, "%s: %d x %d x %d x %d needs more than 2^31 - 1 workgroups", who, B, C, H, W);
  return VAE_OK;
}

}  // namespace

extern "C" int vae_image_metrics_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int64_t* ndoubles) {
  VAE_CHECK(ndoubles, "image_metrics_workspace: null result pointer");
  ImPlan p;
  if (int rc = image_metrics_plan("image_metrics_workspace", B, C, H, W, &p)) return rc;
  *ndoubles = p.cells * B * 3;
  return VAE_OK;
}

extern "C" int vae_image_metrics_partial(const float* pred, int64_t psb, int64_t psc, int64_t psh, int64_t psw, const float* target,
                                         int64_t tsb, int64_t tsc, int64_t tsh, int64_t tsw, int32_t B, int32_t C, int32_t H,
                                         int32_t W, double* ws, void* stream) {
  VAE_CHECK(pred && target && ws, "image_metrics_partial: null args");
  VAE_CHECK(((uintptr_t)pred & 3u) == 0 && ((uintptr_t)target & 3u) == 0 && ((uintptr_t)ws & 7u) == 0,
            "image_metrics_partial: unaligned operand or workspace");
  ImPlan p;
  if (int rc = image_metrics_plan("image_metrics_partial", B, C, H, W, &p)) return rc;
  ImWindow win;  // the window of evaluate.ssim_per_image: exp(-(i - 5)^2 / (2 sigma^2)), normalised
  double sum = 0.0;
  for (int i = 0; i < IM_K; ++i) {
    const double a = ((double)i - (IM_K - 1) / 2.0) / 1.5;
    win.w[i] = exp(-(a * a) / 2.0);
    sum += win.w[i];
  }
  for (int i = 0; i < IM_K; ++i) win.w[i] /= sum;
  hipLaunchKernelGGL(image_metrics_partial_kernel, dim3((unsigned)(p.cells * B)), dim3(256), 0, (hipStream_t)stream, pred, psb, psc,
                     psh, psw, target, tsb, tsc, tsh, tsw, C, H, W, p.tiles_x, p.tiles_y, win, ws);
  VAE_LAUNCH_CHECK("image_metrics_partial");
  return VAE_OK;
}

extern "C" int vae_image_metrics_final(const double* ws, int32_t B, int32_t C, int32_t H, int32_t W, double* out, void* stream) {
  VAE_CHECK(ws && out, "image_metrics_final: null args");
  VAE_CHECK(((uintptr_t)ws & 7u) == 0 && ((uintptr_t)out & 7u) == 0, "image_metrics_final: unaligned workspace or result");
  ImPlan p;
  if (int rc = image_metrics_plan("image_metrics_final", B, C, H, W, &p)) return rc;
  const double positions = (double)C * (double)(H - (IM_K - 1)) * (double)(W - (IM_K - 1));
  hipLaunchKernelGGL(image_metrics_final_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ws, (int)p.cells, positions, out);
  VAE_LAUNCH_CHECK("image_metrics_final");
  return VAE_OK;
}
