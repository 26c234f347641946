// Channel covariance of y = XF(x) over batch and pixels for the ActivityMonitor (monitor.py: channel_covariance_matrix,
// channel_correlation_matrix, max_abs_correlation_per_channel, effective_rank), in one read of an NHWC activation: the inputs of
// vae_moments_partial (fp32 or bf16 storage, any pixel stride ld >= C, the optional runtime GroupNorm(+SiLU) transform applied on
// the fly).  A Gram product [C] x [C] with contraction length N = B * HW.
//
// Shift: K[c] = y at (image 0, pixel 0, channel c), evaluated by every workgroup itself from that one pixel row with the code
// that evaluates every other y: the same bits everywhere.  z = fp32(y - K) is what is multiplied: a constant channel is z = 0
// exactly (its row, column and variance come out exactly 0), and a channel with |mean| >> sigma keeps its digits.
//
// Partial pass: one workgroup of four waves per (pixel chunk, image, pair of 128-channel tiles ti <= tj).  A step stages 32 pixel
// rows of z of both tiles (one, on the diagonal) as three bf16 planes (split3, bf16_frag.h) into [pixel][channel] LDS images with
// 320-byte rows (64 B mod 256 B: the four rows of a transposing read's block in different bank ranges); channels at or beyond C
// and pixel rows beyond the chunk are zeros in LDS and are never loaded.  Both MFMA operands are the transposed read of such an
// image (frag_tr: 8 consecutive pixels of the lane's channel), a wave owns 64 x 64 of the pair's 128 x 128, and a product is the
// six plane products of mma_x3_term, smallest first, into fp32 accumulators kept over the whole chunk.  d[c] = sum z_c is kept in
// double per thread beside it (diagonal pairs only).  The workgroup stores its fp32 tile, its d partial and (image 0, chunk 0) K
// with plain stores: no global atomics, no zero-fill, repeated launches are bitwise identical.
//
// ws (floats):  S  [B * nchunk][pairs][128][128]   pairs = tiles (tiles + 1) / 2, (ti, tj) in row-major order of the upper triangle
//               d  [B * nchunk][tiles][128]        doubles
//               K  [tiles][128]
// Final pass: sums S and d over the B * nchunk rows in float64 in a fixed order (16 row lanes, then 0..15) and writes
// cov = (S - d d^T / N) / (N - 1) (upper triangle computed, mirrored: bitwise symmetric) and mean = K + d / N.
#include "chanstat_common.h"

namespace {

constexpr int CC_T = 128;             // channels of a tile
constexpr int CC_KB = 32;             // pixel rows of a step: two k-groups of 16
constexpr int CC_LD = CC_T + 32;      // image row stride in elements (320 B)
constexpr int CC_PS = CC_KB * CC_LD;  // plane stride
constexpr int CC_SIDE = 3 * CC_PS;    // the three planes of one tile
constexpr int CC_TT = CC_T * CC_T;

struct Pair {
  int ti, tj;
};
__host__ __device__ inline Pair pair_of(int p, int tiles) {
  int ti = 0;
  while (p >= tiles - ti) {
    p -= tiles - ti;
    ++ti;
  }
  return {ti, ti + p};
}
struct WsLay {
  int64_t d, k, end;  // float offsets of the d and K sections, and the size
};
__host__ __device__ inline WsLay ws_lay(int64_t rows, int tiles) {
  const int64_t pairs = (int64_t)tiles * (tiles + 1) / 2;
  WsLay l;
  l.d = rows * pairs * CC_TT;
  l.k = l.d + rows * tiles * CC_T * 2;
  l.end = l.k + (int64_t)tiles * CC_T;
  return l;
}

// the four channels c0.. of the pixel at element offset `off`; channels at or beyond C and rows that are not `rowok` are not read
template <bool VEC, bool XBF>
__device__ __forceinline__ f32x4 load_quad(const void* x, int64_t off, int c0, int C, bool rowok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    if (rowok && c0 < C) {
      if constexpr (XBF) v = unpack4(*reinterpret_cast<const uint2*>(reinterpret_cast<const u16*>(x) + off));
      else v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(x) + off);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (rowok && c0 + e < C) v[e] = load1(x, off + e, XBF);
  }
  return v;
}

template <bool VEC, bool XBF>
__global__ __launch_bounds__(256) void chancov_partial_kernel(const void* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int xf, int HW, int C, int ld,
                                                              int nchunk, int tiles, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) u16 img[2 * CC_SIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Pair pr = pair_of(blockIdx.z, tiles);
  const bool same = pr.ti == pr.tj;
  const int ns = same ? 1 : 2;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const ChunkRange cr = chunk_range(HW, nchunk, chunk);  // p0 < HW: the host makes every chunk non-empty
  const int p0 = cr.p0, p1 = cr.p1;
  // staging role: channel quad cq of the tile, pixel rows r0 + 8 k of the step
  const int cq = tid & 31, r0 = tid >> 5;
  int c0[2];
  float K[2][4], sc[2][4], sh[2][4];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    c0[s] = (s ? pr.tj : pr.ti) * CC_T + 4 * cq;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0[s] + e;
      const bool ok = c < C;
      sc[s][e] = (ok && xf != VAE_XF_NONE) ? scale[(int64_t)b * ld + c] : 1.f;
      sh[s][e] = (ok && xf != VAE_XF_NONE) ? shift[(int64_t)b * ld + c] : 0.f;
      float k = 0.f;
      if (ok) {
        k = load1(x, c, XBF);
        if (xf != VAE_XF_NONE) k = affine_xf(k, scale[c], shift[c], xf);
      }
      K[s][e] = k;
    }
  }
  const int64_t xb = (int64_t)b * HW * ld;
  f32x4 raw[2][4];
  auto fetch = [&](int step) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (s < ns) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int pix = p0 + step * CC_KB + r0 + 8 * k;
          raw[s][k] = load_quad<VEC, XBF>(x, xb + (int64_t)pix * ld + c0[s], c0[s], C, pix < p1);
        }
      }
  };
  double dacc[4] = {0.0, 0.0, 0.0, 0.0};
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
  const int lh = lane >> 5, trq = (lane & 15) >> 2, trp = lane & 3, trh = (lane >> 4) & 1;
  const int wm = wave & 1, wn = wave >> 1;
  const u16* sA = img + wm * 64;
  const u16* sB = img + (same ? 0 : CC_SIDE) + wn * 64;
  const int nsteps = (p1 - p0 + CC_KB - 1) / CC_KB;
  fetch(0);
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (s < ns) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int row = r0 + 8 * k;
          const bool rowok = p0 + step * CC_KB + row < p1;
          f32x4 z;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = raw[s][k][e];
            const float y = xf != VAE_XF_NONE ? affine_xf(v, sc[s][e], sh[s][e], xf) : v;
            z[e] = (rowok && c0[s] + e < C) ? y - K[s][e] : 0.f;
          }
          if (s == 0 && same) {
#pragma unroll
            for (int e = 0; e < 4; ++e) dacc[e] += (double)z[e];
          }
          uint2 hi, mid, lo;
          split3(z, hi, mid, lo);
          u16* dst = img + s * CC_SIDE + row * CC_LD + 4 * cq;
          *reinterpret_cast<uint2*>(dst) = hi;
          *reinterpret_cast<uint2*>(dst + CC_PS) = mid;
          *reinterpret_cast<uint2*>(dst + 2 * CC_PS) = lo;
        }
      }
    __syncthreads();
    if (step + 1 < nsteps) fetch(step + 1);  // in flight under the MFMAs
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
      const int base = (kg * 16 + lh * 8 + trq) * CC_LD + trh * 16 + trp * 4;
      bf16x8 a[2][3], bb[2][3];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          a[i][q] = frag_tr(sA + q * CC_PS + base + i * 32, CC_LD);
          bb[i][q] = frag_tr(sB + q * CC_PS + base + i * 32, CC_LD);
        }
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mma_x3_term(t, a[mi], bb[ni], acc[mi][ni]);
    }
  }
  const int64_t rows = (int64_t)gridDim.y * nchunk, row = (int64_t)b * nchunk + chunk;
  const int64_t pairs = (int64_t)tiles * (tiles + 1) / 2;
  const WsLay wl = ws_lay(rows, tiles);
  float* tile = ws + (row * pairs + blockIdx.z) * CC_TT;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int tr = wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, tc = wn * 64 + ni * 32 + (lane & 31);
        tile[tr * CC_T + tc] = acc[mi][ni][r];
      }
  if (same) {  // uniform
    __syncthreads();
    double* red = reinterpret_cast<double*>(img);  // [8 pixel-row groups][128 channels]
#pragma unroll
    for (int e = 0; e < 4; ++e) red[r0 * CC_T + 4 * cq + e] = dacc[e];
    __syncthreads();
    if (tid < CC_T) {
      double s = red[tid];
      for (int r = 1; r < 8; ++r) s += red[r * CC_T + tid];
      reinterpret_cast<double*>(ws + wl.d)[(row * tiles + pr.ti) * CC_T + tid] = s;
    }
    if (b == 0 && chunk == 0 && r0 == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ws[wl.k + (int64_t)pr.ti * CC_T + 4 * cq + e] = K[0][e];
    }
  }
}

// one workgroup per 64 consecutive elements of a pair's tile (one tile row, 64 columns): FIN_R row lanes each sum every
// FIN_R-th ws row of S, of the columns' d and of the row's d in float64; lane 0 adds the FIN_R partials in order
constexpr int FIN_W = 64, FIN_R = 16;
__global__ __launch_bounds__(FIN_W * FIN_R) void chancov_final_kernel(const float* __restrict__ ws, int rows, int C, int tiles,
                                                                      double N, double* __restrict__ cov,
                                                                      double* __restrict__ mean) {
  __shared__ double red[3][FIN_R][FIN_W];
  const int wl = threadIdx.x % FIN_W, rl = threadIdx.x / FIN_W;
  const Pair pr = pair_of(blockIdx.y, tiles);
  const bool same = pr.ti == pr.tj;
  const int e0 = blockIdx.x * FIN_W, r = e0 / CC_T, colb = e0 % CC_T;
  const int ci = pr.ti * CC_T + r, cj = pr.tj * CC_T + colb + wl;
  // (uniform) nothing of this block is a channel pair of the upper triangle
  if (ci >= C || pr.tj * CC_T + colb >= C || (same && colb + FIN_W - 1 < r)) return;
  const int64_t pairs = (int64_t)tiles * (tiles + 1) / 2;
  const WsLay l = ws_lay(rows, tiles);
  const float* S = ws + (int64_t)blockIdx.y * CC_TT + e0 + wl;
  const double* dj = reinterpret_cast<const double*>(ws + l.d) + (int64_t)pr.tj * CC_T + colb + wl;
  const double* di = reinterpret_cast<const double*>(ws + l.d) + (int64_t)pr.ti * CC_T + r;
  double s = 0.0, dc = 0.0, dr = 0.0;
#pragma unroll 4
  for (int w = rl; w < rows; w += FIN_R) {
    s += (double)S[(int64_t)w * pairs * CC_TT];
    dc += dj[(int64_t)w * tiles * CC_T];
    dr += di[(int64_t)w * tiles * CC_T];
  }
  red[0][rl][wl] = s, red[1][rl][wl] = dc, red[2][rl][wl] = dr;
  __syncthreads();
  if (rl == 0 && cj < C && (!same || cj >= ci)) {
    for (int k = 1; k < FIN_R; ++k) s += red[0][k][wl], dc += red[1][k][wl], dr += red[2][k][wl];
    const double v = (s - dr * dc / N) / (N - 1.0);
    cov[(int64_t)ci * C + cj] = v;
    cov[(int64_t)cj * C + ci] = v;
    if (same && r == 0) mean[cj] = (double)ws[l.k + cj] + dc / N;
  }
}

// what both passes (and the size query) ask of a shape: the family's checks and two of its own
int check_shape(const char* who, int32_t B, int32_t HW, int32_t C, int32_t nchunk) {
  if (int rc = stat_check_shape(who, B, HW, C, nchunk)) return rc;
  VAE_CHECK((int64_t)B * HW >= 2, "%s: B * HW = %lld: a covariance needs two rows", who, (long long)((int64_t)B * HW));
  const int64_t tiles = ((int64_t)C + CC_T - 1) / CC_T;
  VAE_CHECK(tiles * (tiles + 1) / 2 <= 65535, "%s: C=%d: too many channel tile pairs", who, C);
  return VAE_OK;
}

}  // namespace

extern "C" int vae_chancov_tile(void) { return CC_T; }

extern "C" int vae_chancov_workspace(int32_t B, int32_t HW, int32_t C, int32_t nchunk, int64_t* nfloats) {
  VAE_CHECK(nfloats, "chancov_workspace: null args");
  if (int rc = check_shape("chancov_workspace", B, HW, C, nchunk)) return rc;
  *nfloats = ws_lay((int64_t)B * nchunk, (C + CC_T - 1) / CC_T).end;
  return VAE_OK;
}

extern "C" int vae_chancov_partial(const void* x, int32_t x_bf16, const float* scale, const float* shift, int32_t xf, int32_t B,
                                   int32_t HW, int32_t C, int32_t ld, int32_t nchunk, float* ws, void* stream) {
  VAE_CHECK(x && ws, "chancov_partial: null args");
  if (int rc = check_shape("chancov_partial", B, HW, C, nchunk)) return rc;
  if (int rc = stat_check_xf("chancov_partial", xf, scale, shift, ld, C)) return rc;
  VAE_CHECK(aligned16(ws), "chancov_partial: unaligned workspace");
  const bool vec = vec4_ok(x, x_bf16, C, ld);  // (single elements otherwise)
  const int tiles = (C + CC_T - 1) / CC_T;
  const dim3 grid(nchunk, B, tiles * (tiles + 1) / 2);
  hipStream_t s = (hipStream_t)stream;
  dispatch_bool(vec, [&](auto V) {
    dispatch_bool(x_bf16, [&](auto XB) {
      hipLaunchKernelGGL((chancov_partial_kernel<decltype(V)::value, decltype(XB)::value>), grid, dim3(256), 0, s, x, scale, shift,
                         xf, HW, C, ld, nchunk, tiles, ws);
    });
  });
  VAE_LAUNCH_CHECK("chancov_partial");
  return VAE_OK;
}

extern "C" int vae_chancov_final(const float* ws, int32_t B, int32_t HW, int32_t C, int32_t nchunk, double* cov, double* mean,
                                 void* stream) {
  VAE_CHECK(ws && cov && mean, "chancov_final: null args");
  if (int rc = check_shape("chancov_final", B, HW, C, nchunk)) return rc;
  VAE_CHECK(aligned16(ws), "chancov_final: unaligned workspace");
  const int tiles = (C + CC_T - 1) / CC_T;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(chancov_final_kernel, dim3(CC_TT / FIN_W, tiles * (tiles + 1) / 2), dim3(FIN_W * FIN_R), 0, s, ws, B * nchunk,
                     C, tiles, (double)((int64_t)B * HW), cov, mean);
  VAE_LAUNCH_CHECK("chancov_final");
  return VAE_OK;
}
