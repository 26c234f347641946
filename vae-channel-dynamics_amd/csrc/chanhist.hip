// Per-channel magnitude histogram, near-zero count and max |y| of y = XF(x) for the ActivityMonitor (monitor.py), in one read of
// an NHWC activation: the inputs of vae_moments_partial (fp32 or bf16 storage, any pixel stride ld >= C, the optional runtime
// GroupNorm(+SiLU) transform applied on the fly).
//
// The bin of a value is clamp(floor(log2 |y|) + 31, 0, 47), taken from the fp32 exponent field E as clamp(E - 96, 0, 47): bin 0
// holds |y| < 2^-30 (zeros and denormals included), bin 47 holds |y| >= 2^16, infinities and NaN.
//
// Partial pass: one workgroup per (pixel chunk, image, tile of 128 channels), lanes across channels and pixel rows down the chunk
// as in moments_partial_kernel.  The workgroup keeps ONE table of 50 rows x 128 counters in LDS (25.6 KB: six workgroups fit a
// CU): rows 0..47 are the bins (ds_add_u32 per element), row 48 the near-zero counts and row 49 the largest |y| bit pattern (both
// kept in registers over the chunk and merged once per lane).  A counter column belongs to (channel, private copy): a full tile
// has one copy per channel, so a counter is shared by the workgroup's 8 (vector path) or 2 pixel rows and by at most two lanes of
// a wave; a narrow tile spends the unused columns on private copies per pixel row (128 / channels of them), so that a 4-channel
// tensor does not put 64 lanes of a wave on one counter.  Columns are numbered e * QR + (thread % QR): for each of a lane's W
// channels the lanes of a half-wave touch consecutive banks whatever bins they hit.  All counters are integers and the maximum
// is taken on bit patterns (for |y| the unsigned order of the patterns is the order of the values, NaN above infinity), so the
// order in which LDS serves the atomics cannot change a result: repeated launches are bitwise identical.
//
// Across workgroups nothing is atomic: each workgroup stores its 50 words per channel to ws [B * nchunk][C][50] with plain
// stores, and the final pass sums (row 49: maximises) them per word.
#include "chanstat_common.h"

namespace {

constexpr int CH_BINS = 48;
constexpr int CH_ROWS = CH_BINS + 2;  // bins, near-zero count, max |y| bits
constexpr int CH_NZ = CH_BINS, CH_MAX = CH_BINS + 1;
constexpr int CH_CT = 128;            // counter columns of a workgroup's table = channels of a full tile

__device__ __forceinline__ int bin_of(unsigned a /* bits of |y| */) { return min(max((int)(a >> 23) - 96, 0), CH_BINS - 1); }

// ws: [B * nchunk][C][CH_ROWS] words
template <int W, bool XBF>
__global__ __launch_bounds__(256) void chanhist_partial_kernel(const void* __restrict__ x, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, int xf, int HW, int C, int ld,
                                                               int nchunk, float tau, unsigned* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) unsigned tab[CH_ROWS][CH_CT];
  constexpr int UT = CH_CT / W;                  // channel units of a full tile
  const StatFrame f = stat_frame<UT, W>(HW, C, nchunk);
  const int nut = f.nut, c0 = f.c0, b = f.b;
  const int R = min(f.PR, UT / nut);             // private copies of each channel's counters
  const int QR = nut * R;
  const int col = threadIdx.x % QR;              // (pr % R) * nut + cq
  for (int i = threadIdx.x; i < CH_ROWS * CH_CT / 4; i += 256) reinterpret_cast<uint4*>(&tab[0][0])[i] = uint4{0u, 0u, 0u, 0u};
  __syncthreads();
  if (f.pr < f.PR) {
    float sc[W], sh[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      sc[e] = xf != VAE_XF_NONE ? scale[(int64_t)b * ld + c0 + e] : 1.f;
      sh[e] = xf != VAE_XF_NONE ? shift[(int64_t)b * ld + c0 + e] : 0.f;
    }
    const int64_t xb = (int64_t)b * HW * ld + c0;
    unsigned nz[W], amax[W];
#pragma unroll
    for (int e = 0; e < W; ++e) nz[e] = amax[e] = 0u;
    auto count = [&](float (&v)[W]) {
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float y = xf != VAE_XF_NONE ? affine_xf(v[e], sc[e], sh[e], xf) : v[e];
        const unsigned a = __builtin_bit_cast(unsigned, y) & 0x7fffffffu;
        amax[e] = max(amax[e], a);
        nz[e] += __builtin_bit_cast(float, a) < tau ? 1u : 0u;  // NaN is not below tau
        atomicAdd(&tab[bin_of(a)][e * QR + col], 1u);
      }
    };
    for_rows<W, XBF>(x, xb, ld, f, count);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      atomicAdd(&tab[CH_NZ][e * QR + col], nz[e]);
      atomicMax(&tab[CH_MAX][e * QR + col], amax[e]);
    }
  }
  __syncthreads();
  // the tile's channels are consecutive in ws: word w = (local channel, row), the private copies folded on the way out
  const int64_t row = (int64_t)b * nchunk + f.chunk;
  unsigned* dst = ws + (row * C + (int64_t)f.u0 * W) * CH_ROWS;
  for (int w = threadIdx.x; w < nut * W * CH_ROWS; w += 256) {
    const int cl = w / CH_ROWS, j = w - cl * CH_ROWS;
    const int base = (cl % W) * QR + cl / W;
    unsigned acc = 0u;
    for (int r = 0; r < R; ++r) {
      const unsigned t = tab[j][base + r * nut];
      acc = j == CH_MAX ? max(acc, t) : acc + t;
    }
    dst[w] = acc;
  }
}

// FIN_R row lanes x FIN_W consecutive words of a ws row (128 B per row lane and load); sums are 64-bit, row 49 is a maximum of
// bit patterns.  The workspace is 50 words per (workgroup, channel), 26 MB at the benchmark shape, and there are only
// C * 50 / FIN_W workgroups to read it: 1024 threads and eight loads in flight per thread keep enough of them outstanding.
constexpr int FIN_W = 32, FIN_R = 32;
__global__ __launch_bounds__(FIN_W * FIN_R) void chanhist_final_kernel(const unsigned* __restrict__ ws, int rows, int C,
                                                                       int64_t* __restrict__ hist, int64_t* __restrict__ nzero,
                                                                       float* __restrict__ absmax) {
  __shared__ unsigned long long ssum[FIN_R][FIN_W];
  __shared__ unsigned smax[FIN_R][FIN_W];
  const int wl = threadIdx.x % FIN_W, rl = threadIdx.x / FIN_W;
  const int64_t nw = (int64_t)C * CH_ROWS;
  const int64_t w = (int64_t)blockIdx.x * FIN_W + wl;
  unsigned long long sum = 0ull;
  unsigned mx = 0u;
  if (w < nw) {
    const unsigned* src = ws + w;
    int r = rl;
    for (; r + 7 * FIN_R < rows; r += 8 * FIN_R) {
      unsigned t[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) t[k] = src[(int64_t)(r + k * FIN_R) * nw];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sum += t[k];
        mx = max(mx, t[k]);
      }
    }
    for (; r < rows; r += FIN_R) {
      const unsigned t = src[(int64_t)r * nw];
      sum += t;
      mx = max(mx, t);
    }
  }
  ssum[rl][wl] = sum;
  smax[rl][wl] = mx;
  __syncthreads();
  if (rl == 0 && w < nw) {
    for (int k = 1; k < FIN_R; ++k) {
      sum += ssum[k][wl];
      mx = max(mx, smax[k][wl]);
    }
    const int c = (int)(w / CH_ROWS), j = (int)(w - (int64_t)c * CH_ROWS);
    if (j < CH_BINS) hist[(int64_t)c * CH_BINS + j] = (int64_t)sum;
    else if (j == CH_NZ) nzero[c] = (int64_t)sum;
    else absmax[c] = absmax_of(mx);
  }
}

}  // namespace

extern "C" int vae_chanhist_bins(void) { return CH_BINS; }

extern "C" int vae_chanhist_workspace(int32_t B, int32_t HW, int32_t C, int32_t nchunk, int64_t* nwords) {
  VAE_CHECK(nwords, "chanhist_workspace: null args");
  if (int rc = stat_check_shape("chanhist_workspace", B, HW, C, nchunk)) return rc;
  *nwords = (int64_t)B * nchunk * C * CH_ROWS;
  return VAE_OK;
}

extern "C" int vae_chanhist_partial(const void* x, int32_t x_bf16, const float* scale, const float* shift, int32_t xf, int32_t B,
                                    int32_t HW, int32_t C, int32_t ld, int32_t nchunk, float tau, uint32_t* ws, void* stream) {
  VAE_CHECK(x && ws, "chanhist_partial: null args");
  if (int rc = stat_check_shape("chanhist_partial", B, HW, C, nchunk)) return rc;
  if (int rc = stat_check_xf("chanhist_partial", xf, scale, shift, ld, C)) return rc;
  VAE_CHECK(tau >= 0.f, "chanhist_partial: near-zero threshold tau=%g is negative or NaN", (double)tau);
  VAE_CHECK(aligned16(ws), "chanhist_partial: unaligned workspace");
  const bool vec = vec4_ok(x, x_bf16, C, ld);
  const int tiles = (C + CH_CT - 1) / CH_CT;  // C / W units in tiles of CH_CT / W
  VAE_CHECK(tiles <= 65535, "chanhist_partial: C=%d: too many channel tiles", C);
  const dim3 grid(nchunk, B, tiles);
  hipStream_t s = (hipStream_t)stream;
  dispatch_bool(vec, [&](auto V) {
    dispatch_bool(x_bf16, [&](auto XB) {
      hipLaunchKernelGGL((chanhist_partial_kernel<decltype(V)::value ? 4 : 1, decltype(XB)::value>), grid, dim3(256), 0, s, x, scale,
                         shift, xf, HW, C, ld, nchunk, tau, ws);
    });
  });
  VAE_LAUNCH_CHECK("chanhist_partial");
  return VAE_OK;
}

extern "C" int vae_chanhist_final(const uint32_t* ws, int32_t B, int32_t HW, int32_t C, int32_t nchunk, int64_t* hist, int64_t* nzero,
                                  float* absmax, void* stream) {
  VAE_CHECK(ws && hist && nzero && absmax, "chanhist_final: null args");
  if (int rc = stat_check_shape("chanhist_final", B, HW, C, nchunk)) return rc;
  VAE_CHECK(aligned16(ws), "chanhist_final: unaligned workspace");
  const int64_t blocks = ((int64_t)C * CH_ROWS + FIN_W - 1) / FIN_W;
  VAE_CHECK(blocks <= 0x7fffffff, "chanhist_final: C=%d: too many words", C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(chanhist_final_kernel, dim3((unsigned)blocks), dim3(FIN_W * FIN_R), 0, s, ws, B * nchunk,
                     C, hist, nzero, absmax);
  VAE_LAUNCH_CHECK("chanhist_final");
  return VAE_OK;
}
