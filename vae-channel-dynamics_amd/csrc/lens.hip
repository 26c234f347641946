// Logit lens (src/analysis/logit_lens.py; reference src/analysis/logit_lens.py:90-165, 263-270, 324-413): the arithmetic behind
// its pictures, read in place from the engine's NHWC activation.  x: fp32 or bf16 storage, channels contiguous, pixel stride
// ld >= C (a channel-prefix view of a wider buffer is read in place); the first S of its B samples and the K channels a device
// int32 list names (any order, repeats allowed) are used.  No planar or fp32 copy of the tensor is made; every offset is 64-bit.
// Non-finite inputs are outside the contract: min / max drop NaNs in an order that is not torch's.
//
// Planes, two launches.  Partial: one workgroup per (sample, chunk of LP_CHUNK pixels); a lane owns LP_PER pixels and walks the
// K channels over them (the channel axis is the contiguous one: for neighbouring channels the K reads of a pixel meet the same
// cache lines), writes maps[s][k][pixel] (bf16 widened exactly) and leaves the min / max of its wave per (s, k, chunk, wave).
// Final: one workgroup per (plane, chunk) takes the min / max over the plane's cells -- both are order-free, so the result is
// exact and repeatable -- and writes norm = (x - min) / (max - min), one IEEE subtraction and one IEEE division per element,
// or 0 where max - min <= 1e-6f (the comparison torch makes between an fp32 tensor and the literal 1e-6).
//
// Projection, one launch: Sigmoid(ConvT2(ReLU(ConvT1(x)))) with ConvT = ConvTranspose2d(k 3, stride 2, padding 1,
// output_padding 1), Cin -> 16 -> 3.  For such a layer output row 2m takes tap 1 of input row m, row 2m + 1 tap 2 of row m and
// tap 0 of row m + 1 (columns alike): a tile needs a one-pixel halo on the high side only.  One workgroup per LT x LT input tile
// (+1 halo) of one image: the 17 x 17 x 16 hidden tile is accumulated in registers (a lane owns 4 of the 16 channels of up to 5
// hidden pixels) while the input channels go by in chunks of LC staged in LDS with their slice of w1, then goes through ReLU into
// LDS (zero outside the hidden image: bias alone would leave ReLU(b1) there) and is never written to memory; the second layer
// reads it from LDS, a lane per output pixel, 4 pixels per lane.  fp32 FMA accumulation; expf and an IEEE division for the
// sigmoid.  Vector ALU only: 4 (layer 1) and 65 (layer 2) terms per output are no work for the matrix pipe.
#include <math.h>
#include "stream_common.h"

namespace {

constexpr int LP_PER = 4;                 // pixels per lane of the planes kernels
constexpr int LP_CHUNK = 256 * LP_PER;    // pixels per workgroup
constexpr int LP_WAVES = 4;               // min / max cells per chunk: one per wave

constexpr int LT = 8;                     // input tile edge of the projection
constexpr int LI = LT + 1;                // with the high-side halo
constexpr int LH = 2 * LT + 1;            // hidden tile edge (17)
constexpr int LHP = LH * LH;              // hidden pixels per tile (289)
constexpr int LO = 4 * LT;                // output tile edge (32)
constexpr int LM = 16;                    // hidden channels
constexpr int LC = 32;                    // input channels per staged chunk
constexpr int LXP = LC + 1;               // LDS pitch of a staged input pixel (odd: lanes of different pixels meet different banks)
constexpr int L1_ITEMS = LHP * (LM / 4);  // (hidden pixel, group of 4 channels) work items of layer 1
constexpr int L1_ROUNDS = (L1_ITEMS + 255) / 256;
static_assert(LO * LO == 256 * 4, "layer 2: four output pixels per lane");

// maps [S][K][HW]; ws [S][K][nchunk * LP_WAVES][2] = {min, max} of the wave's pixels (+inf / -inf for a wave with none)
__global__ __launch_bounds__(256) void lens_planes_partial_kernel(const void* __restrict__ x, int bf16, int64_t HW, int C, int ld,
                                                                  const int* __restrict__ channels, int K, int nchunk,
                                                                  float* __restrict__ maps, float* __restrict__ ws) {
  const int tid = threadIdx.x, chunk = blockIdx.x, s = blockIdx.y;
  int64_t p[LP_PER];
#pragma unroll
  for (int i = 0; i < LP_PER; ++i) p[i] = (int64_t)chunk * LP_CHUNK + tid + 256 * i;
  for (int k = 0; k < K; ++k) {
    const int ch = channels[k];
    const bool ch_ok = (unsigned)ch < (unsigned)C;  // (the host refuses such a list when it can see it; nothing outside x is read)
    float v[LP_PER];
#pragma unroll
    for (int i = 0; i < LP_PER; ++i) v[i] = (ch_ok && p[i] < HW) ? load1(x, ((int64_t)s * HW + p[i]) * ld + ch, bf16) : 0.f;
    float mn = INFINITY, mx = -INFINITY;
    float* mp = maps + ((int64_t)s * K + k) * HW;
#pragma unroll
    for (int i = 0; i < LP_PER; ++i) {
      if (p[i] < HW) {
        mp[p[i]] = v[i];
        mn = fminf(mn, v[i]);
        mx = fmaxf(mx, v[i]);
      }
    }
    mn = wave_reduce<OpMin>(mn);
    mx = wave_reduce<OpMax>(mx);
    if ((tid & 63) == 0) {
      float* cell = ws + ((((int64_t)s * K + k) * nchunk + chunk) * LP_WAVES + (tid >> 6)) * 2;
      cell[0] = mn;
      cell[1] = mx;
    }
  }
}

// one workgroup per (plane = s * K + k, chunk): range [S][K][2], norm [S][K][HW]
__global__ __launch_bounds__(256) void lens_planes_final_kernel(const float* __restrict__ maps, const float* __restrict__ ws,
                                                                int64_t HW, int nchunk, float* __restrict__ range,
                                                                float* __restrict__ norm) {
  __shared__ float red[2 * LP_WAVES];
  const int tid = threadIdx.x, chunk = blockIdx.y;
  const int64_t plane = blockIdx.x;
  const float* cells = ws + plane * nchunk * LP_WAVES * 2;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < nchunk * LP_WAVES; i += 256) {
    mn = fminf(mn, cells[2 * i]);
    mx = fmaxf(mx, cells[2 * i + 1]);
  }
  // (block_reduce twice would cost three more barriers: both values go through one)
  mn = wave_reduce<OpMin>(mn);
  mx = wave_reduce<OpMax>(mx);
  if ((tid & 63) == 0) {
    red[tid >> 6] = mn;
    red[LP_WAVES + (tid >> 6)] = mx;
  }
  __syncthreads();
  mn = combine4<OpMin>(red);
  mx = combine4<OpMax>(red + LP_WAVES);
  if (chunk == 0 && tid == 0) {
    range[plane * 2] = mn;
    range[plane * 2 + 1] = mx;
  }
  const float d = mx - mn;
  const bool spread = d > 1e-6f;
#pragma unroll
  for (int i = 0; i < LP_PER; ++i) {
    const int64_t p = (int64_t)chunk * LP_CHUNK + tid + 256 * i;
    if (p < HW) norm[plane * HW + p] = spread ? (maps[plane * HW + p] - mn) / d : 0.f;
  }
}

// taps of a stride-2 transposed convolution along one axis for output index o = 2 j + par: tap 0 -> (input j, weight tap
// par ? 2 : 1), and for par == 1 also tap 1 -> (input j + 1, weight tap 0)
__device__ __forceinline__ int ct_wtap(int par, int a) { return a ? 0 : (par ? 2 : 1); }

// grid (tiles_x * tiles_y, S) in full-map mode, (tiles_x * tiles_y, S * K) in single-channel mode
// out [images][4H][4W][3], images = S (full map: the K channels are the input) or S * K (each channel on its own, Cin = 1)
__global__ __launch_bounds__(256) void lens_project_kernel(const void* __restrict__ x, int bf16, int H, int W, int C, int ld,
                                                           const int* __restrict__ channels, int K, int full_map, int tiles_x,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           float* __restrict__ out) {
  __shared__ float xs[LI * LI * LXP];           // the chunk's input tile [pixel][channel], zero outside the image
  __shared__ __attribute__((aligned(16))) float w1s[LC * 9 * LM];  // the chunk's slice of w1 as [ci][tap][co]
  __shared__ float hid[LM * LHP];               // hidden tile after ReLU [channel][pixel]
  __shared__ float w2s[LM * 9 * 3 + LM + 3];    // w2 as [ci][tap][co], then b1, then b2
  __shared__ int chs[LC];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const int img = blockIdx.y;
  const int s = full_map ? img : img / K;
  const int cin = full_map ? K : 1;
  const int list0 = full_map ? 0 : img % K;     // where this image's channels start in the list
  const int y0 = ty * LT, x0 = tx * LT;
  const int H1 = 2 * H, W1 = 2 * W;

  for (int i = tid; i < LM * 9 * 3; i += 256) {  // torch layout [ci][co][3][3]
    const int ci = i / 27, co = (i / 9) % 3, t = i % 9;
    w2s[(ci * 9 + t) * 3 + co] = w2[i];
  }
  if (tid < LM) w2s[LM * 27 + tid] = b1[tid];
  if (tid < 3) w2s[LM * 27 + LM + tid] = b2[tid];

  // layer 1: a lane's work items, fixed for the whole channel loop
  float acc[L1_ROUNDS][4];
  int ipix[L1_ROUNDS], pary[L1_ROUNDS], parx[L1_ROUNDS];
#pragma unroll
  for (int r = 0; r < L1_ROUNDS; ++r) {
    const int it = min(tid + 256 * r, L1_ITEMS - 1);  // (items past the end repeat the last one and are dropped at the store)
    const int hp = it >> 2, hy = hp / LH, hx = hp % LH;
    pary[r] = hy & 1;
    parx[r] = hx & 1;
    ipix[r] = (hy >> 1) * LI + (hx >> 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 0.f;
  }
  const int cg4 = (tid & 3) * 4;  // 256 % 4 == 0: a lane keeps its channel group over the rounds

  for (int c0 = 0; c0 < cin; c0 += LC) {
    const int nc = min(LC, cin - c0);
    __syncthreads();  // the previous chunk's readers are done (first pass: orders nothing that matters)
    if (tid < nc) chs[tid] = channels[list0 + c0 + tid];
    for (int i = tid; i < nc * LM * 9; i += 256) {  // w1: torch layout [ci][co][3][3]
      const int ci = i / (LM * 9), co = (i / 9) % LM, t = i % 9;
      w1s[(ci * 9 + t) * LM + co] = w1[(int64_t)(c0 + ci) * LM * 9 + co * 9 + t];
    }
    __syncthreads();
    for (int i = tid; i < LI * LI * nc; i += 256) {  // channel fastest: neighbouring lanes read neighbouring channels of a pixel
      const int ci = i % nc, pix = i / nc;
      const int y = y0 + pix / LI, xx = x0 + pix % LI;
      const int ch = chs[ci];
      float v = 0.f;
      if (y < H && xx < W && (unsigned)ch < (unsigned)C) v = load1(x, (((int64_t)s * H + y) * W + xx) * ld + ch, bf16);
      xs[pix * LXP + ci] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < L1_ROUNDS; ++r) {
      for (int a = 0; a <= pary[r]; ++a) {
        for (int b = 0; b <= parx[r]; ++b) {
          const float* xp = xs + (ipix[r] + a * LI + b) * LXP;
          const float* wp = w1s + (ct_wtap(pary[r], a) * 3 + ct_wtap(parx[r], b)) * LM + cg4;
          for (int ci = 0; ci < nc; ++ci) {
            const float xv = xp[ci];
            const f32x4 w = *reinterpret_cast<const f32x4*>(wp + ci * 9 * LM);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[r][e] = fmaf(xv, w[e], acc[r][e]);
          }
        }
      }
    }
  }

  // bias, ReLU, and zero where the hidden image ends
#pragma unroll
  for (int r = 0; r < L1_ROUNDS; ++r) {
    const int it = tid + 256 * r;
    if (it < L1_ITEMS) {
      const int hp = it >> 2, hy = hp / LH, hx = hp % LH;
      const bool in = 2 * y0 + hy < H1 && 2 * x0 + hx < W1;
#pragma unroll
      for (int e = 0; e < 4; ++e) hid[(cg4 + e) * LHP + hp] = in ? fmaxf(acc[r][e] + w2s[LM * 27 + cg4 + e], 0.f) : 0.f;
    }
  }
  __syncthreads();

  // layer 2 and the sigmoid: lane -> output pixels (row r * 8 + tid / 32, column tid % 32) of the 32 x 32 tile
  const int H2 = 4 * H, W2 = 4 * W;
  float* ob = out + (int64_t)img * H2 * W2 * 3;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oy = r * 8 + (tid >> 5), ox = tid & 31;
    const int gy = 4 * y0 + oy, gx = 4 * x0 + ox;
    if (gy >= H2 || gx >= W2) continue;
    const int py = oy & 1, px = ox & 1;
    float v[3] = {w2s[LM * 27 + LM], w2s[LM * 27 + LM + 1], w2s[LM * 27 + LM + 2]};
    for (int a = 0; a <= py; ++a) {
      for (int b = 0; b <= px; ++b) {
        const float* hp = hid + ((oy >> 1) + a) * LH + (ox >> 1) + b;
        const float* wp = w2s + (ct_wtap(py, a) * 3 + ct_wtap(px, b)) * 3;
#pragma unroll
        for (int ci = 0; ci < LM; ++ci) {
          const float h = hp[ci * LHP];
#pragma unroll
          for (int co = 0; co < 3; ++co) v[co] = fmaf(h, wp[ci * 27 + co], v[co]);
        }
      }
    }
    float* o = ob + ((int64_t)gy * W2 + gx) * 3;
#pragma unroll
    for (int co = 0; co < 3; ++co) o[co] = 1.0f / (1.0f + expf(-v[co]));
  }
}

struct LensPlan { int64_t HW; int nchunk; };

// the checks every entry point shares; channels_host may be null (then the kernels skip an index outside [0, C) as zeros)
int lens_args(const char* who, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ld, int32_t S, const int32_t* channels_host,
              int32_t K) {
  VAE_CHECK(H >= 1 && W >= 1, "%s: a %d x %d map (need H >= 1 and W >= 1)", who, H, W);
  VAE_CHECK(B >= 1 && S >= 1 && S <= B, "%s: S=%d samples of a batch of B=%d (need 1 <= S <= B)", who, S, B);
  VAE_CHECK(K >= 1, "%s: K=%d channels (need K >= 1)", who, K);
  VAE_CHECK(C >= 1 && ld >= C, "%s: C=%d channels with pixel stride ld=%d (need ld >= C >= 1)", who, C, ld);
  if (channels_host)
    for (int k = 0; k < K; ++k)
      VAE_CHECK(channels_host[k] >= 0 && channels_host[k] < C, "%s: channel index %d (entry %d of the list) is outside [0, %d)", who,
                channels_host[k], k, C);
  return VAE_OK;
}

int lens_plan(const char* who, int32_t S, int32_t K, int32_t H, int32_t W, LensPlan* p) {
  VAE_CHECK(H >= 1 && W >= 1, "%s: a %d x %d map (need H >= 1 and W >= 1)", who, H, W);
  VAE_CHECK(S >= 1 && K >= 1, "%s: S=%d K=%d (need S >= 1 and K >= 1)", who, S, K);
  p->HW = (int64_t)H * W;
  const int64_t nchunk = (p->HW + LP_CHUNK - 1) / LP_CHUNK;
  VAE_CHECK(nchunk <= 65535 && S <= 65535 && (int64_t)S * K <= 0x7fffffff, "%s: %d x %d x %d x %d needs more workgroups than a grid has", who,
            S, K, H, W);
  p->nchunk = (int)nchunk;
  return VAE_OK;
}

}  // namespace

extern "C" int vae_lens_tile(void) { return LT; }

extern "C" int vae_lens_workspace(int32_t S, int32_t K, int32_t H, int32_t W, int64_t* nfloats) {
  VAE_CHECK(nfloats, "lens_workspace: null result pointer");
  LensPlan p;
  if (int rc = lens_plan("lens_workspace", S, K, H, W, &p)) return rc;
  *nfloats = (int64_t)S * K * p.nchunk * LP_WAVES * 2;
  return VAE_OK;
}

extern "C" int vae_lens_planes_partial(const void* x, int32_t x_bf16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ld,
                                       int32_t S, const int32_t* channels, const int32_t* channels_host, int32_t K, float* maps,
                                       float* ws, void* stream) {
  VAE_CHECK(x && channels && maps && ws, "lens_planes_partial: null args");
  if (int rc = lens_args("lens_planes_partial", B, H, W, C, ld, S, channels_host, K)) return rc;
  LensPlan p;
  if (int rc = lens_plan("lens_planes_partial", S, K, H, W, &p)) return rc;
  VAE_CHECK(((uintptr_t)x & (x_bf16 ? 1u : 3u)) == 0 && ((uintptr_t)channels & 3u) == 0 && ((uintptr_t)maps & 3u) == 0 && ((uintptr_t)ws & 3u) == 0,
            "lens_planes_partial: unaligned operand, result or workspace");
  hipLaunchKernelGGL(lens_planes_partial_kernel, dim3(p.nchunk, S), dim3(256), 0, (hipStream_t)stream, x, x_bf16, p.HW, C, ld, channels,
                     K, p.nchunk, maps, ws);
  VAE_LAUNCH_CHECK("lens_planes_partial");
  return VAE_OK;
}

extern "C" int vae_lens_planes_final(const float* maps, const float* ws, int32_t S, int32_t K, int32_t H, int32_t W, float* range,
                                     float* norm, void* stream) {
  VAE_CHECK(maps && ws && range && norm, "lens_planes_final: null args");
  LensPlan p;
  if (int rc = lens_plan("lens_planes_final", S, K, H, W, &p)) return rc;
  VAE_CHECK((((uintptr_t)maps | (uintptr_t)ws | (uintptr_t)range | (uintptr_t)norm) & 3u) == 0, "lens_planes_final: unaligned operand or result");
  hipLaunchKernelGGL(lens_planes_final_kernel, dim3((unsigned)(S * K), p.nchunk), dim3(256), 0, (hipStream_t)stream, maps, ws, p.HW,
                     p.nchunk, range, norm);
  VAE_LAUNCH_CHECK("lens_planes_final");
  return VAE_OK;
}

extern "C" int vae_lens_project(const void* x, int32_t x_bf16, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ld, int32_t S,
                                const int32_t* channels, const int32_t* channels_host, int32_t K, int32_t full_map, const float* w1,
                                const float* b1, const float* w2, const float* b2, float* out, void* stream) {
  VAE_CHECK(x && channels && w1 && b1 && w2 && b2 && out, "lens_project: null args");
  if (int rc = lens_args("lens_project", B, H, W, C, ld, S, channels_host, K)) return rc;
  const int tiles_y = (H + LT - 1) / LT, tiles_x = (W + LT - 1) / LT;
  const int64_t images = full_map ? (int64_t)S : (int64_t)S * K;
  VAE_CHECK((int64_t)tiles_y * tiles_x <= 0x7fffffff && images <= 65535, "lens_project: %d x %d maps for %lld images need more workgroups than a grid has",
            H, W, (long long)images);
  VAE_CHECK(((uintptr_t)x & (x_bf16 ? 1u : 3u)) == 0 && ((uintptr_t)channels & 3u) == 0 && ((uintptr_t)out & 3u) == 0 &&
                (((uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2) & 3u) == 0,
            "lens_project: unaligned operand, weight or result");
  hipLaunchKernelGGL(lens_project_kernel, dim3((unsigned)(tiles_y * tiles_x), (unsigned)images), dim3(256), 0, (hipStream_t)stream, x,
                     x_bf16, H, W, C, ld, channels, K, full_map ? 1 : 0, tiles_x, w1, b1, w2, b2, out);
  VAE_LAUNCH_CHECK("lens_project");
  return VAE_OK;
}
