// Weight-side channel dynamics for the WeightDynamicsTracker (tracking/weightdynamics.py): per output slice and per input slice
// of every listed parameter tensor, in ONE read of the four flat arenas w (parameters), g (gradients), m and v (Adam moments),
//   S_ww = sum w^2, S_gg = sum g^2, S_wg = sum w g, S_mm = sum m^2, S_gm = sum g m, S_uu = sum u^2, A = max |w|
// with u = (m / bc1) / (sqrtf(v) / bc2_sqrt + eps) the Adam direction, in fp32 from the float-rounded constants of adam_args
// (elementwise.hip).  g, and the pair (m, v), may be absent (modes w, w+g, w+g+m+v); a sum a mode cannot form is stored as NaN.
//
// Table (device, int64 [nseg][8]): {off, O, K, I, out0, in0, ws0, chunk0}.  The tensor is [O][K][I] contiguous from element off
// of every arena (OHWI conv weight: K = kh kw; linear [out][in]: K = 1; 1-D: K = I = 1).  out0 / in0: its first row of the
// output-slice / input-slice result vectors (a tensor with I == 1 has no input slices: its in0 is that of the next tensor);
// ws0: its first column row of the workspace; chunk0: its first workgroup.  All four are running sums in table order.
//
// Partial pass: one workgroup per chunk = a run of rpc whole output rows of one tensor (found by bisection on chunk0), with
// rpc = max(1, 32768 / K) when I == 1 and min(8, max(1, 32768 / (K I))) otherwise: a row costs a workgroup one round trip to
// memory and one reduction whatever its length, so the rows of a short-row tensor are spread over workgroups, not queued in
// one.  A row longer than 32768 elements is still one workgroup, so row sums are complete inside it.
//   I > 1: the columns are cut into units of W = 4 (I % 4 == 0: 16-byte loads) or 1 elements and the units into tiles of 256;
//   per tile the 256 threads are PR = 256 / nut thread rows x nut lanes (nut units of the tile).  Row o: thread row pr takes
//   k = pr, pr + PR, ..., adding each element's six products (each rounded once: -ffp-contract=off), unit elements in order,
//   to its row accumulators and to its per-column accumulators.  ASSOCIATION ORDER of a row sum: thread chain over (k, e); then
//   wave_reduce (offsets 32 -> 1); the wave's value is added to the row's LDS slot of that wave, tile after tile; at the end
//   combine4 of the four slots, (r0 + r1) + (r2 + r3).  Of a column partial: thread chain over the chunk's
//   rows and its k in order; then the PR thread rows are added in order pr = 0, 1, ... from zero.  Seven words per column of
//   the chunk go to ws [ws0 + chunk_local * I + i][7] with plain stores; the final pass adds a tensor's chunks in chunk order in
//   float64.
//   I == 1: one thread per row, k in order; nothing goes to the workspace.
// max |w| travels as a bit pattern (for |w| the unsigned order of the patterns is the order of the values, NaN above infinity)
// and comes out exact, NaN if the slice holds one.  No atomics, nothing cleared: repeated launches are bitwise identical.
// Nothing outside the table's tensors is read, no arena is written.
#include "chanstat_common.h"

namespace {

constexpr int WD_CHUNK = 32768;  // elements of a chunk (whole rows: at least one)
constexpr int WD_NS = 6;         // sums
constexpr int WD_WORDS = 7;      // the sums and max |w| bits
constexpr int WD_TAB = 8;        // int64 words of a table entry
constexpr int WD_ROWS = 8;       // most rows of a chunk when I > 1
enum { T_OFF, T_O, T_K, T_I, T_OUT0, T_IN0, T_WS0, T_CHUNK0 };

// whole output rows of a chunk (the head of this file)
__host__ __device__ inline int wd_rpc(int64_t K, int64_t I) {
  const int64_t fit = WD_CHUNK / (K * I) > 0 ? WD_CHUNK / (K * I) : 1;
  return (int)(I == 1 || fit < WD_ROWS ? fit : WD_ROWS);
}

struct WdArgs {
  float bc1, bc2_sqrt, eps;
};
struct OpMaxU {
  __device__ __forceinline__ static unsigned f(unsigned a, unsigned b) { return max(a, b); }
};
__device__ __forceinline__ unsigned fbits(float f) { return __builtin_bit_cast(unsigned, f); }
__device__ __forceinline__ float bitsf(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ bool wd_has(int mode, int word) { return word == 0 || word == 6 || (word <= 2 ? mode >= 1 : mode >= 2); }

// the six products of one element (those of the mode)
template <int MODE>
__device__ __forceinline__ void wd_products(float w, float g, float m, float v, const WdArgs& x, float (&p)[WD_NS]) {
  p[0] = w * w;
  if (MODE >= 1) p[1] = g * g, p[2] = w * g;
  if (MODE >= 2) {
    const float u = (m / x.bc1) / (sqrtf(v) / x.bc2_sqrt + x.eps);
    p[3] = m * m, p[4] = g * m, p[5] = u * u;
  }
}

// the last entry whose field `f` is <= key (the fields are non-decreasing running sums, tab[0][f] == 0)
__device__ __forceinline__ int wd_find(const int64_t* __restrict__ tab, int nseg, int f, int64_t key) {
  int lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[(int64_t)mid * WD_TAB + f] <= key) lo = mid; else hi = mid;
  }
  return lo;
}

template <int W>
__device__ __forceinline__ void wd_load(const float* base, int64_t i, float (&v)[W]) {
  if constexpr (W == 4) {
    const f32x4 q = load4<false>(base + i, 0);
    v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
  } else {
    v[0] = base[i];
  }
}

struct WdTensor {
  int64_t off, out0;
  int O, K, I, r0, r1;  // rows [r0, r1) are this workgroup's
};

// I == 1: one thread per row
template <int MODE>
__device__ __forceinline__ void wd_rows1(const float* __restrict__ w, const float* __restrict__ g, const float* __restrict__ m,
                                         const float* __restrict__ v, const WdTensor& t, const WdArgs& x,
                                         double* __restrict__ out_sums, float* __restrict__ out_absmax) {
  for (int o = t.r0 + threadIdx.x; o < t.r1; o += 256) {
    float s[WD_NS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unsigned a = 0u;
    for (int k = 0; k < t.K; ++k) {
      const int64_t i = t.off + (int64_t)o * t.K + k;
      float p[WD_NS];
      const float wv = w[i];
      wd_products<MODE>(wv, MODE >= 1 ? g[i] : 0.f, MODE >= 2 ? m[i] : 0.f, MODE >= 2 ? v[i] : 0.f, x, p);
      a = max(a, fbits(wv) & 0x7fffffffu);
#pragma unroll
      for (int j = 0; j < WD_NS; ++j)
        if (wd_has(MODE, j)) s[j] += p[j];
    }
    double* dst = out_sums + (t.out0 + o) * WD_NS;
#pragma unroll
    for (int j = 0; j < WD_NS; ++j) dst[j] = wd_has(MODE, j) ? (double)s[j] : (double)bitsf(0x7fc00000u);
    out_absmax[t.out0 + o] = absmax_of(a);
  }
}

// I > 1: lanes across the columns, thread rows across k, one output row at a time (order: the head of this file)
template <int W, int MODE>
__device__ __forceinline__ void wd_body(const float* __restrict__ w, const float* __restrict__ g, const float* __restrict__ m,
                                        const float* __restrict__ v, const WdTensor& t, const WdArgs& x, unsigned* __restrict__ wsp,
                                        double* __restrict__ out_sums, float* __restrict__ out_absmax,
                                        unsigned (*rowpart)[4][WD_WORDS], unsigned (*cred)[256]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nu = t.I / W;
  const int ntile = (nu + 255) / 256;
  float cs[W][WD_NS];
  unsigned ca[W];
  const int nb = t.r1 - t.r0;  // <= WD_ROWS
  if (tid < nb * 4 * WD_WORDS) (&rowpart[0][0][0])[tid] = 0u;  // 0.f and the smallest |w| pattern
  for (int tile = 0; tile < ntile; ++tile) {
    const int u0 = tile * 256;
    const int nut = min(256, nu - u0);
    const Lay l = make_lay_q(nut);
    const bool act = l.pr < l.PR;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      ca[e] = 0u;
#pragma unroll
      for (int j = 0; j < WD_NS; ++j) cs[e][j] = 0.f;
    }
    __syncthreads();  // rowpart is cleared, cred is free
    for (int o = t.r0; o < t.r1; ++o) {
      float rs[WD_NS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      unsigned ra = 0u;
      if (act) {
        for (int k = l.pr; k < t.K; k += l.PR) {
          const int64_t i = t.off + ((int64_t)o * t.K + k) * t.I + (int64_t)(u0 + l.cq) * W;
          float wv[W], gv[W], mv[W], vv[W];
          wd_load<W>(w, i, wv);
          if (MODE >= 1) wd_load<W>(g, i, gv);
          if (MODE >= 2) wd_load<W>(m, i, mv), wd_load<W>(v, i, vv);
#pragma unroll
          for (int e = 0; e < W; ++e) {
            float p[WD_NS];
            wd_products<MODE>(wv[e], MODE >= 1 ? gv[e] : 0.f, MODE >= 2 ? mv[e] : 0.f, MODE >= 2 ? vv[e] : 0.f, x, p);
            const unsigned b = fbits(wv[e]) & 0x7fffffffu;
            ra = max(ra, b);
            ca[e] = max(ca[e], b);
#pragma unroll
            for (int j = 0; j < WD_NS; ++j)
              if (wd_has(MODE, j)) rs[j] += p[j], cs[e][j] += p[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < WD_NS; ++j)
        if (wd_has(MODE, j)) rs[j] = wave_reduce<OpAdd>(rs[j]);
      ra = wave_reduce<OpMaxU>(ra);
      if (lane == 0) {  // this wave's slot of the row: no other thread touches it
        unsigned* slot = rowpart[o - t.r0][wave];
#pragma unroll
        for (int j = 0; j < WD_NS; ++j)
          if (wd_has(MODE, j)) slot[j] = fbits(bitsf(slot[j]) + rs[j]);
        slot[6] = max(slot[6], ra);
      }
    }
    // the chunk's column partials of this tile: thread rows added in order
#pragma unroll
    for (int word = 0; word < WD_WORDS; ++word) {
      if (!wd_has(MODE, word)) continue;
      __syncthreads();
#pragma unroll
      for (int e = 0; e < W; ++e) cred[e][tid] = word < WD_NS ? fbits(cs[e][word < WD_NS ? word : 0]) : ca[e];
      __syncthreads();
      if (tid < nut) {  // pr == 0, cq == tid
#pragma unroll
        for (int e = 0; e < W; ++e) {
          float sum = 0.f;
          unsigned mx = 0u;
          for (int r = 0; r < l.PR; ++r) {
            const unsigned q = cred[e][r * nut + tid];
            if (word < WD_NS) sum += bitsf(q); else mx = max(mx, q);
          }
          wsp[((int64_t)(u0 + tid) * W + e) * WD_WORDS + word] = word < WD_NS ? fbits(sum) : mx;
        }
      }
    }
  }
  __syncthreads();  // every wave's slots are written
  if (tid < nb) {
    const int64_t row = t.out0 + t.r0 + tid;
    double* dst = out_sums + row * WD_NS;
#pragma unroll
    for (int j = 0; j < WD_NS; ++j) {
      if (wd_has(MODE, j)) {
        const float r[4] = {bitsf(rowpart[tid][0][j]), bitsf(rowpart[tid][1][j]), bitsf(rowpart[tid][2][j]), bitsf(rowpart[tid][3][j])};
        dst[j] = (double)combine4<OpAdd>(r);
      } else {
        dst[j] = (double)bitsf(0x7fc00000u);
      }
    }
    const unsigned a[4] = {rowpart[tid][0][6], rowpart[tid][1][6], rowpart[tid][2][6], rowpart[tid][3][6]};
    out_absmax[row] = absmax_of(combine4<OpMaxU>(a));
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void wdyn_partial_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                           const float* __restrict__ m, const float* __restrict__ v,
                                                           const int64_t* __restrict__ tab, int nseg, WdArgs x, unsigned* __restrict__ ws,
                                                           double* __restrict__ out_sums, float* __restrict__ out_absmax) {
  __shared__ unsigned rowpart[WD_ROWS][4][WD_WORDS];
  __shared__ unsigned cred[4][256];
  const int chunk = blockIdx.x;
  const int64_t* e = tab + (int64_t)wd_find(tab, nseg, T_CHUNK0, chunk) * WD_TAB;
  WdTensor t;
  t.off = e[T_OFF], t.out0 = e[T_OUT0];
  t.O = (int)e[T_O], t.K = (int)e[T_K], t.I = (int)e[T_I];
  const int rpc = wd_rpc(t.K, t.I);
  const int cl = chunk - (int)e[T_CHUNK0];  // chunk of the tensor; the host made cl * rpc < O
  t.r0 = cl * rpc;
  t.r1 = min(t.O, t.r0 + rpc);
  if (t.I == 1) {
    wd_rows1<MODE>(w, g, m, v, t, x, out_sums, out_absmax);
    return;
  }
  unsigned* wsp = ws + (e[T_WS0] + (int64_t)cl * t.I) * WD_WORDS;
  if (t.I % 4 == 0) wd_body<4, MODE>(w, g, m, v, t, x, wsp, out_sums, out_absmax, rowpart, cred);
  else wd_body<1, MODE>(w, g, m, v, t, x, wsp, out_sums, out_absmax, rowpart, cred);
}

// one thread per input slice: its tensor's chunks in chunk order, float64
__global__ __launch_bounds__(256) void wdyn_final_kernel(const unsigned* __restrict__ ws, const int64_t* __restrict__ tab, int nseg,
                                                         int64_t n_in, int mode, double* __restrict__ in_sums,
                                                         float* __restrict__ in_absmax) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_in) return;
  const int64_t* e = tab + (int64_t)wd_find(tab, nseg, T_IN0, s) * WD_TAB;
  const int64_t I = e[T_I], i = s - e[T_IN0];
  const int64_t rpc = wd_rpc(e[T_K], I);
  const int64_t nch = (e[T_O] + rpc - 1) / rpc;
  double sum[WD_NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned mx = 0u;
  for (int64_t c = 0; c < nch; ++c) {
    const unsigned* src = ws + (e[T_WS0] + c * I + i) * WD_WORDS;
#pragma unroll
    for (int j = 0; j < WD_NS; ++j)
      if (wd_has(mode, j)) sum[j] += (double)bitsf(src[j]);
    mx = max(mx, src[6]);
  }
#pragma unroll
  for (int j = 0; j < WD_NS; ++j) in_sums[s * WD_NS + j] = wd_has(mode, j) ? sum[j] : (double)bitsf(0x7fc00000u);
  in_absmax[s] = absmax_of(mx);
}

}  // namespace

extern "C" int vae_wdyn_chunk(void) { return WD_CHUNK; }

extern "C" int vae_wdyn_workspace(const int64_t* tab, int32_t nseg, int32_t* nchunk, int64_t* n_out, int64_t* n_in, int64_t* nwords) {
  VAE_CHECK(tab && nchunk && n_out && n_in && nwords, "wdyn_workspace: null args");
  VAE_CHECK(nseg > 0, "wdyn_workspace: nseg=%d", nseg);
  int64_t out0 = 0, in0 = 0, ws0 = 0, chunk0 = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t* e = tab + (int64_t)s * WD_TAB;
    const int64_t off = e[T_OFF], O = e[T_O], K = e[T_K], I = e[T_I];
    VAE_CHECK(off >= 0 && off % 4 == 0, "wdyn_workspace: tensor %d: offset %lld is negative or no multiple of 4 elements", s, (long long)off);
    VAE_CHECK(O > 0 && K > 0 && I > 0 && O < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && I < ((int64_t)1 << 31) &&
                  K * I < ((int64_t)1 << 31),
              "wdyn_workspace: tensor %d: bad shape [%lld][%lld][%lld]", s, (long long)O, (long long)K, (long long)I);
    VAE_CHECK(e[T_OUT0] == out0 && e[T_IN0] == in0 && e[T_WS0] == ws0 && e[T_CHUNK0] == chunk0,
              "wdyn_workspace: tensor %d: out0 / in0 / ws0 / chunk0 are not the running sums of the entries before it", s);
    const int64_t nch = (O + wd_rpc(K, I) - 1) / wd_rpc(K, I);
    out0 += O;
    if (I > 1) in0 += I, ws0 += nch * I;
    chunk0 += nch;
    VAE_CHECK(chunk0 < ((int64_t)1 << 31), "wdyn_workspace: more than 2^31 chunks");
  }
  *nchunk = (int32_t)chunk0, *n_out = out0, *n_in = in0, *nwords = ws0 * WD_WORDS;
  return VAE_OK;
}

extern "C" int vae_wdyn_partial(const float* w, const float* g, const float* m, const float* v, const int64_t* tab, int32_t nseg,
                                int32_t nchunk, int64_t n_out, double beta1, double beta2, double eps, int32_t step, uint32_t* ws,
                                double* out_sums, float* out_absmax, void* stream) {
  VAE_CHECK(w && tab && ws && out_sums && out_absmax, "wdyn_partial: null args");
  VAE_CHECK((m == nullptr) == (v == nullptr) && (m == nullptr || g != nullptr), "wdyn_partial: the modes are w, w+g and w+g+m+v");
  VAE_CHECK(nseg > 0 && nchunk >= nseg && n_out >= nseg, "wdyn_partial: counts do not add up (nseg=%d nchunk=%d n_out=%lld)", nseg,
            nchunk, (long long)n_out);
  VAE_CHECK(aligned16(w) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ws) && aligned16(tab), "wdyn_partial: unaligned");
  VAE_CHECK(m == nullptr || step >= 1, "wdyn_partial: step=%d with Adam moments", step);
  WdArgs x{1.f, 1.f, 0.f};
  if (m) {  // as adam_args (elementwise.hip): python doubles, rounded to float once
    x.bc1 = (float)(1.0 - pow(beta1, (double)step));
    x.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    x.eps = (float)eps;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nchunk);
  if (m) hipLaunchKernelGGL(wdyn_partial_kernel<2>, grid, dim3(256), 0, s, w, g, m, v, tab, nseg, x, ws, out_sums, out_absmax);
  else if (g) hipLaunchKernelGGL(wdyn_partial_kernel<1>, grid, dim3(256), 0, s, w, g, m, v, tab, nseg, x, ws, out_sums, out_absmax);
  else hipLaunchKernelGGL(wdyn_partial_kernel<0>, grid, dim3(256), 0, s, w, g, m, v, tab, nseg, x, ws, out_sums, out_absmax);
  VAE_LAUNCH_CHECK("wdyn_partial");
  return VAE_OK;
}

extern "C" int vae_wdyn_final(const uint32_t* ws, const int64_t* tab, int32_t nseg, int64_t n_in, int32_t mode, double* in_sums,
                              float* in_absmax, void* stream) {
  VAE_CHECK(ws && tab && in_sums && in_absmax, "wdyn_final: null args");
  VAE_CHECK(nseg > 0 && n_in >= 0 && n_in < ((int64_t)1 << 39) && mode >= 0 && mode <= 2,
            "wdyn_final: counts do not add up (nseg=%d n_in=%lld mode=%d)", nseg, (long long)n_in, mode);
  VAE_CHECK(aligned16(ws) && aligned16(tab), "wdyn_final: unaligned");
  if (n_in == 0) return VAE_OK;  // no listed tensor has input slices
  hipLaunchKernelGGL(wdyn_final_kernel, dim3((unsigned)((n_in + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, tab, nseg, n_in,
                     mode, in_sums, in_absmax);
  VAE_LAUNCH_CHECK("wdyn_final");
  return VAE_OK;
}
