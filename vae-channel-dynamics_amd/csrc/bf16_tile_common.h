// What the three bf16 halo-tile files (conv3_tile_bf16.hip, conv3_wide_bf16.hip, wgrad3_tile_bf16.hip) agree on, once: the
// persistent tile schedule, where a piece of a weight stage goes, the pieces of the output epilogue, the weight gradients'
// roles, unit cursor, slab and bias tails, and the host preambles.  Device and host inlines only; the step and stage bodies,
// their pipelines, sched_barriers, wait counts and opaque-thread-id tricks stay in their files.
// Not here, because conv3_tile_bf16_kernel's register counts moved with it: the byte offset of a weight piece into Wh (7-10 VGPRs,
// up to 5 scalar spills) and the B-fragment base with its lane constants (3 VGPRs in dgrad); conv3_wide_bf16_kernel compiles to
// the same resources either way and keeps its copy, since a function with one caller shares nothing.  wgrad3_dma_bf16_kernel
// keeps its lane constants (one VGPR) and its per-unit descriptors (five scalar instructions per request).  Figures:
// profiles/bf16_tile_common_measured.json, "spelled_out".
#pragma once
#include "bf16_frag.h"
#include "launchers.h"
#include <algorithm>

namespace bf16_tile {

template <int A, int B>
__device__ __forceinline__ void clear_acc(f32x16 (&acc)[A][B]) {
#pragma unroll
  for (int a = 0; a < A; ++a)
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// descriptor over image b of a tensor of H x W pixels with ld elements of type T each
template <typename T>
__device__ __forceinline__ auto image_rsrc(T* base, int b, int H, int W, int ld) {
  return VAE_BUF_RSRC(base + (int64_t)b * H * W * ld, (size_t)H * W * ld * sizeof(T));
}

// ---- A. the two convolution kernels: TH x 32-pixel tiles x 128 channels, 32-channel chunks, 4 waves ----
namespace conv {
constexpr int BK = 32, TW = 32, HW_ = TW + 2;
constexpr int LDH = BK + 8;    // halo pixel stride in bf16 (80 B: conflict-free ds_read_b128)
constexpr int BN = 128, NT = 256;
constexpr int LDBK = BK + 8;   // weight tile [n][k] row stride (forward)
constexpr int LDBN = BN + 32;  // weight tile [k][n] row stride (dgrad): 320 B => the transposing reads are conflict-free
constexpr int SB1 = BN * LDBK;  // one tap of a weight stage (5120 bf16)
static_assert(BN * LDBK == BK * LDBN, "forward and dgrad weight tiles have the same LDS size");
constexpr int SB = 3 * SB1;    // weight stage: 3 taps (a kernel row or a kernel column)

// persistent schedule: workgroup w runs the logical ids first_tile, + gridDim.x, ...; consecutive ids (co-tile / x neighbours,
// which share halo rows) run on the same XCD (hardware places workgroup i on XCD i % 8) and therefore meet in the same L2
struct Tile { int b, y0, x0, n0, lin; };
__device__ __forceinline__ int first_tile(int G, int w) { return (G % 8 == 0) ? (w % 8) * (G / 8) + w / 8 : w; }
template <int TH>
__device__ __forceinline__ Tile decode(int t, int tilesN, int tiles_x, int tiles_y) {
  Tile id;
  id.lin = t / tilesN;
  const int tn = t - id.lin * tilesN;
  int r = id.lin;
  const int tx = r % tiles_x; r /= tiles_x;
  const int ty = r % tiles_y;
  id.b = r / tiles_y;
  id.y0 = ty * TH; id.x0 = tx * TW; id.n0 = tn * BN;
  return id;
}

// A weight stage is 3 (KS = 2: 2) taps of 128 x 32 bf16, moved as 16-byte pieces: thread `rem` (0..511, two per thread) of a
// tap takes row rem >> 2, k octet rem & 3 of the forward tile [n][k], or row rem >> 4, columns 8 (rem & 15) of the dgrad tile
// [k][n].  Element offset of piece i (tap i >> 1 of the stage) inside the stage in LDS:
template <bool DG>
__device__ __forceinline__ int weight_piece_lds(int i, int rem) {
  return (i >> 1) * SB1 + (DG ? (rem >> 4) * LDBN + (rem & 15) * 8 : (rem >> 2) * LDBK + (rem & 3) * 8);
}

// ---- epilogue.  bf16 output: adjacent lanes hold adjacent channels of the same pixels; they swap every other register, so a
// lane ends up with both channels of its pair (a0, a1: the lane's accumulators 2j, 2j + 1), adds both biases and, RES, the two
// halves of the bf16 residual word, and rounds once.  q0, q1: the rounded values (what the statistics describe) ----
struct Pair16 { unsigned word; float q0, q1; };
template <bool RES>
__device__ __forceinline__ Pair16 pack_pair(float a0, float a1, bool odd, float b0, float b1, unsigned res) {
  const float recv = lane_xor1(odd ? a0 : a1);
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  bf16x2_t h;
  float v0 = (odd ? recv : a0) + b0, v1 = (odd ? a1 : recv) + b1;
  if constexpr (RES) {
    v0 += __builtin_bit_cast(float, res << 16);
    v1 += __builtin_bit_cast(float, res & 0xffff0000u);
  }
  h[0] = (__bf16)v0;
  h[1] = (__bf16)v1;
  return Pair16{__builtin_bit_cast(unsigned, h), (float)h[0], (float)h[1]};
}
// GroupNorm statistics of a lane's outputs as shifted sums around a pivot pv (its first value): s1 = sum(v - pv),
// s2 = sum((v - pv)^2).  Three accumulation orders, each kernel's own choice (they round differently):
//   one value, product then add (fp32 outputs of both kernels)
__device__ __forceinline__ void shifted_add(float pv, float& s1, float& s2, float v) {
  const float dv = v - pv;  // (the statistics epilogue only runs on full tiles)
  s1 += dv;
  s2 += dv * dv;
}
//   a rounded pair into one chain (conv3_tile_bf16_kernel: a pivot per 16 values)
__device__ __forceinline__ void shifted_add_pair(float pv, float& s1, float& s2, float q0, float q1) {
  const float d0 = q0 - pv, d1 = q1 - pv;
  s1 += d0 + d1;
  s2 += d0 * d0 + d1 * d1;
}
//   a rounded pair into two independent fused chains (conv3_wide_bf16_kernel: ONE pivot for the lane's 64 values)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void shifted_add_pair_fma(float pv, f32x2& s1, f32x2& s2, float q0, float q1) {
  const float d0 = q0 - pv, d1 = q1 - pv;
  s1[0] += d0;
  s1[1] += d1;
  s2[0] = fmaf(d0, d0, s2[0]);
  s2[1] = fmaf(d1, d1, s2[1]);
}
// two rows of 16 values each of a lane -> its moments over the 32
__device__ __forceinline__ MeanM2 rows2(float pva, float s1a, float s2a, float pvb, float s1b, float s2b) {
  return mm2_merge_equal(mm2_from_shifted(pva, s1a, s2a, 16.f), mm2_from_shifted(pvb, s1b, s2b, 16.f), 16.f);
}
// The statistics workspace has the layout of vae_gn_stats_partial with one chunk per wave-row band wm of a tile (TH / 2 rows x
// 32 pixels): [image][tile in image][band][group][2].  gstat_write: a lane arrives with the moments of its nlane values of
// channel col; the group's cpg lanes are merged by DPP moves and the first lane writes -- no LDS round trip, no barrier.
__device__ __forceinline__ float* gstat_band(const vae_igemm_args& p, const Tile& cur, int tiles_x, int tiles_y, int wm) {
  const int tile_in_img = cur.lin - cur.b * (tiles_x * tiles_y);
  return p.gstat + (((int64_t)cur.b * (tiles_x * tiles_y) + tile_in_img) * 2 + wm) * p.gstat_groups * 2;
}
__device__ __forceinline__ void gstat_write(MeanM2 lane_mm, float nlane, int cpg, float* gbase, int col, int lr, int lh) {
  const MeanM2 a = mm2_wave_group(lane_mm, cpg, nlane);
  if (lh == 0 && (lr & (cpg - 1)) == 0) {
    float* o = gbase + (col / cpg) * 2;
    o[0] = a.m;
    o[1] = a.M2;
  }
}

// host: chunks per image of the statistics epilogue, one per band of `rows` rows x 32 pixels (0 = not available for these
// arguments; `refuse`: the kernel's own extra condition)
inline int gstat_chunks(const vae_igemm_args& a, int rows, bool refuse) {
  const vae_conv_geom& g = a.g;
  if (refuse || a.gstat_groups <= 0 || a.N % BN != 0 || a.N % a.gstat_groups != 0 || g.mode == VAE_MODE_DGRAD || a.c_step > 1) return 0;
  const int cpg = a.N / a.gstat_groups;
  if (cpg != 4 && cpg != 8 && cpg != 16) return 0;
  return (g.Wo / TW) * (g.Ho / rows);
}
}  // namespace conv

// host: every kernel of the family addresses ONE image per buffer descriptor (32-bit byte offsets, sized as fp32 whatever the
// storage) and the whole weight image through another, and reads 16-byte pieces: the operand view steps by a_step, the
// output-shaped one (ld_out channels) by o_step, `weights` elements of bf16 (0: none), pointers p0, p1 16-byte aligned
inline bool descriptors_fit(const vae_conv_geom& g, int a_step, int ld_out, int o_step, int64_t weights, const void* p0 = nullptr, const void* p1 = nullptr) {
  const size_t as = a_step > 1 ? a_step : 1, os = o_step > 1 ? o_step : 1;
  return (size_t)g.Hs * g.Ws * g.Cs * 4u * as * as < BUF_MAX && (size_t)g.Ho * g.Wo * ld_out * 4u * os * os < BUF_MAX &&
         (size_t)weights * 2u < BUF_MAX && aligned16(p0) && aligned16(p1);
}

// ---- B. the two weight-gradient kernels: 12 waves = 128 co x 64 ci x 9 taps per workgroup, split-K over ranges of units ----
namespace wgrad {
constexpr int TW = 32, BMT = 128, BNT = 64, NT = 768;

// Workgroup id -> (column = (co tile, ci tile), split).  The hardware deals consecutive workgroup ids round-robin over the 8 XCDs
// (one L2 each).  The columns of one split stream through the SAME pixels at the same pace (every ci tile re-reads the dY rows,
// every co tile the X halo): with id = column + columns * split the 8 columns of a 256 -> 256 layer sat on 8 different XCDs and
// every L2 fetched the split's pixels for itself -- 1.08 GB per launch from the memory side, 3.9 TB/s, which is what the staging
// cost (the kernel ran 0.276 ms with its DMA pieces, 0.218 with the same instructions fetching nothing).  Here XCD x takes the
// splits congruent x mod 8, all columns of a split together: one L2 fetches a split's pixels once.
__device__ __forceinline__ void wg_column_split(int nsplit, int& column, int& split) {
  const int cols = gridDim.x, L = blockIdx.y * cols + blockIdx.x;
  if (nsplit % 8 == 0) {
    const int j = L >> 3;
    column = j % cols;
    split = (j / cols) * 8 + (L & 7);
  } else {
    column = blockIdx.x;
    split = blockIdx.y;
  }
}

// what a thread is and what its workgroup covers.  Wave (mt, nt, tg): 64-row co block, 32-column ci block, filter row kh.
// Phase convolutions of an upsampler (vaehip.h): dY is a sub-sampled view (pixel (y,x) at (y*ys+y_oy, x*ys+y_ox)) and only the
// taps of tapmask are computed -- a wave whose kernel row is masked out only helps with the staging, the others skip the
// masked columns (their accumulators stay zero and are written as zeros): wmask, bit t = tap (kh = tg, kw = t).
struct Role {
  int tid, lane, wave, lr, lh, mt, nt, tg;
  int trq, trp, trh;     // the lane's address pattern for the transposing read: group row, column quad, half
  int m0, n0, split;     // first co row, first ci column, split of the workgroup
  int64_t ubeg, uend;    // the split's units [ubeg, uend) of nunits (nu of them; a split beyond the range has nu = 0)
  int nu, units_per_img;
  int Hb, Wb;            // the operand map the halo is cut from (UP: the virtual 2x upsample of X)
  bool do_bias;          // workgroups of the first ci block also sum dY's columns
  int ys, wmask;
};
template <bool UP>
__device__ __forceinline__ Role role(const vae_wgrad_args& p, int tiles_x, int tiles_y, int64_t nunits) {
  Role r;
  r.tid = threadIdx.x, r.lane = r.tid & 63, r.wave = r.tid >> 6;
  r.lr = r.lane & 31, r.lh = r.lane >> 5;
  r.mt = r.wave & 1, r.nt = (r.wave >> 1) & 1, r.tg = r.wave >> 2;
  r.trq = (r.lane & 15) >> 2, r.trp = r.lane & 3, r.trh = (r.lane >> 4) & 1;
  const vae_conv_geom& g = p.g;
  const int tilesN = p.N / BNT;
  int colw;
  wg_column_split(p.nsplit, colw, r.split);
  const int tm = colw / tilesN, tn = colw % tilesN;
  r.m0 = tm * BMT, r.n0 = tn * BNT;
  const int64_t per = (nunits + p.nsplit - 1) / p.nsplit;
  r.ubeg = r.split * per, r.uend = min(nunits, r.ubeg + per);
  r.nu = (int)max((int64_t)0, r.uend - r.ubeg);
  r.Hb = UP ? 2 * g.Hs : g.Hs, r.Wb = UP ? 2 * g.Ws : g.Ws;
  r.do_bias = (p.bias_partial != nullptr) && tn == 0;
  r.units_per_img = tiles_x * tiles_y;
  r.ys = (!UP && p.y_step > 1) ? p.y_step : 1;
  r.wmask = ((p.tapmask ? p.tapmask : 0x1ff) >> (3 * r.tg)) & 7;
  return r;
}

// the unit to request next (image, tile row, tile column), decoded once and then advanced: no division per step.  Every step
// requests one, also beyond the range (`valid` false: the caller makes that request with everything out of range)
struct Unit { bool valid; int b, ty, tx; };
struct UnitCursor {
  int b = 0, ty = 0, tx = 0, left;
  __device__ __forceinline__ UnitCursor(const Role& r, int tiles_x) : left(r.nu) {
    if (r.nu > 0) {
      b = (int)(r.ubeg / r.units_per_img);
      const int rem = (int)(r.ubeg - (int64_t)b * r.units_per_img);
      ty = rem / tiles_x;
      tx = rem - ty * tiles_x;
    }
  }
  __device__ __forceinline__ Unit next(int tiles_x, int tiles_y) {
    const Unit u{left > 0, b, ty, tx};
    --left;
    if (++tx == tiles_x) {
      tx = 0;
      if (++ty == tiles_y) { ty = 0; ++b; }
    }
    return u;
  }
};

// one 16-byte-per-lane LDS-DMA piece: 64 lanes x 16 B from byte offset `off` of the descriptor to LDS address dst (M0, restored).
// Inline asm, as in conv3_wino4.hip: with a DMA it can see in flight hipcc waits for vmcnt(0) at every other load.
template <typename Rsrc>
__device__ __forceinline__ void dma_piece(unsigned dst, unsigned off, Rsrc rsrc) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "s"(dst), "v"(off), "s"(rsrc) : "memory");
}

// column sums of 8 bf16 values of dY (a 16-byte piece), in fp32
__device__ __forceinline__ void add_bf16x8(f32x4& bsum, f32x4& bsum2, uint4 r) {
  bsum[0] += __builtin_bit_cast(float, r.x << 16); bsum[1] += __builtin_bit_cast(float, r.x & 0xffff0000u);
  bsum[2] += __builtin_bit_cast(float, r.y << 16); bsum[3] += __builtin_bit_cast(float, r.y & 0xffff0000u);
  bsum2[0] += __builtin_bit_cast(float, r.z << 16); bsum2[1] += __builtin_bit_cast(float, r.z & 0xffff0000u);
  bsum2[2] += __builtin_bit_cast(float, r.w << 16); bsum2[3] += __builtin_bit_cast(float, r.w & 0xffff0000u);
}

// the split's slab: O[co row][tap][ci column] = alpha * acc, wave (mt, nt, tg) holding taps 3 tg .. + 2 of two 32-row blocks
__device__ __forceinline__ void store_slab(const vae_wgrad_args& p, const Role& r, const f32x16 (&acc)[3][2]) {
  const int64_t ld = (int64_t)9 * p.N;
  float* __restrict__ O = (p.nsplit == 1 ? p.out : p.partial + (int64_t)r.split * p.M * ld);
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int tap = r.tg * 3 + t;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int col = r.n0 + r.nt * 32 + r.lr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = r.m0 + r.mt * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * r.lh;
        if (row < p.M) O[(int64_t)row * ld + (int64_t)tap * p.N + col] = p.alpha * acc[t][mi][e];
      }
    }
  }
}
// bias gradient: the threads' column sums through LDS (`red`, the staging space, free by now), added in fixed order.  A thread
// holds QUADS (1 or 2) quads of columns, (t % (32 / QUADS)) * QUADS .. of the 32, in bsum (and bsum2): red [NT * QUADS / 32][32]
template <int QUADS>
__device__ __forceinline__ void bias_reduce(f32x4* red, const vae_wgrad_args& p, const Role& r, f32x4 bsum, f32x4 bsum2) {
  const int tid = r.tid;
  red[tid * QUADS] = bsum;
  if (QUADS == 2) red[tid * 2 + 1] = bsum2;
  __syncthreads();
  if (tid < BMT / 4) {
    f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < NT * QUADS / 32; ++w) t4 += red[w * 32 + tid];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = r.m0 + tid * 4 + e;
      if (m < p.M) p.bias_partial[(int64_t)r.split * p.M + m] = t4[e];
    }
  }
}
}  // namespace wgrad
}  // namespace bf16_tile
