// What the six kernels of the <= 4-channel convolutions share (skinny.hip: fp32 on the VALU; conv_thin_bf16.hip and
// wgrad_thin_bf16.hip: the same launches on the matrix pipe): the two tile shapes, the gather of the NARROW tensor (matrix pipe), the tile range
// of a split, the GroupNorm(+SiLU) transform of the WIDE tensor (per fp32 element and per bf16 octet), the slab protocol of the
// weight gradients, and the host predicates of their *_eligible functions.  Main loops, LDS layouts and MFMA sequences stay in
// the three files.  Byte offsets are an unsigned element index times an unsigned element size throughout.
#pragma once
#include "bf16_frag.h"
#include <algorithm>

namespace thin {

// ---------------------------------------------------------------------------------------------------------
// tiles
// ---------------------------------------------------------------------------------------------------------
constexpr int TP = 128;       // linear pixels per tile: conv_smallk, wgrad_smallk, conv_thin_bf16, wgrad_thin_bf16
constexpr int TAPS_MAX = 9;
// conv_smalln / conv_thinn: 4 x 32-pixel tiles with a one-pixel halo (6 x 34 = 204 halo pixels), one workgroup each
constexpr int TH = 4, TW = 32, HW = TW + 2, HP = (TH + 2) * HW;

struct Tile {
  int b, y0, x0;  // image, first row and column of the tile
};
__device__ __forceinline__ Tile decode(int t, int tiles_x, int tiles_y) {
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y;
  return Tile{t / tiles_y, ty * TH, tx * TW};
}
// the grid `decode` reads (the eligibility holds Wo, Ho to whole tiles)
inline dim3 tile_grid(const vae_conv_geom& g, int& tiles_x, int& tiles_y) {
  tiles_x = g.Wo / TW;
  tiles_y = g.Ho / TH;
  return dim3((unsigned)((int64_t)tiles_x * tiles_y * g.B));
}

// tiles [beg, end) of part `part` (a split of a weight gradient, a workgroup of conv_thin_bf16) when every part takes `per`
struct TileRange {
  int beg, end;
};
__host__ __device__ __forceinline__ int tiles_per_part(int ntiles, int nparts) { return (ntiles + nparts - 1) / nparts; }
__device__ __forceinline__ TileRange tile_range(int part, int per, int ntiles) {
  const int beg = part * per;
  return TileRange{beg, min(ntiles, beg + per)};
}

// ---------------------------------------------------------------------------------------------------------
// the narrow tensor: S[pixel][Cs] fp32, of which channels 0 .. narrow-1 (<= 4) are read
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t narrow_rsrc(const float* S, const vae_conv_geom& g, int Cs) {
  return VAE_BUF_RSRC(S, (size_t)g.B * g.Hs * g.Ws * Cs * 4u);  // (< BUF_MAX: narrow_fits below)
}
// S[src(m, tap)][0..3] of a 3x3 gather: m = linear pixel of the row grid of `g` (hw = g.Ho * g.Wo), tap = 3 kh + kw; zeros for
// channels >= narrow, at padding and where !valid (tiles past the range, slots past the tile).  The form of the matrix-pipe
// kernels' register prefetch: one opaque offset, the channel as the scalar offset of the load.  (stage_small of skinny.hip
// writes LDS directly and keeps its own copy, 1x1 gathers included: see there.)
__device__ __forceinline__ f32x4 gather4(const vae_conv_geom& g, __amdgpu_buffer_rsrc_t rsS, int Cs, int narrow, int hw, int m,
                                         int tap, bool valid) {
  const int b = m / hw, rem = m - b * hw;
  const int y = rem / g.Wo, x = rem - y * g.Wo;
  const int kh = tap / 3, kw = tap - kh * 3;
  int sy = 0, sx = 0;
  const bool ok = valid && src_pixel(g, y, x, kh, kw, sy, sx);
  const unsigned base = oob_unless(ok, (unsigned)(((b * g.Hs + sy) * g.Ws + sx) * Cs) * 4u);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < narrow) v[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsS, base, 4u * s, 0));
  return v;
}

// ---------------------------------------------------------------------------------------------------------
// GroupNorm(+SiLU) on the wide tensor while it is staged.  Padding must stay zero AFTER the transform: !ok gives 0
// (XF == NONE: the value as loaded, which is 0 there already).
// (xform4_tab of common.h is the same arithmetic from an LDS table of scale / shift; these kernels hold them in registers.)
// ---------------------------------------------------------------------------------------------------------
template <int XF>
__device__ __forceinline__ float xform1(float v, float sc, float sh, bool ok) {
  if (XF == VAE_XF_NONE) return v;
  float u = v * sc + sh;
  if (XF == VAE_XF_AFFINE_SILU) u = silu_f(u);
  return ok ? u : 0.f;
}
// eight bf16 values of one uint4 (one channel octet, sc / sh its 8 scales and shifts): transformed in fp32, rounded once.
// (The loop that loads sc / sh stays in the two kernels: through a shared function, with the row passed as a pointer or as an
// index, conv_thinn_bf16_kernel<1|2> took one VGPR more, and with the index wgrad_thin_bf16_kernel<false,1|2> spilt 3 SGPRs.)
template <int XF>
__device__ __forceinline__ uint4 xform8_bf16(uint4 v, const float (&sc)[8], const float (&sh)[8], bool ok) {
  if (XF == VAE_XF_NONE) return v;
  const f32x4 lo = unpack4(uint2{v.x, v.y}), hi = unpack4(uint2{v.z, v.w});
  f32x4 a, c;
#pragma unroll
  for (int e = 0; e < 4; ++e) {  // (both affine forms before both SiLUs, not two xform1 in a row: that order moved the instruction
                                 // stream of wgrad_thin_bf16_kernel<false,2> and conv_thinn_bf16_kernel<2>)
    float u = lo[e] * sc[e] + sh[e], w = hi[e] * sc[4 + e] + sh[4 + e];
    if (XF == VAE_XF_AFFINE_SILU) {
      u = silu_f(u);
      w = silu_f(w);
    }
    a[e] = ok ? u : 0.f;
    c[e] = ok ? w : 0.f;
  }
  const uint2 pa = pack4(a), pc = pack4(c);
  return uint4{pa.x, pa.y, pc.x, pc.y};
}

// ---------------------------------------------------------------------------------------------------------
// slab protocol of the weight gradients: grid = splits x 128-channel blocks of the wide side; split `split` writes its own slab
// (the output itself when there is one split) and its own row of bias partials; vae_reduce_splits adds them in a fixed order
// ---------------------------------------------------------------------------------------------------------
struct Slab {
  float* __restrict__ O;
  int64_t ld;  // taps * N: one row of out[M][taps][N]
  int N;
  float alpha;
};
__device__ __forceinline__ Slab slab_of(const vae_wgrad_args& p, int split, int taps) {
  const int64_t ld = (int64_t)taps * p.N;
  return Slab{p.nsplit == 1 ? p.out : p.partial + (int64_t)split * p.M * ld, ld, p.N, p.alpha};
}
// element (wide channel ch, tap t, narrow channel s): SMALL_X (the narrow side is X) out[ch][t][s], else out[s][t][ch]
template <bool SMALL_X>
__device__ __forceinline__ void slab_store(const Slab& sl, int ch, int t, int s, float r) {
  if (SMALL_X) sl.O[(int64_t)ch * sl.ld + (int64_t)t * sl.N + s] = sl.alpha * r;
  else sl.O[(int64_t)s * sl.ld + (int64_t)t * sl.N + ch] = sl.alpha * r;
}
__device__ __forceinline__ float* bias_partial_row(const vae_wgrad_args& p, int split) { return p.bias_partial + (int64_t)split * p.M; }

// ---------------------------------------------------------------------------------------------------------
// host: what the *_eligible functions of the three files ask
// ---------------------------------------------------------------------------------------------------------
// stride 1 and an output map that is the source map ...
inline bool same_map(const vae_conv_geom& g) { return g.stride == 1 && g.Ho == g.Hs && g.Wo == g.Ws; }
// ... as the plain forward 3x3 'same' convolution (padding 1)
inline bool fwd_same_3x3(const vae_conv_geom& g) { return g.mode == VAE_MODE_FWD && g.taps == 9 && same_map(g) && g.pad_t == 1 && g.pad_l == 1; }
// one buffer descriptor covers `elems` elements of `esize` bytes
inline bool desc_fits(size_t elems, unsigned esize) { return elems * esize < BUF_MAX; }
inline size_t source_elems(const vae_conv_geom& g) { return (size_t)g.B * g.Hs * g.Ws * g.Cs; }  // the whole source tensor
inline size_t image_elems(const vae_conv_geom& g) { return (size_t)g.Hs * g.Ws * g.Cs; }          // one image of it
inline bool narrow_fits(const vae_conv_geom& g) { return desc_fits(source_elems(g), 4u); }        // narrow_rsrc with Cs = g.Cs

// weight gradient with a <= 4-channel side: 0 = not served, 1 = the narrow side is X (N <= 4), 2 = the narrow side is dY (M <= 4)
inline int wgrad_kind(const vae_wgrad_args& a) {
  const vae_conv_geom& g = a.g;
  if (a.batch != 1 || g.taps > TAPS_MAX) return 0;
  if (!desc_fits((size_t)a.npix * a.ldy, 4u) || !narrow_fits(g)) return 0;
  if (a.N <= 4 && a.xf == VAE_XF_NONE && (g.mode == VAE_MODE_FWD || g.mode == VAE_MODE_UP2X)) return 1;
  // transposed gather: plain stride-1 'same' geometry only (every input pixel is the centre tap of one output pixel)
  if (a.M <= 4 && (fwd_same_3x3(g) || (g.mode == VAE_MODE_FWD && g.taps == 1 && same_map(g) && g.pad_t == 0 && g.pad_l == 0))) return 2;
  return 0;
}
inline int wgrad_tiles(const vae_wgrad_args& a) { return (int)(((int64_t)a.g.B * a.g.Ho * a.g.Wo + TP - 1) / TP); }
// how a pixel of V (the wide tensor) and a tap map to a pixel of S (the narrow one)
inline vae_conv_geom wgrad_geom(const vae_wgrad_args& a, int kind) {
  vae_conv_geom gs = a.g;
  if (kind == 2) {  // V = X over input pixels; S = dY at (y + pad - kh, x + pad - kw)
    gs.mode = VAE_MODE_DGRAD;
    gs.Cs = a.ldy;
  }
  return gs;
}
inline dim3 wgrad_grid(const vae_wgrad_args& a, int kind) { return dim3((unsigned)a.nsplit, (unsigned)(((kind == 1 ? a.M : a.N) + 127) / 128)); }

}  // namespace thin
