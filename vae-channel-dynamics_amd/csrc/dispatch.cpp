// Kernel selection for the two contraction forms (vae_igemm_rows: conv forward / dgrad / GEMM rows; vae_wgrad: weight
// gradients).  select_rows and select_wgrad hold the only copy of each selection order, including every library option
// that chooses a kernel; the launches, the profiler labels and every query below are a validation step plus a switch on
// (or a predicate over) what they select.  Host code only: the kernels and their launchers live in the .hip files.
#include <stdio.h>
#include <algorithm>
#include "launchers.h"

namespace {

constexpr int BK = 32;  // K step of the flat kernels (igemm.hip)
const char* const TF[2] = {"false", "true"};

int check_geom(const char* who, const vae_conv_geom& g) {
  VAE_CHECK(g.B > 0 && g.Hs > 0 && g.Ws > 0 && g.Cs > 0 && g.Ho > 0 && g.Wo > 0, "%s: non-positive geometry", who);
  VAE_CHECK(g.taps == 1 || g.taps == 9, "%s: taps must be 1 or 9 (got %d)", who, g.taps);
  VAE_CHECK(g.stride == 1 || g.stride == 2, "%s: stride must be 1 or 2", who);
  VAE_CHECK(g.mode >= 0 && g.mode <= 4, "%s: bad mode", who);
  VAE_CHECK(g.mode != VAE_MODE_UP2X_DGRAD || (g.taps == 9 && g.stride == 1 && g.Hs == 2 * g.Ho && g.Ws == 2 * g.Wo),
            "%s: UP2X_DGRAD needs 3x3 stride 1, source twice the row grid", who);
  VAE_CHECK(g.mode != VAE_MODE_DGRAD_S2 ||
                (g.taps == 9 && g.stride == 2 && g.pad_t == 0 && g.pad_l == 0 && g.Ho % 2 == 0 && g.Wo % 2 == 0 &&
                 ((int64_t)g.B * g.Ho * g.Wo / 4) % 128 == 0),
            "%s: DGRAD_S2 needs 3x3 stride 2 pad 0, even row grid and B*Ho*Wo/4 %% 128 == 0", who);
  VAE_CHECK(g.mode != VAE_MODE_UP2X || (g.taps == 9 && g.stride == 1), "%s: up2x needs 3x3 stride 1", who);
  return 0;
}

// rows of one 128-row tile span at most nb batch items; the LDS table holds SS_HALF scale entries
bool xf_rows_ok(const vae_conv_geom& g, int M, int K) {
  const int hw = g.Ho * g.Wo;
  const int nb = (hw % 128 == 0) ? 1 : (127 / hw + 2);
  return (K % 4 == 0) && ((int64_t)std::min(nb, g.B) * K <= SS_HALF);
}
bool xf_wgrad_ok(const vae_conv_geom& g, int npix, int nsplit, int N) {
  const int hw = g.Ho * g.Wo;
  int chunk = (npix + nsplit - 1) / nsplit;
  chunk = ((chunk + BK - 1) / BK) * BK;
  const int nb = (hw % chunk == 0) ? 1 : ((chunk - 1) / hw + 2);
  const int bn = 128;  // conservative: the widest N tile any instantiation uses
  return (N % 4 == 0) && ((int64_t)std::min(nb, g.B) * bn <= SS_HALF);
}

// ------------------------------------------------------------------------------------------------------------------------
// rows: eligibility of the kernel families under the library options (the building blocks of select_rows)
// ------------------------------------------------------------------------------------------------------------------------
bool rows_bkm(const vae_igemm_args& a) { return (a.sn == 1) && (a.sk != 1); }
bool rows_vec(const vae_igemm_args& a, bool bkm) {
  bool vec = aligned16(a.A) && aligned16(a.W) && (a.g.Cs % 4 == 0) && (a.K % 4 == 0) && (a.st % 4 == 0) &&
             (a.sAb % 4 == 0) && (a.sWb % 4 == 0);
  if (bkm) vec = vec && (a.sk % 4 == 0) && (a.N % 4 == 0);
  else vec = vec && (a.sn % 4 == 0);
  if (a.xf != VAE_XF_NONE) vec = vec && aligned16(a.scale) && aligned16(a.shift);
  return vec;
}
bool rows_is_phase(const vae_igemm_args& a) { return a.tapmask != 0 || a.a_step > 1 || a.c_step > 1; }
bool rows_use_tile(const vae_igemm_args& a, bool vec, bool bkm) { return conv3_tile_eligible(a, vec, bkm) && !vae_opt().flat_conv; }
// the bf16 halo-tile kernel reads the weights from their bf16 image; without one the bf16 flat kernel serves the layer
bool rows_use_tile_bf16(const vae_igemm_args& a, bool vec, bool bkm) {
  return a.prec == VAE_PREC_BF16 && rows_use_tile(a, vec, bkm) && conv3_tile_bf16_packed(a);
}
// the wide-tile kernel serves a layer the 128-pixel bf16 halo-tile kernel would serve, when both operands are bf16 images
bool rows_use_wide_bf16(const vae_igemm_args& a, bool vec, bool bkm) {
  return rows_use_tile_bf16(a, vec, bkm) && conv3_wide_bf16_eligible(a) && !vae_opt().no_wide;
}

enum class RowsKernel { UpWino, Wino4, Wino, WideBf16, TileBf16, Tile, ThinBf16, SmallK, ThinnBf16, SmallN, Conv1Bf16, RowsBf16, RowsF32, None };

// The Winograd family, for the layer `a` describes (a.Wu ignored): the upsampler convolution (forward over the virtual
// nearest-2x upsample, or its dgrad with the 2x2 sum-pool folded in) as the 9-position scheme; the plain 3x3 stride-1
// layers whose maps are whole 16 x 32 tiles with whole 64-channel blocks as F(4x4,3x3) (36 instead of 64 multiplications per
// 4x4 outputs; option "no_wino4" keeps them on F(2x2,3x3)), the others as F(2x2,3x3).
RowsKernel select_wino(const vae_igemm_args& a) {
  if (vae_opt().flat_conv || vae_opt().no_wino) return RowsKernel::None;
  if (conv3_upwino_eligible(a)) return RowsKernel::UpWino;
  if (!conv3_wino_eligible(a) || !rows_vec(a, rows_bkm(a)) || conv_smallk_eligible(a) || conv_smalln_eligible(a)) return RowsKernel::None;
  return (conv3_wino4_eligible(a) && !vae_opt().no_wino4) ? RowsKernel::Wino4 : RowsKernel::Wino;
}

// An operand image (A16, xf == NONE) on a layer that no halo-tile kernel serves is, for the flat / <= 4-channel kernels, the
// same thing as "A is stored as bf16": the dispatcher rewrites it that way, so a host may hand over a bf16 tensor as A16
// without knowing which kernel will run.
vae_igemm_args rows_canon(const vae_igemm_args& a) {
  vae_igemm_args b = a;
  if (b.A16 != nullptr && b.prec == VAE_PREC_BF16 && b.xf == VAE_XF_NONE && !rows_is_phase(b)) {
    vae_igemm_args t = b;  // (the vectorisation test reads the pointer the kernel would read)
    if (t.A == nullptr) t.A = reinterpret_cast<const float*>(t.A16);
    const bool bkm = rows_bkm(t);
    if (!rows_use_tile_bf16(t, rows_vec(t, bkm), bkm)) {
      b.A = reinterpret_cast<const float*>(b.A16);
      b.A16 = nullptr;
      b.a_bf16 = 1;
    }
  }
  return b;
}

struct RowsSel {
  vae_igemm_args a;  // canonicalised arguments: what the kernel receives
  bool bkm, vec;
  RowsKernel k;
};

// THE selection order of vae_igemm_rows
RowsSel select_rows(const vae_igemm_args& in) {
  RowsSel s;
  s.a = rows_canon(in);
  const vae_igemm_args& a = s.a;
  s.bkm = rows_bkm(a);
  s.vec = rows_vec(a, s.bkm);
  const bool bf16 = a.prec == VAE_PREC_BF16;
  s.k = [&] {
    if (a.Wu != nullptr) {  // transformed weights: the Winograd kernel they were built for (elsewhere the launch refuses them)
      const RowsKernel w = select_wino(a);
      if (w != RowsKernel::None) return w;
    }
    if (rows_is_phase(a)) {  // sub-sampled views / tap subsets: only the halo-tile kernels implement them (vae_conv_phase_ok)
      if (rows_use_wide_bf16(a, s.vec, s.bkm)) return RowsKernel::WideBf16;
      return bf16 ? RowsKernel::TileBf16 : RowsKernel::Tile;
    }
    if (a.A16 == nullptr && conv_smallk_eligible(a))  // bf16 output in bf16 mode: the same launch on the matrix pipe
      return (conv_thin_bf16_eligible(a) && !vae_opt().no_thin_mfma) ? RowsKernel::ThinBf16 : RowsKernel::SmallK;
    if (conv_smalln_eligible(a))  // bf16 input in bf16 mode: the same launch on the matrix pipe
      return (conv_thinn_bf16_eligible(a) && !vae_opt().no_thin_mfma) ? RowsKernel::ThinnBf16 : RowsKernel::SmallN;
    if (rows_use_wide_bf16(a, s.vec, s.bkm)) return RowsKernel::WideBf16;
    if (rows_use_tile_bf16(a, s.vec, s.bkm)) return RowsKernel::TileBf16;
    if (!bf16 && rows_use_tile(a, s.vec, s.bkm)) return RowsKernel::Tile;  // 3x3 stride-1: LDS halo tile shared by the 9 taps
    if (bf16 && s.vec) return (!vae_opt().flat_conv && conv1_bf16_eligible(a)) ? RowsKernel::Conv1Bf16 : RowsKernel::RowsBf16;
    return RowsKernel::RowsF32;
  }();
  return s;
}

bool is_wino(RowsKernel k) { return k == RowsKernel::UpWino || k == RowsKernel::Wino4 || k == RowsKernel::Wino; }

// Storage flags (vaehip.h: out_bf16 / a_bf16 / res_bf16): does the kernel that serves `a` honour them as they are set?
bool tile16_flags_ok(const vae_igemm_args& a) {  // the 128-pixel bf16 halo-tile kernel (conv3_tile_bf16.hip)
  return !a.a_bf16 && (!a.out_bf16 || (a.track == nullptr && a.ldc % 2 == 0 && a.N % 2 == 0)) &&
         (a.res == nullptr || (a.res_bf16 != 0) == (a.out_bf16 != 0));
}
bool rows_io16_ok(const RowsSel& s) {
  const vae_igemm_args& a = s.a;
  if (!a.out_bf16 && !a.a_bf16 && !a.res_bf16) return true;
  if (a.prec != VAE_PREC_BF16 || a.Wu != nullptr) return false;  // fp32-arithmetic kernels: fp32 storage
  if (a.res_bf16 && a.res == nullptr) return false;
  switch (s.k) {
    case RowsKernel::WideBf16: return true;  // (its eligibility covers the flags)
    case RowsKernel::TileBf16:
      return tile16_flags_ok(a) && (!rows_is_phase(a) || (a.A16 == nullptr && a.xf == VAE_XF_NONE && rows_use_tile_bf16(a, s.vec, s.bkm)));
    case RowsKernel::ThinBf16: case RowsKernel::SmallK: return !a.a_bf16 && !a.res_bf16;  // wide side = the output
    case RowsKernel::ThinnBf16: case RowsKernel::SmallN: return !a.out_bf16 && !a.res_bf16;  // wide side = the input
    case RowsKernel::Conv1Bf16: case RowsKernel::RowsBf16: return a.A16 == nullptr;  // the bf16 flat kernels take any combination
    default: return false;  // unvectorised shapes run the fp32 kernel
  }
}

int rows_gstat_chunks(const RowsSel& s) {
  const vae_igemm_args& a = s.a;
  if (a.Wu != nullptr) return s.k == RowsKernel::Wino4 ? conv3_wino4_gstat_chunks(a) : conv3_wino_eligible(a) ? conv3_wino_gstat_chunks(a) : 0;
  // (a phase form selects a halo-tile kernel before it is known to serve the layer; the launch refuses statistics there, after
  // this answer: the answer is that of the plain form)
  switch (s.k) {
    case RowsKernel::WideBf16: return conv3_wide_bf16_gstat_chunks(a);
    case RowsKernel::TileBf16: return rows_use_tile_bf16(a, s.vec, s.bkm) ? conv3_tile_bf16_gstat_chunks(a) : 0;
    case RowsKernel::Tile:
      return (rows_use_tile(a, s.vec, s.bkm) && !(a.A16 == nullptr && conv_smallk_eligible(a))) ? conv3_tile_gstat_chunks(a) : 0;
    default: return 0;
  }
}

int rows_gnb_chunks(const RowsSel& s) {
  if (s.a.Wu == nullptr) return 0;  // (the other dgrad kernels have no such epilogue yet)
  if (s.k == RowsKernel::Wino4) return conv3_wino4_gnb_chunks(s.a);
  if (s.k == RowsKernel::Wino) return conv3_wino_gnb_chunks(s.a);
  return 0;
}

// name of the kernel instantiation the launch runs (the rocprofv3 kernel name, profiling labels); the template arguments
// are the ones the launcher picks
void rows_kernel_name(const RowsSel& s, char* buf, int n) {
  const vae_igemm_args& a = s.a;
  const bool dg = a.g.mode == VAE_MODE_DGRAD, up = a.g.mode == VAE_MODE_UP2X;
  switch (s.k) {
    case RowsKernel::UpWino: snprintf(buf, n, "conv3_upwino_kernel<%s>", TF[a.g.mode == VAE_MODE_UP2X_DGRAD]); break;
    case RowsKernel::Wino4: snprintf(buf, n, "conv3_wino4_kernel<%d>", a.xf); break;
    case RowsKernel::Wino: snprintf(buf, n, "conv3_wino_kernel<%d,%d>", a.xf, CONV3_WINO_NB); break;
    case RowsKernel::WideBf16: snprintf(buf, n, "conv3_wide_bf16_kernel<%s,%d>", TF[dg], a.tapmask != 0 ? 2 : 3); break;
    case RowsKernel::TileBf16:  // (a phase form never reads an operand image there)
      snprintf(buf, n, "conv3_tile_bf16_kernel<%s,%s,%d,%s>", TF[dg], TF[up], a.xf, TF[a.A16 != nullptr && !rows_is_phase(a)]);
      break;
    case RowsKernel::Tile: snprintf(buf, n, "conv3_tile_kernel<%s,%s,%s,%d>", TF[s.bkm], TF[dg], TF[up], a.xf); break;
    case RowsKernel::ThinBf16: snprintf(buf, n, "conv_thin_bf16_kernel"); break;
    case RowsKernel::SmallK: snprintf(buf, n, "conv_smallk_kernel"); break;
    case RowsKernel::ThinnBf16: snprintf(buf, n, "conv_thinn_bf16_kernel<%d>", a.xf); break;
    case RowsKernel::SmallN: snprintf(buf, n, "conv_smalln_kernel<%d>", a.xf); break;
    case RowsKernel::Conv1Bf16: snprintf(buf, n, "conv1_bf16_kernel<%s,%d>", TF[dg], a.K / 16); break;
    case RowsKernel::RowsBf16: snprintf(buf, n, "igemm_rows_bf16_kernel<%s,%s,%d>", a.N <= 32 ? "128,32,4,1" : "128,128,4,2", TF[s.bkm], a.xf); break;
    default: snprintf(buf, n, "igemm_rows_kernel<%s,%s,%s,%d>", a.N <= 32 ? "128,32,4,1" : "128,128,4,2", TF[s.bkm], TF[s.vec], a.xf); break;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// wgrad
// ------------------------------------------------------------------------------------------------------------------------
bool wgrad_vec(const vae_wgrad_args& a) {
  bool vec = aligned16(a.dY) && aligned16(a.X) && (a.g.Cs % 4 == 0) && (a.ldy % 4 == 0) && (a.M % 4 == 0) &&
             (a.N % 4 == 0) && (a.sYb % 4 == 0) && (a.sXb % 4 == 0);
  if (a.xf != VAE_XF_NONE) vec = vec && aligned16(a.scale) && aligned16(a.shift);
  return vec;
}
bool wgrad_is_phase(const vae_wgrad_args& a) { return a.tapmask != 0 || a.y_step > 1; }
bool wgrad_use_tile(const vae_wgrad_args& a) { return wgrad3_tile_eligible(a, wgrad_vec(a)) && !vae_opt().flat_conv; }
// option "no_wgrad_dma": the bf16 images are staged through registers, and the stride-2 layers (which only the LDS-DMA kernel
// serves) go to the flat kernel
bool wgrad_dma(const vae_wgrad_args& a) { return wgrad3_dma_bf16_operands(a) && !vae_opt().no_wgrad_dma; }
bool wgrad_use_tile_bf16(const vae_wgrad_args& a) {
  return a.prec == VAE_PREC_BF16 && wgrad3_tile_bf16_eligible(a, wgrad_vec(a), wgrad_dma(a)) && !vae_opt().flat_conv;
}

// operand images (X16 with xf == NONE, dY16) on a layer the bf16 halo-tile kernel does not serve become "X / dY is stored as
// bf16" for the flat / <= 4-channel kernels (as rows_canon does for A16)
vae_wgrad_args wgrad_canon(const vae_wgrad_args& a) {
  vae_wgrad_args b = a;
  if ((b.X16 != nullptr || b.dY16 != nullptr) && b.prec == VAE_PREC_BF16 && !wgrad_is_phase(b)) {
    vae_wgrad_args t = b;
    if (t.X16 != nullptr && t.xf == VAE_XF_NONE) t.X = reinterpret_cast<const float*>(t.X16);
    if (t.dY16 != nullptr && t.dY == nullptr) t.dY = reinterpret_cast<const float*>(t.dY16);
    // (a tensor the halo-tile kernels cannot take as an image -- rows that are no whole 16-byte pieces -- is a stored tensor too)
    const bool images = (t.dY16 == nullptr || (aligned16(t.dY16) && t.ldy % 8 == 0 && t.M % 8 == 0)) &&
                        (t.X16 == nullptr || t.xf != VAE_XF_NONE || (aligned16(t.X16) && t.g.Cs % 8 == 0));
    if (!wgrad_use_tile_bf16(t) || !images) {
      if (b.X16 != nullptr && b.xf == VAE_XF_NONE) { b.X = reinterpret_cast<const float*>(b.X16); b.X16 = nullptr; b.x_bf16 = 1; }
      if (b.dY16 != nullptr) { b.dY = reinterpret_cast<const float*>(b.dY16); b.dY16 = nullptr; b.y_bf16 = 1; }
    }
  }
  return b;
}

enum class WgradKernel { DmaBf16, TileBf16, Tile, ThinBf16, SmallK, Bf16, F32 };

struct WgradSel {
  vae_wgrad_args a;  // canonicalised arguments
  bool vec;
  WgradKernel k;
};

// THE selection order of vae_wgrad
WgradSel select_wgrad(const vae_wgrad_args& in) {
  WgradSel s;
  s.a = wgrad_canon(in);
  const vae_wgrad_args& a = s.a;
  s.vec = wgrad_vec(a);
  const bool bf16 = a.prec == VAE_PREC_BF16;
  s.k = [&] {
    if (wgrad_is_phase(a)) {  // sub-sampled dY / tap subsets: the halo-tile kernels implement them (vae_wgrad_phase_ok)
      if (!bf16) return WgradKernel::Tile;
      return wgrad_dma(a) ? WgradKernel::DmaBf16 : WgradKernel::TileBf16;
    }
    if (a.X16 == nullptr && wgrad_smallk_kind(a))  // bf16 mode, wide side stored as bf16: the same launch on the matrix pipe
      return (wgrad_thin_bf16_eligible(a, wgrad_smallk_kind(a)) && !vae_opt().no_thin_mfma) ? WgradKernel::ThinBf16 : WgradKernel::SmallK;
    if (wgrad_use_tile_bf16(a)) return wgrad_dma(a) ? WgradKernel::DmaBf16 : WgradKernel::TileBf16;
    if (wgrad_use_tile(a)) return WgradKernel::Tile;  // 3x3 stride-1: the nine taps share one staged dY tile + X halo
    return (bf16 && s.vec) ? WgradKernel::Bf16 : WgradKernel::F32;
  }();
  return s;
}

// storage flags of the weight gradient's operands (vaehip.h: x_bf16 / y_bf16)
bool wgrad_io16_ok(const WgradSel& s) {
  const vae_wgrad_args& a = s.a;
  if (!a.x_bf16 && !a.y_bf16) return true;
  if (a.prec != VAE_PREC_BF16 || wgrad_is_phase(a)) return false;  // the halo-tile kernels take images through X16 / dY16
  switch (s.k) {
    case WgradKernel::ThinBf16: case WgradKernel::SmallK:  // only the wide side may be bf16 (kind 1: dY, kind 2: X)
      return wgrad_smallk_kind(a) == 1 ? !a.x_bf16 : !a.y_bf16;
    case WgradKernel::Bf16: return a.X16 == nullptr && a.dY16 == nullptr;  // the bf16 flat kernel
    default: return false;
  }
}

void wgrad_kernel_name(const WgradSel& s, char* buf, int n) {
  const vae_wgrad_args& a = s.a;
  const bool phase = wgrad_is_phase(a);  // (a phase form is a FWD stride-1 geometry)
  const bool up = a.g.mode == VAE_MODE_UP2X;
  const char* tile = a.M <= 32 ? "32,128,1,4" : (a.N <= 32 ? "128,32,4,1" : "128,128,4,2");
  switch (s.k) {
    case WgradKernel::DmaBf16: snprintf(buf, n, "wgrad3_dma_bf16_kernel<%s,%d>", TF[up && !phase], phase ? 1 : a.g.stride); break;
    case WgradKernel::TileBf16:
      snprintf(buf, n, "wgrad3_tile_bf16_kernel<%s,%d,%s,%s>", TF[up && !phase], a.xf, TF[a.X16 != nullptr], TF[a.dY16 != nullptr]);
      break;
    case WgradKernel::Tile: snprintf(buf, n, "wgrad3_tile_kernel<%s,%d>", TF[up], a.xf); break;
    case WgradKernel::ThinBf16: snprintf(buf, n, "wgrad_thin_bf16_kernel<%s,%d>", TF[wgrad_smallk_kind(a) == 1], a.xf); break;
    case WgradKernel::SmallK: snprintf(buf, n, "wgrad_smallk_kernel<%s,%d>", TF[wgrad_smallk_kind(a) == 1], a.xf); break;
    case WgradKernel::Bf16: snprintf(buf, n, "wgrad_bf16_kernel<%s,%d>", tile, a.xf); break;
    default: snprintf(buf, n, "wgrad_kernel<%s,%s,%d>", tile, TF[s.vec], a.xf); break;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------
// C ABI: rows
// ------------------------------------------------------------------------------------------------------------------------
extern "C" int vae_xf_fusable_rows(const vae_conv_geom* g, int32_t M, int32_t K) { return g && xf_rows_ok(*g, M, K) ? 1 : 0; }

// both the forward and the wgrad of this 3x3 stride-1 layer run on the bf16 halo-tile kernels (which can read a bf16
// activation image); pointers are placeholders with the alignment the real ones must have
extern "C" int vae_bf16_act_image_ok(const vae_conv_geom* gp, int32_t Cout, int32_t Cin) {
  if (!gp) return 0;
  const vae_conv_geom& g = *gp;
  if (g.mode != VAE_MODE_FWD || Cin % 8 != 0 || g.Cs != Cin) return 0;
  static const float dummy[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};
  vae_igemm_args f{};
  f.A = f.W = dummy; f.C = const_cast<float*>(dummy); f.Wh = dummy;
  f.g = g; f.M = g.B * g.Ho * g.Wo; f.N = Cout; f.K = Cin; f.ldc = Cout;
  f.sn = (int64_t)g.taps * Cin; f.sk = 1; f.st = Cin; f.batch = 1; f.alpha = 1.f; f.prec = VAE_PREC_BF16; f.xf = VAE_XF_NONE;
  if (select_rows(f).k != RowsKernel::TileBf16) return 0;
  vae_wgrad_args w{};
  w.dY = w.X = dummy; w.g = g; w.M = Cout; w.N = Cin; w.ldy = Cout; w.npix = f.M; w.nsplit = 1; w.batch = 1; w.alpha = 1.f;
  w.prec = VAE_PREC_BF16; w.xf = VAE_XF_NONE;
  return select_wgrad(w).k == WgradKernel::TileBf16 ? 1 : 0;
}

// the output gradient of this 3x3 stride-1 layer may be handed over as a bf16 image: its dgrad (A16) and its weight
// gradient (dY16) both run on the bf16 halo-tile kernels
extern "C" int vae_bf16_grad_image_ok(const vae_conv_geom* gp, int32_t Cout, int32_t Cin) {
  if (!gp) return 0;
  const vae_conv_geom& g = *gp;
  if (g.mode != VAE_MODE_FWD || g.taps != 9 || g.stride != 1 || Cin % 8 != 0 || Cout % 8 != 0 || g.Ho != g.Hs || g.Wo != g.Ws) return 0;
  static const float dummy[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};
  vae_igemm_args d{};  // the dgrad launch ops.conv_dgrad builds
  d.A = d.W = dummy; d.C = const_cast<float*>(dummy); d.Wh = dummy;
  d.g = g; d.g.Cs = Cout; d.g.mode = VAE_MODE_DGRAD;
  d.M = g.B * g.Ho * g.Wo; d.N = Cin; d.K = Cout; d.ldc = Cin;
  d.sn = 1; d.sk = (int64_t)g.taps * Cin; d.st = Cin; d.batch = 1; d.alpha = 1.f; d.prec = VAE_PREC_BF16; d.xf = VAE_XF_NONE;
  if (select_rows(d).k != RowsKernel::TileBf16) return 0;
  vae_wgrad_args w{};
  w.dY = w.X = dummy; w.g = g; w.g.Cs = Cin; w.M = Cout; w.N = Cin; w.ldy = Cout; w.npix = d.M; w.nsplit = 1; w.batch = 1; w.alpha = 1.f;
  w.prec = VAE_PREC_BF16; w.xf = VAE_XF_NONE;
  return select_wgrad(w).k == WgradKernel::TileBf16 ? 1 : 0;
}

extern "C" int vae_wino_ok(const vae_igemm_args* ap) { return (ap && select_wino(*ap) != RowsKernel::None) ? 1 : 0; }
extern "C" int64_t vae_wino_weight_floats(const vae_igemm_args* ap) {
  if (!ap) return 0;
  const bool up = ap->g.mode == VAE_MODE_UP2X || ap->g.mode == VAE_MODE_UP2X_DGRAD;
  return (int64_t)(up ? 9 : (select_wino(*ap) == RowsKernel::Wino4 ? 36 : 16)) * ap->N * ap->K;
}
// bytes Wu must hold for the kernel that serves the launch: the upsampler kernel's image may be bf16 planes, 6 bytes per value
extern "C" int64_t vae_wino_weight_bytes(const vae_igemm_args* ap) {
  if (!ap) return 0;
  if (select_wino(*ap) == RowsKernel::UpWino) return conv3_upwino_weight_bytes(*ap);
  return 4 * vae_wino_weight_floats(ap);
}
extern "C" int vae_wino_weights(const vae_igemm_args* ap, float* Wu, void* stream) {
  VAE_CHECK(ap && Wu && ap->W && aligned16(Wu), "wino_weights: null or unaligned pointer");
  const RowsKernel k = select_wino(*ap);
  VAE_CHECK(k != RowsKernel::None, "wino_weights: the layer is not served by the Winograd kernel (vae_wino_ok)");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = (k == RowsKernel::UpWino ? launch_upwino_weights : k == RowsKernel::Wino4 ? launch_wino4_weights : launch_wino_weights)(*ap, Wu, st)) return rc;
  VAE_LAUNCH_CHECK(k == RowsKernel::UpWino ? "upwino_weights" : "wino_weights");
  return VAE_OK;
}

extern "C" int vae_conv_io16_ok(const vae_igemm_args* ap) { return (ap && rows_io16_ok(select_rows(*ap))) ? 1 : 0; }
extern "C" int vae_conv_phase_ok(const vae_igemm_args* ap) {
  if (!ap) return 0;
  const vae_igemm_args& a = *ap;
  const bool bkm = rows_bkm(a), vec = rows_vec(a, bkm);
  if (a.A16 != nullptr) return rows_use_wide_bf16(a, vec, bkm) ? 1 : 0;  // operand image: the wide-tile kernel's 2x2 tap blocks
  if (a.prec == VAE_PREC_BF16) return (a.xf == VAE_XF_NONE && rows_use_tile_bf16(a, vec, bkm)) ? 1 : 0;  // no transform variant there
  return rows_use_tile(a, vec, bkm) ? 1 : 0;
}
extern "C" int vae_conv_gnb_chunks(const vae_igemm_args* ap) { return ap ? rows_gnb_chunks(select_rows(*ap)) : 0; }
extern "C" int vae_conv_gstat_chunks(const vae_igemm_args* ap) { return ap ? rows_gstat_chunks(select_rows(*ap)) : 0; }

extern "C" int vae_igemm_kernel_name(const vae_igemm_args* ap, char* buf, int32_t n) {
  VAE_CHECK(ap && buf && n > 0, "igemm_kernel_name: bad args");
  rows_kernel_name(select_rows(*ap), buf, n);
  return VAE_OK;
}

extern "C" int vae_igemm_rows(const vae_igemm_args* ap, void* stream) {
  VAE_CHECK(ap != nullptr, "igemm_rows: null args");
  const RowsSel s = select_rows(*ap);
  const vae_igemm_args& a = s.a;
  if (int e = check_geom("igemm_rows", a.g)) return e;
  VAE_CHECK(a.A && a.W && a.C, "igemm_rows: null operand");
  VAE_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.batch > 0, "igemm_rows: bad sizes M=%d N=%d K=%d", a.M, a.N, a.K);
  VAE_CHECK(a.K <= a.g.Cs, "igemm_rows: K=%d exceeds source channels %d", a.K, a.g.Cs);
  VAE_CHECK((int64_t)a.g.B * a.g.Ho * a.g.Wo == a.M, "igemm_rows: M=%d != B*Ho*Wo", a.M);
  VAE_CHECK(a.ldc >= a.N, "igemm_rows: ldc < N");
  VAE_CHECK((size_t)a.M * a.ldc * 4u < BUF_MAX, "igemm_rows: output too large for 32-bit byte offsets");
  VAE_CHECK(a.prec == VAE_PREC_F32 || a.prec == VAE_PREC_BF16, "igemm_rows: bad prec %d", a.prec);
  VAE_CHECK(a.sk == 1 || a.sn == 1, "igemm_rows: one of sn, sk must be 1 (sn=%lld sk=%lld)", (long long)a.sn,
            (long long)a.sk);
  VAE_CHECK(a.xf == VAE_XF_NONE || (a.scale && a.shift), "igemm_rows: xf needs scale/shift");
  VAE_CHECK(a.xf == VAE_XF_NONE || xf_rows_ok(a.g, a.M, a.K),
            "igemm_rows: fused GroupNorm needs the tile's scale/shift rows to fit LDS (see vae_xf_fusable_rows)");
  VAE_CHECK(a.gstat == nullptr || rows_gstat_chunks(s) > 0, "igemm_rows: no statistics epilogue for these arguments (vae_conv_gstat_chunks)");
  VAE_CHECK(a.gnb_ws == nullptr || rows_gnb_chunks(s) > 0, "igemm_rows: no GroupNorm-backward epilogue for these arguments (vae_conv_gnb_chunks)");
  VAE_CHECK(a.gnb_ws == nullptr || (a.gnb_mean && a.gnb_rstd && a.gnb_gamma && a.gnb_beta && aligned16(a.gnb_x)), "igemm_rows: gnb_* pointers");
  VAE_CHECK(rows_io16_ok(s), "igemm_rows: the kernel serving these arguments does not take this combination of out_bf16 / a_bf16 / res_bf16 (vae_conv_io16_ok)");
  VAE_CHECK(a.g.mode != VAE_MODE_UP2X_DGRAD || a.Wu != nullptr, "igemm_rows: UP2X_DGRAD exists only as the Winograd-type kernel (vae_wino_ok, Wu)");
  // Winograd: Wu holds the transformed weights vae_wino_weights built for THIS layer under the same options
  VAE_CHECK(a.Wu == nullptr || is_wino(s.k), "igemm_rows: Wu needs a layer vae_wino_ok accepts");
  if (s.k == RowsKernel::Wino) VAE_CHECK(aligned16(a.Wu), "igemm_rows: Wu needs a layer vae_wino_ok accepts");
  else if (is_wino(s.k)) VAE_CHECK(aligned16(a.Wu), "igemm_rows: unaligned Wu");
  if (rows_is_phase(a) && !is_wino(s.k)) {
    VAE_CHECK(vae_conv_phase_ok(&a), "igemm_rows: tapmask / a_step / c_step need a halo-tile kernel (vae_conv_phase_ok)");
    VAE_CHECK(a.track == nullptr && a.gstat == nullptr, "igemm_rows: no tracker / statistics epilogue on a sub-sampled output");
    VAE_CHECK(s.k == RowsKernel::WideBf16 || a.A16 == nullptr, "igemm_rows: a sub-sampled view of an operand image needs the wide-tile kernel (vae_conv_phase_ok)");
  } else if (s.k == RowsKernel::WideBf16 || s.k == RowsKernel::TileBf16 || s.k == RowsKernel::Tile || s.k == RowsKernel::Conv1Bf16 ||
             s.k == RowsKernel::RowsBf16 || s.k == RowsKernel::RowsF32) {
    VAE_CHECK(a.A16 == nullptr || (a.xf == VAE_XF_NONE && rows_use_tile_bf16(a, s.vec, s.bkm) && aligned16(a.A16) && a.g.Cs % 8 == 0),
              "igemm_rows: A16 needs bf16 mode, xf == NONE and a layer vae_bf16_act_image_ok accepts");
  }
  const bool flat = s.k == RowsKernel::Conv1Bf16 || s.k == RowsKernel::RowsBf16 || s.k == RowsKernel::RowsF32;
  if (flat && s.vec) {  // flat vectorised kernels address one tile's images / the weights with 32-bit byte offsets
    const int64_t rows_per_img = (a.g.mode == VAE_MODE_DGRAD_S2) ? (int64_t)a.g.Ho * a.g.Wo / 4 : (int64_t)a.g.Ho * a.g.Wo;
    const int64_t span = std::min<int64_t>(a.g.B, rows_per_img % 128 == 0 ? 1 : 127 / rows_per_img + 2);
    VAE_CHECK((size_t)span * a.g.Hs * a.g.Ws * a.g.Cs * 4u < BUF_MAX && (size_t)std::max(a.K * a.sk, a.N * a.sn) * 4u < BUF_MAX,
              "igemm_rows: operand too large for 32-bit byte offsets");
  }
  VAE_CHECK(s.k != RowsKernel::RowsBf16 || !s.bkm || a.xf == VAE_XF_NONE, "igemm_rows: xf unsupported with n-contiguous weights");
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  const char* what = "igemm_rows";
  switch (s.k) {
    case RowsKernel::UpWino: rc = launch_conv3_upwino(a, a.Wu, st); what = "conv3_upwino"; break;
    case RowsKernel::Wino4: rc = launch_conv3_wino4(a, a.Wu, st); what = "conv3_wino4"; break;
    case RowsKernel::Wino: rc = launch_conv3_wino(a, a.Wu, st); what = "conv3_wino"; break;
    case RowsKernel::WideBf16: rc = launch_conv3_wide_bf16(a, st); what = "conv3_wide_bf16"; break;
    case RowsKernel::TileBf16: rc = launch_conv3_tile_bf16(a, st); what = "conv3_tile_bf16"; break;
    case RowsKernel::Tile: rc = launch_conv3_tile(a, st); what = "conv3_tile"; break;
    case RowsKernel::ThinBf16: rc = launch_conv_thin_bf16(a, st); what = "conv_thin_bf16"; break;
    case RowsKernel::SmallK: rc = launch_conv_smallk(a, st); what = "conv_smallk"; break;
    case RowsKernel::ThinnBf16: rc = launch_conv_thinn_bf16(a, st); what = "conv_thinn_bf16"; break;
    case RowsKernel::SmallN: rc = launch_conv_smalln(a, st); what = "conv_smalln"; break;
    case RowsKernel::Conv1Bf16: rc = launch_conv1_bf16(a, st); what = "conv1_bf16"; break;
    case RowsKernel::RowsBf16: rc = launch_rows_bf16(a, s.bkm, st); what = "igemm_rows_bf16"; break;
    default: rc = launch_rows_f32(a, s.bkm, s.vec, st); break;
  }
  if (rc) return rc;
  VAE_LAUNCH_CHECK(what);
  return VAE_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// C ABI: weight gradients
// ------------------------------------------------------------------------------------------------------------------------
// split-K plan: which nsplit to use for these arguments (a->nsplit is ignored) and whether a->xf can be fused.
// The caller allocates partial[nsplit][M*taps*N] (+ bias_partial[nsplit][M]) accordingly.
extern "C" int vae_wgrad_plan(const vae_wgrad_args* ap, int32_t* nsplit, int32_t* xf_fusable) {
  VAE_CHECK(ap && nsplit && xf_fusable, "wgrad_plan: null argument");
  const WgradSel s = select_wgrad(*ap);
  const vae_wgrad_args& a = s.a;
  // a workgroup keeps the GroupNorm scale/shift rows of every batch item its unit range touches in LDS
  // (SS_HALF entries): the split count is raised until that fits
  auto min_split = [&](int64_t units, int ci_tile) -> int64_t {
    if (a.xf == VAE_XF_NONE) return 1;
    const int64_t upi = units / a.g.B;                         // units per image
    const int64_t nb_max = SS_HALF / ci_tile;                  // batch items whose rows fit
    const int64_t per_max = std::max<int64_t>(1, (nb_max - 1) * upi);
    return (units + per_max - 1) / per_max;
  };
  *xf_fusable = 1;
  switch (s.k) {
    case WgradKernel::ThinBf16: case WgradKernel::SmallK:  // one slab per workgroup, 128-pixel tiles dealt out in ranges
      *nsplit = (int32_t)std::max(1, std::min(1024, wgrad_smallk_tiles(a)));
      return VAE_OK;
    case WgradKernel::DmaBf16: case WgradKernel::TileBf16:
      if (wgrad_use_tile_bf16(a)) {  // (a phase form selects the halo-tile kernels before it is known to be served)
        const int64_t units = wgrad3_tile_bf16_units(a.g);
        const int64_t cols = wgrad3_tile_bf16_columns(a);
        int64_t ns = std::max<int64_t>(1, std::min<int64_t>(256 / std::max<int64_t>(cols, 1), units / 4));
        *nsplit = (int32_t)std::max(ns, min_split(units, 64));
        return VAE_OK;
      }
      [[fallthrough]];
    case WgradKernel::Tile:
      if (wgrad_use_tile(a)) {
        const int64_t units = wgrad3_tile_units(a.g);
        const int64_t wgs = (int64_t)((a.M + 127) / 128) * (a.N / 32);
        int64_t ns = std::max<int64_t>(1, std::min<int64_t>(256 / std::max<int64_t>(wgs, 1), units / 8));  // one 12-wave workgroup per CU
        *nsplit = (int32_t)std::max(ns, min_split(units, 32));
        return VAE_OK;
      }
      [[fallthrough]];
    default: {
      const int64_t tiles = (int64_t)((a.M + 127) / 128) * ((a.N + 127) / 128) * a.g.taps;
      const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(512 / std::max<int64_t>(tiles, 1), a.npix / 256));
      *nsplit = (int32_t)ns;
      *xf_fusable = xf_wgrad_ok(a.g, a.npix, (int)ns, a.N) ? 1 : 0;
      return VAE_OK;
    }
  }
}

extern "C" int vae_wgrad_phase_ok(const vae_wgrad_args* ap) {
  if (!ap || wgrad_smallk_kind(*ap)) return 0;
  if (ap->prec == VAE_PREC_BF16) return (ap->xf == VAE_XF_NONE && wgrad_use_tile_bf16(*ap)) ? 1 : 0;  // the bf16 halo-tile kernel
  return (ap->X16 == nullptr && wgrad_use_tile(*ap)) ? 1 : 0;
}
extern "C" int vae_wgrad_io16_ok(const vae_wgrad_args* ap) { return (ap && wgrad_io16_ok(select_wgrad(*ap))) ? 1 : 0; }

extern "C" int vae_wgrad_kernel_name(const vae_wgrad_args* ap, char* buf, int32_t n) {
  VAE_CHECK(ap && buf && n > 0, "wgrad_kernel_name: bad args");
  wgrad_kernel_name(select_wgrad(*ap), buf, n);
  return VAE_OK;
}

extern "C" int vae_wgrad(const vae_wgrad_args* ap, void* stream) {
  VAE_CHECK(ap != nullptr, "wgrad: null args");
  const WgradSel s = select_wgrad(*ap);
  const vae_wgrad_args& a = s.a;
  VAE_CHECK(wgrad_io16_ok(s), "wgrad: the kernel serving these arguments does not take x_bf16 / y_bf16 as set (vae_wgrad_io16_ok)");
  if (int e = check_geom("wgrad", a.g)) return e;
  VAE_CHECK((a.dY || a.dY16) && a.X, "wgrad: null operand");
  VAE_CHECK(a.dY16 == nullptr || (wgrad_use_tile_bf16(a) && !(a.X16 == nullptr && wgrad_smallk_kind(a)) && aligned16(a.dY16) && a.ldy % 8 == 0 && a.M % 8 == 0),
            "wgrad: dY16 needs bf16 mode and a layer vae_bf16_grad_image_ok accepts");
  VAE_CHECK(a.M > 0 && a.N > 0 && a.npix > 0 && a.nsplit > 0 && a.batch > 0, "wgrad: bad sizes");
  VAE_CHECK(a.N <= a.g.Cs, "wgrad: N exceeds source channels");
  VAE_CHECK((int64_t)a.g.B * a.g.Ho * a.g.Wo == a.npix, "wgrad: npix != B*Ho*Wo");
  VAE_CHECK(a.ldy >= a.M, "wgrad: ldy < M");
  VAE_CHECK(a.g.mode != VAE_MODE_DGRAD && a.g.mode != VAE_MODE_DGRAD_S2, "wgrad: dgrad geometry not valid here");
  VAE_CHECK(a.nsplit == 1 ? a.out != nullptr : a.partial != nullptr, "wgrad: missing output buffer");
  VAE_CHECK(a.xf == VAE_XF_NONE || (a.scale && a.shift), "wgrad: xf needs scale/shift");
  VAE_CHECK(a.bias_partial == nullptr || a.batch == 1, "wgrad: bias_partial is for batch == 1 only");
  VAE_CHECK(a.prec == VAE_PREC_F32 || a.prec == VAE_PREC_BF16, "wgrad: bad prec %d", a.prec);
  const bool flat = s.k == WgradKernel::Bf16 || s.k == WgradKernel::F32;
  if (wgrad_is_phase(a)) {
    VAE_CHECK(vae_wgrad_phase_ok(&a), "wgrad: tapmask / y_step need a halo-tile kernel (vae_wgrad_phase_ok)");
    VAE_CHECK(a.nsplit <= 65535, "wgrad: nsplit too large");
    if (a.prec == VAE_PREC_BF16) {
      VAE_CHECK(a.X16 == nullptr || (aligned16(a.X16) && a.g.Cs % 8 == 0), "wgrad: unaligned X16");
      VAE_CHECK(a.dY16 == nullptr || (aligned16(a.dY16) && a.ldy % 8 == 0 && a.M % 8 == 0), "wgrad: unaligned dY16");
    }
  } else {
    if (s.k != WgradKernel::ThinBf16 && s.k != WgradKernel::SmallK)
      VAE_CHECK(a.X16 == nullptr || (a.xf == VAE_XF_NONE && wgrad_use_tile_bf16(a) && aligned16(a.X16) && a.g.Cs % 8 == 0),
                "wgrad: X16 needs bf16 mode, xf == NONE and a layer vae_bf16_act_image_ok accepts");
    if (!flat) VAE_CHECK(a.nsplit <= 65535, "wgrad: nsplit too large");
  }
  if (flat) {
    VAE_CHECK(a.xf == VAE_XF_NONE || xf_wgrad_ok(a.g, a.npix, a.nsplit, a.N),
              "wgrad: fused GroupNorm needs the split's scale/shift rows to fit LDS (see vae_wgrad_plan)");
    if (s.vec) {  // 32-bit byte offsets inside one split's pixel range
      const int64_t hw = (int64_t)a.g.Ho * a.g.Wo;
      int64_t chunk = (a.npix + a.nsplit - 1) / a.nsplit;
      chunk = (chunk + 31) / 32 * 32;
      const int64_t span = std::min<int64_t>(a.g.B, chunk / hw + 2);
      VAE_CHECK((size_t)chunk * a.ldy * 4u < BUF_MAX && (size_t)span * a.g.Hs * a.g.Ws * a.g.Cs * 4u < BUF_MAX,
                "wgrad: operand too large for 32-bit byte offsets (raise nsplit)");
    }
  }
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  const char* what = "wgrad";
  switch (s.k) {
    case WgradKernel::DmaBf16: rc = launch_wgrad3_dma_bf16(a, st); what = "wgrad3_dma_bf16"; break;
    case WgradKernel::TileBf16: rc = launch_wgrad3_tile_bf16(a, st); what = "wgrad3_tile_bf16"; break;
    case WgradKernel::Tile: rc = launch_wgrad3_tile(a, st); what = "wgrad3_tile"; break;
    case WgradKernel::ThinBf16: rc = launch_wgrad_thin(a, st); what = "wgrad_thin_bf16"; break;
    case WgradKernel::SmallK: rc = launch_wgrad_smallk(a, st); what = "wgrad_smallk"; break;
    case WgradKernel::Bf16: rc = launch_wgrad_bf16(a, st); what = "wgrad_bf16"; break;
    default: rc = launch_wgrad_f32(a, s.vec, st); break;
  }
  if (rc) return rc;
  VAE_LAUNCH_CHECK(what);
  return VAE_OK;
}

// Winograd weight gradient (wgrad3_wino.hip: 16 positions; wgrad3_upwino.hip: the upsampler convolution, 9 positions): plan
// (nsplit = 0: not served), launch into the transform-domain slab [nsplit][positions][Cin][Cout] (a->partial; a->bias_partial
// optional); vae_wgrad_wino_reduce (igemm.hip) reduces it and applies the output transform into OHWI
extern "C" int vae_wgrad_wino_plan(const vae_wgrad_args* ap, int32_t* nsplit) {
  VAE_CHECK(ap && nsplit, "wgrad_wino_plan: null argument");
  *nsplit = 0;
  if (vae_opt().flat_conv || vae_opt().no_wino) return VAE_OK;
  const bool up = wgrad3_upwino_eligible(*ap);
  if (!up && !wgrad3_wino_eligible(*ap)) return VAE_OK;
  const int64_t units = up ? wgrad3_upwino_units(ap->g) : wgrad3_wino_units(ap->g);
  const int64_t wgs = (int64_t)(ap->M / 128) * (ap->N / 32);
  *nsplit = (int32_t)std::max<int64_t>(1, std::min<int64_t>(256 / std::max<int64_t>(wgs, 1), units / 8));  // one 8-wave workgroup per CU
  return VAE_OK;
}
extern "C" int vae_wgrad_wino_positions(const vae_wgrad_args* ap) { return (ap && wgrad3_upwino_eligible(*ap)) ? 9 : 16; }
extern "C" int vae_wgrad_wino(const vae_wgrad_args* ap, void* stream) {
  VAE_CHECK(ap != nullptr, "wgrad_wino: null args");
  const vae_wgrad_args& a = *ap;
  if (int e = check_geom("wgrad_wino", a.g)) return e;
  VAE_CHECK(a.dY && a.X && a.partial, "wgrad_wino: null operand");
  VAE_CHECK(a.nsplit > 0 && a.nsplit <= 65535, "wgrad_wino: bad nsplit");
  VAE_CHECK((int64_t)a.g.B * a.g.Ho * a.g.Wo == a.npix && a.N <= a.g.Cs && a.ldy >= a.M, "wgrad_wino: inconsistent sizes");
  const bool up = wgrad3_upwino_eligible(a);
  if (!up) {
    VAE_CHECK(wgrad3_wino_eligible(a), "wgrad_wino: the layer is not served by the Winograd kernel (vae_wgrad_wino_plan)");
    VAE_CHECK(a.xf == VAE_XF_NONE || (a.scale && a.shift), "wgrad_wino: xf needs scale/shift");
  }
  if (int rc = (up ? launch_wgrad3_upwino : launch_wgrad3_wino)(a, (hipStream_t)stream)) return rc;
  VAE_LAUNCH_CHECK(up ? "wgrad3_upwino" : "wgrad3_wino");
  return VAE_OK;
}
