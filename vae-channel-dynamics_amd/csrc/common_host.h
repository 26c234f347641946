// Host-side declarations shared by every translation unit of libvaehip (no device code).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>
#include <hip/hip_runtime_api.h>
#include "../../include/vaehip.h"

void vae_set_error(const char* fmt, ...);

#define VAE_CHECK(cond, ...)                 \
  do {                                       \
    if (!(cond)) {                           \
      vae_set_error(__VA_ARGS__);            \
      return VAE_EINVAL;                     \
    }                                        \
  } while (0)

#define VAE_LAUNCH_CHECK(name)                                                 \
  do {                                                                         \
    hipError_t e_ = hipGetLastError();                                         \
    if (e_ != hipSuccess) {                                                    \
      vae_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));     \
      return VAE_ELAUNCH;                                                      \
    }                                                                          \
  } while (0)

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

template <int V>
using int_c = std::integral_constant<int, V>;
// THE xf switch: launch(int_c<xf>) for a valid xf, false for any other value
template <class Launch>
bool dispatch_xf(int xf, Launch launch) {
  switch (xf) {
    case VAE_XF_NONE: launch(int_c<VAE_XF_NONE>{}); return true;
    case VAE_XF_AFFINE: launch(int_c<VAE_XF_AFFINE>{}); return true;
    case VAE_XF_AFFINE_SILU: launch(int_c<VAE_XF_AFFINE_SILU>{}); return true;
    default: return false;
  }
}
// The kernel files behind dispatch.cpp (which checks the operands of a transform, not the value of xf) have always run any
// other value as AFFINE_SILU: their launchers keep that.
template <class Launch>
void dispatch_xf_or_silu(int xf, Launch launch) {
  if (!dispatch_xf(xf, launch)) launch(int_c<VAE_XF_AFFINE_SILU>{});
}

constexpr int SS_HALF = 512;             // floats of GroupNorm scale (and of shift) kept in LDS per workgroup
constexpr size_t BUF_MAX = 0xFFFFFFF0u;  // bytes one buffer descriptor can cover

// process-wide kernel-selection switches (error.cpp): VAEHIP_FLAT_CONV / VAEHIP_NO_WINO / VAEHIP_NO_WIDE are read once at
// load time; vae_set_option changes them afterwards (tests compare two algorithms that way)
struct vae_options {
  int flat_conv;  // flat implicit-GEMM kernels everywhere (the second algorithm of the two-algorithm tests)
  int no_wino;    // fp32: direct halo-tile kernels instead of the Winograd ones (the parity reference)
  int no_wino4;   // fp32: Winograd F(2x2,3x3) also where F(4x4,3x3) would serve the layer (A/B switch, second Winograd algorithm of the tests)
  int no_thin_mfma;  // bf16: the <= 4-channel-side layers on the VALU kernels (skinny.hip) also where the matrix-pipe kernels would serve them
  int no_wide;    // bf16: the 128-pixel halo-tile kernel instead of the wide-tile one
  int no_wgrad_dma;  // bf16: the 3x3 weight gradient stages its bf16 images through registers (A/B switch for the LDS-DMA kernel)
  // bf16, data parallel: the persistent wide-tile kernel launches (256 - n) workgroups instead of one per CU, leaving n CUs
  // to RCCL's workgroups while gradient buckets are in flight (0 = all 256; a count 0..128, not a switch)
  int wide_reserved_cus;
};
const vae_options& vae_opt();

// Kernels with more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize set once per kernel AND device
// (one bit per device ordinal; a local static per call site, i.e. per template instantiation).  Returns VAE_ELAUNCH from the caller.
#define VAE_RESERVE_LDS(kern, bytes, what)                                                                                  \
  do {                                                                                                                      \
    static unsigned long long done_ = 0;                                                                                    \
    int dev_ = 0;                                                                                                           \
    (void)hipGetDevice(&dev_);                                                                                              \
    if (!((done_ >> (dev_ & 63)) & 1ull)) {                                                                                 \
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)) != hipSuccess) { \
        vae_set_error("%s: cannot reserve %d bytes of LDS", what, (int)(bytes));                                            \
        return VAE_ELAUNCH;                                                                                                 \
      }                                                                                                                     \
      done_ |= 1ull << (dev_ & 63);                                                                                         \
    }                                                                                                                       \
  } while (0)
