// Host entry points of the contraction kernels (one .hip file each), for the dispatcher (dispatch.cpp).  A *_eligible
// function answers only "can this kernel serve these arguments"; which kernel serves them is decided in dispatch.cpp.
// Every launcher expects arguments dispatch.cpp has validated and returns 0 or a VAE_E* code.
#pragma once
#include "common_host.h"

// igemm.hip: the flat implicit-GEMM kernels (any geometry) under the fp32 policy and under the bf16-compute policy
// (vectorised shapes only), and the split reduction
int launch_rows_f32(const vae_igemm_args& a, bool bkm, bool vec, hipStream_t st);
int launch_wgrad_f32(const vae_wgrad_args& a, bool vec, hipStream_t st);
int launch_rows_bf16(const vae_igemm_args& a, bool bkm, hipStream_t st);
int launch_wgrad_bf16(const vae_wgrad_args& a, hipStream_t st);

// conv3_tile.hip / conv3_tile_bf16.hip: 3x3 stride-1 halo tiles (fp32 / bf16; the two share the tile shape and epilogue layout)
bool conv3_tile_eligible(const vae_igemm_args& a, bool vec, bool bkm);
int conv3_tile_gstat_chunks(const vae_igemm_args& a);
int launch_conv3_tile(const vae_igemm_args& a, hipStream_t st);
bool conv3_tile_bf16_packed(const vae_igemm_args& a);  // the bf16 image of the weights the bf16 kernel reads
int conv3_tile_bf16_gstat_chunks(const vae_igemm_args& a);
int launch_conv3_tile_bf16(const vae_igemm_args& a, hipStream_t st);
// conv3_wide_bf16.hip: both operands bf16 images, 8 x 32-pixel tiles
bool conv3_wide_bf16_eligible(const vae_igemm_args& a);
int conv3_wide_bf16_gstat_chunks(const vae_igemm_args& a);
int launch_conv3_wide_bf16(const vae_igemm_args& a, hipStream_t st);
// conv3_wino.hip / conv3_wino4.hip / conv3_upwino.hip: fp32 Winograd F(2x2,3x3), F(4x4,3x3), the upsampler's 9 positions
bool conv3_wino_eligible(const vae_igemm_args& a);
// channel blocks (of 32) per F(2x2) workgroup: 2 = 64 channels, 128 VGPRs per wave, TWO workgroups per CU (the template also
// instantiates with 4 = 128 channels, one workgroup per CU: measured 4-10 % slower in round 2 and no longer built)
constexpr int CONV3_WINO_NB = 2;
int conv3_wino_gstat_chunks(const vae_igemm_args& a);
int conv3_wino_gnb_chunks(const vae_igemm_args& a);
int launch_wino_weights(const vae_igemm_args& a, float* U, hipStream_t st);
int launch_conv3_wino(const vae_igemm_args& a, const float* U, hipStream_t st);
bool conv3_wino4_eligible(const vae_igemm_args& a);
int conv3_wino4_gstat_chunks(const vae_igemm_args& a);
int conv3_wino4_gnb_chunks(const vae_igemm_args& a);
int launch_wino4_weights(const vae_igemm_args& a, float* U, hipStream_t st);
int launch_conv3_wino4(const vae_igemm_args& a, const float* U, hipStream_t st);
bool conv3_upwino_eligible(const vae_igemm_args& a);
int64_t conv3_upwino_weight_bytes(const vae_igemm_args& a);  // of its U image: fp32, or three bf16 planes (VAE_UPW_X3)
int launch_upwino_weights(const vae_igemm_args& a, float* U, hipStream_t st);
int launch_conv3_upwino(const vae_igemm_args& a, const float* U, hipStream_t st);
// conv1_bf16.hip: bf16 1x1 convolutions, weights resident in LDS
bool conv1_bf16_eligible(const vae_igemm_args& a);
int launch_conv1_bf16(const vae_igemm_args& a, hipStream_t st);
// skinny.hip (<= 4-channel sides on the VALU) and conv_thin_bf16.hip / wgrad_thin_bf16.hip (the same launches on the matrix pipe)
bool conv_smallk_eligible(const vae_igemm_args& a);
int launch_conv_smallk(const vae_igemm_args& a, hipStream_t st);
bool conv_smalln_eligible(const vae_igemm_args& a);
int launch_conv_smalln(const vae_igemm_args& a, hipStream_t st);
bool conv_thin_bf16_eligible(const vae_igemm_args& a);
int launch_conv_thin_bf16(const vae_igemm_args& a, hipStream_t st);
bool conv_thinn_bf16_eligible(const vae_igemm_args& a);
int launch_conv_thinn_bf16(const vae_igemm_args& a, hipStream_t st);
int wgrad_smallk_kind(const vae_wgrad_args& a);  // 0 = not served, 1 = the narrow side is X (N <= 4), 2 = it is dY (M <= 4)
int wgrad_smallk_tiles(const vae_wgrad_args& a);
int launch_wgrad_smallk(const vae_wgrad_args& a, hipStream_t st);
bool wgrad_thin_bf16_eligible(const vae_wgrad_args& a, int kind);
int launch_wgrad_thin(const vae_wgrad_args& a, hipStream_t st);

// wgrad3_tile.hip / wgrad3_tile_bf16.hip: 3x3 weight gradients on halo tiles; the bf16 file also holds the LDS-DMA kernel
bool wgrad3_tile_eligible(const vae_wgrad_args& a, bool vec);
int64_t wgrad3_tile_units(const vae_conv_geom& g);
int launch_wgrad3_tile(const vae_wgrad_args& a, hipStream_t st);
bool wgrad3_dma_bf16_operands(const vae_wgrad_args& a);          // the LDS-DMA kernel can stage these operands
bool wgrad3_tile_bf16_eligible(const vae_wgrad_args& a, bool vec, bool dma);  // dma: the LDS-DMA kernel serves (stride 2 exists only there)
int64_t wgrad3_tile_bf16_units(const vae_conv_geom& g);
int wgrad3_tile_bf16_columns(const vae_wgrad_args& a);
int launch_wgrad3_tile_bf16(const vae_wgrad_args& a, hipStream_t st);
int launch_wgrad3_dma_bf16(const vae_wgrad_args& a, hipStream_t st);
// wgrad3_wino.hip / wgrad3_upwino.hip: fp32 Winograd weight gradients (16 / 9 positions); their slabs are reduced by
// vae_wgrad_wino_reduce (igemm.hip)
bool wgrad3_wino_eligible(const vae_wgrad_args& a);
int64_t wgrad3_wino_units(const vae_conv_geom& g);
int launch_wgrad3_wino(const vae_wgrad_args& a, hipStream_t st);
bool wgrad3_upwino_eligible(const vae_wgrad_args& a);
int64_t wgrad3_upwino_units(const vae_conv_geom& g);
int launch_wgrad3_upwino(const vae_wgrad_args& a, hipStream_t st);
