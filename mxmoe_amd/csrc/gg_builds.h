// gg_builds.h — what the library's kernel translation units share: the product variant's mainloop flags, and the
// launchers of the kernels compiled outside gg_api.hip (gg_f8g128.hip, gg_f8g128_small.hip: the builds with the
// w8a8_g128_sym_E4M3 bodies; gg_mxf6.hip: the exact w6a6_g32_sym_MXFP6 build).
#pragma once

#include <hip/hip_runtime.h>

#include "gg_device.h"

namespace mxmoe {

// the round-3 AUTO default's mainloop flags (variant v2x_256x256_w8_b3_buf_spread_edma, without the
// weight-only options)
constexpr int kV2x = V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | (4 << V2_SPREAD_SHIFT);
[[maybe_unused]] constexpr int kV2xProduct = kV2x | WO_PIPE | WO_STAG | V2_I4NOPAIR | V2_I4EDMA;

// the small-batch kernel's loop options (gg_tile_wo) and its product variant's (wo3_64x256_w8_3wg)
constexpr int kWo3 = WO_SCLATE | WO_ANDOR | WO_MSKIP | WO_SPLIT | WO_NIBPOS;
[[maybe_unused]] constexpr int kWo3Product = kWo3 | WO_PCH;

[[maybe_unused]] constexpr int kMx4 = 1 << QT_MXF4;   // w4a4_g32_sym_MXFP4
[[maybe_unused]] constexpr int kMxW = 1 << QT_MXF4W;  // weight-only MXFP4
[[maybe_unused]] constexpr int kMx8 = 1 << QT_MXF8A;  // w4a8_g32_sym_MXFP8 (gg_tile_v2's 64 x 128 body)
[[maybe_unused]] constexpr int kF8G = 1 << QT_F8G;    // w8a8_g128_sym_E4M3 (gg_tile_f8g128; wo3 alone: gg_tile_f8g128s)
[[maybe_unused]] constexpr int kMx6 = 1 << QT_MXF6;   // w6a6_g32_sym_MXFP6 (gg_tile_mxf6, gg_mxf6.h)
constexpr int kV2Widest = 511 | kMx4 | kMxW | kMx8 | kF8G | kMx6;  // every tile body of gg_v2_kernel

#pragma GCC visibility push(hidden)
// gg_f8g128.hip (product library): gg_v2_kernel<kV2xProduct, kF8G> and gg_v2_kernel<0, kV2Widest>
void launch_v2x_f8g(const GGArgs& a, int grid, hipStream_t s);
void launch_v2_widest(const GGArgs& a, int grid, hipStream_t s);
// gg_f8g128_small.hip (product library): gg_wo2_kernel<kWo3Product, kF8G, 3>
void launch_wo3_f8g(const GGArgs& a, int grid, hipStream_t s);
// gg_mxf6.hip (product library): gg_v2_kernel<kV2xProduct, kMx6>
void launch_v2x_mxf6(const GGArgs& a, int grid, hipStream_t s);
#pragma GCC visibility pop

}  // namespace mxmoe
