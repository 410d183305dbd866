// gg_f8g128_small.hip — the small-batch kernel's build for calls of w8a8_g128_sym_E4M3 problems alone:
// gg_wo2_kernel<kWo3Product, kF8G, 3>, the 64 x 128 tile body gg_tile_f8g128s (gg_device.h) at three workgroups per
// CU. A unit of its own (gg_f8g128.hip holds exactly the two gg_v2_kernel builds of the type), compiled like that one
// with packed f32 arithmetic off (build.py): the fold's scalar fmas stay scalar.
#define MXMOE_GG_UNIT2
#include "gg_builds.h"

namespace mxmoe {
#ifndef MXMOE_LAB  // (the lab library plans no problem of the type)
void launch_wo3_f8g(const GGArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((gg_wo2_kernel<kWo3Product, kF8G, 3>), dim3(grid), dim3(512), 0, s, a);
}
#endif
}  // namespace mxmoe
