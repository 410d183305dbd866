// gg_f8g128.hip — the two builds of gg_v2_kernel that carry the w8a8_g128_sym_E4M3 tile body (gg_tile_f8g128,
// gg_device.h): the exact v2x build for calls of the type alone and the widest fallback (every tile body) for any
// mix holding it. A unit of its own: it compiles beside gg_api.hip instead of lengthening it, and with packed f32
// arithmetic off (build.py: the fold's scalar fmas stay scalar whatever the optimiser would prefer).
// No V2_TRACE build here: this unit's copy of the trace buffer is unused and dropped (MXMOE_GG_UNIT2).
#define MXMOE_GG_UNIT2
#include "gg_builds.h"

namespace mxmoe {
#ifndef MXMOE_LAB  // (the lab library plans no problem of the type)
void launch_v2x_f8g(const GGArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((gg_v2_kernel<kV2xProduct, kF8G>), dim3(grid), dim3(512), 0, s, a);
}
void launch_v2_widest(const GGArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((gg_v2_kernel<0, kV2Widest>), dim3(grid), dim3(512), 0, s, a);
}
#endif
}  // namespace mxmoe
