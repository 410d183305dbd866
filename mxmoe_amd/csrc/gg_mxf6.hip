// gg_mxf6.hip — the exact v2x build for calls of w6a6_g32_sym_MXFP6 problems alone, gg_v2_kernel<kV2xProduct, kMx6>
// (tile body gg_tile_mxf6, gg_mxf6.h). A unit of its own, as gg_f8g128.hip: it compiles beside gg_api.hip and leaves
// every other kernel's text as it was. A mix holding the type runs the widest fallback (gg_f8g128.hip).
// No V2_TRACE build here: this unit's copy of the trace buffer is unused and dropped (MXMOE_GG_UNIT2).
#define MXMOE_GG_UNIT2
#include "gg_builds.h"

namespace mxmoe {
#ifndef MXMOE_LAB  // (the lab library plans no problem of the type)
void launch_v2x_mxf6(const GGArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((gg_v2_kernel<kV2xProduct, kMx6>), dim3(grid), dim3(512), 0, s, a);
}
#endif
}  // namespace mxmoe
