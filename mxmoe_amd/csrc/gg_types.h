// gg_types.h — the plain data the host planner (gg_plan.cpp) writes and the kernels (gg_device.h) read: the
// quant-type codes, one row of the plan table, one output tile, the kernel arguments. No HIP type in it: it
// compiles with a host compiler alone.
#pragma once

#include <stdint.h>

namespace mxmoe {

// QT_I4G: w4a4_g128_sym (A and B int4 with one fp16 scale per 128-K group)
// QT_F8: w8a8_g-1_sym_E4M3 (A and B OCP fp8 e4m3, per-channel fp16 scales, f32 accumulate)
// QT_BF16: bf16 A and B, f32 accumulate, fp16 C
// QT_I4F6: w4a4_g-1_sym with A and B given as fp6 e3m2 images of the int4 codes (gg_f6.h): the
//          block-scaled fp6 MFMA, f32 accumulate (exact: integer partial sums below 2^24)
// QT_MXF4: w4a4_g32_sym_MXFP4 (A and B OCP MXFP4: e2m1 codes, one e8m0 scale per 32-K block; the
//          block-scaled fp4 MFMA applies the scales, f32 accumulate, C = fp16_rn(acc))
// QT_MXF4W: w4a16_g32_sym_MXFP4 (fp16 A, B as QT_MXF4's B: weight-only, gg_tile_wo's WO_FMT_MX body)
// QT_MXF8A: w4a8_g32_sym_MXFP8 (A OCP MXFP8: e4m3 codes + e8m0 block scales, B as QT_MXF4's B; the
//           block-scaled MFMA with one format per operand, f32 accumulate, C = fp16_rn(acc))
enum QType : int32_t {
  QT_F16 = 0, QT_I8 = 1, QT_I4 = 2, QT_W4A16 = 3, QT_W8A16 = 4, QT_I4G = 5, QT_W2A16 = 6, QT_F8 = 7, QT_BF16 = 8,
  QT_I4F6 = 9, QT_MXF4 = 10, QT_MXF4W = 11, QT_MXF8A = 12,
  QT_COUNT = 13
};
// quant types whose epilogue applies the per-channel scales sa[m] * sb[n]
constexpr bool qt_scaled(int qt) { return qt == QT_I8 || qt == QT_I4 || qt == QT_F8 || qt == QT_I4F6; }

// One row of the plan table (64 B), written by the host planner into the workspace.
struct GGMeta {
  int32_t M, N, K, qtype;
  int32_t tiles_n;     // cdiv(N, BN of this qtype)
  int32_t tile_begin;  // first global tile id of this problem
  int32_t kbytes;      // bytes of one K row (K * bits / 8; weight-only: of the fp16 A row)
  int32_t reserved;    // weight-only: 64-K stages per scale group
  int64_t lda_b, ldb_b;  // row strides of A / B in bytes
  int64_t ldc;           // row stride of C in fp16 elements
  int64_t reserved2;     // weight-only: 1 = sym codes; fp16 / w8a8 / w4a4: META_SILU
};
// GGMeta::reserved2 bit of a problem whose epilogue writes act = silu(gate) * up (MXMOE_GG_EPI_SILU_MUL):
// B rows interleaved in 16-row blocks (gate block b at rows 32 b, up block b at 32 b + 16), C has
// N / 2 columns
constexpr int64_t META_SILU = 2;
static_assert(sizeof(GGMeta) == 64, "GGMeta must stay 64 bytes");

// One output tile (32 B), host-built in dispatch order: tile b is run by workgroup b.
struct TileDesc {
  int32_t prob;  // row of the plan table; -1 = empty slot (padding of the XCD interleave)
  int32_t m0;    // first output row
  int32_t n0;    // first output column
  int32_t cls;   // bits 0-7 tile-height class; split-K: bits 8-15 slice index, bits 16-23 slices
  int32_t ks0, ks1;  // K stages [ks0, ks1) of this tile (all of K unless split)
  int32_t slab;      // split-K: first partial slab of the tile's slices, else -1
  int32_t grp;       // split-K: arrival counter of the tile, else -1
};
static_assert(sizeof(TileDesc) == 32, "TileDesc must stay 32 bytes");
constexpr TileDesc kEmptySlot = {-1, 0, 0, 0, 0, 0, -1, -1};

constexpr int SPLITK_SLAB_BYTES = 256 * 256 * 4;  // one 256 x 256 tile of 32-bit accumulators

struct GGArgs {
  const GGMeta* meta;
  const TileDesc* tiles;
  const void* const* ptr_A;
  const void* const* ptr_B;
  const void* const* ptr_SA;
  const void* const* ptr_SB;
  void* const* ptr_C;
  int32_t P;
  int32_t n_slots;  // gridDim.x
  uint8_t* slabs;     // split-K partial slabs (SPLITK_SLAB_BYTES each)
  int32_t* counters;  // split-K arrival counters (zero between launches)
};

}  // namespace mxmoe
