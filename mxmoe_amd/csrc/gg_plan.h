// gg_plan.h — the host tile planner of libmxmoe_gg.so (gg_plan.cpp): what the ABI layer (gg_api.hip) and a
// stand-alone host program (tests/cpp/plan_host_check.cpp) need of it. Plain host C++: no HIP header, no kernel
// text. The planner sees a kernel variant as a PlanVariant — tile geometry, classes, chunk size — and gets the
// library's list of them once (set_plan_variants); the compiled kernels behind a variant stay with the ABI layer.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/mxmoe_gg.h"
#include "gg_dyn.h"
#include "gg_types.h"

namespace mxmoe {
#pragma GCC visibility push(hidden)  // (internal to the library: not among its exported symbols)

struct TileGeom {
  int bm, bn, bkb, threads;
};

// AUTO policy: v2x (the staggered 256x256 v2 on v2s3's LDS image with the buffer-form, spread
// LDS-DMA) for every call with fp16 / bf16 / w8a8 / E4M3 / weight-only problems: same-run A/B on the
// qwen2_moe layer-11 calls, +5-11 % over v2s and +3-9 % over v2s3 at every K (the round-1/2 short-K
// rule between those two is gone: profiles/r03/lab/). int4-only sets run 256x128 tiles, 2 WG/CU
// (v3), unless they are low-fill enough to need split-K (v2 kernels only).
constexpr const char* kDefaultVariantName = "v2x_256x256_w8_b3_buf_spread_edma";
constexpr const char* kInt4Variant = "v3_256x128_w4_dma_ring3_2wg";
constexpr const char* kWoSmallVariant = "wo3_64x256_w8_3wg";
constexpr const char* kF6Variant = "f6_256x256_w8_ring3";  // (lab library)
// weight-only calls whose rows per weight byte are this small or smaller run kWoSmallVariant:
// the weight-bytes-weighted mean M over the call's problems (qwen2_moe layer 11: ~60 at bs = 128,
// ~250 at bs = 2048, ~1030 at bs = 8192, where v2x's 256-row tiles are as fast or faster)
constexpr double kWoSmallMeanRows = 512.0;
// calls of fp16 / w8a8 / w4a4 problems only (no weight-only one) take wo3 below a mean M of
// kSmallMeanRows (kSmallMeanRowsI4 with int4 problems), twice that when the call is K-skewed (its
// longest K >= 2x the weighted mean K: the qwen2_moe down call, whose shared expert has 4x the
// routed K — few long tiles the general kernels balance poorly). Measured on qwen2_moe layer 11
// (mean M ~ bs / 8; profiles/r03/wo2/wo3_fp16_w8a8.jsonl, wo3_w4a4_mixed.jsonl, wo3_mid.jsonl):
// gate_up wins to bs 512 (fp16 -3.5 .. w4a4 +33 %) and 768 with int4, down calls to bs 1024 (fp16)
// / 1536 (int4), the general kernels beyond.
constexpr double kSmallMeanRows = 80.0;
constexpr double kSmallMeanRowsI4 = 112.0;
// calls with a w4a8_g32_sym_MXFP8 problem (and no weight-only one): the int4 cut
constexpr double kSmallMeanRowsMx8 = 112.0;
constexpr double kSplitCUs = 256.0;  // MI355X compute units: the planner's notion of "one CU's share"

// What AUTO does with a call that has a problem of the type (resolve_variant):
//   General    v2x;
//   WeightOnly the small-batch kernel (kWoSmallVariant) up to a mean M of auto_rows, v2x beyond;
//   Small      may ride on the small-batch kernel: a call of Small types only takes it up to the
//              largest auto_rows among them (x 2 when K-skewed), beside a weight-only problem up to that one's;
//   Alone      cannot share a call: a kernel of its own (auto_alone).
enum class AutoClass { General, WeightOnly, Small, Alone };

// Everything the host knows about a quant type, one row per QType.
struct QTypeInfo {
  int qt;                    // the row's QType
  const char* name;          // mxmoe_gg_list_variants (weight-only: every group size / sym of a bit width under the base name)
  int staged_bits;           // bits per K element of a staged row (the listing's BK = bkb * 8 / staged_bits)
  bool weight_only;          // fp16 A on quantised B (gg_tile_wo; validated by build_meta_weightonly)
  bool float16;              // 16-bit operands, no scales
  const char* dword_scales;  // block scales the kernel reads as dwords (4-byte aligned): what the error calls them
  int k_mult;                // K granularity of its own, beyond 16-byte rows (0 = none), what the error calls the type,
  const char* k_what;        // and whether the rule is checked before the row rule
  bool k_first;
  bool group_fold;           // k_mult-element scale groups folded in f32: GGMeta::reserved counts them, and the
                             // type never splits K (summing f32 partial folds would change the rounding)
  bool int32_bound;          // exact int32 accumulation: K <= 131072
  bool silu;                 // its tile body carries the fused SiLU epilogue (weight-only: Variant::silu_wo kernels)
  bool small_class;          // takes the 64-row class (Variant::tail2_bm)
  // cost model (full_tile_cost, stage_time)
  double passes;             // MFMA passes per staged byte: int4 2; g128 adds the per-group f32 fold (~25 %); fp6 images: one
                             // fp6 MFMA (the int8 one's cycles) per 96 B of K-128; MXFP4: the int8 tile's count and cycles, so 1
  int el_bits;               // K elements per stage = bkb * 8 / el_bits (0: 128, the fp6 images' K-128 blocks)
  double rate;               // MFMA flop per LDS byte-time, fp16 = 128
  double fold;               // per-group f32 fold on top of the MFMAs
  int code_bits;             // weight-only: bits per staged B code (MXFP4: its 2 scale bytes per column are 1/16 of the codes)
  AutoClass auto_class;
  double auto_rows;          // WeightOnly / Small: the mean-M limit of the small-batch kernel
  const char* auto_alone;    // the variant AUTO takes for a call of this type only (Small: unless it splits K)
  bool auto_counts_empty;    // an empty problem still counts for AUTO (only v2x plans the type; types are checked before shapes)
};
constexpr AutoClass kGen = AutoClass::General, kWo = AutoClass::WeightOnly, kSm = AutoClass::Small;
constexpr QTypeInfo kQTypes[] = {
    // qt, name, bits | wo, f16 | dword scales | K rule | fold, i32, silu, 64-row | passes, el, rate, fold, code | AUTO
    {QT_F16, "fp16", 16, false, true, nullptr, 0, nullptr, false, false, false, true, true,
     1.0, 16, 128, 1.0, 0, kSm, kSmallMeanRows, nullptr, false},
    {QT_I8, "w8a8_g-1_sym", 8, false, false, nullptr, 0, nullptr, false, false, true, true, false,
     1.0, 8, 256, 1.0, 0, kSm, kSmallMeanRows, nullptr, false},
    {QT_I4, "w4a4_g-1_sym", 4, false, false, nullptr, 0, nullptr, false, false, true, true, false,
     2.0, 4, 256, 1.0, 0, kSm, kSmallMeanRowsI4, kInt4Variant, false},
    {QT_W4A16, "w4a16", 4, true, false, nullptr, 0, nullptr, false, false, false, true, true,
     1.0, 0, 0, 1.0, 4, kWo, kWoSmallMeanRows, nullptr, false},
    {QT_W8A16, "w8a16", 8, true, false, nullptr, 0, nullptr, false, false, false, true, true,
     1.0, 0, 0, 1.0, 8, kWo, kWoSmallMeanRows, nullptr, false},
    {QT_I4G, "w4a4_g128_sym", 4, false, false, nullptr, 128, "w4a4_g128", false, true, true, false, false,
     2.5, 4, 256, 1.25, 0, kGen, 0, nullptr, false},
    {QT_W2A16, "w2a16", 2, true, false, nullptr, 0, nullptr, false, false, false, true, true,
     1.0, 0, 0, 1.0, 2, kWo, kWoSmallMeanRows, nullptr, false},
    {QT_F8, "w8a8_g-1_sym_E4M3", 8, false, false, nullptr, 0, nullptr, false, false, false, false, false,
     1.0, 8, 256, 1.0, 0, kGen, 0, nullptr, false},
    {QT_BF16, "bf16", 16, false, true, nullptr, 0, nullptr, false, false, false, false, true,
     1.0, 16, 128, 1.0, 0, kGen, 0, nullptr, false},
    {QT_I4F6, "w4a4_g-1_sym_F6", 6, false, false, nullptr, 0, nullptr, false, false, true, false, false,
     128.0 / 96 / 2, 0, 512, 1.0, 0, AutoClass::Alone, 0, kF6Variant, false},
    {QT_MXF4, "w4a4_g32_sym_MXFP4", 4, false, false, "MXFP4", 0, nullptr, false, false, false, false, false,
     1.0, 4, 512, 1.0, 0, kGen, 0, nullptr, true},
    {QT_MXF4W, "w4a16_g32_sym_MXFP4", 4, true, false, "MXFP4", 0, nullptr, false, false, false, true, true,
     1.0, 0, 0, 1.0, 4, kWo, kWoSmallMeanRows, nullptr, false},
    {QT_MXF8A, "w4a8_g32_sym_MXFP8", 8, false, false, "w4a8_g32_sym_MXFP8", 32, "w4a8_g32_sym_MXFP8", true, false,
     false, true, false, 1.0, 8, 256, 1.0, 0, kSm, kSmallMeanRowsMx8, nullptr, false},
};
constexpr bool qtypes_in_order() {
  for (int i = 0; i < QT_COUNT; ++i)
    if (kQTypes[i].qt != i) return false;
  return true;
}
static_assert(sizeof(kQTypes) / sizeof(kQTypes[0]) == QT_COUNT, "one row per QType");
static_assert(qtypes_in_order(), "row i describes QType i");
constexpr const QTypeInfo& qinfo(int qt) { return kQTypes[qt]; }
constexpr int auto_mask(AutoClass c) {  // 1 << QType of the class's types
  int m = 0;
  for (const QTypeInfo& t : kQTypes)
    if (t.auto_class == c) m |= 1 << t.qt;
  return m;
}

enum class Kind { V0, V2, V3 };  // (the fp6 kernel is planned as V3: no split-K, no XCD regions)

// What the planner knows of a kernel variant (the launch half, its compiled builds: gg_api.hip's Variant).
struct PlanVariant {
  const char* name;
  Kind kind;
  TileGeom geom[QT_COUNT] = {};  // indexed by QType (main tile); bn == 0: no tile body for the type. Every
                                 // plan_* / make_* sets the types its kernel has one for
  int threads;
  int lds_bytes;       // the family's LDS image (a build's own: Build::lds_bytes)
  int chunk;           // tiles per XCD chunk (workgroups that run together on one XCD)
  int k_stage_bytes = 0;  // K bytes per row must be a multiple of this (0 = any multiple of 16; v2: K tails are
                          // handled in-kernel, fp6 image rows are whole stages by construction)
  int tail_bm = 0;     // v2: height of the tail-tile class (0 = none)
  int tail2_bm = 0;    // v2: height of the small-remainder class (0 = none)
  bool persistent = false;  // v2p / v2q: a workgroup walks a planned tile list
  bool silu_epi = false;    // the fp16 / w8a8 / w4a4 tile bodies carry the fused SiLU epilogue
  bool silu_wo = false;     // ... and its weight-only tiles (wo2: the WO_SILU builds)
  int persist_len = 0;      // v2q: 0 = one list per CU (static); L > 0 = lists of L consecutive XCD-queue
                            // tiles, one per block, the hardware dispatching blocks as CUs free up
  int (*pick)(int qmask);   // index among the variant's builds of the one a plan's quant-type set (1 << QType
                            // present, kQmaskWoSilu) launches: the launch and the plan info's LDS size both use it
};
// plan-info qtype_mask bit: a weight-only problem carries MXMOE_GG_EPI_SILU_MUL (selects the WO_SILU
// builds of wo2)
constexpr int kQmaskWoSilu = 1 << 16;

// the fused SiLU epilogue (MXMOE_GG_EPI_SILU_MUL) lives in the fp16 / w8a8 / w4a4 tile bodies of the
// v2 / v3 kernels (gg_tile_v2, epilogue_v3) — the small-batch wo3 kernel's 64 x 128 bodies of those
// types included (round 6); the persistent, v4d and fp6 lab kernels have none (mxmoe_gg_variant_caps
// reports it). Weight-only problems may carry the flag on wo3 only (Variant::silu_wo, build_meta).
inline bool has_silu_epilogue(const PlanVariant& v) { return v.silu_epi && !v.persistent; }

// ---- The plan parameters of the kernel families. gg_api.hip's make_* call these, then attach the name, the LDS
// image and the compiled builds; where a number here has a kernel-side constant, make_* passes that constant in.
inline PlanVariant plan_base(Kind kind, int threads, int chunk, int tail_bm) {
  PlanVariant v{};
  v.kind = kind, v.threads = threads, v.chunk = chunk, v.tail_bm = tail_bm;
  return v;
}
// the v2 family's plan parameters: 256 x 256 tiles + 128 / 64-row classes, one 512-thread workgroup per CU (32 CUs
// per XCD); the 64-row class takes <= 64 remaining rows of fp16 / weight-only problems (small batches)
inline PlanVariant plan_v2_base(int threads = 512) {
  PlanVariant v = plan_base(Kind::V2, threads, 32, 128);
  v.tail2_bm = 64;
  return v;
}
// gg_v2_kernel's tile bodies (mx: the MX types' too)
inline PlanVariant plan_v2(bool mx) {
  PlanVariant v = plan_v2_base();
  // (w4a4 g128, gg_tile_g128: 256 / 128-row classes as int4)
  for (int q : {QT_F16, QT_I8, QT_I4, QT_I4G, QT_F8, QT_BF16}) v.geom[q] = {256, 256, 128, 512};
  v.geom[QT_W4A16] = {256, 256, 32, 512};  // 64-K stages: 32 B of 4-bit codes per row
  v.geom[QT_W8A16] = {256, 256, 64, 512};
  v.geom[QT_W2A16] = {256, 256, 16, 512};  // 64-K stages: 16 B of 2-bit codes per row
  if (mx) {
    v.geom[QT_MXF4] = v.geom[QT_MXF8A] = {256, 256, 128, 512};
    v.geom[QT_MXF4W] = {256, 256, 32, 512};  // weight-only MXFP4: the 4-bit stage
  }
  v.silu_epi = true;  // gg_tile_v2's epilogue
  return v;
}
// v3: 256 x bn tiles (+ the 128-row class) of fp16 / w8a8 / w4a4, two workgroups per CU where two LDS images fit
inline PlanVariant plan_v3(int bn, int threads, int lds_bytes) {
  PlanVariant v = plan_base(Kind::V3, threads, 32 * (160 * 1024 / lds_bytes >= 2 ? 2 : 1), 128);
  v.lds_bytes = lds_bytes;
  for (int q : {QT_F16, QT_I8, QT_I4}) v.geom[q] = {256, bn, 64, threads};
  v.silu_epi = true;  // epilogue_v3
  return v;
}
// wo2: 64-row tiles only at nwg workgroups per CU (silu_wo: it has the WO_SILU builds for weight-only problems)
inline PlanVariant plan_wo2(int nwg, bool mx, bool silu_wo) {
  PlanVariant v = plan_v2_base();
  v.geom[QT_W4A16] = {64, 256, 32, 512};  // 64-K stages: 32 B of 4-bit codes per row
  v.geom[QT_W8A16] = {64, 256, 64, 512};
  v.geom[QT_W2A16] = {64, 256, 16, 512};
  // 64 x 128 tiles: w8a8 (int8), fp16 (64-K stages), w4a4 (256-K stages)
  v.geom[QT_I8] = v.geom[QT_F16] = v.geom[QT_I4] = {64, 128, 128, 512};
  if (mx) {
    v.geom[QT_MXF4W] = {64, 256, 32, 512};   // weight-only MXFP4: the 4-bit stage
    v.geom[QT_MXF8A] = {64, 128, 128, 512};  // w4a8_g32_sym_MXFP8: 64 x 128 tiles (128-K stages)
  }
  v.chunk = 32 * nwg;  // nwg workgroups per CU, 32 CUs per XCD
  v.tail_bm = v.tail2_bm = 0;
  v.silu_epi = true;  // its fp16 / w8a8 / w4a4 problems run gg_tile_v2 64 x 128 bodies (their epilogue)
  v.silu_wo = silu_wo;
  return v;
}

struct HostProblem {
  const void *A, *B, *SA, *SB;
  void* C;
  int M, N, K, a_bits, w_bits, gsize, sym;
  int64_t lda, ldb, ldc;  // 16-bit words, 0 = dense
  int fmt;                // MXMOE_GG_FMT_*
};

// Workspace: [GGMeta x P][ptr_A x P][ptr_B x P][ptr_SA x P][ptr_SB x P][ptr_C x P][TileDesc x grid]
// workspace: plan table | 5 pointer columns | tile table | split-K counters (one per tile slot,
// zero between launches) | split-K slabs
struct WsLayout {
  size_t meta, ptr, tiles, counters, slabs, total;
};

struct Plan {
  std::vector<GGMeta> meta;     // table rows (planned problems only)
  std::vector<int> order;       // table row -> caller's problem index
  std::vector<TileDesc> tiles;  // indexed by blockIdx
  int total_tiles = 0;
  int launch_grid = 0;          // workgroups launched (= tiles.size() unless persistent)
  int slabs = 0;                // split-K partial slabs
  int tail_slabs = 0;           // of which for the tail split (split_tails)
};

// a dynamic plan's own data behind the planned layout: geometry rows | table order | per-workgroup scratch
// (rows, tile prefix) | status
struct DynLayout {
  size_t geom, order, rows, cum, status, total;
};
struct DynPlan {
  int variant = 0;
  std::vector<GGMeta> meta;    // row i = the caller's problem i (M and tile_begin are the device planner's)
  std::vector<DynGeom> geom;
  std::vector<int32_t> order;  // tile-table order: problem indices, longest K stages first
  int64_t rows_total = 0;
  int slots = 0;
  int qtype_mask = 0;
};

// The library's variants, in ABI order: set once, by gg_api.hip when the library loads (the pointers stay valid).
void set_plan_variants(const PlanVariant* const* variants, int count);
int variant_index(const char* name);  // 0 when there is none of that name
int check_variant(int variant);

int qtype_of(int a_bits, int w_bits, int gsize, int sym, int fmt, int* qt);
std::vector<HostProblem> to_host(const mxmoe_gg_problem* problems, int problem_count);
// Validate one problem and fill its table row.
int build_meta(const HostProblem& p, int idx, const PlanVariant& v, bool check_ptrs, GGMeta* m);
// MXMOE_GG_VARIANT_AUTO -> concrete variant from the quant types present.
int resolve_variant(int variant, const std::vector<HostProblem>& hp, int* out);
// Tile generation + scheduling (a problem that fails validation leaves `plan` as it was).
int plan_host(const std::vector<HostProblem>& probs, int variant, bool check_ptrs, Plan* plan);

WsLayout ws_layout(int P, int grid, int slabs);
std::vector<const void*> pointer_columns(const std::vector<int>& order, const std::vector<HostProblem>& hp);
std::vector<uint8_t> workspace_image(const Plan& plan, const std::vector<const void*>& cols, WsLayout* out);
uint64_t plan_signature(const Plan& plan);

// The host half of a fixed-capacity ("dynamic") plan (gg_dyn.h).
DynLayout dyn_layout(int P, int slots);
int plan_dynamic_host(const mxmoe_gg_problem* problems, int P, int variant, const int32_t* joint_idx, int n_joint,
                      int64_t rows_total, const mxmoe_gg_dyn_extent* extents, bool check_ptrs, DynPlan* out);

#pragma GCC visibility pop
}  // namespace mxmoe
