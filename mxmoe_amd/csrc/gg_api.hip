// gg_api.hip — host side of libmxmoe_gg.so: the C-ABI declared in include/mxmoe_gg.h.
//
// Reference behaviour replaced (SeaCatComplexes/MxMoE):
//   host API groupgemm_hz_fused_<i> ........ kernel_sketch.py:82-145 (prefix sum on host,
//                                             cudaMalloc/Memcpy/Free per call, grid = #SMs)
//   tile -> (problem, m, n) by prefix scan .. tile_scheduler.cuh:25-50
//   registry FuncType / kernel selection ... registry.cuh:28-107, compose_kernel.py:482-529
//   qtype dispatch + "quant type not supported" ... compose_kernel.py:47-57, 421-479
// Here: the planner builds an explicit tile table once into a caller-owned workspace — tiles of
// the longest problems first (LPT), grouped into chunks of neighbouring tiles that run together on
// one XCD (shared A rows / B columns hit that XCD's L2) — and the launch is allocation- and
// sync-free (hipGraph capturable). Errors are status codes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mxmoe_gg.h"
#include "gg_device.h"
#include "gg_dyn.h"
#ifdef MXMOE_LAB
#include "gg_f6.h"   // lab-only fp6 w4a4 route: measured slower than the int4 path
#include "gg_v2q.h"  // lab-only persistent kernel: not compiled into the product library
#include "gg_v4.h"   // lab-only one-wave-per-SIMD 256 x 256 tile
// lab-only operand format: w4a4_g-1_sym with A / B as fp6 images (mxmoe_gg_pack_f6, gg_f6.h)
#define MXMOE_GG_FMT_F6 3
#define MXMOE_GG_F6_ROW_BYTES(K) ((((int64_t)(K) + 127) / 128) * 96)
#endif

using namespace mxmoe;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(MXMOE_GG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// the small-batch weight-only tile's loop options (gg_tile_wo)
constexpr int kWo3 = WO_SCLATE | WO_ANDOR | WO_MSKIP | WO_SPLIT | WO_NIBPOS;
// the round-3 AUTO default's mainloop flags (variant v2x_256x256_w8_b3_buf_spread_edma, without the
// weight-only options)
constexpr int kV2x = V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | (4 << V2_SPREAD_SHIFT);
[[maybe_unused]] constexpr int kV2xProduct = kV2x | WO_PIPE | WO_STAG | V2_I4NOPAIR | V2_I4EDMA;
[[maybe_unused]] constexpr int kWo3Product = kWo3 | WO_PCH;

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

// One compiled kernel of a variant's family: the tile bodies of the quant types in `qmask`.
struct Build {
  int qmask;      // 1 << QType it has a body for (wo2: | kQmaskWoSilu, a WO_SILU build)
  bool fallback;  // also runs any subset of qmask no entry matches exactly
  int lds_bytes;  // reported in the plan info
  void (*launch)(const GGArgs&, int grid, hipStream_t);
};
template <size_t N>
using Builds = std::array<Build, N>;
template <size_t A, size_t B>
constexpr Builds<A + B> operator+(const Builds<A>& a, const Builds<B>& b) {
  Builds<A + B> r{};
  for (size_t i = 0; i < A + B; ++i) r[i] = i < A ? a[i] : b[i - A];
  return r;
}
struct BuildTable {
  const Build* rows;
  int n;
};
template <size_t N>
constexpr BuildTable table_of(const Builds<N>& b) { return {b.data(), (int)N}; }
// The build a quant-type set (`key`: the call's mask, cut to the bits the family looks at) launches:
// the entry with that mask, else the first fallback — they are listed narrowest first — that has every
// type of the call the fallbacks know at all. -1: not compiled (the lab tables).
constexpr int pick_build(BuildTable t, int key) {
  int known = 0;
  for (int i = 0; i < t.n; ++i) {
    if (t.rows[i].qmask == key) return i;
    if (t.rows[i].fallback) known |= t.rows[i].qmask;
  }
  for (int i = 0; i < t.n; ++i)
    if (t.rows[i].fallback && (key & known & ~t.rows[i].qmask) == 0) return i;
  return -1;
}
constexpr bool exact_entries_pick_themselves(BuildTable t, int (*pick)(int)) {
  for (int i = 0; i < t.n; ++i)
    if (t.rows[pick(t.rows[i].qmask)].qmask != t.rows[i].qmask) return false;
  return true;
}
template <auto Kernel, int THREADS>
void launch_k(const GGArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(THREADS), 0, s, a);
}

enum class Kind { V0, V2, V3 };  // (the fp6 kernel is planned as V3: no split-K, no XCD regions)

struct Variant {
  const char* name;
  Kind kind;
  TileGeom geom[QT_COUNT] = {};  // indexed by QType (main tile); bn == 0: no tile body for the type. Every
                                 // make_* below sets the types its kernel has one for
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
  BuildTable builds;        // the family's compiled kernels
  int (*pick)(int qmask);   // index in `builds` of the one a plan's quant-type set (1 << QType present,
                            // kQmaskWoSilu) launches: the launch and the plan info's LDS size both use it
};
Variant variant_base(const char* name, Kind kind, int threads, int lds_bytes, int chunk, int tail_bm, BuildTable builds,
                     int (*pick)(int)) {
  Variant v;
  v.name = name, v.kind = kind, v.threads = threads, v.lds_bytes = lds_bytes, v.chunk = chunk, v.tail_bm = tail_bm;
  v.builds = builds, v.pick = pick;
  return v;
}
constexpr int pick_only(int) { return 0; }  // (families of one build)

[[maybe_unused]] constexpr int kMx4 = 1 << QT_MXF4;   // w4a4_g32_sym_MXFP4
[[maybe_unused]] constexpr int kMxW = 1 << QT_MXF4W;  // weight-only MXFP4
[[maybe_unused]] constexpr int kMx8 = 1 << QT_MXF8A;  // w4a8_g32_sym_MXFP8 (gg_tile_v2's 64 x 128 body)
// plan-info qtype_mask bit: a weight-only problem carries MXMOE_GG_EPI_SILU_MUL (selects the WO_SILU
// builds of wo2)
constexpr int kQmaskWoSilu = 1 << 16;
// the MX types have tile bodies in the product library's v2 / wo2 build tables only
#ifdef MXMOE_LAB
constexpr bool kMxBodies = false;
#else
constexpr bool kMxBodies = true;
#endif

template <class C16, class C8, class C4>
constexpr Builds<1> kV0Builds = {{{7, true, FusedCfg<C16, C8, C4>::LDS_BYTES, &launch_k<&gg_fused_kernel<C16, C8, C4>, C16::kThreads>}}};
template <class C16, class C8, class C4>
Variant make_v0(const char* name) {
  constexpr int lds = FusedCfg<C16, C8, C4>::LDS_BYTES;
  Variant v = variant_base(name, Kind::V0, C16::kThreads, lds, lds <= 80 * 1024 ? 64 : 32 /* workgroups per XCD at once */, 0,
                           table_of(kV0Builds<C16, C8, C4>), &pick_only);
  v.geom[QT_F16] = {C16::BM, C16::BN, C16::BKB, C16::kThreads};
  v.geom[QT_I8] = {C8::BM, C8::BN, C8::BKB, C8::kThreads};
  v.geom[QT_I4] = {C4::BM, C4::BN, C4::BKB, C4::kThreads};
  return v;
}

// ---- v2: specialised on the set of quant types the plan contains (QM) and the mainloop flags (ABL)
template <int ABL>
constexpr int kV2Lds = (ABL & V2_B3) ? 160 * 1024 : V2Cfg<256>::LDS_BYTES + V2_LDS_EXTRA;
template <int ABL, int LDS, int... QM>
constexpr Builds<sizeof...(QM)> v2_rows(bool fallback = false) {
  return {{Build{QM, fallback, LDS, &launch_k<&gg_v2_kernel<ABL, QM>, 512>}...}};
}
// Exact sets run a kernel of the variant's flags: fp16, w8a8, w4a4, w4a4 + w8a8 (LP-1 mixed), all three, w4a16,
// w4a16 + w8a8 (the reference's hz_fused pairing), w8a16, w4a4 g128, w2a16, E4M3, bf16, and each MX type alone
// (w4a8_g32_sym_MXFP8: a ring of three K = 128 stages in the variant's LDS image).
// Any other mix: every tile body in one kernel. The staggered int bodies leave no register
// room for that (the compiler spilled inside their K loops), so the fallbacks are plain v2 (ABL = 0; the
// plan info still reports the variant's LDS image); the 2-bit weight-only body only joins when the mix has
// one (it costs 12 B of prologue spill there, tests/test_codegen.py), the MX bodies likewise — builds apart
// from the narrower ones, which come out unchanged.
// (lab builds: fp16, w8a8, w4a4, w8a8 + w4a4, w4a16, E4M3, bf16 only; fast: fp16, w8a8, w4a16)
template <int ABL>
constexpr auto kV2Builds =
#if defined(MXMOE_LAB) && defined(MXMOE_LAB_FAST)
    v2_rows<ABL, kV2Lds<ABL>, 1, 2, 8>();
#elif defined(MXMOE_LAB)
    v2_rows<ABL, kV2Lds<ABL>, 1, 2, 4, 6, 8, 128, 256>();
#else
    v2_rows<ABL, kV2Lds<ABL>, 1, 2, 4, 6, 7, 8, 10, 16, 32, 64, 128, 256, kMx4, kMxW, kMx8>() +
    v2_rows<0, kV2Lds<ABL>, 63, 127, 511, 511 | kMx4, 511 | kMx4 | kMxW, 511 | kMx4 | kMxW | kMx8>(true);
#endif
// timing ablations: int8 tiles only (kAblMask) / w4a16 tiles only (kWoAblMask), whatever the call holds
template <int ABL>
constexpr auto kV2AblBuilds = v2_rows<ABL, kV2Lds<ABL>, (ABL & kAblMask) ? 7 : 8>(true);
template <int ABL>
constexpr BuildTable v2_builds() {
  if constexpr ((ABL & (kAblMask | kWoAblMask)) != 0) return table_of(kV2AblBuilds<ABL>);
  else return table_of(kV2Builds<ABL>);
}
template <int ABL>
constexpr int pick_v2(int qmask) {
#ifdef MXMOE_LAB
  return pick_build(v2_builds<ABL>(), qmask & 511);
#else
  // (all 13 type bits beside an MX type, the low 9 otherwise: the only other bit is the lab's fp6 type, which no
  // product variant plans)
  return pick_build(v2_builds<ABL>(), qmask & ((qmask & (kMx4 | kMxW | kMx8)) ? 8191 : 511));
#endif
}
#ifndef MXMOE_LAB
static_assert(exact_entries_pick_themselves(v2_builds<kV2xProduct>(), &pick_v2<kV2xProduct>));
constexpr const Build& v2x_picked(int qmask) { return kV2Builds<kV2xProduct>[pick_v2<kV2xProduct>(qmask)]; }
static_assert(v2x_picked(2).launch == &launch_k<&gg_v2_kernel<kV2xProduct, 2>, 512>);  // exact: the variant's flags
static_assert(v2x_picked(3).launch == &launch_k<&gg_v2_kernel<0, 63>, 512>);           // fallback: plain v2
static_assert(v2x_picked((1 << QT_F16) | (1 << QT_I4G)).qmask == 63 && v2x_picked((1 << QT_W2A16) | (1 << QT_I8)).qmask == 127);
static_assert(v2x_picked((1 << QT_I8) | (1 << QT_F8)).qmask == 511 && v2x_picked((1 << QT_BF16) | (1 << QT_W2A16)).qmask == 511);
static_assert(v2x_picked(kMx4 | (1 << QT_F16)).qmask == (511 | kMx4) && v2x_picked(kMx4 | kMxW).qmask == (511 | kMx4 | kMxW));
static_assert(v2x_picked(kMxW | (1 << QT_I8)).qmask == (511 | kMx4 | kMxW));
static_assert(v2x_picked(kMx8 | (1 << QT_W4A16)).qmask == (511 | kMx4 | kMxW | kMx8) && v2x_picked(kMx8 | kMx4).qmask == v2x_picked(8191).qmask);
#endif

// the v2 family's plan parameters: 256 x 256 tiles + 128 / 64-row classes, one 512-thread workgroup per CU (32 CUs
// per XCD); the 64-row class takes <= 64 remaining rows of fp16 / weight-only problems (small batches)
Variant v2_base(const char* name, int lds_bytes, BuildTable builds, int (*pick)(int), int threads = 512) {
  Variant v = variant_base(name, Kind::V2, threads, lds_bytes, 32, 128, builds, pick);
  v.tail2_bm = 64;
  return v;
}
// gg_v2_kernel's tile bodies (mx: the MX types' too)
void set_v2_geom(Variant* v, bool mx) {
  // (w4a4 g128, gg_tile_g128: 256 / 128-row classes as int4)
  for (int q : {QT_F16, QT_I8, QT_I4, QT_I4G, QT_F8, QT_BF16}) v->geom[q] = {256, 256, 128, 512};
  v->geom[QT_W4A16] = {256, 256, 32, 512};  // 64-K stages: 32 B of 4-bit codes per row
  v->geom[QT_W8A16] = {256, 256, 64, 512};
  v->geom[QT_W2A16] = {256, 256, 16, 512};  // 64-K stages: 16 B of 2-bit codes per row
  if (mx) {
    v->geom[QT_MXF4] = v->geom[QT_MXF8A] = {256, 256, 128, 512};
    v->geom[QT_MXF4W] = {256, 256, 32, 512};  // weight-only MXFP4: the 4-bit stage
  }
}
template <int ABL = 0>
Variant make_v2(const char* name) {
  Variant v = v2_base(name, kV2Lds<ABL>, v2_builds<ABL>(), &pick_v2<ABL>);
  set_v2_geom(&v, kMxBodies);
  v.silu_epi = true;  // gg_tile_v2's epilogue
  return v;
}

// ---- v3: fp16 / w8a8 / w4a4, specialised on the set the plan contains
template <int BN, int WN, int NBUF, int DIST, int OPT, int... QM>
constexpr Builds<sizeof...(QM)> v3_rows(bool fallback = false) {
  return {{Build{QM, fallback, V3Cfg<256, BN, WN, NBUF, DIST>::LDS_BYTES,
                 &launch_k<&gg_v3_kernel<BN, WN, NBUF, DIST, QM, OPT>, V3Cfg<256, BN, WN>::NT>}...}};
}
template <int BN, int WN, int NBUF, int DIST, int OPT>
constexpr auto kV3Builds = v3_rows<BN, WN, NBUF, DIST, OPT, 1, 2, 4, 6>() + v3_rows<BN, WN, NBUF, DIST, OPT, 7>(true);
template <int BN, int WN, int NBUF, int DIST, int OPT>
constexpr int pick_v3(int qmask) { return pick_build(table_of(kV3Builds<BN, WN, NBUF, DIST, OPT>), qmask & 7); }
static_assert(exact_entries_pick_themselves(table_of(kV3Builds<128, 2, 3, 2, 0>), &pick_v3<128, 2, 3, 2, 0>));
static_assert(pick_v3<128, 2, 3, 2, 0>(3) == 4 && pick_v3<128, 2, 3, 2, 0>(5) == 4 && pick_v3<128, 2, 3, 2, 0>(0) == 4);
template <int BN, int WN, int NBUF, int DIST, int OPT = 0>
Variant make_v3(const char* name) {
  typedef V3Cfg<256, BN, WN, NBUF, DIST> CT;
  Variant v = variant_base(name, Kind::V3, CT::NT, CT::LDS_BYTES, 32 * (160 * 1024 / CT::LDS_BYTES >= 2 ? 2 : 1), 128,
                           table_of(kV3Builds<BN, WN, NBUF, DIST, OPT>), &pick_v3<BN, WN, NBUF, DIST, OPT>);
  for (int q : {QT_F16, QT_I8, QT_I4}) v.geom[q] = {256, BN, 64, CT::NT};
  v.silu_epi = true;  // epilogue_v3
  return v;
}

#ifdef MXMOE_LAB
// fp6 w4a4 tiles (gg_f6.h): 256 x 256 (+ 128-row tail class), one 512-thread workgroup per CU
template <int NBUF, int DIST, int OPT>
constexpr Builds<1> kF6Builds = {{{1 << QT_I4F6, true, F6Cfg<256, 256, 2, 4, NBUF, DIST>::LDS_BYTES, &launch_k<&gg_f6_kernel<NBUF, DIST, OPT>, 512>}}};
template <int NBUF, int DIST, int OPT = 0>
Variant make_f6(const char* name) {
  typedef F6Cfg<256, 256, 2, 4, NBUF, DIST> CT;
  Variant v = variant_base(name, Kind::V3, CT::NT, CT::LDS_BYTES, 32, 128, table_of(kF6Builds<NBUF, DIST, OPT>), &pick_only);
  v.geom[QT_I4F6] = {256, 256, CT::SKB, CT::NT};
  return v;
}
#endif  // MXMOE_LAB

// ---- wo2: 64-row tiles at NWG workgroups per CU (gg_wo2_kernel): the weight-only types, and fp16 / w8a8 / w4a4 /
// w4a8_g32_sym_MXFP8 problems beside them on gg_tile_v2's 64 x 128 bodies. SILU: a WO_SILU build (weight-only
// problems with the fused SiLU epilogue, Build::qmask | kQmaskWoSilu)
template <int ABL, int NWG, bool SILU, int... QM>
constexpr Builds<sizeof...(QM)> wo2_rows(bool fallback = false) {
  return {{Build{QM | (SILU ? kQmaskWoSilu : 0), fallback, wo2_lds_bytes<NWG>(),
                 &launch_k<&gg_wo2_kernel<ABL | (SILU ? WO_SILU : 0), QM, NWG>, 512>}...}};
}
// At the variant's NWG: w4a16, w2a16, w4a16 + w8a8 (hz_fused pairing), fp16, w8a8, w4a4, w4a4 + w8a8 (LP-1 mixed),
// weight-only MXFP4 and w4a8_g32_sym_MXFP8, each alone. The 8-bit body does not fit 80 VGPRs (3 workgroups
// per CU) without spilling: calls with w8a16 problems, and any other mix, run 2-WG/CU builds of the same tiles
// (same plan: placement only assumes more slots). WO_SILU builds: only the w4a16, w4a16 + w8a8 and weight-only
// MXFP4 sets at the variant's NWG; w4a8_g32_sym_MXFP8 beside flagged problems always takes the widest.
// (fast lab build: the w4a16, w4a16 + w8a8 and w8a16 sets only, all at the variant's NWG)
template <int ABL, int NWG>
constexpr auto kWo2Builds =
#ifdef MXMOE_LAB_FAST
    wo2_rows<ABL, NWG, false, 8, 10, 16>();
#else
    wo2_rows<ABL, NWG, false, 8, 64, 10, 1, 2, 4, 6, kMxW, kMx8>() + wo2_rows<ABL, 2, false, 16>() +
    wo2_rows<ABL, 2, false, 95, 95 | kMxW, 95 | kMxW | kMx8>(true) +
    wo2_rows<ABL, NWG, true, 8, 10, kMxW>() + wo2_rows<ABL, 2, true, 16>() +
    wo2_rows<ABL, 2, true, 95, 95 | kMxW, 95 | kMxW | kMx8>(true);
#endif
template <int ABL, int NWG>
constexpr int pick_wo2(int qmask) {
#ifdef MXMOE_LAB_FAST
  return pick_build(table_of(kWo2Builds<ABL, NWG>), qmask & 511);
#else
  return pick_build(table_of(kWo2Builds<ABL, NWG>), qmask & (511 | kMxW | kMx8 | kQmaskWoSilu));  // (the type bits wo2 looks at)
#endif
}
#ifndef MXMOE_LAB_FAST
static_assert(exact_entries_pick_themselves(table_of(kWo2Builds<kWo3Product, 3>), &pick_wo2<kWo3Product, 3>));
constexpr bool wo3_picks(int qmask, int build_mask, int nwg) {  // (SiLU builds: both masks | kQmaskWoSilu)
  const Build& b = kWo2Builds<kWo3Product, 3>[pick_wo2<kWo3Product, 3>(qmask)];
  return b.qmask == build_mask && b.lds_bytes == (nwg == 3 ? wo2_lds_bytes<3>() : wo2_lds_bytes<2>());
}
constexpr int kS = kQmaskWoSilu, kW4 = 1 << QT_W4A16;
static_assert(wo3_picks(kW4, 8, 3) && wo3_picks(1 << QT_W8A16, 16, 2) && wo3_picks(kMx8, kMx8, 3));
static_assert(wo3_picks(kW4 | (1 << QT_F16), 95, 2) && wo3_picks(kW4 | (1 << QT_W8A16), 95, 2));
static_assert(wo3_picks(kMxW | (1 << QT_I8), 95 | kMxW, 2) && wo3_picks(kMx8 | kW4, 95 | kMxW | kMx8, 2));
static_assert(wo3_picks(kS | kW4, kS | 8, 3) && wo3_picks(kS | (1 << QT_W2A16), kS | 95, 2));
static_assert(wo3_picks(kS | kMxW | kW4, kS | 95 | kMxW, 2) && wo3_picks(kS | kMx8 | kW4, kS | 95 | kMxW | kMx8, 2));
static_assert(wo3_picks(kS | kMx8 | kMxW, kS | 95 | kMxW | kMx8, 2));
#endif
template <int ABL = 0, int NWG = 2>
Variant make_wo2(const char* name) {
  Variant v = v2_base(name, wo2_lds_bytes<NWG>(), table_of(kWo2Builds<ABL, NWG>), &pick_wo2<ABL, NWG>);
  v.geom[QT_W4A16] = {64, 256, 32, 512};  // 64-K stages: 32 B of 4-bit codes per row
  v.geom[QT_W8A16] = {64, 256, 64, 512};
  v.geom[QT_W2A16] = {64, 256, 16, 512};
  // 64 x 128 tiles: w8a8 (int8), fp16 (64-K stages), w4a4 (256-K stages)
  v.geom[QT_I8] = v.geom[QT_F16] = v.geom[QT_I4] = {64, 128, 128, 512};
  if (kMxBodies) {
    v.geom[QT_MXF4W] = {64, 256, 32, 512};   // weight-only MXFP4: the 4-bit stage
    v.geom[QT_MXF8A] = {64, 128, 128, 512};  // w4a8_g32_sym_MXFP8: 64 x 128 tiles (128-K stages)
  }
  v.chunk = 32 * NWG;  // NWG workgroups per CU, 32 CUs per XCD
  v.tail_bm = v.tail2_bm = 0;
  v.silu_epi = true;  // its fp16 / w8a8 / w4a4 problems run gg_tile_v2 64 x 128 bodies (their epilogue)
#ifndef MXMOE_LAB_FAST
  v.silu_wo = true;   // weight-only problems: the WO_SILU builds
#endif
  return v;
}

// ---- v2p: the persistent v2x (lab; no MX body in the persistent kernels)
template <int TRACE, int... QM>
constexpr Builds<sizeof...(QM)> v2p_rows(bool fallback = false) {
  return {{Build{QM, fallback, 160 * 1024, &launch_k<&gg_v2p_kernel<QM, TRACE>, 512>}...}};
}
template <int TRACE>
constexpr auto kV2pBuilds = v2p_rows<TRACE, 1, 2, 256>() + v2p_rows<TRACE, 511>(true);  // (511: every tile body)
template <int TRACE>
constexpr int pick_v2p(int qmask) { return pick_build(table_of(kV2pBuilds<TRACE>), qmask & 511); }
template <int TRACE = 0>
Variant make_v2p(const char* name) {
  Variant v = v2_base(name, 160 * 1024, table_of(kV2pBuilds<TRACE>), &pick_v2p<TRACE>);
  set_v2_geom(&v, false);
  v.persistent = true;
  v.silu_epi = true;  // (its tile body's; has_silu_epilogue: not from a persistent kernel)
  return v;
}

#ifdef MXMOE_LAB
// v2q: the persistent v2x with the register epilogue and the next tile's ring fill before it
// (gg_v2q.h); planned like v2p (per-workgroup tile lists)
template <int TRACE, int SAUX, int FILLALL, int... QM>
constexpr Builds<sizeof...(QM)> v2q_rows(bool fallback = false) {
  return {{Build{QM, fallback, 160 * 1024, &launch_k<&gg_v2q_kernel<QM, TRACE, SAUX, FILLALL>, 512>}...}};
}
template <int TRACE, int SAUX, int FILLALL>
constexpr auto kV2qBuilds =
#ifdef MXMOE_LAB_FAST
    v2q_rows<TRACE, SAUX, FILLALL, 1, 2>();
#else
    v2q_rows<TRACE, SAUX, FILLALL, 1, 2, 4, 6, 256>() + v2q_rows<TRACE, SAUX, FILLALL, 511>(true);
#endif
template <int TRACE, int SAUX, int FILLALL>
constexpr int pick_v2q(int qmask) { return pick_build(table_of(kV2qBuilds<TRACE, SAUX, FILLALL>), qmask & 511); }
template <int TRACE = 0, int SAUX = 16, int FILLALL = 0>
Variant make_v2q(const char* name, int persist_len = 0) {
  Variant v = make_v2p<0>(name);
  v.builds = table_of(kV2qBuilds<TRACE, SAUX, FILLALL>);
  v.pick = &pick_v2q<TRACE, SAUX, FILLALL>;
  v.persist_len = persist_len;
  return v;
}
// v4d (gg_v4.h): 256 x 256 tiles (+ 128 / 64-row classes), 4 waves at one per SIMD, fp16 / w8a8 / w4a4 only
template <int OPT, int... QM>
constexpr Builds<sizeof...(QM)> v4_rows(bool fallback = false) {
  return {{Build{QM, fallback, V4Cfg<256>::LDS_BYTES, &launch_k<&gg_v4_kernel<QM, OPT>, 256>}...}};
}
template <int OPT>
constexpr auto kV4Builds =
#ifdef MXMOE_LAB_FAST
    v4_rows<OPT, 1, 2, 4>() + v4_rows<OPT, 3>(true);  // (the fast build's only mix; any other set lands there too)
#else
    v4_rows<OPT, 1, 2, 4, 6>() + v4_rows<OPT, 7>(true);
#endif
template <int OPT>
constexpr int pick_v4(int qmask) { return pick_build(table_of(kV4Builds<OPT>), qmask & 511); }
template <int OPT = 0>
Variant make_v4(const char* name) {
  Variant v = v2_base(name, V4Cfg<256>::LDS_BYTES, table_of(kV4Builds<OPT>), &pick_v4<OPT>, 256);
  for (int q : {QT_F16, QT_I8, QT_I4}) v.geom[q] = {256, 256, 128, 256};
  return v;
}
#endif  // MXMOE_LAB

typedef TileCfg<128, 128, 2, 2, 2> T128x128;
typedef TileCfg<256, 128, 2, 2, 1> T256x128;
typedef TileCfg<128, 256, 2, 2, 1> T128x256;

// the fused SiLU epilogue (MXMOE_GG_EPI_SILU_MUL) lives in the fp16 / w8a8 / w4a4 tile bodies of the
// v2 / v3 kernels (gg_tile_v2, epilogue_v3) — the small-batch wo3 kernel's 64 x 128 bodies of those
// types included (round 6); the persistent, v4d and fp6 lab kernels have none (mxmoe_gg_variant_caps
// reports it). Weight-only problems may carry the flag on wo3 only (Variant::silu_wo, build_meta).
bool has_silu_epilogue(const Variant& v) { return v.silu_epi && !v.persistent; }

// Production variants (libmxmoe_gg.so): every one computes correct results. The lab build
// (-DMXMOE_LAB -> libmxmoe_gg_lab.so, tools only: `python -m mxmoe_amd.build --lab`) compiles the
// v2 family only, with the timing ablations (abl_*, WRONG RESULTS by design) and the mainloop
// experiments, for tools/kbench.py A/B runs (MXMOE_GG_LIB=mxmoe_amd/lib/libmxmoe_gg_lab.so).
const std::vector<Variant>& variants() {
  static const std::vector<Variant> v = {
#ifndef MXMOE_LAB
      // round 4: the product lists what AUTO picks; the round-1/2 kernels (v0
      // register-staged tiles, plain / staggered v2, v3 256 x 256) live on in the lab build
      make_v3<128, 2, 3, 2>("v3_256x128_w4_dma_ring3_2wg"),
      // round 3 (AUTO default): v2s3's LDS image, buffer-form LDS-DMA spread over the first MFMA
      // group of each half stage, issued by waves 0-3 for their SIMD partners too (not on int4
      // tiles) — profiles/r03/lab/
      // (+ the weight-only tiles' pipelined fragment reads and, at 64 rows, the late-wave deferral:
      // +1-4 % on the small-batch w4a16 calls, profiles/r03/wo/)
      // round 5: int4 fragment reads kept unpaired (V2_I4NOPAIR: ds_read_b64 instead of 2-way-conflicted
      // ds_read2st64_b64; lab A/B mixed gate_up / down -3.1 / -1.5 %, ds2_mixed -2.1 / -1.9 %,
      // w4a4 on v2x -7.5 / -5.1 %: profiles/r05/nopair/)
      // + the early-wave DMA issue on int4 tiles too (V2_I4EDMA: with the unpaired reads it now pays,
      // lab A/B w4a4 / mixed / ds2_mixed gate_up -2.7..-2.8 %, down -1.3..-3.7 %: profiles/r05/i4edma/)
      make_v2<kV2xProduct>("v2x_256x256_w8_b3_buf_spread_edma"),
      // round 3 (AUTO for small-batch weight-only calls): the 64-row weight-only tile at three
      // workgroups per CU (gg_wo2_kernel<.., 3>; weight-only problems only) — profiles/r03/wo2/;
      // round 4: scale groups by LDS-DMA, register constants for the code -> fp16 step, codes
      // converted where they sit, no MFMAs for row blocks past M, steady / tail loops (-10 to
      // -16 % per call at bs 512, -15 to -25 % at bs 128: profiles/r04/wo/)
      // round 6: tiles whose K stages lie in one scale group (per-channel scales) run a loop without
      // the group bookkeeping, unrolled by the ring depth (WO_PCH): ~58 fewer SALU and ~17 fewer VALU
      // per 3 stages, bit-identical; lab A/B -2.6 to -4.0 % on the per-channel bs 512 / 128 calls,
      // g128 unchanged (profiles/r06/pch/)
      make_wo2<kWo3Product, 3>("wo3_64x256_w8_3wg"),
#elif defined(MXMOE_LAB_FAST)
      // fast lab build (`python -m mxmoe_amd.build --lab-fast`): the product default and the
      // experiments under test only, fp16 / w8a8 bodies only
      make_v2<kV2x>("x_v2x"),
      make_v4("x_v4d_256x256_w4_1wave"),
      make_v4<1>("abl_v4d_stamp"),
      make_v3<128, 2, 3, 2>("v3_256x128_w4_dma_ring3_2wg"),  // the w4a4 AUTO kernel (A/B reference)
      make_v2<kV2x | V2_I4NOPAIR>("x_v2x_i4nopair"),
      make_v2<kV2x | V2_PLAINST>("x_v2x_plainst"),
      make_v2<kV2x | V2_TRACE>("abl_v2x_trace"),
      make_v2<kV2x | V2_TRACE | V2_TRACE_PRO>("abl_v2x_trace_pro"),
      make_v2<kV2x | V2_TRACE | V2_TRACE_DESC>("abl_v2x_trace_desc"),
      make_v2q("x_v2q"),
      make_v2q<0, 0>("x_v2q_plain"),
      make_v2q<0, 0, 1>("x_v2q_plain_fillall"),
      make_v2q<0, 16, 1>("x_v2q_fillall"),
      make_v2q<1, 0, 1>("abl_v2q_plain_fillall_trace"),
      // the small-batch weight-only tile: where its time goes (ablations: WRONG RESULTS by design)
      make_wo2<0, 3>("x_wo3_r3"),  // the round-3 loop
      make_wo2<kWo3, 3>("x_wo3"),
      make_wo2<kWo3Product, 3>("x_wo3_pch"),  // round 6: one-group loop (per-channel scales)
      make_wo2<kWo3, 2>("x_wo2"),
      make_wo2<kWo3 | WO_BUF, 3>("x_wo3_buf"),
      make_wo2<kWo3 | WO_ADEAD, 3>("x_wo3_adead"),
      make_wo2<kWo3 | V2_TRACE, 3>("abl_wo3_trace"),
      make_wo2<kWo3 | WO_PCH | V2_TRACE, 3>("abl_wo3_pch_trace"),  // the product loop, tile timeline
      make_wo2<kWo3 | ABL_WO_NODMA, 3>("abl_wo3_nodma"),
      make_wo2<kWo3 | ABL_WO_NOCOMPUTE, 3>("abl_wo3_nocompute"),
#else
      make_v0<T128x128, T128x128, T128x128>("v0_128x128_w4"),
      make_v0<T256x128, T256x128, T256x128>("v0_256x128_w4"),
      make_v0<T128x256, T128x256, T128x256>("v0_128x256_w4"),
      make_v2("v2_256x256_w8_dma"),
      make_v3<256, 4, 4, 3>("v3_256x256_w8_dma_ring4"),
      make_v2<kV2x>("x_v2x"),
      make_v2<kV2x | V2_I4NOPAIR>("x_v2x_i4nopair"),
      make_v2<kV2x | V2_I4NOPAIR | V2_I4EDMA>("x_v2x_i4edma"),
      // the product's default and small-batch kernels, for planner A/B runs (MXMOE_GG_XCD_PACK, _MIX)
      make_v2<kV2xProduct>("x_v2x_product"),
      make_wo2<kWo3, 3>("x_wo3"),
      make_wo2<kWo3Product, 3>("x_wo3_pch"),  // round 6: one-group loop (per-channel scales)
      // round 6: v4d, one wave per SIMD (gg_v4.h; fp16 / w8a8)
      make_v4("x_v4d_256x256_w4_1wave"),
      make_v2<kV2x | V2_PLAINST>("x_v2x_plainst"),
      make_v2<kV2x | V2_EPIPE>("x_v2x_epipe"),
      make_v2<kV2x | V2_LATEIL>("x_v2x_lateil"),
      make_v2<V2_STAGGER>("v2s_256x256_w8_dma_stagger"),
      make_v2<V2_STAGGER | V2_B3>("v2s3_256x256_w8_dma_stagger_bring3"),
      // mainloop experiments (correct results)
      make_v2<V2_STAGGER | (4 << V2_SPREAD_SHIFT)>("x_v2s_spread4"),
      make_v2<V2_STAGGER | V2_BUF | (4 << V2_SPREAD_SHIFT)>("x_v2s_buf_spread4"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | (4 << V2_SPREAD_SHIFT)>("x_v2s3_buf_spread4"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | (2 << V2_SPREAD_SHIFT)>("x_v2s3_buf_edma2"),
      make_v2<V2_STAGGER | V2_BUF | V2_EARLYDMA | (2 << V2_SPREAD_SHIFT)>("x_v2s_buf_edma2"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | (4 << V2_SPREAD_SHIFT)>("x_v2s3_buf_edma4"),
      make_v2p("x_v2p_256x256_w8_persistent"),
      make_v2p<1>("abl_v2p_trace"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_TRACE | (4 << V2_SPREAD_SHIFT)>("abl_v2x_trace"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | V2_TRACE | (2 << V2_SPREAD_SHIFT)>("abl_v2x_edma_trace"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | V2_STAMP | (2 << V2_SPREAD_SHIFT)>("abl_v2s3_buf_edma2_stamp"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_STAMP | (4 << V2_SPREAD_SHIFT)>("abl_v2s3_buf_sp4_stamp"),
      make_v3<128, 2, 3, 2>("v3_256x128_w4_dma_ring3_2wg"),
      // round 5: v3 at one wave per SIMD on 256 x 256 tiles (128 x 128 wave tiles, accumulators in
      // AGPRs: half the int4 widening per MFMA) — 23-33 % slower, profiles/r05/v3w/
      make_v3<256, 2, 4, 3, 4>("x_v3_256x256_w4_1wg"),
      // round 5: w4a4 on fp6 images and the fp6 MFMA (gg_f6.h; exact, 9-18 % slower than v3's int4
      // tiles on the layer calls: profiles/r05/f6/); OPT 1 unpaired reads, 2 spread DMA
      make_f6<3, 2>("f6_256x256_w8_ring3"),
      make_f6<3, 2, 1>("xf6_nopair"),
      make_f6<3, 2, 2>("xf6_spread"),
      make_f6<3, 2, 3>("xf6_nopair_spread"),
      // timing ablations of the staggered v2 (WRONG RESULTS by design; int8 tiles only)
      make_v2<V2_STAGGER | ABL_NO_DMA>("abl_v2s_nodma"),
      make_v2<V2_STAGGER | ABL_NO_EPI>("abl_v2s_noepi"),
      make_v2<V2_STAGGER | ABL_NO_DMA | ABL_NO_EPI>("abl_v2s_nodma_noepi"),
      make_v2<V2_STAGGER | V2_TRACE>("abl_v2s_trace"),
      make_v2<V2_STAGGER | ABL_DMA_HOT>("abl_v2s_dmahot"),
      // where the DMA cost goes (plain v2; int8 tiles only)
      make_v2<ABL_B_NODMA>("abl_v2_b_nodma"),
      make_v2<ABL_B_REGLOAD>("abl_v2_b_regload"),
      make_v2<ABL_B_TILED>("abl_v2_b_tiled"),
      // weight-only timing ablations (w4a16 tiles only)
      make_v2<V2_STAGGER | ABL_WO_BTILED>("abl_v2s_wo_btiled"),
      make_v2<V2_STAGGER | ABL_WO_NODMA>("abl_v2s_wo_nodma"),
      make_v2<V2_STAGGER | ABL_WO_NOCOMPUTE>("abl_v2s_wo_nocompute"),
      // weight-only experiment (correct results): v2x + the pipelined 128 / 64-row weight-only loop
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | (4 << V2_SPREAD_SHIFT) | WO_PIPE>("x_v2x_wopipe"),
      make_v2<V2_STAGGER | V2_B3 | V2_BUF | V2_EARLYDMA | (4 << V2_SPREAD_SHIFT) | WO_PIPE | WO_STAG>("x_v2x_wopipe_stag"),
#endif
  };
  return v;
}

int variant_index(const char* name) {
  for (size_t i = 0; i < variants().size(); ++i)
    if (!strcmp(variants()[i].name, name)) return (int)i;
  return 0;
}

int qtype_of(int a_bits, int w_bits, int gsize, int sym, int fmt, int* qt) {
  fmt &= 0xFF;  // (epilogue flags, MXMOE_GG_EPI_*, live above the operand format)
  auto take = [&](int q) { return *qt = q, (int)MXMOE_GG_OK; };
  if (fmt == MXMOE_GG_FMT_E4M3) {  // w8a8_g-1_sym_E4M3 (tile_config.py:45, 104-106, 192)
    if (a_bits == 8 && w_bits == 8 && gsize == -1 && sym) return take(QT_F8);
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "quant type not supported: w%da%d_g%d_%s_E4M3 (only w8a8_g-1_sym_E4M3)",
                w_bits, a_bits, gsize, sym ? "sym" : "asym");
  }
  if (fmt == MXMOE_GG_FMT_BF16) {  // bf16 (tile_config.py:42, 99-102)
    if (a_bits == 16 && w_bits == 16) return take(QT_BF16);
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "quant type not supported: w%da%d bf16 (only 16-bit bf16 operands)", w_bits,
                a_bits);
  }
  if (fmt == MXMOE_GG_FMT_MXFP4) {  // OCP MXFP4: e2m1 codes, one e8m0 scale per 32-K block
    if (a_bits == 4 && w_bits == 4 && gsize == 32 && sym) return take(QT_MXF4);
    if (a_bits == 16 && w_bits == 4 && gsize == 32 && sym) return take(QT_MXF4W);  // weight-only: fp16 A on the same B operand
    return fail(MXMOE_GG_ERR_UNSUPPORTED,
                "quant type not supported: w%da%d_g%d_%s_MXFP4 (only w4a4_g32_sym_MXFP4 and w4a16_g32_sym_MXFP4)",
                w_bits, a_bits, gsize, sym ? "sym" : "asym");
  }
  if (fmt == MXMOE_GG_FMT_MXFP8) {  // OCP MXFP8 (e4m3) activations on MXFP4 weights
    if (a_bits == 8 && w_bits == 4 && gsize == 32 && sym) return take(QT_MXF8A);
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "quant type not supported: w%da%d_g%d_%s_MXFP8 (only w4a8_g32_sym_MXFP8)", w_bits,
                a_bits, gsize, sym ? "sym" : "asym");
  }
#ifdef MXMOE_LAB
  if (fmt == MXMOE_GG_FMT_F6) {  // w4a4_g-1_sym with fp6 images of the int4 codes (mxmoe_gg_pack_f6)
    if (a_bits == 4 && w_bits == 4 && gsize == -1 && sym) return take(QT_I4F6);
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "quant type not supported: w%da%d_g%d_%s as fp6 images (only w4a4_g-1_sym)",
                w_bits, a_bits, gsize, sym ? "sym" : "asym");
  }
#endif
  if (fmt != MXMOE_GG_FMT_DEFAULT) return fail(MXMOE_GG_ERR_UNSUPPORTED, "unknown operand format %d", fmt);
  if (a_bits == 16 && w_bits == 16) return take(QT_F16);
  if (a_bits == 8 && w_bits == 8 && gsize == -1 && sym) return take(QT_I8);
  if (a_bits == 4 && w_bits == 4 && gsize == -1 && sym) return take(QT_I4);
  if (a_bits == 4 && w_bits == 4 && gsize == 128 && sym) return take(QT_I4G);  // w4a4_g128_sym (cta_gemm.cuh:610-772)
  if (a_bits == 16 && (w_bits == 2 || w_bits == 4 || w_bits == 8))  // weight-only; group size checked per problem
    return take(w_bits == 2 ? QT_W2A16 : w_bits == 4 ? QT_W4A16 : QT_W8A16);
  return fail(MXMOE_GG_ERR_UNSUPPORTED, "quant type not supported: w%da%d_g%d_%s", w_bits, a_bits, gsize,
              sym ? "sym" : "asym");
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

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
WsLayout ws_layout(int P, int grid, int slabs) {
  WsLayout l;
  l.meta = align_up((size_t)std::max(P, 1) * sizeof(GGMeta), 256);
  l.ptr = align_up((size_t)std::max(P, 1) * sizeof(void*), 256);
  l.tiles = align_up((size_t)std::max(grid, 1) * sizeof(TileDesc), 256);
  l.counters = slabs ? align_up((size_t)grid * sizeof(int32_t), 256) : 0;
  l.slabs = (size_t)slabs * SPLITK_SLAB_BYTES;
  l.total = l.meta + 5 * l.ptr + l.tiles + l.counters + l.slabs;
  return l;
}

// The strides of a problem whose dense A / B rows are arow / brow bytes, checked, and its table row filled but for
// GGMeta::reserved and the type's reserved2 bits.
int meta_row(const HostProblem& p, int idx, int qt, const Variant& v, int64_t arow, int64_t brow, bool dma_rows, GGMeta* m) {
  const bool silu = (p.fmt & MXMOE_GG_EPI_SILU_MUL) != 0;
  const int64_t lda_b = p.lda ? p.lda * 2 : arow;
  const int64_t ldb_b = p.ldb ? p.ldb * 2 : brow;
  const int64_t ncols = silu ? p.N / 2 : p.N;  // columns of C
  const int64_t ldc = p.ldc ? p.ldc : ncols;
  if (lda_b < arow || ldb_b < brow || (lda_b % 16) || (ldb_b % 16))
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: lda/ldb must be >= K row and a multiple of 8 words", idx);
  // the buffer-form LDS-DMA addresses a 256-row tile with 32-bit offsets below 2^31
  if (dma_rows && (lda_b >= (int64_t)1 << 23 || ldb_b >= (int64_t)1 << 23))
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: A / B row strides must be below 8 MiB", idx);
  if (ldc < ncols || (ldc % 8))
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: ldc must be >= %s and a multiple of 8", idx, silu ? "N / 2" : "N");
  memset(m, 0, sizeof(*m));
  m->M = p.M, m->N = p.N, m->K = p.K, m->qtype = qt;
  m->tiles_n = (p.N + v.geom[qt].bn - 1) / v.geom[qt].bn;
  m->kbytes = (int32_t)arow;
  m->reserved2 = silu ? META_SILU : 0;
  m->lda_b = lda_b, m->ldb_b = ldb_b, m->ldc = ldc;
  return MXMOE_GG_OK;
}

// Validate one problem and fill its table row.
// Weight-only WxA16: A fp16 [M][K], B codes [N][K * w_bits / 8] (mxmoe_gg_repack_weightonly
// layout), scale_b = scale / zp in the reference permute_scale layout; K in 64-element stages.
// Weight-only MXFP4 (g32, QTypeInfo::dword_scales): B canonical e2m1 codes, scale_b e8m0 bytes in the MXFP4
// device layout — no repack, no fp16 scale groups: the kernel sees one group over all K stages.
int build_meta_weightonly(const HostProblem& p, int idx, int qt, const Variant& v, bool check_ptrs, GGMeta* m) {
  const bool mx = qinfo(qt).dword_scales != nullptr;
  if (p.K % 64) return fail(MXMOE_GG_ERR_INVALID, "problem %d: weight-only needs K %% 64 == 0 (K=%d)", idx, p.K);
  if (!mx && p.gsize != -1 && (p.gsize <= 0 || p.gsize % 64 || p.K % p.gsize))
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "problem %d: weight-only group size %d must be -1 or a multiple of 64 dividing K=%d",
                idx, p.gsize, p.K);
  if (p.N % 8 != 0) return fail(MXMOE_GG_ERR_INVALID, "problem %d: N=%d must be a multiple of 8", idx, p.N);
  // (the SiLU flag: build_meta checked N % 32 and the variant)
  if (int st = meta_row(p, idx, qt, v, (int64_t)p.K * 2, (int64_t)p.K * p.w_bits / 8, false, m)) return st;
  if (check_ptrs && p.M > 0 && p.N > 0) {
    if (!p.A || !p.B || !p.C) return fail(MXMOE_GG_ERR_INVALID, "problem %d: NULL A/B/C", idx);
    if (!p.SB) return fail(MXMOE_GG_ERR_INVALID, "problem %d: NULL scale pointer (weight-only scale_b)", idx);
    if (((uintptr_t)p.A | (uintptr_t)p.B | (uintptr_t)p.C) & 15)
      return fail(MXMOE_GG_ERR_INVALID, "problem %d: A/B/C must be 16-byte aligned", idx);
    if (mx && (((uintptr_t)p.SB) & 3))  // (the kernel reads scale dwords)
      return fail(MXMOE_GG_ERR_INVALID, "problem %d: %s scales must be 4-byte aligned", idx, qinfo(qt).dword_scales);
    if (((uintptr_t)p.SB) & (p.sym ? 1 : 3))
      return fail(MXMOE_GG_ERR_INVALID, "problem %d: scales must be %d-byte aligned", idx, p.sym ? 2 : 4);
  }
  // the scale loads address a 256-column tile's rows with a 32-bit offset
  if (mx && p.K > (1 << 20)) return fail(MXMOE_GG_ERR_INVALID, "problem %d: K=%d exceeds 2^20 (MXFP4 weight-only)", idx, p.K);
  m->reserved = (p.gsize == -1 || mx) ? std::max(1, p.K / 64) : p.gsize / 64;  // 64-K stages per scale group
  m->reserved2 |= p.sym ? 1 : 0;
  return MXMOE_GG_OK;
}

int build_meta(const HostProblem& p, int idx, const Variant& v, bool check_ptrs, GGMeta* m) {
  if (p.M < 0 || p.N < 0 || p.K < 0) return fail(MXMOE_GG_ERR_INVALID, "problem %d: negative shape", idx);
  int qt = 0;
  int st = qtype_of(p.a_bits, p.w_bits, p.gsize, p.sym, p.fmt, &qt);
  if (st) return fail(st, "problem %d: %s", idx, g_last_error.c_str());
  if (v.geom[qt].bn == 0)
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "problem %d: variant %s does not implement w%da%d (quant type not supported)",
                idx, v.name, p.w_bits, p.a_bits);
  const bool silu = (p.fmt & MXMOE_GG_EPI_SILU_MUL) != 0;
  if (p.fmt & ~(0xFF | MXMOE_GG_EPI_SILU_MUL)) return fail(MXMOE_GG_ERR_INVALID, "problem %d: unknown fmt flags %#x", idx, p.fmt);
  const QTypeInfo& t = qinfo(qt);
  if (silu && !(t.silu && (!t.weight_only || v.silu_wo)))
    return fail(MXMOE_GG_ERR_UNSUPPORTED,
                "problem %d: the SiLU epilogue needs fp16, w8a8_g-1_sym, w4a4_g-1_sym or w4a8_g32_sym_MXFP8 (weight-only: "
                "the small-batch kernel wo3)", idx);
  if (silu && !has_silu_epilogue(v))
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "problem %d: variant %s has no SiLU epilogue", idx, v.name);
  if (silu && p.N % 32) return fail(MXMOE_GG_ERR_INVALID, "problem %d: the SiLU epilogue needs N %% 32 == 0 (N=%d)", idx, p.N);
  if (t.weight_only) return build_meta_weightonly(p, idx, qt, v, check_ptrs, m);
  const bool k_rule_fails = t.k_mult && p.K % t.k_mult != 0;  // the type's own K granularity
  if (k_rule_fails && t.k_first)
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: %s needs K %% %d == 0 (K=%d)", idx, t.k_what, t.k_mult, p.K);
  const int abits = t.float16 ? 16 : p.a_bits;
  const int64_t kbits = (int64_t)p.K * abits;  // (fp6 images: K of the int4 codes they encode)
  if (kbits % 128 != 0)
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: K=%d must be a multiple of %d for %d-bit data (16-B rows)", idx,
                p.K, (int)(128 / abits), abits);
  if (v.k_stage_bytes && (kbits / 8) % v.k_stage_bytes != 0)
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: variant %s needs K*bits/8 to be a multiple of %d bytes (K=%d)",
                idx, v.name, v.k_stage_bytes, p.K);
  if (k_rule_fails)
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: %s needs K %% %d == 0 (K=%d)", idx, t.k_what, t.k_mult, p.K);
  if (t.int32_bound && p.K > 131072)
    return fail(MXMOE_GG_ERR_INVALID, "problem %d: K=%d exceeds the exact int32 accumulation bound 131072", idx, p.K);
  if (p.N % 8 != 0) return fail(MXMOE_GG_ERR_INVALID, "problem %d: N=%d must be a multiple of 8", idx, p.N);
  // rows staged at another width than their codes (fp6 images of int4 codes: 96 B per K-128 block, K padded
  // to whole blocks, mxmoe_gg_pack_f6)
  const int64_t kbytes = t.staged_bits == abits ? kbits / 8 : ((int64_t)p.K + 127) / 128 * (128 * t.staged_bits / 8);
  const int64_t kbytes_b = kbytes * p.w_bits / abits;  // (w4a8 MXFP8: 4-bit B rows under 8-bit A rows)
  if ((st = meta_row(p, idx, qt, v, kbytes, kbytes_b, true, m))) return st;
  if (check_ptrs && p.M > 0 && p.N > 0) {  // empty problems are dropped by the planner
    if (!p.A || !p.B || !p.C) return fail(MXMOE_GG_ERR_INVALID, "problem %d: NULL A/B/C", idx);
    if (!t.float16 && (!p.SA || !p.SB)) return fail(MXMOE_GG_ERR_INVALID, "problem %d: NULL scale pointer", idx);
    if (((uintptr_t)p.A | (uintptr_t)p.B | (uintptr_t)p.C) & 15)
      return fail(MXMOE_GG_ERR_INVALID, "problem %d: A/B/C must be 16-byte aligned", idx);
    if (!t.float16 && (((uintptr_t)p.SA | (uintptr_t)p.SB) & 1))
      return fail(MXMOE_GG_ERR_INVALID, "problem %d: scales must be 2-byte aligned", idx);
    if (t.dword_scales && (((uintptr_t)p.SA | (uintptr_t)p.SB) & 3))  // (the kernel reads scale dwords)
      return fail(MXMOE_GG_ERR_INVALID, "problem %d: %s scales must be 4-byte aligned", idx, t.dword_scales);
  }
  m->reserved = t.group_fold ? p.K / t.k_mult : 0;  // w4a4 g128: scale groups
  return MXMOE_GG_OK;
}

// The planner's A/B switches: defaults are what the product plans with. Only the tools-only lab build
// (-DMXMOE_LAB, libmxmoe_gg_lab.so) reads them from the environment (MXMOE_GG_<NAME>), once per plan: the
// product library's tile placement never depends on the caller's environment.
struct PlannerOpts {
  double split_ratio_mul = 1.0;  // SPLIT_RATIO_MUL: scales the split-K ratio
  int splitk_all = 0;            // SPLITK_ALL = S > 1: every problem in at least S K slices (where it has >= 4 S stages)
  int band = 4;                  // BAND: m-tiles per band (n-major inside a band): a 32-tile chunk is band x (32 / band)
  int ngroup = 1;                // NGROUP = G: inside a band, n-tiles in groups of G, m-major inside a group (1: n-major)
  int region = 2;                // REGION: XCD regions 0 off, 1 at the queue head, 2 after the chunked tiles (measured 1-5 %
                                 // faster than at the head on the w8a8 gate_up / down / mixed calls, profiles/r02/region/)
  bool region_rot = false;       // REGION_ROT: XCD x starts its sweep x/8 along the swept axis (XCDs stream different panels)
  bool align = true;             // ALIGN: problem-aligned chunks
  int xcd_pack = 4;              // XCD_PACK: 0 off, 1 always head, 2 always tail, 3 head for long region tiles, 4 (pack_xcds)
  int tail_chunk = 16;           // TAIL_CHUNK: tail chunk size
  bool xcd_rr = false;           // XCD_RR: plain round-robin chunks
  int tail_split = 0;            // TAIL_SPLIT: 1 on, 2 weight-only tiles too (split_tails)
  bool mix = false;              // MIX (mix_residency)
  bool lowfill_lpt = false;      // LOWFILL_LPT (lowfill_lpt)
};
PlannerOpts planner_opts() {
  PlannerOpts o;
#ifdef MXMOE_LAB
  auto flag = [](const char* name, char c) { return getenv(name) && getenv(name)[0] == c; };
  auto positive = [](const char* name, int dflt) { return getenv(name) && atoi(getenv(name)) > 0 ? atoi(getenv(name)) : dflt; };
  if (const char* e = getenv("MXMOE_GG_SPLIT_RATIO_MUL")) o.split_ratio_mul = atof(e);
  if (const char* e = getenv("MXMOE_GG_SPLITK_ALL")) o.splitk_all = atoi(e);
  o.band = positive("MXMOE_GG_BAND", o.band);
  o.ngroup = positive("MXMOE_GG_NGROUP", o.ngroup);
  o.region = flag("MXMOE_GG_REGION", '0') ? 0 : flag("MXMOE_GG_REGION", '1') ? 1 : 2;
  o.region_rot = flag("MXMOE_GG_REGION_ROT", '1');
  o.align = !flag("MXMOE_GG_ALIGN", '0');
  if (const char* e = getenv("MXMOE_GG_XCD_PACK")) o.xcd_pack = atoi(e);
  o.tail_chunk = positive("MXMOE_GG_TAIL_CHUNK", o.tail_chunk);
  o.xcd_rr = flag("MXMOE_GG_XCD_RR", '1');
  o.tail_split = flag("MXMOE_GG_TAIL_SPLIT", '1') ? 1 : flag("MXMOE_GG_TAIL_SPLIT", '2') ? 2 : 0;
  o.mix = flag("MXMOE_GG_MIX", '1');
  o.lowfill_lpt = flag("MXMOE_GG_LOWFILL_LPT", '1');
#endif
  return o;
}

struct Plan {
  std::vector<GGMeta> meta;     // table rows (planned problems only)
  std::vector<int> order;       // table row -> caller's problem index
  std::vector<TileDesc> tiles;  // indexed by blockIdx
  int total_tiles = 0;
  int launch_grid = 0;          // workgroups launched (= tiles.size() unless persistent)
  int slabs = 0;                // split-K partial slabs
  int tail_slabs = 0;           // of which for the tail split (split_tails)
};

constexpr TileDesc kEmptySlot = {-1, 0, 0, 0, 0, 0, -1, -1};

// K stages of a problem in its tile body (v2: 128 B per stage; weight-only: 64 elements)
int stages_of(const Variant& v, const GGMeta& m) {
  if (qinfo(m.qtype).weight_only) return m.K / 64;
  return (m.kbytes + v.geom[m.qtype].bkb - 1) / v.geom[m.qtype].bkb;
}
double full_tile_cost(const Variant& v, const GGMeta& m) {
  return qinfo(m.qtype).passes * (double)m.kbytes * v.geom[m.qtype].bm * v.geom[m.qtype].bn;
}
// rows of an m-tile class; v2 classes 256 / 128 / 64 rows (see Variant::tail_bm)
int class_rows(const Variant& v, int cls, const TileGeom& g) { return cls == 0 ? g.bm : cls == 1 ? v.tail_bm : v.tail2_bm; }
// m-tiles of a problem: (m0, class). v2: 256-row tiles while > tail_bm rows remain, then one tail_bm (128)
// or tail2_bm (64) tile
std::vector<std::pair<int, int>> m_tiles(const Variant& v, const GGMeta& m) {
  const TileGeom& g = v.geom[m.qtype];
  std::vector<std::pair<int, int>> mt;
  for (int m0 = 0; m0 < m.M;) {
    const int rem = m.M - m0;
    if (v.kind != Kind::V0 && v.tail2_bm && qinfo(m.qtype).small_class && rem <= v.tail2_bm) {
      mt.push_back({m0, 2});
      m0 += v.tail2_bm;
    } else if (v.kind != Kind::V0 && v.tail_bm && rem <= v.tail_bm) {
      mt.push_back({m0, 1});
      m0 += v.tail_bm;
    } else {
      mt.push_back({m0, 0});
      m0 += g.bm;
    }
  }
  return mt;
}

// split-K (v2 kernels): a problem whose largest tile is far longer than one CU's share of the
// whole call (low-fill calls: small batches, long-K shared experts, per-rank work lists) has its
// tiles cut into split[i] K slices of >= 4 stages each, at most 8
std::vector<int> split_factors(const Variant& v, const std::vector<GGMeta>& all, const std::vector<int>& order,
                               const PlannerOpts& o) {
  std::vector<int> split(all.size(), 1);
  if (v.kind != Kind::V2) return split;
  double total = 0;
  std::vector<double> biggest(all.size(), 0.0);
  for (int i : order) {
    const GGMeta& m = all[i];
    const TileGeom& g = v.geom[m.qtype];
    const double per_row = full_tile_cost(v, m) / g.bm;
    for (const auto& t : m_tiles(v, m)) {
      const double c = per_row * class_rows(v, t.second, g);
      total += c * m.tiles_n;
      biggest[i] = std::max(biggest[i], c);
    }
  }
  const double share = total / (kSplitCUs * v.chunk / 32);  // workgroup slots: CUs x workgroups per CU
  for (int i : order) {
    const double ratio = o.split_ratio_mul * biggest[i] / std::max(share, 1.0);
    if (ratio > 2.0 && !qinfo(all[i].qtype).group_fold)
      split[i] = std::max(1, std::min({8, (int)ratio, stages_of(v, all[i]) / 4}));
  }
  if (o.splitk_all > 1)
    for (int i : order)
      if (!qinfo(all[i].qtype).group_fold)
        split[i] = std::max(split[i], std::max(1, std::min({8, o.splitk_all, stages_of(v, all[i]) / 4})));
  return split;
}

// Tile time model (per K stage, in "bytes": one stage's LDS-DMA bytes or its MFMA work at the
// fp16 rate of 128 flop/B, whichever is larger, plus a fixed 24 KiB-equivalent per stage).
// Fitted to the tile timelines (profiles/r01/session3/trace_bs512.jsonl): 64-row /
// 256-row tile time ratios 1.3 (fp16) and 2.1 (w4a16), where tile area alone says 4.
double stage_time(const Variant& v, const GGMeta& m, int cls) {
  const TileGeom& g = v.geom[m.qtype];
  const QTypeInfo& t = qinfo(m.qtype);
  const double rows = class_rows(v, cls, g), cols = g.bn;
  double bytes, equiv;
  if (t.weight_only) {  // 64 K elements per stage, fp16 A
    bytes = rows * 128 + cols * 64 * t.code_bits / 8.0;
    equiv = 2.0 * rows * cols * 64 / 128;
  } else {
    const double kel = t.el_bits ? g.bkb * 8.0 / t.el_bits : 128.0;
    bytes = (rows + cols) * g.bkb;
    equiv = 2.0 * rows * cols * kel / t.rate * t.fold;
  }
  return std::max(bytes, equiv) + 24576.0;
}
// modelled time of a planned tile (td.prob: a row of `meta`)
struct TileTimer {
  const Variant& v;
  const std::vector<GGMeta>& meta;
  double operator()(const TileDesc& td) const { return stage_time(v, meta[td.prob], td.cls & 0xFF) * (td.ks1 - td.ks0); }
};

// XCD regions. Within one XCD, consecutive tiles run together (the XCD hands each freed CU its
// next block), so a band's A rows and B columns are re-read from that XCD's L2 while they are
// hot; but under chunked LPT a 4-m-tile band of the 44 n-tile shared expert lands on ~5 XCDs and
// each fetches the band's A panels again (and every band its B panels): 528 MB of panel reads
// for 78 MB of operands at bs=8192. One rectangle per XCD (r m-tiles x c n-tiles, enumerated in
// bands of `band` along the cheaper axis) reads r A panels + ceil(r / band) * c B panels (or the
// transpose) — the split of the grid into 8 rectangles is chosen to minimise that sum.
struct Region {
  int gm = 0, gn = 0, r = 0, c = 0;
  bool nband = false;  // true: bands of n-tiles, m-major inside
};
// the regions of a problem of >= 8 chunks of tiles (mt x m.tiles_n, unsplit), if it is cut into any
bool region_of(const Variant& v, const GGMeta& m, int w_bits, int mt, const PlannerOpts& o, Region* out) {
  const int nt = m.tiles_n;
  if (o.region == 0 || v.kind != Kind::V2 || (int64_t)mt * nt < 8 * (int64_t)v.chunk) return false;
  const TileGeom& g = v.geom[m.qtype];
  const double a_panel = (double)g.bm * m.kbytes, b_panel = (double)g.bn * m.K * w_bits / 8.0;
  double best = 0;
  for (int gm = 1; gm <= 8; gm *= 2) {
    const int gn = 8 / gm;
    if (mt < gm || nt < gn) continue;
    const int r = (mt + gm - 1) / gm, c = (nt + gn - 1) / gn;
    // every region non-empty and within 25 % of the largest (the LPT fill evens out the rest)
    const int r_last = mt - (gm - 1) * r, c_last = nt - (gn - 1) * c;
    if (r_last <= 0 || c_last <= 0 || 4 * (int64_t)r_last * c_last < 3 * (int64_t)r * c) continue;
    const int b = o.band;
    const double mband = r * a_panel + (double)((r + b - 1) / b) * c * b_panel;
    const double nband = c * b_panel + (double)((c + b - 1) / b) * r * a_panel;
    const double cost = std::min(mband, nband);
    if (out->gm == 0 || cost < best) {
      *out = Region{gm, gn, r, c, nband < mband};
      best = cost;
    }
  }
  return out->gm != 0;
}

// The call's tiles in enumeration order, before they are placed on XCDs.
struct TileLists {
  std::vector<TileDesc> seq;                          // chunked tiles, problem after problem
  std::vector<int> seq_end;                           // per seq tile: end of its problem's run in seq
  std::vector<std::vector<TileDesc>> region_tiles{8}; // region problems' tiles, per XCD
  int groups = 0;                                     // split-K groups so far
  int n_region = 0;                                   // region problems
  bool region_a16 = false;                            // ... one of them with 16-bit A
};
// Tile enumeration, problems in `plan->order` (table-row order): a region problem's rectangles go to
// region_tiles; every other problem's tiles to seq in 4-m-tile bands, n-major inside a band, so 32
// consecutive tiles form a ~4 x 8 block sharing A rows and B columns. Fills plan->meta and counts plan->slabs.
TileLists enumerate_tiles(const Variant& v, const std::vector<GGMeta>& all, const std::vector<HostProblem>& probs,
                          const std::vector<int>& split, const PlannerOpts& o, Plan* plan) {
  TileLists tl;
  const int band = o.band;
  for (int row = 0; row < (int)plan->order.size(); ++row) {
    const int i = plan->order[row];
    GGMeta m = all[i];
    const TileGeom& g = v.geom[m.qtype];
    const std::vector<std::pair<int, int>> mt = m_tiles(v, m);  // (m0, cls)
    m.tile_begin = (int32_t)tl.seq.size();
    const int nt = m.tiles_n, S = split[i], nst = stages_of(v, m);
    Region rg;
    if (S == 1 && region_of(v, m, probs[i].w_bits, (int)mt.size(), o, &rg)) {
      ++tl.n_region;
      tl.region_a16 = tl.region_a16 || probs[i].a_bits == 16;
      for (int x = 0; x < 8; ++x) {
        const int mb0 = (x / rg.gn) * rg.r, mb1 = std::min((int)mt.size(), mb0 + rg.r);
        const int nb0 = (x % rg.gn) * rg.c, nb1 = std::min(nt, nb0 + rg.c);
        auto put = [&](int mi, int n) {
          tl.region_tiles[x].push_back(TileDesc{row, mt[mi].first, n * g.bn, mt[mi].second, 0, nst, -1, -1});
        };
        const int span_n = nb1 - nb0, span_m = mb1 - mb0;
        const int rot_n = o.region_rot && span_n > 0 ? (x * span_n / 8) : 0;
        const int rot_m = o.region_rot && span_m > 0 ? (x * span_m / 8) : 0;
        if (rg.nband) {
          for (int nb = nb0; nb < nb1; nb += band)
            for (int k = 0; k < span_m; ++k) {
              const int mi = mb0 + (k + rot_m) % span_m;
              for (int n = nb; n < std::min(nb1, nb + band); ++n) put(mi, n);
            }
        } else {
          for (int mb = mb0; mb < mb1; mb += band)
            for (int k = 0; k < span_n; ++k) {
              const int n = nb0 + (k + rot_n) % span_n;
              for (int mi = mb; mi < std::min(mb1, mb + band); ++mi) put(mi, n);
            }
        }
      }
      plan->meta.push_back(m);
      continue;
    }
    for (size_t mb = 0; mb < mt.size(); mb += band)
      for (int ng = 0; ng < nt; ng += o.ngroup)
        for (size_t mi = mb; mi < std::min(mt.size(), mb + band); ++mi)
          for (int n = ng; n < std::min(nt, ng + o.ngroup); ++n) {
            if (S == 1) {
              tl.seq.push_back(TileDesc{row, mt[mi].first, n * g.bn, mt[mi].second, 0, nst, -1, -1});
              continue;
            }
            const int grp = tl.groups++, slab = plan->slabs;
            plan->slabs += S;
            for (int k = 0; k < S; ++k)  // slices of one tile are consecutive: they start together
              tl.seq.push_back(TileDesc{row, mt[mi].first, n * g.bn, mt[mi].second | (k << 8) | (S << 16),
                                        k * nst / S, (k + 1) * nst / S, slab, grp});
          }
    tl.seq_end.resize(tl.seq.size(), (int)tl.seq.size());
    plan->meta.push_back(m);
  }
  return tl;
}

// One XCD simulated as `chunk` workgroup slots taking its queue in order (the hardware hands a freed slot the next block).
struct XcdSim {
  std::vector<double> slot;  // min-heap of slot free times
  double finish = 0, load = 0;
  void add(double t) {
    std::pop_heap(slot.begin(), slot.end(), std::greater<double>());
    slot.back() += t;
    finish = std::max(finish, slot.back());
    std::push_heap(slot.begin(), slot.end(), std::greater<double>());
    load += t;
  }
};
// XCD queues (XCD x's i-th tile is block 8 i + x, round-robin dispatch; placement affects speed and HBM traffic only).
struct XcdQueues {
  std::vector<XcdSim> sim{8};
  std::vector<std::vector<int>> queue{8};  // indices into `tiles`
  std::vector<TileDesc> tiles;             // the chunked tiles (TileLists::seq) first
};
void put_regions(const TileLists& tl, const TileTimer& tile_time, XcdQueues* q) {
  for (int x = 0; x < 8; ++x)
    for (const TileDesc& td : tl.region_tiles[x]) {
      q->sim[x].add(tile_time(td));
      q->queue[x].push_back((int)q->tiles.size());
      q->tiles.push_back(td);
    }
}

// XCD packing, step 1: every small problem WHOLE to one XCD (LPT over the problems' modelled loads), then
// how many region tiles each XCD takes to level the loads, and where in the queue they go.
struct XcdPacking {
  std::vector<std::vector<int>> small_q{8};  // per XCD: seq indices of its small problems' tiles
  std::vector<TileDesc> big;                 // the region tiles in rectangle order
  int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // region tiles per XCD
  bool head = false;                         // region tiles at the queue head
};
XcdPacking pack_loads(const TileLists& tl, const TileTimer& tile_time, int pack) {
  XcdPacking p;
  const int TS = (int)tl.seq.size();
  std::vector<std::pair<int, int>> runs;  // [s0, s1) of one problem's tiles in seq
  for (int s0 = 0; s0 < TS; s0 = tl.seq_end[s0]) runs.push_back({s0, tl.seq_end[s0]});
  std::vector<double> rl(runs.size(), 0.0);
  for (size_t r = 0; r < runs.size(); ++r)
    for (int s = runs[r].first; s < runs[r].second; ++s) rl[r] += tile_time(tl.seq[s]);
  std::vector<int> ro(runs.size());
  for (size_t r = 0; r < ro.size(); ++r) ro[r] = (int)r;
  std::stable_sort(ro.begin(), ro.end(), [&](int a, int b) { return rl[a] > rl[b]; });
  double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r : ro) {
    int x = 0;
    for (int y = 1; y < 8; ++y)
      if (load[y] < load[x]) x = y;
    load[x] += rl[r];
    for (int s = runs[r].first; s < runs[r].second; ++s) p.small_q[x].push_back(s);
  }
  for (int x = 0; x < 8; ++x) p.big.insert(p.big.end(), tl.region_tiles[x].begin(), tl.region_tiles[x].end());
  for (const TileDesc& td : p.big) {
    int x = 0;
    for (int y = 1; y < 8; ++y)
      if (load[y] < load[x]) x = y;
    load[x] += tile_time(td);
    ++p.cnt[x];
  }
  // pack 3: at the head when the region tiles are the long ones (the down call's shared expert, 4x
  // the routed K: LPT), at the tail otherwise (gate_up: every tile the same length)
  p.head = pack == 1;
  if (pack >= 3) {
    double tb = 0, ts = 0;
    for (const TileDesc& td : p.big) tb += tile_time(td);
    for (int e = 0; e < TS; ++e) ts += tile_time(tl.seq[e]);
    p.head = !p.big.empty() && TS > 0 && tb / p.big.size() >= 1.5 * ts / TS;
    if (pack == 4) p.head = p.head || tl.region_a16;  // a 16-bit region problem (fp16 / bf16 / weight-only A)
  }
  return p;
}

// XCD packing (lab A/B: MXMOE_GG_XCD_PACK = 1 region tiles at the queue head,
// 2 at the tail). A call with region problems (the shared expert) and small ones (routed experts):
// every small problem goes WHOLE to one XCD — LPT over the problems' modelled loads, so its A / B
// panels live in one L2 — and the region problems' tiles, taken in rectangle order, are the filler
// that levels the XCDs: tile by tile to the XCD of least modelled load, then cut into consecutive
// pieces (XCD x's piece overlaps its rectangle, so the panel reuse of the rectangles is kept).
// Default (pack 4, product): packing for the MoE call shape — ONE region problem (the shared expert)
// beside >= 8 whole small problems — with the region tiles at the queue head when they are the long
// ones (down: K 4x the routed K; LPT) or when the region problem's A is 16-bit (its panels stream
// twice the bytes per flop: the fp16 gate_up call's head placement cut its counter bytes 2.97 ->
// 2.35 GB and ran 2.4 % faster, where w8a8 gate_up at the head ran 4 % slower, profiles/r06/pack/;
// an arithmetic-intensity cut in its place also sent the int calls of small batches to the head,
// 3-8 % slower at bs 2048, profiles/r06/plan3/); every other call keeps the chunked placement. Lab A/B:
// MXMOE_GG_XCD_PACK = 0 off, 1 always head, 2 always tail, 3 head only for long region tiles.
// Returns false (queues untouched) when the call is not packed.
bool pack_xcds(const Variant& v, const TileLists& tl, const TileTimer& tile_time, const PlannerOpts& o, XcdQueues* out) {
  const int pack = o.xcd_pack, chunk = v.chunk, TS = (int)tl.seq.size();
  size_t T_head = 0;
  for (const auto& h : tl.region_tiles) T_head += h.size();
  int n_small = 0;
  for (int s0 = 0; s0 < TS; s0 = tl.seq_end[s0]) ++n_small;
  const bool moe_shape = tl.n_region == 1 && n_small >= 8;
  if (!(pack > 0 && T_head > 0 && v.kind == Kind::V2 && !v.persistent && (pack != 4 || moe_shape))) return false;
  XcdPacking p = pack_loads(tl, tile_time, pack);
  const std::vector<TileDesc>& big = p.big;
  // XCD x's region tiles: first its own rectangle (region_tiles[x], in band order) up to cnt[x]; the
  // rectangles' surplus tails then fill the XCDs that take more than their own (a piece stays one
  // rectangle plus at most a band's worth of a neighbour: the panel reuse the rectangles bought)
  std::vector<size_t> rb(9, 0);
  for (int x = 0; x < 8; ++x) rb[x + 1] = rb[x] + tl.region_tiles[x].size();
  std::vector<std::vector<int>> pieces(8);
  auto assign_pieces = [&]() {
    std::vector<int> pool;
    for (int x = 0; x < 8; ++x) {
      pieces[x].clear();
      const size_t own = rb[x + 1] - rb[x], take = std::min(own, (size_t)p.cnt[x]);
      for (size_t k = 0; k < own; ++k) (k < take ? pieces[x] : pool).push_back((int)(rb[x] + k));
    }
    size_t n = 0;
    for (int x = 0; x < 8; ++x)
      while ((int)pieces[x].size() < p.cnt[x] && n < pool.size()) pieces[x].push_back(pool[n++]);
  };
  auto tt = [&](int e) { return e < 0 ? tile_time(big[-1 - e]) : tile_time(tl.seq[e]); };
  // the XCD's queue as its slots take it: region tiles first (head) or last, and the queue's last
  // 2 * chunk tiles longest first (the tail tiles of the routed bands are the short ones: LPT at the
  // end evens the slots' finish; earlier tiles keep the band order)
  auto build_q = [&](int x, std::vector<int>* q) {
    q->clear();
    std::vector<int> bq;
    for (int k : pieces[x]) bq.push_back(-1 - k);  // (big tiles: -1 - index)
    if (p.head) *q = bq;
    q->insert(q->end(), p.small_q[x].begin(), p.small_q[x].end());
    if (!p.head) q->insert(q->end(), bq.begin(), bq.end());
    const size_t n = q->size(), tail = std::min(n, (size_t)(2 * chunk));
    std::stable_sort(q->end() - tail, q->end(), [&](int a, int b) { return tt(a) > tt(b); });
  };
  auto finish_of = [&](const std::vector<int>& q) {
    XcdSim xs;
    xs.slot.assign(chunk, 0.0);
    for (int e : q) xs.add(tt(e));
    return xs.finish;
  };
  // local search: move one region tile from the XCD that finishes last to the one that finishes
  // first while the modelled makespan drops (the loads above are level; the slots' finish is not)
  std::vector<std::vector<int>> q(8);
  double fin[8];
  auto rebuild = [&]() {
    assign_pieces();
    for (int x = 0; x < 8; ++x) {
      build_q(x, &q[x]);
      fin[x] = finish_of(q[x]);
    }
  };
  rebuild();
  // (compared as the sorted finish vector, latest first: a move that takes one of several XCDs off
  // the makespan counts as a gain)
  auto key = [&]() {
    std::vector<double> f(fin, fin + 8);
    std::sort(f.begin(), f.end(), std::greater<double>());
    return f;
  };
  for (int it = 0; it < 128; ++it) {
    int hi = 0, lo = 0;
    for (int x = 1; x < 8; ++x) {
      if (fin[x] > fin[hi]) hi = x;
      if (fin[x] < fin[lo]) lo = x;
    }
    if (p.cnt[hi] == 0 || hi == lo) break;
    const std::vector<double> before = key();
    --p.cnt[hi];
    ++p.cnt[lo];
    rebuild();
    if (!(key() < before)) {  // no gain: undo and stop
      ++p.cnt[hi];
      --p.cnt[lo];
      rebuild();
      break;
    }
  }
  const int base = (int)out->tiles.size();
  out->tiles.insert(out->tiles.end(), big.begin(), big.end());
  for (int x = 0; x < 8; ++x) {
    out->queue[x].clear();
    for (int e : q[x]) out->queue[x].push_back(e < 0 ? base + (-1 - e) : e);
  }
  return true;
}

// Chunked LPT placement of the chunked tiles (tl.seq, problems longest first): full chunks of about
// `chunk` tiles that do not straddle problems join the XCD queue with the least modelled time; the last
// 16 chunks' worth of tiles go in chunks of `tail_chunk`, each to the XCD whose simulated finish grows
// least (ties: least total time). Plain round-robin chunks let a low-fill call's few long tiles pile
// onto 2-3 XCDs (bs=512: per-XCD busy time 40 % apart).
void place_chunks(const Variant& v, const TileLists& tl, const TileTimer& tile_time, const PlannerOpts& o, XcdQueues* q) {
  const int chunk = v.chunk, TS = (int)tl.seq.size();
  for (int s0 = 0, c = 0; s0 < TS; ++c) {
    const bool head = TS - s0 > 16 * chunk;
    int len = (o.xcd_rr || head) ? chunk : std::min(chunk, o.tail_chunk);
    if (head && !o.xcd_rr && o.align) {
      // whole problems per chunk: split the rest of this problem's run into near-equal chunks of
      // about `chunk` tiles (a 33-tile expert stays on one XCD instead of spilling 1 tile onto
      // another that re-fetches its A rows), at most 64
      const int rem = tl.seq_end[s0] - s0, nc = std::max(1, (rem + chunk / 2) / chunk);
      len = std::min(64, (rem + nc - 1) / nc);
    }
    const int s1 = std::min(TS, s0 + len);
    // (a chunk can be a whole XCD's slots: 96 for the 3-WG/CU kernel — sized per chunk, not fixed)
    std::vector<double> times(std::max(0, s1 - s0));
    for (int s = s0; s < s1; ++s) times[s - s0] = tile_time(tl.seq[s]);
    int best = c % 8;
    if (!o.xcd_rr && head) {  // full chunks: least total time (cheap; the tail evens out)
      best = 0;
      for (int x = 1; x < 8; ++x)
        if (q->sim[x].load < q->sim[best].load) best = x;
    } else if (!o.xcd_rr) {  // tail: least simulated finish
      double best_finish = 0, best_load = 0;
      for (int x = 0; x < 8; ++x) {
        XcdSim trial = q->sim[x];
        for (int s = s0; s < s1; ++s) trial.add(times[s - s0]);
        if (x == 0 || trial.finish < best_finish || (trial.finish == best_finish && trial.load < best_load)) {
          best = x;
          best_finish = trial.finish;
          best_load = trial.load;
        }
      }
    }
    for (int s = s0; s < s1; ++s) {
      q->sim[best].add(times[s - s0]);
      q->queue[best].push_back(s);
    }
    s0 = s1;
  }
}

#ifdef MXMOE_LAB
// Tail split (v2, not persistent). An XCD hands its blocks to its CUs in queue order, so the
// queue's last tiles run while most of the XCD's CUs have gone idle for good (w8a8 down at
// bs=8192: 194 tiles per XCD = 6 rounds of 32 + 2; tile timelines put the ragged finish at
// 6-8 % of CU time). Per XCD, the tiles that start after the first CU's last tile ended are cut
// along K into S consecutive slices (the split-K path), S in 2..8 (>= 3 stages a slice,
// each slice priced at 2 extra stages for its fill and partial-sum traffic) chosen to minimise
// the XCD's simulated finish; kept only if that gains >= 1 %.
// MEASURED NEGATIVE: 1.5-2 % slower on the w8a8 / fp16 / mixed gate_up calls, the
// only layer-11 calls it cuts (the partial-sum round trip costs more than the ragged finish
// it removes). Lab library only, opt-in: MXMOE_GG_TAIL_SPLIT=1.
void split_tails(const Variant& v, const TileTimer& tile_time, int mode, int* groups, XcdQueues* xq, Plan* plan) {
  const int chunk = v.chunk;
  std::vector<TileDesc>& all_tiles = xq->tiles;
  auto simulate = [&](const std::vector<double>& t, std::vector<double>* starts) {
    std::vector<double> slot(chunk, 0.0);  // min-heap of slot free times
    double finish = 0;
    for (size_t j = 0; j < t.size(); ++j) {
      std::pop_heap(slot.begin(), slot.end(), std::greater<double>());
      if (starts) (*starts)[j] = slot.back();
      slot.back() += t[j];
      finish = std::max(finish, slot.back());
      std::push_heap(slot.begin(), slot.end(), std::greater<double>());
    }
    return std::make_pair(finish, *std::min_element(slot.begin(), slot.end()));
  };
  auto splittable = [&](const TileDesc& td) {
    const QTypeInfo& t = qinfo(plan->meta[td.prob].qtype);
    // (mode 2: weight-only tiles too — the small-batch wo3 calls run ~1.3 rounds of equal tiles)
    return ((td.cls >> 16) & 0xFF) <= 1 && (!t.weight_only || mode == 2) && !t.group_fold && td.ks1 - td.ks0 >= 6;
  };
  for (int x = 0; x < 8; ++x) {
    std::vector<int>& q = xq->queue[x];
    const size_t n = q.size();
    if (n <= (size_t)chunk) continue;  // one round: nothing runs after a CU went idle
    std::vector<double> t(n), st(n);
    for (size_t j = 0; j < n; ++j) t[j] = tile_time(all_tiles[q[j]]);
    const auto base = simulate(t, &st);
    size_t j0 = n;
    while (j0 > 0 && st[j0 - 1] >= base.second) --j0;  // starts are non-decreasing in queue order
    int best_s = 1;
    double best_finish = base.first;
    for (int S = 2; S <= 8; ++S) {
      std::vector<double> t2(t.begin(), t.begin() + j0);
      for (size_t j = j0; j < n; ++j) {
        const TileDesc& td = all_tiles[q[j]];
        const int nst = td.ks1 - td.ks0;
        if (!splittable(td) || nst / S < 3) {
          t2.push_back(t[j]);
          continue;
        }
        const double per_stage = t[j] / nst;
        for (int k = 0; k < S; ++k) t2.push_back(per_stage * ((k + 1) * nst / S - k * nst / S + 2));
      }
      const double f = simulate(t2, nullptr).first;
      if (f < best_finish) {
        best_finish = f;
        best_s = S;
      }
    }
    if (best_s == 1 || best_finish > 0.99 * base.first) continue;
    std::vector<int> q2(q.begin(), q.begin() + j0);
    for (size_t j = j0; j < n; ++j) {
      const TileDesc td = all_tiles[q[j]];
      const int nst = td.ks1 - td.ks0, S = best_s;
      if (!splittable(td) || nst / S < 3) {
        q2.push_back(q[j]);
        continue;
      }
      const int grp = (*groups)++, slab = plan->slabs;
      plan->slabs += S;
      plan->tail_slabs += S;
      for (int k = 0; k < S; ++k) {
        q2.push_back((int)all_tiles.size());
        all_tiles.push_back(TileDesc{td.prob, td.m0, td.n0, (td.cls & 0xFF) | (k << 8) | (S << 16),
                                     td.ks0 + k * nst / S, td.ks0 + (k + 1) * nst / S, slab, grp});
      }
    }
    q.swap(q2);
  }
}

// Mixed residency (lab A/B, MXMOE_GG_MIX = 1): each XCD queue interleaved so a
// CU's co-resident workgroups (wo3: three) hold one full-height tile (a shared-expert tile, MFMA-
// heavy) beside the routed tiles of ~35 rows (weight-stream-heavy) instead of all-shared, then
// all-routed rounds: the routed tiles' stream then runs under the shared tiles' MFMAs. "Full" =
// a tile whose modelled time is at least 1.3x the queue's median.
void mix_residency(const TileTimer& tile_time, XcdQueues* xq) {
  for (auto& q : xq->queue) {
    if (q.size() < 4) continue;
    std::vector<double> t(q.size());
    for (size_t j = 0; j < q.size(); ++j) t[j] = tile_time(xq->tiles[q[j]]);
    std::vector<double> srt(t);
    std::nth_element(srt.begin(), srt.begin() + srt.size() / 2, srt.end());
    const double med = srt[srt.size() / 2];
    std::vector<int> lo, hi;
    for (size_t j = 0; j < q.size(); ++j) ((t[j] >= 1.3 * med) ? hi : lo).push_back(q[j]);
    if (hi.empty() || lo.empty()) continue;
    std::vector<int> out;
    size_t a = 0, b = 0;
    while (a < hi.size() || b < lo.size()) {  // keep the hi : lo proportion along the queue
      if (b >= lo.size() || (a < hi.size() && a * lo.size() <= b * hi.size())) out.push_back(hi[a++]);
      else out.push_back(lo[b++]);
    }
    q.swap(out);
  }
}

// Low-fill LPT (lab opt-in, MXMOE_GG_LOWFILL_LPT=1): a call of at most 4 tiles per CU is laid out
// as one list in descending modelled tile time (stable: a tile's split-K slices and a band's
// m-tiles stay adjacent); block b then lands on XCD b % 8 and each XCD hands its sublist to its
// CUs in LPT order. At 2-3 tiles per CU the XCD chunks concentrate the long tiles (the
// shared expert's split slices) on 2-3 XCDs, and the tile traces show 15-36 % ragged finish.
void lowfill_lpt(const Variant& v, const TileTimer& tile_time, Plan* plan) {
  if (plan->total_tiles > 4 * 8 * v.chunk) return;
  std::vector<TileDesc> list;
  for (const TileDesc& td : plan->tiles)
    if (td.prob >= 0) list.push_back(td);
  std::stable_sort(list.begin(), list.end(), [&](const TileDesc& a, const TileDesc& b) { return tile_time(a) > tile_time(b); });
  plan->tiles = list;
  plan->launch_grid = (int)list.size();
}
#endif  // MXMOE_LAB

// The tile table: XCD x's i-th tile is block 8 i + x.
void emit_tiles(const XcdQueues& xq, Plan* plan) {
  size_t qmax = 0;
  for (const auto& q : xq.queue) qmax = std::max(qmax, q.size());
  int grid = 0;
  plan->tiles.assign(8 * qmax, kEmptySlot);
  for (int x = 0; x < 8; ++x)
    for (size_t i = 0; i < xq.queue[x].size(); ++i) {
      const int b = (int)(8 * i) + x;
      plan->tiles[b] = xq.tiles[xq.queue[x][i]];
      grid = std::max(grid, b + 1);
    }
  plan->tiles.resize(grid);
  plan->total_tiles = 0;
  for (const auto& q : xq.queue) plan->total_tiles += (int)q.size();
  plan->launch_grid = grid;
}
// The persistent kernels' tile table: per-workgroup tile lists [k][G] with a terminating row of empty slots.
void emit_persistent(const Variant& v, const XcdQueues& xq, const TileTimer& tile_time, bool any_tiles, Plan* plan) {
  if (v.persist_len > 0) {
    // v2q with block lists: XCD x's queue cut into groups of L consecutive tiles, group g run by
    // block 8 g + x (that XCD under round-robin placement: speed only); the hardware hands a freed
    // CU the next block, as for the one-tile blocks.
    const int L = v.persist_len;
    size_t ngroups = 0;
    for (const auto& q : xq.queue) ngroups = std::max(ngroups, (q.size() + L - 1) / L);
    const int G = (int)(8 * ngroups);
    plan->tiles.assign((size_t)(L + 1) * G, kEmptySlot);
    for (int x = 0; x < 8; ++x)
      for (size_t j = 0; j < xq.queue[x].size(); ++j) {
        const size_t g = j / L, k = j % L;
        plan->tiles[k * G + 8 * g + x] = xq.tiles[xq.queue[x][j]];
      }
    plan->launch_grid = any_tiles ? G : 0;
    return;
  }
  // v2p: each XCD's queue handed out to its `chunk` workgroups in queue order, every tile to the
  // workgroup whose modelled finish is earliest (what the hardware's dispatch does with blocks,
  // planned once here); workgroup w = 8 * slot + x sits on XCD x under round-robin placement
  // (speed only).
  const int G = 8 * v.chunk;
  std::vector<std::vector<int>> lists(G);
  for (int x = 0; x < 8; ++x) {
    std::vector<std::pair<double, int>> heap;
    for (int sl = 0; sl < v.chunk; ++sl) heap.push_back({0.0, sl});
    std::make_heap(heap.begin(), heap.end(), std::greater<std::pair<double, int>>());
    for (int idx : xq.queue[x]) {
      std::pop_heap(heap.begin(), heap.end(), std::greater<std::pair<double, int>>());
      auto& top = heap.back();
      lists[8 * top.second + x].push_back(idx);
      top.first += tile_time(xq.tiles[idx]);
      std::push_heap(heap.begin(), heap.end(), std::greater<std::pair<double, int>>());
    }
  }
  size_t maxlen = 0;
  for (const auto& l : lists) maxlen = std::max(maxlen, l.size());
  plan->tiles.assign((maxlen + 1) * G, kEmptySlot);
  for (int w = 0; w < G; ++w)
    for (size_t k = 0; k < lists[w].size(); ++k) plan->tiles[k * G + w] = xq.tiles[lists[w][k]];
  plan->launch_grid = any_tiles ? G : 0;
}

// Tile generation + scheduling: validation, one table row per problem (build_meta; empty problems are dropped);
// m-tile classes and split-K factors (m_tiles, split_factors); problems by descending modelled time of their
// first (tallest) tile (stage_time); tile enumeration, a problem of >= 8 chunks of tiles (the shared expert at
// large batch) cut into one rectangle per XCD (enumerate_tiles, region_of); placement — the MoE call shape packed
// problem by problem (pack_xcds), any other call in chunks of about `chunk` tiles, each to the XCD with the least
// modelled time so far, the regions after them (place_chunks); emission in dispatch order (emit_tiles).
int plan_host(const std::vector<HostProblem>& probs, int variant, bool check_ptrs, Plan* plan) {
  const Variant& v = variants()[variant];
  const PlannerOpts o = planner_opts();
  const int P = (int)probs.size();
  std::vector<GGMeta> all(P);
  for (int i = 0; i < P; ++i) {
    int st = build_meta(probs[i], i, v, check_ptrs, &all[i]);
    if (st) return st;
  }
  std::vector<int> order;
  for (int i = 0; i < P; ++i)
    if (probs[i].M > 0 && probs[i].N > 0) order.push_back(i);
  const std::vector<int> split = split_factors(v, all, order, o);
  std::vector<double> tile_cost(P, 0.0);
  for (int i : order) tile_cost[i] = stage_time(v, all[i], m_tiles(v, all[i])[0].second) * stages_of(v, all[i]) / split[i];
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tile_cost[a] > tile_cost[b]; });

  plan->meta.clear();
  plan->order = order;
  plan->slabs = 0;
  plan->tail_slabs = 0;
  TileLists tl = enumerate_tiles(v, all, probs, split, o, plan);
  size_t T = tl.seq.size();
  for (const auto& h : tl.region_tiles) T += h.size();
  if (T > ((size_t)1 << 28)) return fail(MXMOE_GG_ERR_INVALID, "too many tiles (%d)", (int)T);
  const TileTimer tile_time{v, plan->meta};

  XcdQueues xq;
  for (auto& x : xq.sim) x.slot.assign(v.chunk, 0.0);
  xq.tiles = tl.seq;
  if (!pack_xcds(v, tl, tile_time, o, &xq)) {
    if (o.region == 1) put_regions(tl, tile_time, &xq);
    place_chunks(v, tl, tile_time, o, &xq);
    if (o.region != 1) put_regions(tl, tile_time, &xq);
  }
#ifdef MXMOE_LAB
  const bool plain_v2 = v.kind == Kind::V2 && !v.persistent;
  if (o.tail_split && plain_v2) split_tails(v, tile_time, o.tail_split, &tl.groups, &xq, plan);
  if (o.mix && plain_v2) mix_residency(tile_time, &xq);
#endif
  emit_tiles(xq, plan);
#ifdef MXMOE_LAB
  if (o.lowfill_lpt && plain_v2) lowfill_lpt(v, tile_time, plan);
#endif
  if (v.persistent) emit_persistent(v, xq, tile_time, T > 0, plan);
  return MXMOE_GG_OK;
}

int check_variant(int variant) {
  if (variant < 0 || variant >= (int)variants().size())
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "variant %d not compiled (have %d)", variant, (int)variants().size());
  return MXMOE_GG_OK;
}

// MXMOE_GG_VARIANT_AUTO -> concrete variant from the quant types present (policy above).
int resolve_variant(int variant, const std::vector<HostProblem>& hp, int* out) {
  if (variant != MXMOE_GG_VARIANT_AUTO) {
    *out = variant;
    return check_variant(variant);
  }
  int mask = 0;
  for (const HostProblem& p : hp) {
    int qt;
    if (qtype_of(p.a_bits, p.w_bits, p.gsize, p.sym, p.fmt, &qt) != MXMOE_GG_OK) continue;
    if (p.M > 0 || qinfo(qt).auto_counts_empty) mask |= 1 << qt;
  }
  *out = variant_index(kDefaultVariantName);
  // (weight-only MXFP4 counts as weight-only; beside a w4a4 MXFP4 problem the call keeps v2x, the
  // only variant with that body; w4a8_g32_sym_MXFP8 has a wo3 body)
  constexpr int wo_mask = auto_mask(AutoClass::WeightOnly), small_mask = wo_mask | auto_mask(AutoClass::Small);
  // (fused SiLU calls too: the small-batch kernel's fp16 / w8a8 / w4a4 bodies carry the epilogue)
  if (mask != 0 && (mask & ~small_mask) == 0) {
    // (w8a8 / fp16 problems may ride along: the reference's small-batch w4a16 + w8a8 pairing)
    double wsum = 0, ksum = 0, msum = 0;
    int kmax = 0;
    for (const HostProblem& p : hp) {
      if (p.M <= 0 || p.N <= 0) continue;
      const double w = (double)p.N * p.K;
      wsum += w;
      ksum += w * p.K;
      msum += w * p.M;
      kmax = std::max(kmax, p.K);
    }
    const bool kskew = wsum > 0 && kmax >= 2.0 * ksum / wsum;
    double wo_rows = 0, small_rows = 0;  // the largest limit among the types present, per class
    for (const QTypeInfo& t : kQTypes)
      if (mask & (1 << t.qt)) {
        double& rows = t.weight_only ? wo_rows : small_rows;
        rows = std::max(rows, t.auto_rows);
      }
    const double limit = (mask & wo_mask) ? wo_rows : small_rows * (kskew ? 2.0 : 1.0);
    // weight-only: the 3-WG/CU 64-row kernel while the rows per weight byte are few (small batches:
    // the 64-row tile is bound by its instruction stream and barriers, a second and third resident
    // workgroup fill each other's waits — +15-70 % on the qwen2_moe calls at bs 128-2048,
    // profiles/r03/wo2/); v2x's 256-row tiles at large batch
    if (wsum > 0 && msum / wsum <= limit) {
      const int wi = variant_index(kWoSmallVariant);
      if (!strcmp(variants()[wi].name, kWoSmallVariant)) {
        *out = wi;
        return MXMOE_GG_OK;
      }
    }
  }
  for (const QTypeInfo& t : kQTypes) {
    if (!(mask & (1 << t.qt)) || !t.auto_alone) continue;
    if (t.auto_class == AutoClass::Alone) {  // fp6 images: the fp6 kernel (no other variant reads them)
      if (mask != (1 << t.qt))
        return fail(MXMOE_GG_ERR_UNSUPPORTED,
                    "fp6-image w4a4 problems (MXMOE_GG_FMT_F6) cannot share a call with other quant types: plan them "
                    "as a call of their own");
      *out = variant_index(t.auto_alone);
      return MXMOE_GG_OK;
    }
    if (mask == (1 << t.qt)) {
      // int4-only: the 256x128 2-WG/CU kernel, unless the call is low-fill enough for the v2s plan
      // to split K (that kernel cannot)
      Plan p;
      if (plan_host(hp, *out, false, &p) == MXMOE_GG_OK && p.slabs == p.tail_slabs) *out = variant_index(t.auto_alone);
    }
  }
  return MXMOE_GG_OK;
}

std::vector<HostProblem> to_host(const mxmoe_gg_problem* problems, int problem_count) {
  std::vector<HostProblem> hp(problem_count);
  for (int i = 0; i < problem_count; ++i) {
    const mxmoe_gg_problem& p = problems[i];
    hp[i] = HostProblem{p.A,      p.B,      p.scale_a, p.scale_b, p.C,   p.M,   p.N,  p.K,
                        p.a_bits, p.w_bits, p.gsize,   p.sym,     p.lda, p.ldb, p.ldc, p.fmt};
  }
  return hp;
}

// Host image of the workspace for a plan; pointer columns from `hp` in table-row order.
// The 5 pointer columns (A, B, scale_a, scale_b, C) of the planned problems in table-row order, one after the other.
std::vector<const void*> pointer_columns(const std::vector<int>& order, const std::vector<HostProblem>& hp) {
  std::vector<const void*> cols;
  cols.reserve(5 * order.size());
  for (int c = 0; c < 5; ++c)
    for (int r : order) cols.push_back(c == 0 ? hp[r].A : c == 1 ? hp[r].B : c == 2 ? hp[r].SA : c == 3 ? hp[r].SB : hp[r].C);
  return cols;
}

std::vector<uint8_t> workspace_image(const Plan& plan, const std::vector<const void*>& cols, WsLayout* out) {
  const int P = (int)plan.meta.size();
  const WsLayout l = ws_layout(P, (int)plan.tiles.size(), plan.slabs);
  std::vector<uint8_t> img(l.total - l.slabs, 0);  // counters start at zero; slabs need no init
  memcpy(img.data(), plan.meta.data(), (size_t)P * sizeof(GGMeta));
  for (int c = 0; c < 5; ++c) memcpy(img.data() + l.meta + c * l.ptr, cols.data() + c * P, (size_t)P * sizeof(void*));
  memcpy(img.data() + l.meta + 5 * l.ptr, plan.tiles.data(), plan.tiles.size() * sizeof(TileDesc));
  *out = l;
  return img;
}

// FNV-1a over the plan table and the tile table: equal for two calls with the same shapes, quant
// params and strides (the planner is deterministic), whatever their buffers.
uint64_t plan_signature(const Plan& plan) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  };
  mix(plan.meta.data(), plan.meta.size() * sizeof(GGMeta));
  mix(plan.tiles.data(), plan.tiles.size() * sizeof(TileDesc));
  mix(plan.order.data(), plan.order.size() * sizeof(int));
  return h;
}

void fill_info(const Plan& plan, int variant, const WsLayout& l, void* ws, mxmoe_gg_plan_info* info) {
  const Variant& v = variants()[variant];
  info->variant = variant;
  info->problem_count = (int)plan.meta.size();
  info->total_tiles = plan.total_tiles;
  info->grid = plan.launch_grid;
  info->tile_slots = (int)plan.tiles.size();
  info->reserved = 0;
  info->block = v.threads;
  info->qtype_mask = 0;
  for (const GGMeta& m : plan.meta) {
    info->qtype_mask |= 1 << m.qtype;
    if (qinfo(m.qtype).weight_only && (m.reserved2 & META_SILU)) info->qtype_mask |= kQmaskWoSilu;
  }
  const int build = v.pick(info->qtype_mask);  // (the build mxmoe_gg_launch will run)
  info->lds_bytes = build >= 0 ? v.builds.rows[build].lds_bytes : v.lds_bytes;
  info->splitk_slabs = plan.slabs;
  info->workspace_bytes = (int64_t)l.total;
  info->workspace = ws;
  info->signature = plan_signature(plan);
}

template <class T>
int debug_read(const T& symbol, void* dst, size_t bytes, int reset) {  // mxmoe_gg_debug_*: read / clear a __device__ array
  const size_t n = std::min(bytes, sizeof(T));
  if (dst && n) HIP_TRY(hipMemcpyFromSymbol(dst, symbol, n, 0, hipMemcpyDeviceToHost));
  if (reset) {
    void* p = nullptr;
    HIP_TRY(hipGetSymbolAddress(&p, symbol));
    HIP_TRY(hipMemset(p, 0, sizeof(T)));
    HIP_TRY(hipDeviceSynchronize());
  }
  return MXMOE_GG_OK;
}

}  // namespace

namespace mxmoe {
namespace detail {
// error channel shared with the MoE plumbing (moe_ops.hip)
int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
}  // namespace detail
}  // namespace mxmoe

extern "C" {

int mxmoe_gg_abi_version(void) { return MXMOE_GG_ABI_VERSION; }

const char* mxmoe_gg_last_error(void) { return g_last_error.c_str(); }

int mxmoe_gg_variant_count(void) { return (int)variants().size(); }

int mxmoe_gg_default_variant(void) { return variant_index(kDefaultVariantName); }

int mxmoe_gg_list_variants(char* buf, size_t n) {
  std::string out;
  const auto& vs = variants();
  for (size_t i = 0; i < vs.size(); ++i) {
    char line[2048];
    size_t off = (size_t)snprintf(line, sizeof(line), "%zu %s", i, vs[i].name);
    for (int q = 0; q < QT_COUNT; ++q) {
      const TileGeom& g = vs[i].geom[q];
      if (g.bn == 0) continue;  // quant type not implemented by this variant
      const int bits = qinfo(q).staged_bits;
      const int waves = g.threads / 64;
      const int wm = 2, wn = waves / wm;
      if (off >= sizeof(line) - 1) break;  // (snprintf returns the untruncated length)
      off += (size_t)snprintf(line + off, sizeof(line) - off,
                              " %s=TileConfig(BM=%d, BN=%d, BK=%d, WM=%d, WN=%d, WK=1, STAGE=2)", qinfo(q).name, g.bm, g.bn,
                              g.bkb * 8 / bits, wm, wn);
    }
    out += line;
    out += "\n";
  }
  if (buf && n > 0) {
    size_t c = std::min(n - 1, out.size());
    memcpy(buf, out.data(), c);
    buf[c] = 0;
  }
  return (int)vs.size();
}

int mxmoe_gg_variant_caps(int variant, uint32_t* caps) {
  if (!caps) return fail(MXMOE_GG_ERR_INVALID, "caps is NULL");
  if (int st = check_variant(variant)) return st;
  *caps = has_silu_epilogue(variants()[variant]) ? MXMOE_GG_CAP_SILU_MUL : 0u;
  return MXMOE_GG_OK;
}

int mxmoe_gg_variant_tile(int variant, int a_bits, int w_bits, int32_t* bm, int32_t* bn, int32_t* bk_bytes,
                          int32_t* threads) {
  int st = check_variant(variant);
  if (st) return st;
  int qt = 0;
  st = qtype_of(a_bits, w_bits, -1, 1, MXMOE_GG_FMT_DEFAULT, &qt);
  if (st) return st;
  const TileGeom& g = variants()[variant].geom[qt];
  if (bm) *bm = g.bm;
  if (bn) *bn = g.bn;
  if (bk_bytes) *bk_bytes = g.bkb;
  if (threads) *threads = g.threads;
  return MXMOE_GG_OK;
}

#ifdef MXMOE_LAB
// lab-only exports (tools/f6_bench.py, tests/test_f6.py): int4 rows -> fp6 images (gg_f6.h layout)
namespace {
int f6_args(const void* src, int rows, int K, int64_t ld_src, const void* dst, int64_t ld_dst, int64_t* ls, int64_t* ld) {
  if (rows < 0 || K < 0 || (rows > 0 && (!src || !dst))) return fail(MXMOE_GG_ERR_INVALID, "pack_f6: bad arguments");
  if (K % 32) return fail(MXMOE_GG_ERR_INVALID, "pack_f6: K=%d must be a multiple of 32 (16-B int4 rows)", K);
  *ls = ld_src ? ld_src * 2 : K / 2;
  *ld = ld_dst ? ld_dst * 2 : MXMOE_GG_F6_ROW_BYTES(K);
  if (*ls < K / 2 || *ld < MXMOE_GG_F6_ROW_BYTES(K) || (*ls % 16) || (*ld % 16))
    return fail(MXMOE_GG_ERR_INVALID, "pack_f6: row strides must cover the row and be multiples of 8 words");
  if (rows > 0 && (((uintptr_t)src | (uintptr_t)dst) & 15))
    return fail(MXMOE_GG_ERR_INVALID, "pack_f6: buffers must be 16-B aligned");
  return MXMOE_GG_OK;
}
}  // namespace

int mxmoe_gg_pack_f6(const void* src, int rows, int K, int64_t ld_src, void* dst, int64_t ld_dst, void* stream) {
  int64_t ls, ld;
  int st = f6_args(src, rows, K, ld_src, dst, ld_dst, &ls, &ld);
  if (st) return st;
  const int64_t threads = (int64_t)rows * ((K + 127) / 128) * 4;
  if (threads == 0) return MXMOE_GG_OK;
  hipLaunchKernelGGL(f6_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const uint8_t*>(src), ls, static_cast<uint8_t*>(dst), ld, rows, K);
  HIP_TRY(hipGetLastError());
  return MXMOE_GG_OK;
}

int mxmoe_gg_pack_f6_host(const void* src, int rows, int K, int64_t ld_src, void* dst, int64_t ld_dst) {
  int64_t ls, ld;
  int st = f6_args(src, rows, K, ld_src, dst, ld_dst, &ls, &ld);
  if (st) return st;
  const int nblk = (K + 127) / 128;
  for (int64_t r = 0; r < rows; ++r)
    for (int b = 0; b < nblk; ++b)
      for (int g = 0; g < 4; ++g) {
        const int e0 = b * 128 + g * 32;
        uint32_t w[4] = {0, 0, 0, 0};
        if (e0 < K) memcpy(w, static_cast<const uint8_t*>(src) + r * ls + e0 / 2, 16);  // (K % 32 == 0)
        uint32_t d[6];
        f6_pack32(w, d);
        uint8_t* o = static_cast<uint8_t*>(dst) + r * ld + b * 96;
        memcpy(o + g * 16, d, 16);
        memcpy(o + 64 + g * 8, d + 4, 8);
      }
  return MXMOE_GG_OK;
}
#endif  // MXMOE_LAB

int mxmoe_gg_resolve_variant(const mxmoe_gg_problem* problems, int problem_count, int variant, int* out) {
  if (!out) return fail(MXMOE_GG_ERR_INVALID, "out is NULL");
  if (problem_count < 0 || (problem_count > 0 && !problems))
    return fail(MXMOE_GG_ERR_INVALID, "bad problem array (count %d)", problem_count);
  return resolve_variant(variant, to_host(problems, problem_count), out);
}

int mxmoe_gg_workspace_size(const mxmoe_gg_problem* problems, int problem_count, int variant, size_t* bytes) {
  if (problem_count < 0 || (problem_count > 0 && !problems) || !bytes)
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to mxmoe_gg_workspace_size");
  const std::vector<HostProblem> hp = to_host(problems, problem_count);
  int st = resolve_variant(variant, hp, &variant);
  if (st) return st;
  Plan plan;
  st = plan_host(hp, variant, false, &plan);
  if (st) return st;
  *bytes = ws_layout((int)plan.meta.size(), (int)plan.tiles.size(), plan.slabs).total;
  return MXMOE_GG_OK;
}

int mxmoe_gg_plan_tiles(const mxmoe_gg_problem* problems, int problem_count, int variant, int32_t* tiles,
                        int32_t* rows, int* slots) {
  if (problem_count < 0 || (problem_count > 0 && !problems) || !slots || *slots < 0 || (*slots > 0 && !tiles))
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to mxmoe_gg_plan_tiles");
  const std::vector<HostProblem> hp = to_host(problems, problem_count);
  int st = resolve_variant(variant, hp, &variant);
  if (st) return st;
  Plan plan;
  st = plan_host(hp, variant, false, &plan);
  if (st) return st;
  const int n = std::min(*slots, (int)plan.tiles.size());
  if (n > 0) memcpy(tiles, plan.tiles.data(), (size_t)n * sizeof(TileDesc));
  if (rows)
    for (size_t r = 0; r < plan.order.size(); ++r) rows[r] = plan.order[r];
  *slots = (int)plan.tiles.size();
  return MXMOE_GG_OK;
}

// What mxmoe_gg_rebind needs of a plan to skip the host planner: per workspace, a key over
// everything plan_host reads except the pointers, the plan's signature and its table-row order.
// A later mxmoe_gg_plan into the same workspace replaces the entry.
struct RebindEntry {
  uint64_t key = 0, signature = 0;
  std::vector<int> order;
};
static std::mutex g_rebind_mu;
static std::unordered_map<const void*, RebindEntry> g_rebind;
static uint64_t rebind_key(const std::vector<HostProblem>& hp, int variant) {
  uint64_t h = 1469598103934665603ull ^ (uint64_t)variant;
  auto mix = [&](int64_t v) {
    h ^= (uint64_t)v;
    h *= 1099511628211ull;
  };
  mix((int64_t)hp.size());
  for (const HostProblem& p : hp)
    for (int64_t v : {(int64_t)p.M, (int64_t)p.N, (int64_t)p.K, (int64_t)p.a_bits, (int64_t)p.w_bits, (int64_t)p.gsize,
                      (int64_t)p.sym, (int64_t)p.fmt, p.lda, p.ldb, p.ldc})
      mix(v);
  return h;
}
// Invariant: every plan written into a workspace goes through mxmoe_gg_plan, which calls
// remember_plan and so replaces the workspace's entry. An entry outlives its workspace only as a
// stale key: a new workspace at the same address is planned (and re-remembered) before any rebind,
// and mxmoe_gg_forget_workspace drops the entry when the caller frees the buffer.
static void remember_plan(const void* ws, const std::vector<HostProblem>& hp, int variant, const Plan& plan) {
  std::lock_guard<std::mutex> lk(g_rebind_mu);
  if (g_rebind.size() >= 1024 && !g_rebind.count(ws)) g_rebind.clear();
  RebindEntry& e = g_rebind[ws];
  e.key = rebind_key(hp, variant);
  e.signature = plan_signature(plan);
  e.order = plan.order;
}

int mxmoe_gg_plan(const mxmoe_gg_problem* problems, int problem_count, int variant, void* workspace,
                  size_t workspace_bytes, void* stream, mxmoe_gg_plan_info* info) {
  if (problem_count < 0 || (problem_count > 0 && !problems) || !info)
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to mxmoe_gg_plan");
  const std::vector<HostProblem> hp = to_host(problems, problem_count);
  int st = resolve_variant(variant, hp, &variant);
  if (st) return st;
  Plan plan;
  st = plan_host(hp, variant, true, &plan);
  if (st) return st;
  std::vector<const void*> cols = pointer_columns(plan.order, hp);
  WsLayout l;
  std::vector<uint8_t> img = workspace_image(plan, cols, &l);
  if (!workspace || workspace_bytes < l.total)
    return fail(MXMOE_GG_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", l.total, workspace_bytes);
  HIP_TRY(hipMemcpyAsync(workspace, img.data(), img.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // pageable host image must outlive the copy
  fill_info(plan, variant, l, workspace, info);
  remember_plan(workspace, hp, variant, plan);
  return MXMOE_GG_OK;
}

int mxmoe_gg_forget_workspace(const void* workspace) {
  std::lock_guard<std::mutex> lk(g_rebind_mu);
  g_rebind.erase(workspace);
  return MXMOE_GG_OK;
}

int mxmoe_gg_rebind(const mxmoe_gg_problem* problems, int problem_count, const mxmoe_gg_plan_info* info,
                    void* stream) {
  if (problem_count < 0 || (problem_count > 0 && !problems) || !info || !info->workspace)
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to mxmoe_gg_rebind");
  int st = check_variant(info->variant);
  if (st) return st;
  const std::vector<HostProblem> hp = to_host(problems, problem_count);
  // fast path: the same shapes / quant params / strides as this workspace's plan -> only the
  // pointers are checked (build_meta's NULL / alignment checks), the tile planner is skipped
  // (only a real key + signature hit takes it: an all-empty plan has an empty order too, and rebinding
  // it with non-empty problems must go through the planner and fail the signature check)
  std::vector<int> order;
  bool hit = false;
  {
    const uint64_t key = rebind_key(hp, info->variant);
    std::lock_guard<std::mutex> lk(g_rebind_mu);
    auto it = g_rebind.find(info->workspace);
    if (it != g_rebind.end() && it->second.key == key && it->second.signature == info->signature) {
      order = it->second.order;
      hit = true;
    }
  }
  if (hit) {
    const Variant& v = variants()[info->variant];
    for (int i = 0; i < (int)hp.size(); ++i) {
      GGMeta m;
      st = build_meta(hp[i], i, v, true, &m);
      if (st) return st;
    }
  } else {
    Plan plan;
    st = plan_host(hp, info->variant, true, &plan);
    if (st) return st;
    if (plan_signature(plan) != info->signature || (int)plan.meta.size() != info->problem_count)
      return fail(MXMOE_GG_ERR_INVALID, "mxmoe_gg_rebind: problems differ from the planned call (shapes, quant "
                                        "params or strides); plan again");
    order = plan.order;
  }
  if ((int)order.size() != info->problem_count)
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_gg_rebind: problems differ from the planned call; plan again");
  const WsLayout l = ws_layout(info->problem_count, info->tile_slots, info->splitk_slabs);
  const std::vector<const void*> ptrs = pointer_columns(order, hp);
  std::vector<uint8_t> cols(5 * l.ptr, 0);
  for (int c = 0; c < 5; ++c) memcpy(cols.data() + c * l.ptr, ptrs.data() + c * order.size(), order.size() * sizeof(void*));
  HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(info->workspace) + l.meta, cols.data(), cols.size(),
                         hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // pageable host columns must outlive the copy
  return MXMOE_GG_OK;
}

int mxmoe_gg_launch(const mxmoe_gg_plan_info* info, void* stream) {
  if (!info) return fail(MXMOE_GG_ERR_INVALID, "NULL plan");
  int st = check_variant(info->variant);
  if (st) return st;
  if (info->total_tiles == 0) return MXMOE_GG_OK;
  const int P = info->problem_count;
  const WsLayout l = ws_layout(P, info->tile_slots, info->splitk_slabs);
  const uint8_t* ws = static_cast<const uint8_t*>(info->workspace);
  GGArgs a;
  a.meta = reinterpret_cast<const GGMeta*>(ws);
  a.tiles = reinterpret_cast<const TileDesc*>(ws + l.meta + 5 * l.ptr);
  a.ptr_A = reinterpret_cast<const void* const*>(ws + l.meta);
  a.ptr_B = reinterpret_cast<const void* const*>(ws + l.meta + l.ptr);
  a.ptr_SA = reinterpret_cast<const void* const*>(ws + l.meta + 2 * l.ptr);
  a.ptr_SB = reinterpret_cast<const void* const*>(ws + l.meta + 3 * l.ptr);
  a.ptr_C = reinterpret_cast<void* const*>(ws + l.meta + 4 * l.ptr);
  a.P = P;
  a.n_slots = info->grid;
  a.counters = reinterpret_cast<int32_t*>(const_cast<uint8_t*>(ws) + l.meta + 5 * l.ptr + l.tiles);
  a.slabs = const_cast<uint8_t*>(ws) + l.meta + 5 * l.ptr + l.tiles + l.counters;
  const Variant& v = variants()[info->variant];
  const int build = v.pick(info->qtype_mask);
  if (build < 0) {  // (the lab libraries compile a few quant-type sets per kernel only)
    fprintf(stderr, "libmxmoe_gg: variant %s: quant-type mix %#x not compiled\n", v.name, info->qtype_mask);
    abort();
  }
  v.builds.rows[build].launch(a, info->grid, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return MXMOE_GG_OK;
}

int mxmoe_gg_run(const mxmoe_gg_problem* problems, int problem_count, int variant, void* workspace,
                 size_t workspace_bytes, void* stream) {
  mxmoe_gg_plan_info info;
  int st = mxmoe_gg_plan(problems, problem_count, variant, workspace, workspace_bytes, stream, &info);
  if (st) return st;
  return mxmoe_gg_launch(&info, stream);
}

// ---- Device planning (include/mxmoe_gg.h, gg_dyn.h): the static half of a fixed-capacity plan.
// Workspace: the planned layout (plan table | 5 pointer columns | tile table, no split-K areas), then the
// dynamic plan's own data: geometry rows | table order | per-workgroup scratch (rows, tile prefix) | status.
namespace {
constexpr int32_t kDynMagic = 0x44594E;  // mxmoe_gg_plan_info::reserved of a dynamic plan
static_assert(sizeof(GGMeta) == kDynMetaWords * 4 && offsetof(GGMeta, M) == kDynMetaM * 4 &&
                  offsetof(GGMeta, tile_begin) == kDynMetaTileBegin * 4 && sizeof(TileDesc) == kDynTileWords * 4 &&
                  offsetof(TileDesc, ks1) == 20 && offsetof(TileDesc, grp) == 28,
              "gg_dyn.h writes GGMeta / TileDesc by their raw layout");
static_assert(sizeof(mxmoe_gg_dyn_row) == sizeof(DynRow) && offsetof(mxmoe_gg_dyn_row, c_off) == offsetof(DynRow, c_off),
              "mxmoe_gg_dyn_row is DynRow");
struct DynLayout {
  size_t geom, order, rows, cum, status, total;
};
DynLayout dyn_layout(int P, int slots) {
  DynLayout d;
  const size_t p = (size_t)std::max(P, 1);
  size_t o = align_up(ws_layout(P, slots, 0).total, 256);
  d.geom = o, o += align_up(p * sizeof(DynGeom), 256);
  d.order = o, o += align_up(p * sizeof(int32_t), 256);
  d.rows = o, o += align_up(kDynMaxBlocks * p * sizeof(int32_t), 256);
  d.cum = o, o += align_up(kDynMaxBlocks * (p + 1) * sizeof(int32_t), 256);
  d.status = o, o += 256;
  d.total = o;
  return d;
}
struct DynPlan {
  int variant = 0;
  std::vector<GGMeta> meta;    // row i = the caller's problem i (M and tile_begin are the device planner's)
  std::vector<DynGeom> geom;
  std::vector<int32_t> order;  // tile-table order: problem indices, longest K stages first
  int64_t rows_total = 0;
  int slots = 0;
  int qtype_mask = 0;
};
// bytes of one row's activation scales (0: the type has none)
int64_t sa_row_bytes(int qt, int K) {
  const QTypeInfo& t = qinfo(qt);
  if (t.weight_only || t.float16) return 0;
  if (t.dword_scales) return 16 * (((int64_t)K / 32 + 15) / 16);  // e8m0 bytes, the device layout
  if (t.group_fold) return 2 * ((int64_t)K / t.k_mult);
  return 2;
}
bool dyn_variant_ok(const Variant& v) {
  if (v.persistent || (v.kind != Kind::V2 && v.kind != Kind::V3)) return false;
  return !strcmp(v.name, kDefaultVariantName) || !strcmp(v.name, kInt4Variant) || !strcmp(v.name, kWoSmallVariant);
}
int plan_dynamic_host(const mxmoe_gg_problem* problems, int P, int variant, const int32_t* joint_idx, int n_joint,
                      int64_t rows_total, const mxmoe_gg_dyn_extent* extents, bool check_ptrs, DynPlan* out) {
  if (P < 0 || (P > 0 && !problems) || n_joint < 0 || n_joint > P || (n_joint > 0 && !joint_idx) || rows_total < 0 ||
      rows_total > INT32_MAX)
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to the dynamic plan (problems %d, joint %d, rows_total %lld)", P,
                n_joint, (long long)rows_total);
  std::vector<char> joint(P, 0);
  for (int j = 0; j < n_joint; ++j) {
    if (joint_idx[j] < 0 || joint_idx[j] >= P || joint[joint_idx[j]])
      return fail(MXMOE_GG_ERR_INVALID, "joint_idx[%d] = %d is out of range or listed twice", j, joint_idx[j]);
    joint[joint_idx[j]] = 1;
  }
  const std::vector<HostProblem> hp = to_host(problems, P);
  std::vector<HostProblem> balanced = hp;  // what AUTO sees: the joint rows spread evenly
  const int64_t share = n_joint ? (rows_total + n_joint - 1) / n_joint : 0;
  for (int i = 0; i < P; ++i)
    if (joint[i]) balanced[i].M = (int)std::min<int64_t>(hp[i].M, share);
  int st = resolve_variant(variant, balanced, &variant);
  if (st) return st;
  const Variant& v = variants()[variant];
  if (!dyn_variant_ok(v))
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "variant %s has no dynamic plan (v2x, v3 and wo3 only)", v.name);
  out->variant = variant;
  out->rows_total = rows_total;
  out->meta.assign(P, GGMeta{});
  out->geom.assign(P, DynGeom{});
  out->qtype_mask = 0;
  std::vector<double> cost(P, 0.0);
  for (int i = 0; i < P; ++i) {
    GGMeta& m = out->meta[i];
    if ((st = build_meta(hp[i], i, v, check_ptrs, &m))) return st;
    const QTypeInfo& t = qinfo(m.qtype);
    const TileGeom& tg = v.geom[m.qtype];
    DynGeom& g = out->geom[i];
    g.cap = hp[i].M;
    g.bm = tg.bm, g.bn = tg.bn;
    g.tail_bm = v.tail_bm;  // (m_tiles' rule; dyn_variant_ok leaves no V0 kernel)
    g.tail2_bm = t.small_class ? v.tail2_bm : 0;
    g.tiles_n = m.tiles_n;
    g.nst = stages_of(v, m);
    g.joint = joint[i];
    g.a_row = m.lda_b, g.sa_row = sa_row_bytes(m.qtype, hp[i].K), g.c_row = m.ldc * 2;
    g.a_bytes = extents ? extents[i].a_bytes : g.cap * g.a_row;
    g.sa_bytes = extents ? extents[i].sa_bytes : g.cap * g.sa_row;
    g.c_bytes = extents ? extents[i].c_bytes : g.cap * g.c_row;
    if (g.a_bytes < 0 || g.sa_bytes < 0 || g.c_bytes < 0) return fail(MXMOE_GG_ERR_INVALID, "problem %d: negative extent", i);
    g.base_a = (uint64_t)(uintptr_t)hp[i].A, g.base_sa = (uint64_t)(uintptr_t)hp[i].SA, g.base_c = (uint64_t)(uintptr_t)hp[i].C;
    g.sa_align = t.dword_scales ? 4 : 2;
    cost[i] = stage_time(v, m, 0) * g.nst;
    out->qtype_mask |= 1 << m.qtype;
    if (t.weight_only && (m.reserved2 & META_SILU)) out->qtype_mask |= kQmaskWoSilu;
    m.M = 0;  // the device planner's columns
    m.tile_begin = 0;
  }
  if (P > 0 && v.pick(out->qtype_mask) < 0)
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "variant %s: quant-type mix %#x not compiled", v.name, out->qtype_mask);
  out->order.resize(P);
  for (int i = 0; i < P; ++i) out->order[i] = i;
  std::stable_sort(out->order.begin(), out->order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
  std::vector<int32_t> scratch(std::max(P, 1));
  const int64_t slots = dyn_capacity_slots(out->geom.data(), P, rows_total, scratch.data());
  if (slots > ((int64_t)1 << 28)) return fail(MXMOE_GG_ERR_INVALID, "too many tile slots (%lld)", (long long)slots);
  out->slots = (int)slots;
  return MXMOE_GG_OK;
}
}  // namespace

int mxmoe_gg_dynamic_workspace_size(const mxmoe_gg_problem* problems, int problem_count, int variant,
                                    const int32_t* joint_idx, int n_joint, int64_t rows_total, size_t* bytes) {
  if (!bytes) return fail(MXMOE_GG_ERR_INVALID, "bytes is NULL");
  DynPlan plan;
  if (int st = plan_dynamic_host(problems, problem_count, variant, joint_idx, n_joint, rows_total, nullptr, false, &plan))
    return st;
  *bytes = dyn_layout(problem_count, plan.slots).total;
  return MXMOE_GG_OK;
}

int mxmoe_gg_plan_dynamic(const mxmoe_gg_problem* problems, int problem_count, int variant, const int32_t* joint_idx,
                          int n_joint, int64_t rows_total, const mxmoe_gg_dyn_extent* extents, void* workspace,
                          size_t workspace_bytes, void* stream, mxmoe_gg_plan_info* info) {
  if (!info) return fail(MXMOE_GG_ERR_INVALID, "bad arguments to mxmoe_gg_plan_dynamic");
  DynPlan plan;
  if (int st = plan_dynamic_host(problems, problem_count, variant, joint_idx, n_joint, rows_total, extents, true, &plan))
    return st;
  const int P = problem_count;
  const WsLayout l = ws_layout(P, plan.slots, 0);
  const DynLayout d = dyn_layout(P, plan.slots);
  if (!workspace || workspace_bytes < d.total)
    return fail(MXMOE_GG_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", d.total, workspace_bytes);
  std::vector<uint8_t> img(d.total, 0);  // (scratch and status start at zero)
  if (P > 0) memcpy(img.data(), plan.meta.data(), (size_t)P * sizeof(GGMeta));
  for (int i = 0; i < P; ++i) {  // the static columns (B, scale_b) and, until the first launch, the base pointers
    const mxmoe_gg_problem& p = problems[i];
    const void* cols[5] = {p.A, p.B, p.scale_a, p.scale_b, p.C};
    for (int c = 0; c < 5; ++c) memcpy(img.data() + l.meta + c * l.ptr + (size_t)i * sizeof(void*), &cols[c], sizeof(void*));
  }
  TileDesc* tiles = reinterpret_cast<TileDesc*>(img.data() + l.meta + 5 * l.ptr);
  for (int s = 0; s < plan.slots; ++s) tiles[s] = kEmptySlot;
  if (P > 0) {
    memcpy(img.data() + d.geom, plan.geom.data(), (size_t)P * sizeof(DynGeom));
    memcpy(img.data() + d.order, plan.order.data(), (size_t)P * sizeof(int32_t));
  }
  memcpy(img.data() + d.status + 8, &plan.rows_total, sizeof(int64_t));
  HIP_TRY(hipMemcpyAsync(workspace, img.data(), img.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // pageable host image must outlive the copy
  mxmoe_gg_forget_workspace(workspace);                // (a dynamic plan is never rebound)
  const Variant& v = variants()[plan.variant];
  info->variant = plan.variant;
  info->problem_count = P;
  info->total_tiles = info->grid = info->tile_slots = plan.slots;
  info->block = v.threads;
  info->qtype_mask = plan.qtype_mask;
  const int build = P > 0 ? v.pick(plan.qtype_mask) : -1;
  info->lds_bytes = build >= 0 ? v.builds.rows[build].lds_bytes : v.lds_bytes;
  info->splitk_slabs = 0;
  info->workspace_bytes = (int64_t)d.total;
  info->workspace = workspace;
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < d.status && i < img.size(); ++i) h = (h ^ img[i]) * 1099511628211ull;
  info->signature = h;
  info->reserved = kDynMagic;
  return MXMOE_GG_OK;
}

int mxmoe_gg_launch_dynamic(const mxmoe_gg_plan_info* info, const mxmoe_gg_dyn_row* dyn, void* stream) {
  if (!info || info->reserved != kDynMagic || !info->workspace || info->problem_count < 0 || info->tile_slots < 0)
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_gg_launch_dynamic: not a plan of mxmoe_gg_plan_dynamic");
  if (int st = check_variant(info->variant)) return st;
  const int P = info->problem_count, slots = info->tile_slots;
  if (P == 0 || slots == 0) return MXMOE_GG_OK;
  if (!dyn || ((uintptr_t)dyn & 7)) return fail(MXMOE_GG_ERR_INVALID, "mxmoe_gg_launch_dynamic: NULL or misaligned row table");
  const WsLayout l = ws_layout(P, slots, 0);
  const DynLayout d = dyn_layout(P, slots);
  uint8_t* ws = static_cast<uint8_t*>(info->workspace);
  DynArgs a;
  a.geom = reinterpret_cast<const DynGeom*>(ws + d.geom);
  a.order = reinterpret_cast<const int32_t*>(ws + d.order);
  a.rows = reinterpret_cast<int32_t*>(ws + d.rows);
  a.cum = reinterpret_cast<int32_t*>(ws + d.cum);
  a.status = reinterpret_cast<int32_t*>(ws + d.status);
  a.meta = reinterpret_cast<int32_t*>(ws);
  a.ptr_A = reinterpret_cast<const void**>(ws + l.meta);
  a.ptr_SA = reinterpret_cast<const void**>(ws + l.meta + 2 * l.ptr);
  a.ptr_C = reinterpret_cast<void**>(ws + l.meta + 4 * l.ptr);
  a.tiles = reinterpret_cast<int32_t*>(ws + l.meta + 5 * l.ptr);
  a.dyn = reinterpret_cast<const DynRow*>(dyn);
  a.rows_total = reinterpret_cast<const int64_t*>(ws + d.status + 8);  // (static plan data, beside the status word)
  a.P = P, a.tile_slots = slots;
  detail::launch_dyn_plan(a, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return mxmoe_gg_launch(info, stream);
}

int mxmoe_gg_dynamic_status(const mxmoe_gg_plan_info* info, void* stream, int32_t* status, int reset) {
  if (!info || info->reserved != kDynMagic || !info->workspace || !status)
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_gg_dynamic_status: not a plan of mxmoe_gg_plan_dynamic");
  void* word = static_cast<uint8_t*>(info->workspace) + dyn_layout(info->problem_count, info->tile_slots).status;
  HIP_TRY(hipMemcpyAsync(status, word, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  if (reset) HIP_TRY(hipMemsetAsync(word, 0, sizeof(int32_t), (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return MXMOE_GG_OK;
}

int mxmoe_gg_dynamic_tiles(const mxmoe_gg_problem* problems, int problem_count, int variant, const int32_t* joint_idx,
                           int n_joint, int64_t rows_total, const mxmoe_gg_dyn_extent* extents,
                           const mxmoe_gg_dyn_row* dyn, int slot_limit, int32_t* tiles, int32_t* planned_rows,
                           int* slots, int32_t* status) {
  if (!slots || *slots < 0 || (*slots > 0 && !tiles) || (problem_count > 0 && !dyn))
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to mxmoe_gg_dynamic_tiles");
  DynPlan plan;
  if (int st = plan_dynamic_host(problems, problem_count, variant, joint_idx, n_joint, rows_total, extents, false, &plan))
    return st;
  const int P = problem_count, tile_slots = slot_limit > 0 ? slot_limit : plan.slots;
  std::vector<int32_t> rows(std::max(P, 1)), cum(P + 1);
  const int32_t st = dyn_plan_rows(plan.geom.data(), plan.order.data(), P, rows_total, tile_slots,
                                   reinterpret_cast<const DynRow*>(dyn), rows.data(), cum.data());
  const int n = std::min(*slots, tile_slots);
  for (int s = 0; s < n; ++s) dyn_tile_at(plan.geom.data(), plan.order.data(), P, rows.data(), cum.data(), s, tiles + 8 * (size_t)s);
  if (planned_rows)
    for (int i = 0; i < P; ++i) planned_rows[i] = rows[i];
  if (status) *status = st;
  *slots = tile_slots;
  return MXMOE_GG_OK;
}

// Reference-compatible entry point (registry.cuh:28-39): device pointer arrays, host copies of
// the sizes and QParams, legacy default stream, per-call planning (as the reference host API).
// Per-device resources of the reference-ABI shim (the only entry that allocates): a device
// workspace grown on demand and a pinned host staging buffer for the pointer gather and the
// workspace image. Keyed by the calling thread's current device; one mutex per process guards the
// table and serialises shim calls (the reference's host API is not reentrant either, it runs
// cudaMalloc / cudaMemcpy / cudaFree on the legacy stream every call, kernel_sketch.py:102-143).
namespace {
struct ShimDev {
  void* ws = nullptr;
  size_t ws_cap = 0;
  uint8_t* pinned = nullptr;
  size_t pin_cap = 0;
  // plan cache: the last call's shapes / quant params (key), its plan, and the pointer columns the
  // workspace holds. A call with the same key skips planning and the tile-table upload (a caller
  // runs the same layer shapes call after call); new pointers re-upload the columns only.
  bool cached = false;
  std::vector<int64_t> key;
  Plan plan;
  int variant = -1;
  WsLayout layout{};
  std::vector<const void*> cols;  // 5 x P, plan order, as in the workspace
};
std::mutex g_shim_mu;
std::vector<ShimDev> g_shim;  // indexed by device ordinal

int shim_grow(ShimDev& d, size_t ws_bytes, size_t pin_bytes) {
  if ((d.ws_cap < ws_bytes && d.ws) || (d.pin_cap < pin_bytes && d.pinned))
    HIP_TRY(hipStreamSynchronize(nullptr));  // a previous shim copy / launch may still use the old buffer
  if (d.ws_cap < ws_bytes) {
    if (d.ws) HIP_TRY(hipFree(d.ws));
    d.ws = nullptr;
    d.ws_cap = 0;
    HIP_TRY(hipMalloc(&d.ws, ws_bytes));
    d.ws_cap = ws_bytes;
  }
  if (d.pin_cap < pin_bytes) {
    if (d.pinned) HIP_TRY(hipHostFree(d.pinned));
    d.pinned = nullptr;
    d.pin_cap = 0;
    HIP_TRY(hipHostMalloc((void**)&d.pinned, pin_bytes, hipHostMallocDefault));
    d.pin_cap = pin_bytes;
  }
  return MXMOE_GG_OK;
}
}  // namespace

int mxmoe_gg_release_shim_workspaces(void) {
  std::lock_guard<std::mutex> lk(g_shim_mu);
  int dev0 = 0;
  HIP_TRY(hipGetDevice(&dev0));
  for (size_t i = 0; i < g_shim.size(); ++i) {
    ShimDev& d = g_shim[i];
    if (!d.ws && !d.pinned) continue;
    HIP_TRY(hipSetDevice((int)i));
    HIP_TRY(hipDeviceSynchronize());  // the last shim launch on this device may still read the workspace
    if (d.ws) HIP_TRY(hipFree(d.ws));
    if (d.pinned) HIP_TRY(hipHostFree(d.pinned));
    d = ShimDev{};
  }
  HIP_TRY(hipSetDevice(dev0));
  return MXMOE_GG_OK;
}

int groupgemm_mxmoe(void** ptr_As, void** ptr_Bs, void** ptr_scale_a, void** ptr_scale_b, void** ptr_Cs,
                    void** ptr_Ds, int64_t* ldas, int64_t* ldbs, int64_t* ldcs, int64_t* ldds,
                    mxmoe_dim3* problem_sizes, mxmoe_dim3* h_problem_sizes, mxmoe_qparams* qbits_list,
                    mxmoe_qparams* h_qbits_list, int problem_count) {
  return groupgemm_mxmoe_fmt(ptr_As, ptr_Bs, ptr_scale_a, ptr_scale_b, ptr_Cs, ptr_Ds, ldas, ldbs, ldcs, ldds,
                             problem_sizes, h_problem_sizes, qbits_list, h_qbits_list, problem_count, nullptr);
}

int groupgemm_mxmoe_fmt(void** ptr_As, void** ptr_Bs, void** ptr_scale_a, void** ptr_scale_b, void** ptr_Cs,
                        void** ptr_Ds, int64_t* ldas, int64_t* ldbs, int64_t* ldcs, int64_t* ldds,
                        mxmoe_dim3* problem_sizes, mxmoe_dim3* h_problem_sizes, mxmoe_qparams* qbits_list,
                        mxmoe_qparams* h_qbits_list, int problem_count, const int32_t* h_fmts) {
  (void)ptr_Ds;
  (void)ldas;
  (void)ldbs;
  (void)ldcs;
  (void)ldds;
  (void)problem_sizes;
  (void)qbits_list;
  if (problem_count < 0 || !h_problem_sizes || !h_qbits_list)
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to groupgemm_mxmoe");
  if (problem_count == 0) return MXMOE_GG_OK;
  void** src[5] = {ptr_As, ptr_Bs, ptr_scale_a, ptr_scale_b, ptr_Cs};
  for (int c = 0; c < 5; ++c)
    if (!src[c]) return fail(MXMOE_GG_ERR_INVALID, "groupgemm_mxmoe: NULL device pointer array");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_shim_mu);
  if ((int)g_shim.size() <= dev) g_shim.resize(dev + 1);
  ShimDev& d = g_shim[dev];
  // 1. gather the caller's device pointer arrays: 5 async copies into pinned memory, ONE sync (the
  //    reference pays one blocking cudaMemcpy per call, kernel_sketch.py:102-104)
  const size_t col = (size_t)problem_count * sizeof(void*);
  int st = shim_grow(d, 0, 5 * col);
  if (st) return st;
  for (int c = 0; c < 5; ++c)
    HIP_TRY(hipMemcpyAsync(d.pinned + c * col, src[c], col, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  void* const* h = reinterpret_cast<void* const*>(d.pinned);
  std::vector<HostProblem> hp(problem_count);
  for (int i = 0; i < problem_count; ++i)
    hp[i] = HostProblem{h[0 * problem_count + i], h[1 * problem_count + i], h[2 * problem_count + i],
                        h[3 * problem_count + i], h[4 * problem_count + i], (int)h_problem_sizes[i].x,
                        (int)h_problem_sizes[i].y, (int)h_problem_sizes[i].z, h_qbits_list[i].a_bits,
                        h_qbits_list[i].w_bits, h_qbits_list[i].gsize, h_qbits_list[i].sym, 0, 0, 0,
                        h_fmts ? (int)h_fmts[i] : (int)MXMOE_GG_FMT_DEFAULT};  // never QParams' padding
  // 2. same shapes as the last call on this device: reuse its plan (the pointers still get the same
  //    NULL / alignment checks as mxmoe_gg_plan)
  std::vector<int64_t> key;
  key.reserve((size_t)problem_count * 8);
  for (const HostProblem& p : hp)
    key.insert(key.end(), {p.M, p.N, p.K, p.a_bits, p.w_bits, p.gsize, p.sym, p.fmt});
  if (d.cached && key == d.key) {
    const Variant& v = variants()[d.variant];
    for (int r : d.plan.order) {
      GGMeta m;
      st = build_meta(hp[r], r, v, true, &m);
      if (st) return st;
    }
    std::vector<const void*> cols = pointer_columns(d.plan.order, hp);
    if (cols != d.cols) {  // new buffers, same shapes: upload the 5 pointer columns only
      const size_t P = d.plan.order.size();
      std::memset(d.pinned, 0, 5 * d.layout.ptr);
      for (int c = 0; c < 5; ++c) memcpy(d.pinned + c * d.layout.ptr, cols.data() + c * P, P * sizeof(void*));
      HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(d.ws) + d.layout.meta, d.pinned, 5 * d.layout.ptr,
                             hipMemcpyHostToDevice, nullptr));
      d.cols = std::move(cols);
    }
    mxmoe_gg_plan_info info;
    fill_info(d.plan, d.variant, d.layout, d.ws, &info);
    return mxmoe_gg_launch(&info, nullptr);
  }
  d.cached = false;
  // 3. plan with the same NULL / alignment checks as mxmoe_gg_plan (a bad pointer is an error code,
  //    never a fault inside the LDS-DMA kernel)
  int variant;
  st = resolve_variant(MXMOE_GG_VARIANT_AUTO, hp, &variant);
  if (st) return st;
  Plan plan;
  st = plan_host(hp, variant, true, &plan);
  if (st) return st;
  if (plan.total_tiles == 0) return MXMOE_GG_OK;
  std::vector<const void*> cols = pointer_columns(plan.order, hp);
  WsLayout l;
  std::vector<uint8_t> img = workspace_image(plan, cols, &l);
  // 4. upload from pinned memory and launch, both on the legacy stream, no further host sync: the
  //    next shim call on this device synchronises that stream before it rewrites either buffer
  st = shim_grow(d, l.total, std::max(std::max(5 * col, img.size()), 5 * l.ptr));
  if (st) return st;
  memcpy(d.pinned, img.data(), img.size());
  HIP_TRY(hipMemcpyAsync(d.ws, d.pinned, img.size(), hipMemcpyHostToDevice, nullptr));
  mxmoe_gg_plan_info info;
  fill_info(plan, variant, l, d.ws, &info);
  st = mxmoe_gg_launch(&info, nullptr);
  if (st) return st;
  d.key = std::move(key);
  d.variant = variant;
  d.layout = l;
  d.cols = std::move(cols);
  d.plan = std::move(plan);
  d.cached = true;
  return MXMOE_GG_OK;
}

int mxmoe_gg_debug_trace(void* dst, size_t bytes, int reset) { return debug_read(g_gg_trace, dst, bytes, reset); }
#ifdef MXMOE_LAB
// lab library only (not in include/mxmoe_gg.h): the spread mainloop's per-wave stage stamps
int mxmoe_gg_debug_stamps(void* dst, size_t bytes, int reset) { return debug_read(g_gg_stamp, dst, bytes, reset); }
#endif

// Inverse of the reference's permute_weight(Row) + pack_weightonly (quantize.cuh:318-421), then
// the kernel layout (include/mxmoe_gg.h). Host code, run once per weight at load time.
int mxmoe_gg_repack_weightonly(const uint16_t* ref_words, int N, int K, int w_bits, uint8_t* out) {
  if (!ref_words || !out || N <= 0 || K <= 0)
    return fail(MXMOE_GG_ERR_INVALID, "bad arguments to mxmoe_gg_repack_weightonly");
  if (w_bits != 2 && w_bits != 4 && w_bits != 8)
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "weight-only repack: w_bits must be 2, 4 or 8 (got %d)", w_bits);
  const int pack = 16 / w_bits, mask = (1 << w_bits) - 1;
  if (N % (pack * 8) || K % 64)
    return fail(MXMOE_GG_ERR_INVALID, "weight-only repack: need N %% %d == 0 and K %% 64 == 0 (N=%d, K=%d)",
                pack * 8, N, K);
  // 1. unpack: word (r, k) holds columns (r/8)*8*pack + f*8 + r%8, f = 0 in the high bits
  std::vector<uint8_t> res((size_t)N * K), orig((size_t)N * K);
  for (int r = 0; r < N / pack; ++r)
    for (int f = 0; f < pack; ++f) {
      const size_t n = (size_t)(r / 8) * 8 * pack + f * 8 + r % 8;
      const int sh = (pack - 1 - f) * w_bits;
      for (int k = 0; k < K; ++k) res[n * K + k] = (uint8_t)((ref_words[(size_t)r * K + k] >> sh) & mask);
    }
  // 2. undo permute_weight: res[idx[x]] = orig[idx[perm[x]]] inside every 16(K) x 8*pack(N) block
  int perm[32];
  {
    const int* proj;
    const int* desired;
    int plen;
    static const int p8[4] = {1, 0, 3, 2}, d8[8] = {0, 2, 4, 6, 1, 3, 5, 7};
    static const int p4[8] = {3, 7, 2, 6, 1, 5, 0, 4};
    static const int d4[16] = {0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15};
    static const int p2[16] = {7, 15, 6, 14, 5, 13, 4, 12, 3, 11, 2, 10, 1, 9, 0, 8};  // quantize.cuh:343-347
    static const int d2[32] = {0, 8,  16, 24, 1, 9,  17, 25, 2, 10, 18, 26, 3, 11, 19, 27,
                               4, 12, 20, 28, 5, 13, 21, 29, 6, 14, 22, 30, 7, 15, 23, 31};
    if (w_bits == 8) {
      proj = p8, desired = d8, plen = 4;
    } else if (w_bits == 4) {
      proj = p4, desired = d4, plen = 8;
    } else {
      proj = p2, desired = d2, plen = 16;
    }
    for (int i = 0; i < 4 * pack; i += plen)
      for (int j = 0; j < plen; ++j) perm[proj[j] + i] = desired[i + j];
  }
  for (int j = 0; j < N; j += pack * 8)
    for (int i = 0; i < K; i += 16)
      for (int tj = 0; tj < 8; ++tj)
        for (int ti = 0; ti < 8; ti += 2) {
          size_t idx[32];
          int x = 0;
          for (int ii = 0; ii < 16; ii += 8)
            for (int tii = 0; tii < 2; ++tii)
              for (int f = 0; f < pack; ++f) idx[x++] = (size_t)(i + ii + ti + tii) + (size_t)(j + f * 8 + tj) * K;
          for (int y = 0; y < x; ++y) orig[idx[perm[y]]] = res[idx[y]];
        }
  // 3. kernel layout
  const size_t row_bytes = (size_t)K * w_bits / 8;
  for (int n = 0; n < N; ++n) {
    uint8_t* o = out + (size_t)n * row_bytes;
    if (w_bits < 8) memset(o, 0, row_bytes);
    for (int k = 0; k < K; ++k) {
      const int seg = k / 64, kl = k % 64, kc = kl / 32, g = (kl % 32) / 8, e = kl % 8;
      // 4-bit: code e of a unit at nibble (e >> 1) | (e & 1) << 2, so codes 2q and 2q+1 are the
      // nibbles at bits 4q and 16 + 4q of the unit's word (one v_and_or_b32 per fp16 pair)
      const int ep = w_bits == 4 ? (e >> 1) | ((e & 1) << 2) : e;
      const size_t pos = (size_t)seg * 64 + g * 16 + kc * 8 + ep;
      const uint8_t u = orig[(size_t)n * K + k];
      if (w_bits == 8) {
        o[pos] = u;
      } else if (w_bits == 4) {
        o[pos / 2] |= (uint8_t)(u << (4 * (pos & 1)));
      } else {
        // 2-bit: the unit (seg, g) is one 32-bit word holding both K halves; code (kc, e) at bit
        // 2 (4 kc + e / 2) for even e and 16 + 2 (4 kc + e / 2) for odd e (fp16 pairs, one and_or)
        const int bit = (e & 1) * 16 + 2 * (4 * kc + e / 2);
        o[(size_t)seg * 16 + g * 4 + bit / 8] |= (uint8_t)(u << (bit % 8));
      }
    }
  }
  return MXMOE_GG_OK;
}

}  // extern "C"
