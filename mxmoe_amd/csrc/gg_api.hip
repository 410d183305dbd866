// gg_api.hip — host side of libmxmoe_gg.so: the C-ABI declared in include/mxmoe_gg.h, the kernel-build
// tables and the variant list. The host tile planner is a host-only unit of its own (gg_plan.h, gg_plan.cpp).
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
#include "gg_error.h"
#include "gg_plan.h"
#ifdef MXMOE_LAB
#include "gg_f6.h"   // lab-only fp6 w4a4 route: measured slower than the int4 path
#include "gg_v2q.h"  // lab-only persistent kernel: not compiled into the product library
#include "gg_v4.h"   // lab-only one-wave-per-SIMD 256 x 256 tile
// rows of the lab-only fp6 images of int4 codes (mxmoe_gg_pack_f6, gg_f6.h; the format code: gg_plan.cpp)
#define MXMOE_GG_F6_ROW_BYTES(K) ((((int64_t)(K) + 127) / 128) * 96)
#endif

using namespace mxmoe;

namespace {

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

// A kernel variant: what the planner plans with (gg_plan.h) and, the launch half, its compiled kernels.
struct Variant : PlanVariant {
  BuildTable builds;  // the family's compiled kernels (PlanVariant::pick: the index in `builds`)
};
Variant variant_of(const PlanVariant& plan, const char* name, int lds_bytes, BuildTable builds, int (*pick)(int)) {
  Variant v{plan, builds};
  v.name = name, v.lds_bytes = lds_bytes, v.pick = pick;
  return v;
}
constexpr int pick_only(int) { return 0; }  // (families of one build)

[[maybe_unused]] constexpr int kMx4 = 1 << QT_MXF4;   // w4a4_g32_sym_MXFP4
[[maybe_unused]] constexpr int kMxW = 1 << QT_MXF4W;  // weight-only MXFP4
[[maybe_unused]] constexpr int kMx8 = 1 << QT_MXF8A;  // w4a8_g32_sym_MXFP8 (gg_tile_v2's 64 x 128 body)
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
  Variant v = variant_of(plan_base(Kind::V0, C16::kThreads, lds <= 80 * 1024 ? 64 : 32 /* workgroups per XCD at once */, 0),
                         name, lds, table_of(kV0Builds<C16, C8, C4>), &pick_only);
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

static_assert(V2Cfg<256>::BM == 256 && V2Cfg<256>::BN == 256 && V2Cfg<256>::BKB == 128 && V2Cfg<256>::NT == 512,
              "plan_v2's main tile (gg_plan.h) is gg_v2_kernel's");
template <int ABL = 0>
Variant make_v2(const char* name) {
  return variant_of(plan_v2(kMxBodies), name, kV2Lds<ABL>, v2_builds<ABL>(), &pick_v2<ABL>);
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
  static_assert(CT::BM == 256 && CT::BKB == 64, "plan_v3's tile (gg_plan.h) is gg_v3_kernel's");
  return variant_of(plan_v3(BN, CT::NT, CT::LDS_BYTES), name, CT::LDS_BYTES, table_of(kV3Builds<BN, WN, NBUF, DIST, OPT>),
                    &pick_v3<BN, WN, NBUF, DIST, OPT>);
}

#ifdef MXMOE_LAB
// fp6 w4a4 tiles (gg_f6.h): 256 x 256 (+ 128-row tail class), one 512-thread workgroup per CU
template <int NBUF, int DIST, int OPT>
constexpr Builds<1> kF6Builds = {{{1 << QT_I4F6, true, F6Cfg<256, 256, 2, 4, NBUF, DIST>::LDS_BYTES, &launch_k<&gg_f6_kernel<NBUF, DIST, OPT>, 512>}}};
template <int NBUF, int DIST, int OPT = 0>
Variant make_f6(const char* name) {
  typedef F6Cfg<256, 256, 2, 4, NBUF, DIST> CT;
  Variant v = variant_of(plan_base(Kind::V3, CT::NT, 32, 128), name, CT::LDS_BYTES, table_of(kF6Builds<NBUF, DIST, OPT>), &pick_only);
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
#ifdef MXMOE_LAB_FAST
  constexpr bool silu_wo = false;
#else
  constexpr bool silu_wo = true;  // weight-only problems: the WO_SILU builds
#endif
  return variant_of(plan_wo2(NWG, kMxBodies, silu_wo), name, wo2_lds_bytes<NWG>(), table_of(kWo2Builds<ABL, NWG>),
                    &pick_wo2<ABL, NWG>);
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
  Variant v = variant_of(plan_v2(false), name, 160 * 1024, table_of(kV2pBuilds<TRACE>), &pick_v2p<TRACE>);
  v.persistent = true;  // (silu_epi is its tile body's; has_silu_epilogue: not from a persistent kernel)
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
  Variant v = variant_of(plan_v2_base(256), name, V4Cfg<256>::LDS_BYTES, table_of(kV4Builds<OPT>), &pick_v4<OPT>);
  for (int q : {QT_F16, QT_I8, QT_I4}) v.geom[q] = {256, 256, 128, 256};
  return v;
}
#endif  // MXMOE_LAB

typedef TileCfg<128, 128, 2, 2, 2> T128x128;
typedef TileCfg<256, 128, 2, 2, 1> T256x128;
typedef TileCfg<128, 256, 2, 2, 1> T128x256;

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
// the planner's view of the list (gg_plan.h), handed over once when the library loads
[[maybe_unused]] const bool g_planner_has_variants = [] {
  static std::vector<const PlanVariant*> views;
  for (const Variant& v : variants()) views.push_back(&v);
  set_plan_variants(views.data(), (int)views.size());
  return true;
}();

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

extern "C" {

int mxmoe_gg_abi_version(void) { return MXMOE_GG_ABI_VERSION; }

const char* mxmoe_gg_last_error(void) { return last_error(); }

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
