// gg_plan.cpp — the host tile planner of libmxmoe_gg.so: problem validation, the AUTO variant policy, tile
// generation and XCD placement, the workspace image, and the host half of the device plan. Plain host C++ (no
// HIP header, no kernel text): built into the library with the other sources, and with the host compiler alone
// under its sanitizers by tests/cpp/plan_host_check.cpp.
//
// Reference behaviour replaced (SeaCatComplexes/MxMoE):
//   host API groupgemm_hz_fused_<i> ........ kernel_sketch.py:82-145 (prefix sum on host)
//   tile -> (problem, m, n) by prefix scan .. tile_scheduler.cuh:25-50
//   qtype dispatch + "quant type not supported" ... compose_kernel.py:47-57, 421-479
// Here: the planner builds an explicit tile table once into a caller-owned workspace — tiles of
// the longest problems first (LPT), grouped into chunks of neighbouring tiles that run together on
// one XCD (shared A rows / B columns hit that XCD's L2). Errors are status codes.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mxmoe_gg.h"
#include "gg_dyn.h"
#define MXMOE_ERROR_DEFINE  // the error channel's one definition
#include "gg_error.h"
#include "gg_plan.h"
#include "gg_types.h"
#ifdef MXMOE_LAB
// lab-only operand format: w4a4_g-1_sym with A / B as fp6 images (mxmoe_gg_pack_f6, gg_f6.h)
#define MXMOE_GG_FMT_F6 3
#endif

namespace mxmoe {

namespace {
const PlanVariant* const* g_variants = nullptr;
int g_variant_count = 0;
const PlanVariant& variant_at(int i) { return *g_variants[i]; }

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
}  // namespace

void set_plan_variants(const PlanVariant* const* variants, int count) { g_variants = variants, g_variant_count = count; }

int variant_index(const char* name) {
  for (int i = 0; i < g_variant_count; ++i)
    if (!strcmp(variant_at(i).name, name)) return i;
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

namespace {
// The strides of a problem whose dense A / B rows are arow / brow bytes, checked, and its table row filled but for
// GGMeta::reserved and the type's reserved2 bits.
int meta_row(const HostProblem& p, int idx, int qt, const PlanVariant& v, int64_t arow, int64_t brow, bool dma_rows, GGMeta* m) {
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
int build_meta_weightonly(const HostProblem& p, int idx, int qt, const PlanVariant& v, bool check_ptrs, GGMeta* m) {
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
}  // namespace

int build_meta(const HostProblem& p, int idx, const PlanVariant& v, bool check_ptrs, GGMeta* m) {
  if (p.M < 0 || p.N < 0 || p.K < 0) return fail(MXMOE_GG_ERR_INVALID, "problem %d: negative shape", idx);
  int qt = 0;
  int st = qtype_of(p.a_bits, p.w_bits, p.gsize, p.sym, p.fmt, &qt);
  if (st) return fail(st, "problem %d: %s", idx, last_error());
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

namespace {
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


// K stages of a problem in its tile body (v2: 128 B per stage; weight-only: 64 elements)
int stages_of(const PlanVariant& v, const GGMeta& m) {
  if (qinfo(m.qtype).weight_only) return m.K / 64;
  return (m.kbytes + v.geom[m.qtype].bkb - 1) / v.geom[m.qtype].bkb;
}
double full_tile_cost(const PlanVariant& v, const GGMeta& m) {
  return qinfo(m.qtype).passes * (double)m.kbytes * v.geom[m.qtype].bm * v.geom[m.qtype].bn;
}
// rows of an m-tile class; v2 classes 256 / 128 / 64 rows (see Variant::tail_bm)
int class_rows(const PlanVariant& v, int cls, const TileGeom& g) { return cls == 0 ? g.bm : cls == 1 ? v.tail_bm : v.tail2_bm; }
// m-tiles of a problem: (m0, class). v2: 256-row tiles while > tail_bm rows remain, then one tail_bm (128)
// or tail2_bm (64) tile
std::vector<std::pair<int, int>> m_tiles(const PlanVariant& v, const GGMeta& m) {
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
std::vector<int> split_factors(const PlanVariant& v, const std::vector<GGMeta>& all, const std::vector<int>& order,
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
double stage_time(const PlanVariant& v, const GGMeta& m, int cls) {
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
  const PlanVariant& v;
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
bool region_of(const PlanVariant& v, const GGMeta& m, int w_bits, int mt, const PlannerOpts& o, Region* out) {
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
TileLists enumerate_tiles(const PlanVariant& v, const std::vector<GGMeta>& all, const std::vector<HostProblem>& probs,
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
bool pack_xcds(const PlanVariant& v, const TileLists& tl, const TileTimer& tile_time, const PlannerOpts& o, XcdQueues* out) {
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
void place_chunks(const PlanVariant& v, const TileLists& tl, const TileTimer& tile_time, const PlannerOpts& o, XcdQueues* q) {
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
void split_tails(const PlanVariant& v, const TileTimer& tile_time, int mode, int* groups, XcdQueues* xq, Plan* plan) {
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
void lowfill_lpt(const PlanVariant& v, const TileTimer& tile_time, Plan* plan) {
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
void emit_persistent(const PlanVariant& v, const XcdQueues& xq, const TileTimer& tile_time, bool any_tiles, Plan* plan) {
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
}  // namespace


// Tile generation + scheduling: validation, one table row per problem (build_meta; empty problems are dropped);
// m-tile classes and split-K factors (m_tiles, split_factors); problems by descending modelled time of their
// first (tallest) tile (stage_time); tile enumeration, a problem of >= 8 chunks of tiles (the shared expert at
// large batch) cut into one rectangle per XCD (enumerate_tiles, region_of); placement — the MoE call shape packed
// problem by problem (pack_xcds), any other call in chunks of about `chunk` tiles, each to the XCD with the least
// modelled time so far, the regions after them (place_chunks); emission in dispatch order (emit_tiles).
int plan_host(const std::vector<HostProblem>& probs, int variant, bool check_ptrs, Plan* plan) {
  const PlanVariant& v = variant_at(variant);
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
  if (variant < 0 || variant >= g_variant_count)
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "variant %d not compiled (have %d)", variant, g_variant_count);
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
      if (!strcmp(variant_at(wi).name, kWoSmallVariant)) {
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
  if (P > 0) {  // (an empty plan's vectors have no storage to copy from)
    memcpy(img.data(), plan.meta.data(), (size_t)P * sizeof(GGMeta));
    for (int c = 0; c < 5; ++c) memcpy(img.data() + l.meta + c * l.ptr, cols.data() + c * P, (size_t)P * sizeof(void*));
    memcpy(img.data() + l.meta + 5 * l.ptr, plan.tiles.data(), plan.tiles.size() * sizeof(TileDesc));
  }
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

namespace {
// bytes of one row's activation scales (0: the type has none)
int64_t sa_row_bytes(int qt, int K) {
  const QTypeInfo& t = qinfo(qt);
  if (t.weight_only || t.float16) return 0;
  if (t.dword_scales) return 16 * (((int64_t)K / 32 + 15) / 16);  // e8m0 bytes, the device layout
  if (t.group_fold) return 2 * ((int64_t)K / t.k_mult);
  return 2;
}
bool dyn_variant_ok(const PlanVariant& v) {
  if (v.persistent || (v.kind != Kind::V2 && v.kind != Kind::V3)) return false;
  return !strcmp(v.name, kDefaultVariantName) || !strcmp(v.name, kInt4Variant) || !strcmp(v.name, kWoSmallVariant);
}
}  // namespace

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
  const PlanVariant& v = variant_at(variant);
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

}  // namespace mxmoe
