// plan_host_check.cpp — the host tile planner (mxmoe_amd/csrc/gg_plan.cpp) run as a program of its own under the
// host compiler's sanitizers (-fsanitize=address,undefined): no hipcc, no GPU, nothing loaded into Python. The
// planner's index arithmetic on tile tables, XCD queues and split-K slabs runs on exactly-sized heap tables, so a
// write past one or a signed overflow stops the program.
// It plans with the product's three variants, built from the same functions as the library's (gg_plan.h plan_v3,
// plan_v2, plan_wo2), and asserts on the Plan itself what tests/test_planner.py's check_coverage asserts through
// the ABI: every output tile of every non-empty problem is planned exactly once, split-K slices partition the K
// stages of their tile, slab == grp == -1 unless a tile is split, `order` is a permutation of the non-empty
// problems, and the tile table, the slab count, ws_layout and workspace_image agree. Then one call per error
// return of the problem validation: the code, the text, and an untouched Plan.
// Built and run by tests/test_planner.py; prints one line and exits 0 when every check holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../mxmoe_amd/csrc/gg_error.h"
#include "../../mxmoe_amd/csrc/gg_plan.h"

using namespace mxmoe;

static long g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s (%s)\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)
static std::string g_case;

// ---- the product's variants, in the library's order, and one more that no product call sees: a persistent
// kernel with whole-stage K rows, for the two validation errors no product variant returns
static int pick_first(int) { return 0; }
static PlanVariant named(PlanVariant v, const char* name, int lds_bytes) {
  v.name = name, v.lds_bytes = lds_bytes, v.pick = &pick_first;
  return v;
}
static const PlanVariant kV3 = named(plan_v3(128, 256, 72 * 1024), kInt4Variant, 72 * 1024);
static const PlanVariant kV2x = named(plan_v2(true), kDefaultVariantName, 160 * 1024);
static const PlanVariant kWo3 = named(plan_wo2(3, true, true), kWoSmallVariant, 52 * 1024);
static PlanVariant extra_variant() {
  PlanVariant v = named(plan_v2(false), "check_persistent_kstage", 160 * 1024);
  v.persistent = true, v.k_stage_bytes = 256;
  return v;
}
static const PlanVariant kExtra = extra_variant();
static const PlanVariant* const kVariants[] = {&kV3, &kV2x, &kWo3, &kExtra};
enum { V3 = 0, V2X = 1, WO3 = 2, EXTRA = 3 };

// ---- problems
struct QT {
  const char* name;
  int a_bits, w_bits, gsize, sym, fmt;
};
static const QT FP16 = {"fp16", 16, 16, -1, 1, MXMOE_GG_FMT_DEFAULT}, W8A8 = {"w8a8", 8, 8, -1, 1, MXMOE_GG_FMT_DEFAULT},
                W4A4 = {"w4a4", 4, 4, -1, 1, MXMOE_GG_FMT_DEFAULT}, W4A4G = {"w4a4_g128", 4, 4, 128, 1, MXMOE_GG_FMT_DEFAULT},
                W4A16 = {"w4a16_g128", 16, 4, 128, 0, MXMOE_GG_FMT_DEFAULT}, E4M3 = {"e4m3", 8, 8, -1, 1, MXMOE_GG_FMT_E4M3},
                BF16 = {"bf16", 16, 16, -1, 1, MXMOE_GG_FMT_BF16}, MX4 = {"mxfp4", 4, 4, 32, 1, MXMOE_GG_FMT_MXFP4},
                MX4W = {"mxfp4w", 16, 4, 32, 1, MXMOE_GG_FMT_MXFP4}, MX8 = {"mxfp8", 8, 4, 32, 1, MXMOE_GG_FMT_MXFP8};

alignas(16) static char g_buf[64];  // addresses for the pointer checks (never read)
static HostProblem problem(int M, int N, int K, const QT& q, bool ptrs = false) {
  HostProblem p{};
  if (ptrs) p.A = p.B = p.SA = p.SB = p.C = g_buf;
  p.M = M, p.N = N, p.K = K, p.a_bits = q.a_bits, p.w_bits = q.w_bits, p.gsize = q.gsize, p.sym = q.sym, p.fmt = q.fmt;
  return p;
}

// ---- what must hold for the plan of any call
static int class_rows(const PlanVariant& v, const TileGeom& g, int cls) { return cls == 0 ? g.bm : cls == 1 ? v.tail_bm : v.tail2_bm; }

namespace {
struct Planned {
  int variant = -1;
  Plan plan;
};
}  // namespace
static Planned check_plan(const std::vector<HostProblem>& hp, int variant) {
  Planned out;
  CHECK(resolve_variant(variant, hp, &out.variant) == MXMOE_GG_OK);
  CHECK(out.variant >= 0 && out.variant < 4 && (variant == MXMOE_GG_VARIANT_AUTO ? out.variant < 3 : out.variant == variant));
  const PlanVariant& v = *kVariants[out.variant];
  Plan& plan = out.plan;
  CHECK(plan_host(hp, out.variant, false, &plan) == MXMOE_GG_OK);

  // `order` is a permutation of the non-empty problems, one table row each
  std::vector<int> want, got = plan.order;
  for (int i = 0; i < (int)hp.size(); ++i)
    if (hp[i].M > 0 && hp[i].N > 0) want.push_back(i);
  std::sort(got.begin(), got.end());
  CHECK(got == want && plan.meta.size() == plan.order.size());

  // every live slot once; its slices per output tile
  typedef std::tuple<int, int, int> Tile;  // (table row, m0, n0)
  std::map<Tile, std::vector<TileDesc>> slices;
  std::set<std::tuple<int, int, int, int, int, int, int, int>> seen;
  int live = 0;
  for (const TileDesc& t : plan.tiles) {
    if (t.prob < 0) {
      CHECK(std::memcmp(&t, &kEmptySlot, sizeof(t)) == 0);
      continue;
    }
    ++live;
    CHECK(t.prob < (int)plan.meta.size());
    CHECK(seen.insert(std::make_tuple(t.prob, t.m0, t.n0, t.cls, t.ks0, t.ks1, t.slab, t.grp)).second);
    slices[Tile(t.prob, t.m0, t.n0)].push_back(t);
  }
  CHECK(live == plan.total_tiles && plan.launch_grid == (int)plan.tiles.size());
  CHECK(plan.tiles.empty() || plan.tiles.back().prob >= 0);

  std::vector<char> slab_used(plan.slabs, 0);
  std::set<int> groups;
  size_t tiles_of_all = 0;
  for (int row = 0; row < (int)plan.meta.size(); ++row) {
    const GGMeta& m = plan.meta[row];
    const HostProblem& p = hp[plan.order[row]];
    const TileGeom& g = v.geom[m.qtype];
    CHECK(m.M == p.M && m.N == p.N && m.K == p.K && g.bn > 0);
    const int nm = (m.M + g.bm - 1) / g.bm, nn = (m.N + g.bn - 1) / g.bn;
    const int stages = qinfo(m.qtype).weight_only ? m.K / 64 : (m.kbytes + g.bkb - 1) / g.bkb;
    CHECK(m.tiles_n == nn && stages > 0);
    for (int mi = 0; mi < nm; ++mi)
      for (int ni = 0; ni < nn; ++ni) {
        auto it = slices.find(Tile(row, mi * g.bm, ni * g.bn));
        CHECK(it != slices.end());  // the output tile is planned
        std::vector<TileDesc>& sl = it->second;
        std::sort(sl.begin(), sl.end(), [](const TileDesc& a, const TileDesc& b) { return a.ks0 < b.ks0; });
        const int S = (int)sl.size(), cls = sl[0].cls & 0xFF;
        // its rows: a main tile unless it is the problem's last m-tile, whose class covers the rest
        CHECK(cls >= 0 && cls <= 2 && (cls == 0 || mi == nm - 1) && mi * g.bm + class_rows(v, g, cls) >= std::min(m.M, (mi + 1) * g.bm));
        CHECK(class_rows(v, g, cls) > 0);
        // its K stages [0, stages), slice after slice
        CHECK(sl[0].ks0 == 0 && sl[S - 1].ks1 == stages);
        for (int k = 0; k < S; ++k) {
          CHECK(sl[k].ks0 < sl[k].ks1 && (k == 0 || sl[k].ks0 == sl[k - 1].ks1) && (sl[k].cls & 0xFF) == cls);
          if (S == 1) {
            CHECK(sl[k].slab == -1 && sl[k].grp == -1 && (sl[k].cls >> 8) == 0);
          } else {  // split-K: slice index and count in cls, one slab group of S slabs, one arrival counter
            CHECK(((sl[k].cls >> 8) & 0xFF) == k && ((sl[k].cls >> 16) & 0xFF) == S);
            CHECK(sl[k].slab == sl[0].slab && sl[k].grp == sl[0].grp);
          }
        }
        if (S > 1) {
          CHECK(!qinfo(m.qtype).group_fold && v.kind == Kind::V2);
          CHECK(sl[0].slab >= 0 && sl[0].slab + S <= plan.slabs && sl[0].grp >= 0 && groups.insert(sl[0].grp).second);
          for (int k = 0; k < S; ++k) CHECK(!slab_used[sl[0].slab + k]++);
        }
        tiles_of_all += sl.size();
      }
  }
  CHECK(tiles_of_all == (size_t)live);  // nothing planned beyond the problems' tiles
  CHECK(std::count(slab_used.begin(), slab_used.end(), 1) == plan.slabs && plan.tail_slabs == 0);
  for (int g : groups) CHECK(g < (int)plan.tiles.size());  // (one arrival counter per tile slot)

  // the workspace: the layout of these counts, and an image that fits it exactly
  const int P = (int)plan.meta.size();
  const WsLayout l = ws_layout(P, (int)plan.tiles.size(), plan.slabs);
  CHECK(l.meta >= P * sizeof(GGMeta) && l.ptr >= P * sizeof(void*) && l.tiles >= plan.tiles.size() * sizeof(TileDesc));
  CHECK(l.counters == 0 ? plan.slabs == 0 : l.counters >= plan.tiles.size() * sizeof(int32_t));
  CHECK(l.slabs == (size_t)plan.slabs * SPLITK_SLAB_BYTES && l.total == l.meta + 5 * l.ptr + l.tiles + l.counters + l.slabs);
  const std::vector<const void*> cols = pointer_columns(plan.order, hp);
  CHECK(cols.size() == 5 * (size_t)P);
  WsLayout li{};
  const std::vector<uint8_t> img = workspace_image(plan, cols, &li);
  CHECK(std::memcmp(&li, &l, sizeof(l)) == 0 && img.size() == l.total - l.slabs);
  CHECK(P == 0 || std::memcmp(img.data(), plan.meta.data(), P * sizeof(GGMeta)) == 0);
  for (int c = 0; c < 5 && P > 0; ++c) CHECK(std::memcmp(img.data() + l.meta + c * l.ptr, cols.data() + c * P, P * sizeof(void*)) == 0);
  CHECK(plan.tiles.empty() ||
        std::memcmp(img.data() + l.meta + 5 * l.ptr, plan.tiles.data(), plan.tiles.size() * sizeof(TileDesc)) == 0);
  for (size_t b = l.meta + 5 * l.ptr + l.tiles; b < img.size(); ++b) CHECK(img[b] == 0);  // the counters start at zero
  Plan again;
  CHECK(plan_host(hp, out.variant, false, &again) == MXMOE_GG_OK && plan_signature(again) == plan_signature(plan));
  return out;
}

static bool plans_all(const PlanVariant& v, const std::vector<QT>& types) {
  for (const QT& q : types) {
    int qt = -1;
    if (qtype_of(q.a_bits, q.w_bits, q.gsize, q.sym, q.fmt, &qt) != MXMOE_GG_OK || v.geom[qt].bn == 0) return false;
  }
  return true;
}

// ---- row counts on either side of the tile classes, N one tile and one tile plus 8
static void check_classes() {
  const QT types[] = {FP16, W8A8, W4A4, W4A4G, W4A16, E4M3, BF16, MX4, MX4W, MX8};
  for (int vi : {V3, V2X, WO3})
    for (const QT& q : types) {
      if (!plans_all(*kVariants[vi], {q})) continue;
      int qt = -1;
      CHECK(qtype_of(q.a_bits, q.w_bits, q.gsize, q.sym, q.fmt, &qt) == MXMOE_GG_OK);
      const int bn = kVariants[vi]->geom[qt].bn;
      std::vector<HostProblem> all;
      for (int M : {0, 1, 63, 64, 65, 128, 129, 256, 257})
        for (int N : {bn, bn + 8}) {
          g_case = std::string("classes ") + kVariants[vi]->name + " " + q.name + " M=" + std::to_string(M) + " N=" + std::to_string(N);
          const Planned r = check_plan({problem(M, N, 1024, q)}, vi);
          CHECK(r.plan.meta.size() == (M > 0 ? 1u : 0u));
          all.push_back(problem(M, N, 1024, q));
        }
      g_case = std::string("classes ") + kVariants[vi]->name + " " + q.name + " all in one call";
      check_plan(all, vi);
      check_plan(all, MXMOE_GG_VARIANT_AUTO);
    }
  g_case = "an empty call";
  CHECK(check_plan({}, MXMOE_GG_VARIANT_AUTO).plan.tiles.empty());
}

// ---- a lone low-fill problem with a long K splits K on v2x; as w4a4 g128 (f32 group folds) it must not
static void check_split() {
  g_case = "split fp16";
  const Planned f = check_plan({problem(8, 256, 16384, FP16)}, V2X);
  CHECK(f.plan.slabs == 8 && f.plan.total_tiles == 8);
  g_case = "split w8a8 beside short problems";
  const Planned i = check_plan({problem(8, 512, 16384, W8A8), problem(8, 256, 1024, W8A8), problem(8, 256, 1024, FP16)}, V2X);
  CHECK(i.plan.slabs >= 16);  // (8 slices for each of the long problem's two tiles)
  g_case = "no split w4a4 g128";
  const Planned g = check_plan({problem(8, 256, 16384, W4A4G)}, V2X);
  CHECK(g.plan.slabs == 0 && g.plan.total_tiles == 1);
  g_case = "no split on v3";
  CHECK(check_plan({problem(8, 256, 16384, W8A8)}, V3).plan.slabs == 0);
}

// block b runs on XCD b % 8
static std::map<int, std::set<int>> xcds_of_rows(const Plan& plan) {
  std::map<int, std::set<int>> x;
  for (size_t b = 0; b < plan.tiles.size(); ++b)
    if (plan.tiles[b].prob >= 0) x[plan.tiles[b].prob].insert((int)(b % 8));
  return x;
}

// ---- a problem of at least 8 chunks of tiles on v2x is cut into one rectangle per XCD
static void check_regions() {
  g_case = "regions";
  const Planned r = check_plan({problem(8192, 4096, 1024, W8A8)}, V2X);  // 32 x 16 tiles = 16 chunks of 32
  for (int x = 0; x < 8; ++x) {
    std::set<int> m0s, n0s;
    int n = 0;
    for (size_t b = x; b < r.plan.tiles.size(); b += 8)
      if (r.plan.tiles[b].prob >= 0) m0s.insert(r.plan.tiles[b].m0), n0s.insert(r.plan.tiles[b].n0), ++n;
    // a rectangle of neighbouring tiles, an eighth of the grid
    CHECK(n == 64 && m0s.size() * n0s.size() == 64);
    CHECK(*m0s.rbegin() - *m0s.begin() == 256 * ((int)m0s.size() - 1) && *n0s.rbegin() - *n0s.begin() == 256 * ((int)n0s.size() - 1));
  }
}

// ---- the MoE call shape: 60 routed experts with a fixed uneven row split (five of them empty) and one shared
// expert of `tokens` rows (qwen2_moe's gate_up geometry: top-4 routing, the shared expert 4x as wide)
static std::vector<HostProblem> moe_call(int tokens, const QT& routed_a, const QT& routed_b, const QT& shared) {
  int weight[60], wsum = 0;
  for (int e = 0; e < 60; ++e) wsum += weight[e] = (e * 7) % 13;  // 0 for e = 0, 13, 26, 39, 52
  std::vector<HostProblem> hp;
  int given = 0;
  for (int e = 0; e < 60; ++e) {
    const int rows = (int)((int64_t)4 * tokens * weight[e] / wsum);
    given += rows;
    hp.push_back(problem(rows, 2816, 2048, e % 3 ? routed_a : routed_b));
  }
  hp[1].M += 4 * tokens - given;  // (the rounding's remainder)
  hp.push_back(problem(tokens, 11264, 2048, shared));
  return hp;
}
static void check_moe() {
  struct Cfg {
    const char* name;
    QT a, b, shared;
  };
  const Cfg cfgs[] = {{"fp16", FP16, FP16, FP16}, {"w8a8", W8A8, W8A8, W8A8}, {"w4a4", W4A4, W4A4, W4A4},
                      {"mixed w4a4 + w8a8", W4A4, W8A8, W8A8}, {"w4a16 + w8a8", W4A16, W8A8, W4A16}};
  for (const Cfg& c : cfgs)
    for (int tokens : {128, 8192}) {
      const std::vector<HostProblem> hp = moe_call(tokens, c.a, c.b, c.shared);
      int empty = 0;
      for (const HostProblem& p : hp) empty += p.M == 0;
      CHECK(hp.size() == 61 && empty >= 2);
      g_case = std::string("moe ") + c.name + " tokens=" + std::to_string(tokens) + " AUTO";
      check_plan(hp, MXMOE_GG_VARIANT_AUTO);
      for (int vi : {V3, V2X, WO3}) {
        if (!plans_all(*kVariants[vi], {c.a, c.b, c.shared})) continue;
        g_case = std::string("moe ") + c.name + " tokens=" + std::to_string(tokens) + " " + kVariants[vi]->name;
        const Planned r = check_plan(hp, vi);
        if (vi != V2X || tokens != 8192) continue;
        // packed (pack_xcds): every routed expert whole on one XCD, the shared expert's tiles on all eight
        const std::map<int, std::set<int>> xcds = xcds_of_rows(r.plan);
        for (int row = 0; row < (int)r.plan.order.size(); ++row)
          CHECK(xcds.at(row).size() == (r.plan.order[row] == 60 ? 8u : 1u));
      }
    }
}

// ---- one call per error return of the problem validation: the code, the text, the Plan untouched
static void expect_error(const char* name, int variant, HostProblem p, bool check_ptrs, int code, const std::string& text) {
  g_case = std::string("error ") + name;
  Plan plan;
  plan.order = {42}, plan.slabs = 7, plan.total_tiles = 3, plan.launch_grid = 5, plan.tail_slabs = 1;
  plan.meta.resize(2), plan.tiles.assign(3, kEmptySlot);
  const std::vector<HostProblem> hp = {problem(64, 256, 1024, FP16, true), p};  // (the bad problem is problem 1)
  const int st = plan_host(hp, variant, check_ptrs, &plan);
  if (st != code || text != last_error()) std::fprintf(stderr, "got %d: %s\nwant %d: %s\n", st, last_error(), code, text.c_str());
  CHECK(st == code && text == last_error());
  CHECK(plan.order == std::vector<int>{42} && plan.slabs == 7 && plan.total_tiles == 3 && plan.launch_grid == 5 &&
        plan.tail_slabs == 1 && plan.meta.size() == 2 && plan.tiles.size() == 3);
  GGMeta m;  // (mxmoe_gg_rebind's fast path validates with build_meta alone)
  CHECK(build_meta(p, 1, *kVariants[variant], check_ptrs, &m) == code && text == last_error());
}
static HostProblem with(HostProblem p, void (*change)(HostProblem&)) {
  change(p);
  return p;
}
static void check_errors() {
  const int INV = MXMOE_GG_ERR_INVALID, UNS = MXMOE_GG_ERR_UNSUPPORTED, SILU = MXMOE_GG_EPI_SILU_MUL;
  const HostProblem f16 = problem(64, 512, 1024, FP16, true), i8 = problem(64, 512, 1024, W8A8, true),
                    wo = problem(64, 512, 1024, W4A16, true), mxw = problem(64, 512, 1024, MX4W, true),
                    mx8 = problem(64, 512, 1024, MX8, true);
  expect_error("negative", V2X, problem(-1, 512, 1024, FP16), false, INV, "problem 1: negative shape");
  // the quant type (qtype_of's texts, under the problem's number)
  expect_error("qtype", V2X, problem(64, 512, 1024, QT{"", 16, 3, -1, 1, 0}), false, UNS,
               "problem 1: quant type not supported: w3a16_g-1_sym");
  expect_error("qtype e4m3", V2X, problem(64, 512, 1024, QT{"", 4, 4, -1, 1, MXMOE_GG_FMT_E4M3}), false, UNS,
               "problem 1: quant type not supported: w4a4_g-1_sym_E4M3 (only w8a8_g-1_sym_E4M3)");
  expect_error("qtype bf16", V2X, problem(64, 512, 1024, QT{"", 8, 8, -1, 1, MXMOE_GG_FMT_BF16}), false, UNS,
               "problem 1: quant type not supported: w8a8 bf16 (only 16-bit bf16 operands)");
  expect_error("qtype mxfp4", V2X, problem(64, 512, 1024, QT{"", 4, 4, 64, 1, MXMOE_GG_FMT_MXFP4}), false, UNS,
               "problem 1: quant type not supported: w4a4_g64_sym_MXFP4 (only w4a4_g32_sym_MXFP4 and w4a16_g32_sym_MXFP4)");
  expect_error("qtype mxfp8", V2X, problem(64, 512, 1024, QT{"", 8, 8, 32, 1, MXMOE_GG_FMT_MXFP8}), false, UNS,
               "problem 1: quant type not supported: w8a8_g32_sym_MXFP8 (only w4a8_g32_sym_MXFP8)");
  expect_error("fmt unknown", V2X, problem(64, 512, 1024, QT{"", 16, 16, -1, 1, 9}), false, UNS, "problem 1: unknown operand format 9");
  expect_error("variant has no body", V3, problem(64, 512, 1024, W4A16), false, UNS,
               "problem 1: variant v3_256x128_w4_dma_ring3_2wg does not implement w4a16 (quant type not supported)");
  expect_error("fmt flags", V2X, with(f16, [](HostProblem& p) { p.fmt |= 0x200; }), false, INV, "problem 1: unknown fmt flags 0x200");
  // the fused SiLU epilogue
  const std::string silu_type =
      "problem 1: the SiLU epilogue needs fp16, w8a8_g-1_sym, w4a4_g-1_sym or w4a8_g32_sym_MXFP8 (weight-only: the small-batch "
      "kernel wo3)";
  expect_error("silu type", V2X, with(problem(64, 512, 1024, BF16), [](HostProblem& p) { p.fmt |= SILU; }), false, UNS, silu_type);
  expect_error("silu weight-only on v2x", V2X, with(wo, [](HostProblem& p) { p.fmt |= SILU; }), false, UNS, silu_type);
  expect_error("silu variant", EXTRA, with(f16, [](HostProblem& p) { p.fmt |= SILU; }), false, UNS,
               "problem 1: variant check_persistent_kstage has no SiLU epilogue");
  expect_error("silu n", V2X, with(problem(64, 528, 1024, FP16), [](HostProblem& p) { p.fmt |= SILU; }), false, INV,
               "problem 1: the SiLU epilogue needs N % 32 == 0 (N=528)");
  // K
  expect_error("k mxfp8", V2X, problem(64, 512, 1040, MX8), false, INV, "problem 1: w4a8_g32_sym_MXFP8 needs K % 32 == 0 (K=1040)");
  expect_error("k rows", V2X, problem(64, 512, 1004, FP16), false, INV,
               "problem 1: K=1004 must be a multiple of 8 for 16-bit data (16-B rows)");
  expect_error("k stage", EXTRA, problem(64, 512, 1032, FP16), false, INV,
               "problem 1: variant check_persistent_kstage needs K*bits/8 to be a multiple of 256 bytes (K=1032)");
  expect_error("k g128", V2X, problem(64, 512, 1088, W4A4G), false, INV, "problem 1: w4a4_g128 needs K % 128 == 0 (K=1088)");
  expect_error("k int32", V2X, problem(64, 512, 131072 + 128, W8A8), false, INV,
               "problem 1: K=131200 exceeds the exact int32 accumulation bound 131072");
  expect_error("n", V2X, problem(64, 100, 1024, FP16), false, INV, "problem 1: N=100 must be a multiple of 8");
  // strides
  const char* ld = "problem 1: lda/ldb must be >= K row and a multiple of 8 words";
  expect_error("lda short", V2X, with(f16, [](HostProblem& p) { p.lda = 1016; }), false, INV, ld);
  expect_error("ldb odd", V2X, with(f16, [](HostProblem& p) { p.ldb = 1028; }), false, INV, ld);
  expect_error("ld 8 MiB", V2X, with(f16, [](HostProblem& p) { p.lda = 1 << 22; }), false, INV,
               "problem 1: A / B row strides must be below 8 MiB");
  expect_error("ldc short", V2X, with(f16, [](HostProblem& p) { p.ldc = 504; }), false, INV, "problem 1: ldc must be >= N and a multiple of 8");
  expect_error("ldc silu", V2X, with(f16, [](HostProblem& p) { p.fmt |= SILU, p.ldc = 248; }), false, INV,
               "problem 1: ldc must be >= N / 2 and a multiple of 8");
  // pointers (mxmoe_gg_plan's checks)
  expect_error("null C", V2X, with(f16, [](HostProblem& p) { p.C = nullptr; }), true, INV, "problem 1: NULL A/B/C");
  expect_error("null scale", V2X, with(i8, [](HostProblem& p) { p.SA = nullptr; }), true, INV, "problem 1: NULL scale pointer");
  expect_error("A misaligned", V2X, with(f16, [](HostProblem& p) { p.A = g_buf + 8; }), true, INV, "problem 1: A/B/C must be 16-byte aligned");
  expect_error("scale misaligned", V2X, with(i8, [](HostProblem& p) { p.SB = g_buf + 1; }), true, INV, "problem 1: scales must be 2-byte aligned");
  expect_error("dword scale misaligned", V2X, with(mx8, [](HostProblem& p) { p.SA = g_buf + 2; }), true, INV,
               "problem 1: w4a8_g32_sym_MXFP8 scales must be 4-byte aligned");
  // weight-only problems
  expect_error("wo k", V2X, problem(64, 512, 1056, W4A16), false, INV, "problem 1: weight-only needs K % 64 == 0 (K=1056)");
  expect_error("wo group size", V2X, problem(64, 512, 1024, QT{"", 16, 4, 96, 0, 0}), false, UNS,
               "problem 1: weight-only group size 96 must be -1 or a multiple of 64 dividing K=1024");
  expect_error("wo n", V2X, problem(64, 100, 1024, W4A16), false, INV, "problem 1: N=100 must be a multiple of 8");
  expect_error("wo ldb short", V2X, with(wo, [](HostProblem& p) { p.ldb = 248; }), false, INV, ld);
  expect_error("wo ldc odd", V2X, with(wo, [](HostProblem& p) { p.ldc = 516; }), false, INV, "problem 1: ldc must be >= N and a multiple of 8");
  expect_error("wo null B", WO3, with(wo, [](HostProblem& p) { p.B = nullptr; }), true, INV, "problem 1: NULL A/B/C");
  expect_error("wo null scale", WO3, with(wo, [](HostProblem& p) { p.SB = nullptr; }), true, INV,
               "problem 1: NULL scale pointer (weight-only scale_b)");
  expect_error("wo C misaligned", WO3, with(wo, [](HostProblem& p) { p.C = g_buf + 8; }), true, INV, "problem 1: A/B/C must be 16-byte aligned");
  expect_error("wo mx scale misaligned", WO3, with(mxw, [](HostProblem& p) { p.SB = g_buf + 2; }), true, INV,
               "problem 1: MXFP4 scales must be 4-byte aligned");
  expect_error("wo asym scale misaligned", WO3, with(wo, [](HostProblem& p) { p.SB = g_buf + 2; }), true, INV,
               "problem 1: scales must be 4-byte aligned");
  expect_error("wo mx k", V2X, problem(64, 512, (1 << 20) + 64, MX4W), false, INV, "problem 1: K=1048640 exceeds 2^20 (MXFP4 weight-only)");
  // the variant itself
  g_case = "error variant";
  CHECK(check_variant(4) == UNS && std::string("variant 4 not compiled (have 4)") == last_error());
  CHECK(check_variant(-2) == UNS && check_variant(0) == MXMOE_GG_OK);
}

int main() {
  set_plan_variants(kVariants, 4);
  CHECK(variant_index(kDefaultVariantName) == V2X && variant_index(kInt4Variant) == V3 && variant_index(kWoSmallVariant) == WO3);
  check_classes();
  check_split();
  check_regions();
  check_moe();
  check_errors();
  std::printf("plan_host_check ok: %ld checks\n", g_checks);
  return 0;
}
