// dyn_plan_check.cpp — the device tile planner's functions (mxmoe_amd/csrc/gg_dyn.h) run on the host under
// the host compiler's sanitizers (-fsanitize=address,undefined): every table is heap-allocated at exactly the
// size the library gives it, so a write past a table or a signed overflow in the rule stops the program.
// Checked over adversarial row tables: the capacity bound is never exceeded, every tile of every problem is
// planned exactly once and lies inside the planned rows, and bad tables (rows above capacity, a joint sum above
// rows_total, a slot table cut short, offsets outside the buffers) only ever set status bits.
// Built and run by tests/test_dynamic_plan.py; prints one line and exits 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../../mxmoe_amd/csrc/gg_dyn.h"

using namespace mxmoe;

static long g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

struct Kind {
  int bm, tail, tail2, bn;
};

// E routed problems of capacity cap (joint) and one shared problem of T rows, as a MoE layer plans them
static std::vector<DynGeom> layer(const Kind& k, int E, int cap, int N, int T, int Ns, bool small_class) {
  std::vector<DynGeom> g(E + 1);
  for (int i = 0; i <= E; ++i) {
    DynGeom& q = g[i];
    q = DynGeom{};
    const bool shared = i == E;
    q.cap = shared ? T : cap;
    q.bm = k.bm, q.tail_bm = k.tail, q.tail2_bm = small_class ? k.tail2 : 0, q.bn = k.bn;
    const int n = shared ? Ns : N;
    q.tiles_n = (n + k.bn - 1) / k.bn;
    q.nst = 4;
    q.joint = shared ? 0 : 1;
    q.a_row = 256, q.sa_row = (i & 1) ? 2 : 0, q.c_row = 2 * n;
    q.a_bytes = (int64_t)q.cap * q.a_row, q.sa_bytes = (int64_t)q.cap * q.sa_row, q.c_bytes = (int64_t)q.cap * q.c_row;
    q.sa_align = 2;
  }
  return g;
}

struct Run {
  int32_t status;
  int tiles;
  std::vector<int32_t> rows;
};

// the planner on exactly-sized tables; checks what must hold for ANY row table
static Run run(const std::vector<DynGeom>& g, int64_t R, const std::vector<DynRow>& dyn, int slots) {
  const int P = (int)g.size();
  std::vector<int32_t> order(P);
  for (int i = 0; i < P; ++i) order[i] = P - 1 - i;  // (any fixed permutation: the shared problem first)
  Run r;
  r.rows.assign(P, -7);
  std::vector<int32_t> cum(P + 1, -7);
  r.status = dyn_plan_rows(g.data(), order.data(), P, R, slots, dyn.data(), r.rows.data(), cum.data());
  r.tiles = cum[P];
  CHECK(r.tiles >= 0 && r.tiles <= slots);
  int64_t joint = 0;
  for (int i = 0; i < P; ++i) {
    CHECK(r.rows[i] >= 0 && r.rows[i] <= g[i].cap);
    if (g[i].joint) joint += r.rows[i];
  }
  CHECK(joint <= R);
  std::vector<int32_t> td((size_t)slots * 8, 0x5a5a5a5a);
  std::map<std::tuple<int, int, int>, int> seen;
  for (int s = 0; s < slots; ++s) {
    int32_t* t = td.data() + (size_t)s * 8;
    dyn_tile_at(g.data(), order.data(), P, r.rows.data(), cum.data(), s, t);
    if (s >= r.tiles) {
      CHECK(t[0] == -1);
      continue;
    }
    const int i = t[0];
    CHECK(i >= 0 && i < P);
    const DynGeom& q = g[i];
    CHECK(t[1] >= 0 && t[1] < r.rows[i] && t[1] % q.bm == 0);        // starts inside the planned rows
    CHECK(t[2] >= 0 && t[2] / q.bn < q.tiles_n && t[2] % q.bn == 0);  // ... and inside N
    const int rem = r.rows[i] - t[1], h = t[3] == 0 ? q.bm : t[3] == 1 ? q.tail_bm : q.tail2_bm;
    CHECK(t[3] >= 0 && t[3] <= 2 && h > 0);
    CHECK(t[3] == 0 ? true : rem <= h);          // a tail tile covers all that is left
    CHECK(t[3] == 0 || t[1] + q.bm >= r.rows[i]);  // ... and is the problem's last
    CHECK(t[4] == 0 && t[5] == q.nst && t[6] == -1 && t[7] == -1);
    CHECK(++seen[std::make_tuple(i, t[1], t[2])] == 1);
  }
  int64_t want = 0;
  for (int i = 0; i < P; ++i) want += (int64_t)g[i].tiles_n * ((r.rows[i] + g[i].bm - 1) / g[i].bm);
  CHECK((int64_t)seen.size() == want && want == r.tiles);  // every tile, once
  return r;
}

static std::vector<DynRow> table(const std::vector<DynGeom>& g, const std::vector<int>& rows) {
  std::vector<DynRow> d(g.size());
  for (size_t i = 0; i < g.size(); ++i) d[i] = DynRow{rows[i], 0, 0, 0, 0};
  return d;
}

int main() {
  const Kind kinds[] = {{256, 128, 64, 256}, {256, 128, 0, 128}, {64, 0, 0, 128}, {64, 0, 0, 256}};
  std::mt19937 rng(1234);
  long tables = 0;
  for (const Kind& k : kinds)
    for (int E : {1, 4, 8, 60, 64})
      for (int T : {1, 7, 60, 300, 1024})
        for (int topk : {1, 2, 6}) {
          if (topk > E) continue;
          const int R = T * topk, N = 384, Ns = 1408;
          for (int small = 0; small < 2; ++small) {
            const std::vector<DynGeom> g = layer(k, E, R, N, T, Ns, small != 0);
            std::vector<int32_t> scratch(g.size());
            const int64_t slots64 = dyn_capacity_slots(g.data(), (int)g.size(), R, scratch.data());
            CHECK(slots64 > 0 && slots64 < (1 << 24));
            const int slots = (int)slots64;
            std::vector<std::vector<int>> cases;
            for (int e = 0; e < E; e += (E > 8 ? 17 : 1)) {  // all rows on one expert
              std::vector<int> r(E + 1, 0);
              r[e] = R, r[E] = T;
              cases.push_back(r);
            }
            {  // one row on each (as many as there are rows), the rest on the last expert
              std::vector<int> r(E + 1, 0);
              int left = R;
              for (int e = 0; e < E && left > 0; ++e) r[e] = 1, --left;
              r[E - 1] += left, r[E] = T;
              cases.push_back(r);
            }
            for (int step : {k.bm, k.tail ? k.tail : k.bm, k.tail2 ? k.tail2 : k.bm}) {  // one past a tile boundary
              std::vector<int> r(E + 1, 0);
              int left = R;
              for (int e = 0; e < E && left > 0; ++e) {
                const int want = step + 1 < left ? step + 1 : left;
                r[e] = want, left -= want;
              }
              r[E] = T;  // (rows left over stay unrouted: the sum may be below R)
              cases.push_back(r);
            }
            for (int it = 0; it < 6; ++it) {  // random splits of R
              std::vector<int> r(E + 1, 0);
              for (int j = 0; j < R; ++j) ++r[(rng() % 3 == 0) ? rng() % E : (rng() % 2 ? 0 : E / 2)];
              r[E] = T;
              cases.push_back(r);
            }
            for (const auto& r : cases) {
              const Run out = run(g, R, table(g, r), slots);
              CHECK(out.status == 0);  // admissible tables never clamp and never run out of slots
              for (size_t i = 0; i < r.size(); ++i) CHECK(out.rows[i] == r[i]);
              ++tables;
            }
            // bad tables: status bits, and run()'s invariants still hold
            std::vector<int> r(E + 1, 0);
            r[0] = R + 5, r[E] = T + 1;
            CHECK(run(g, R, table(g, r), slots).status & DYN_ROWS_CLAMPED);
            r[0] = -3, r[E] = T;
            CHECK(run(g, R, table(g, r), slots).status & DYN_ROWS_CLAMPED);
            if (E > 1) {
              std::vector<int> r2(E + 1, R);
              r2[E] = T;
              const Run o = run(g, R, table(g, r2), slots);
              CHECK((o.status & DYN_JOINT_CLAMPED) && o.rows[0] == R && o.rows[1] == 0);
            }
            {
              std::vector<int> r3(E + 1, 0);
              r3[0] = R, r3[E] = T;
              const int cut = slots > 3 ? 3 : 1;
              const Run o = run(g, R, table(g, r3), cut);
              CHECK(o.tiles <= cut);
              if (g[0].tiles_n + g[E].tiles_n > cut) CHECK(o.status & DYN_SLOTS_CUT);
              std::vector<DynRow> d = table(g, r3);
              d[0].a_off = 16;  // R rows no longer fit behind the base
              Run b = run(g, R, d, slots);
              CHECK((b.status & DYN_BAD_OFFSET) && b.rows[0] == 0 && b.rows[E] == T);
              d[0].a_off = 0, d[E].c_off = -16;
              b = run(g, R, d, slots);
              CHECK((b.status & DYN_BAD_OFFSET) && b.rows[E] == 0);
              d[E].c_off = 8;  // misaligned
              CHECK(run(g, R, d, slots).status & DYN_BAD_OFFSET);
              d[E].c_off = INT64_MAX - 15;
              CHECK(run(g, R, d, slots).status & DYN_BAD_OFFSET);
            }
            tables += 8;
          }
        }
  std::printf("dyn_plan_check ok: %ld row tables, %ld checks\n", tables, g_checks);
  return 0;
}
