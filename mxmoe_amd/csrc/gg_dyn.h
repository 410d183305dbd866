// gg_dyn.h — the device tile planner of a fixed-capacity ("dynamic") GroupGEMM plan.
//
// mxmoe_gg_plan_dynamic writes everything that does not depend on the row counts once, on the host;
// mxmoe_gg_launch_dynamic then runs dyn_plan_kernel in front of the variant's unchanged GEMM kernel:
// from a device table of {rows, a_off, sa_off, c_off} per problem it fills GGMeta::M / tile_begin, the
// A / scale_a / C pointer columns and every TileDesc slot of the workspace (unused slots: prob = -1).
//
// The rule itself — the row clamps, the m-tile classes, the tile enumeration — is plain C++ in
// `__host__ __device__` functions with no HIP type in them, so the host diagnostic
// (mxmoe_gg_dynamic_tiles) and a stand-alone host program (tests/cpp/dyn_plan_check.cpp, built with the
// host compiler's sanitizers) run exactly what the GPU runs. Only the __global__ wrapper at the end
// needs hipcc; it is compiled into moe_ops.hip (MXMOE_DYN_KERNEL) and launched from gg_api.hip.
//
// No reference counterpart: the reference plans on the host every call (kernel_sketch.py:82-145).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MXMOE_HD __host__ __device__
#else
#define MXMOE_HD
#endif

namespace mxmoe {

// Status bits of a dynamic plan (the workspace's status word; OR-ed by the planner, never cleared by it).
constexpr int32_t DYN_ROWS_CLAMPED = 1;   // a row count was negative or above its problem's capacity M
constexpr int32_t DYN_JOINT_CLAMPED = 2;  // the joint problems' rows summed to more than rows_total
constexpr int32_t DYN_SLOTS_CUT = 4;      // more tiles than tile_slots: the surplus was not planned
constexpr int32_t DYN_BAD_OFFSET = 8;     // an offset was negative, misaligned or left its buffer: the problem got 0 rows

// One row of the caller's device table (= mxmoe_gg_dyn_row, include/mxmoe_gg.h).
struct DynRow {
  int32_t rows;
  int32_t reserved;
  int64_t a_off, sa_off, c_off;  // byte offsets added to the planned base pointers
};
static_assert(sizeof(DynRow) == 32, "DynRow is mxmoe_gg_dyn_row");

// Static geometry of one problem, written by mxmoe_gg_plan_dynamic (128 B).
struct DynGeom {
  int32_t cap;       // capacity M of the problem
  int32_t bm;        // main tile height
  int32_t tail_bm;   // height of the tail class (0: the variant has none)
  int32_t tail2_bm;  // height of the small-remainder class (0: none, or the type does not take it)
  int32_t bn;        // tile width
  int32_t tiles_n;   // cdiv(N, bn)
  int32_t nst;       // K stages of a tile
  int32_t joint;     // 1: counts against rows_total
  int64_t a_row;     // bytes per row of A (its stride), of scale_a (all of a row's scales) and of C
  int64_t sa_row;
  int64_t c_row;
  int64_t a_bytes;   // bytes behind each base pointer: an offset must keep its rows inside
  int64_t sa_bytes;
  int64_t c_bytes;
  uint64_t base_a, base_sa, base_c;  // device addresses
  int32_t sa_align;  // alignment of scale_a (4: dword-read block scales)
  int32_t pad_[5];
};
static_assert(sizeof(DynGeom) == 128, "DynGeom must stay 128 bytes");

// THE TILE RULE (the host planner's m_tiles, gg_plan.cpp): with `rem` rows left at m0, the tile is the
// 64-row class if the type takes it and rem fits, else the 128-row tail class if rem fits, else a main
// tile. Returns the class; every tile but a problem's last is a main tile, and m-tile i starts at i * bm.
MXMOE_HD inline int dyn_tile_class(const DynGeom& g, int rem) {
  if (g.tail2_bm && rem <= g.tail2_bm) return 2;
  if (g.tail_bm && rem <= g.tail_bm) return 1;
  return 0;
}
// m-tiles of a problem with r rows. Main tiles step by bm and the one tail tile ends the problem, so this
// is cdiv(r, bm) whatever the classes: an expert with r > 0 rows has floor((r - 1) / bm) + 1 m-tiles.
MXMOE_HD inline int dyn_m_tiles(const DynGeom& g, int r) { return r <= 0 ? 0 : (r - 1) / g.bm + 1; }

// CAPACITY BOUND: the tile slots a dynamic plan needs so that no admissible row table overflows them.
// Admissible: 0 <= r_i <= M_i, and sum of r_i over the joint problems <= R (the planner clamps to both).
// With tn_i = tiles_n and tiles(i) = tn_i * cdiv(r_i, bm_i):
//   (a) per problem, tiles(i) <= tn_i * cdiv(M_i, bm_i);
//   (b) over the joint set J, sum tiles(i) = sum_{r_i > 0} tn_i * (1 + floor((r_i - 1) / bm_i)).
//       Say n problems have r_i > 0 (1 <= n <= min(|J|, R)). The "1" terms sum to at most top_n(tn), the
//       sum of the n largest tn_i; and sum floor((r_i - 1) / bm_i) <= floor(sum (r_i - 1) / bm_min)
//       <= floor((R - n) / bm_min), each weighted by at most tn_max. Hence
//       sum_J tiles(i) <= max over n of [ top_n(tn) + tn_max * floor((R - n) / bm_min) ]   (0 for R = 0).
//       With one tile width and height in J the bracket grows with n and the bound is attained: one row on
//       each of n - 1 experts and R - n + 1 rows on another.
// slots = sum_{i not in J} (a) + min(sum_J (a), (b)). (a) wins when the capacities are small, (b) when they
// are generous (a MoE layer: any expert may take every row). (b) is tighter than the
// sum_J tn_i + tn_max * floor(R / bm) form: at decode sizes (R < |J|) only R experts can be non-empty, and
// the n rows that open the n experts cannot also fill tiles.
// `scratch` holds P int32 (sorted tn of the joint set).
MXMOE_HD inline int64_t dyn_capacity_slots(const DynGeom* g, int P, int64_t rows_total, int32_t* scratch) {
  int64_t alone = 0, joint_a = 0;
  int nj = 0, tn_max = 0, bm_min = 0;
  for (int i = 0; i < P; ++i) {
    const int64_t a = (int64_t)g[i].tiles_n * dyn_m_tiles(g[i], g[i].cap);
    if (!g[i].joint) {
      alone += a;
      continue;
    }
    joint_a += a;
    if (g[i].tiles_n <= 0 || g[i].cap <= 0) continue;  // never a tile
    tn_max = g[i].tiles_n > tn_max ? g[i].tiles_n : tn_max;
    bm_min = (bm_min == 0 || g[i].bm < bm_min) ? g[i].bm : bm_min;
    int j = nj++;  // insertion sort, descending
    for (; j > 0 && scratch[j - 1] < g[i].tiles_n; --j) scratch[j] = scratch[j - 1];
    scratch[j] = g[i].tiles_n;
  }
  int64_t joint_b = 0;
  if (rows_total > 0 && nj > 0) {
    const int64_t npos = rows_total < nj ? rows_total : nj;
    int64_t top = 0;
    for (int64_t n = 1; n <= npos; ++n) {
      top += scratch[n - 1];
      const int64_t b = top + (int64_t)tn_max * ((rows_total - n) / bm_min);
      joint_b = b > joint_b ? b : joint_b;
    }
  }
  return alone + (joint_a < joint_b ? joint_a : joint_b);
}

// Step 1, sequential (one thread): clamp the rows, check the offsets, and prefix-sum the tiles in table
// order `order` (the host's static longest-first order). rows_out[i]: the rows problem i is planned with;
// cum[r]: first tile of order[r], cum[P]: tiles planned (<= tile_slots). Returns the status bits.
MXMOE_HD inline int32_t dyn_plan_rows(const DynGeom* g, const int32_t* order, int P, int64_t rows_total,
                                      int32_t tile_slots, const DynRow* dyn, int32_t* rows_out, int32_t* cum) {
  int32_t status = 0;
  int64_t used = 0;
  for (int i = 0; i < P; ++i) {  // clamps in the caller's problem order
    const DynRow d = dyn[i];
    int64_t r = d.rows;
    if (r < 0 || r > g[i].cap) {
      status |= DYN_ROWS_CLAMPED;
      r = r < 0 ? 0 : g[i].cap;
    }
    if (g[i].joint) {
      if (used + r > rows_total) {
        status |= DYN_JOINT_CLAMPED;
        r = rows_total - used;
      }
      used += r;
    }
    if (r > 0) {
      const bool bad_a = d.a_off < 0 || (d.a_off & 15) || d.a_off > g[i].a_bytes || r * g[i].a_row > g[i].a_bytes - d.a_off;
      const bool bad_c = d.c_off < 0 || (d.c_off & 15) || d.c_off > g[i].c_bytes || r * g[i].c_row > g[i].c_bytes - d.c_off;
      const bool bad_s = g[i].sa_row > 0 && (d.sa_off < 0 || (d.sa_off & (g[i].sa_align - 1)) || d.sa_off > g[i].sa_bytes ||
                                             r * g[i].sa_row > g[i].sa_bytes - d.sa_off);
      if (bad_a || bad_c || bad_s) {
        status |= DYN_BAD_OFFSET;
        r = 0;
      }
    }
    rows_out[i] = (int32_t)r;
  }
  int64_t t = 0;
  for (int k = 0; k < P; ++k) {
    const int i = order[k];
    cum[k] = (int32_t)t;
    int64_t n = (int64_t)g[i].tiles_n * dyn_m_tiles(g[i], rows_out[i]);
    if (t + n > tile_slots) {  // cut at whole m-tile rows of the problem: what is planned is complete in N
      status |= DYN_SLOTS_CUT;
      const int64_t mt = g[i].tiles_n > 0 ? (tile_slots - t) / g[i].tiles_n : 0;
      rows_out[i] = (int32_t)(mt * g[i].bm < rows_out[i] ? mt * g[i].bm : rows_out[i]);
      n = (int64_t)g[i].tiles_n * dyn_m_tiles(g[i], rows_out[i]);
    }
    t += n;
  }
  cum[P] = (int32_t)t;
  return status;
}

// Step 2, per slot (any thread): the tile of slot s as 8 int32 in TileDesc's layout {prob, m0, n0, class,
// first K stage, end K stage, -1, -1}; prob = -1 for s >= cum[P]. Inside a problem: bands of 4 m-tiles,
// n-major inside a band (the host planner's enumeration: neighbouring blocks share A rows and B columns).
MXMOE_HD inline void dyn_tile_at(const DynGeom* g, const int32_t* order, int P, const int32_t* rows, const int32_t* cum,
                                 int s, int32_t* td) {
  if (s >= cum[P]) {
    td[0] = -1, td[1] = 0, td[2] = 0, td[3] = 0, td[4] = 0, td[5] = 0, td[6] = -1, td[7] = -1;
    return;
  }
  int lo = 0, hi = P - 1;  // last k with cum[k] <= s (empty problems repeat a value: the last one holds tiles)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  const int i = order[lo];
  const DynGeom& q = g[i];
  const int t = s - cum[lo], tn = q.tiles_n, mt = dyn_m_tiles(q, rows[i]);
  const int band = t / (4 * tn), r = t - band * 4 * tn;
  const int bh = mt - 4 * band < 4 ? mt - 4 * band : 4;
  const int n = r / bh, mi = 4 * band + r % bh;
  const int m0 = mi * q.bm;
  td[0] = i, td[1] = m0, td[2] = n * q.bn, td[3] = dyn_tile_class(q, rows[i] - m0);
  td[4] = 0, td[5] = q.nst, td[6] = -1, td[7] = -1;
}

// workgroups of the planner kernel: at most kDynMaxBlocks, each taking kDynSlotsPerBlock tile slots (the host
// sizes the per-workgroup scratch of the workspace by the former: gg_plan.cpp's dyn_layout)
constexpr int kDynMaxBlocks = 16;
constexpr int kDynSlotsPerBlock = 2048;

}  // namespace mxmoe

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace mxmoe {

// The two plan-table columns and the tile slots the planner writes, as the raw layout of gg_device.h's GGMeta
// (64-byte rows: int32 M first, int32 tile_begin sixth) and TileDesc (8 int32) — gg_api.hip static_asserts
// both against the structs. Raw, so the kernel can live beside the MoE plumbing kernels (moe_ops.hip): the
// GroupGEMM translation unit's kernel set stays the GEMM kernels alone.
constexpr int kDynMetaWords = 16, kDynMetaM = 0, kDynMetaTileBegin = 5, kDynTileWords = 8;

// Where a dynamic plan's launch finds its data in the workspace.
struct DynArgs {
  const DynGeom* geom;
  const int32_t* order;
  int32_t* rows;    // scratch [workgroups][P]
  int32_t* cum;     // scratch [workgroups][P + 1]
  int32_t* status;  // status word (OR-ed)
  int32_t* meta;    // plan table, kDynMetaWords per problem
  const void** ptr_A;
  const void** ptr_SA;
  void** ptr_C;
  int32_t* tiles;   // tile table, kDynTileWords per slot
  const DynRow* dyn;
  const int64_t* rows_total;  // the joint bound (static plan data in the workspace)
  int32_t P, tile_slots;
};
namespace detail {
// launches dyn_plan_kernel (moe_ops.hip) on min(kDynMaxBlocks, cdiv(tile_slots, kDynSlotsPerBlock)) workgroups
void launch_dyn_plan(const DynArgs& a, hipStream_t stream);
}  // namespace detail

#ifdef MXMOE_DYN_KERNEL
// A few workgroups, by the slot count. In each, the threads first copy the plan's geometry rows, the table
// order and the caller's row table into LDS together (one round of memory latency instead of one per problem:
// the sequential step below took 40-100 us out of global memory, profiles/r12/graph_forward/), thread 0 then
// clamps and prefix-sums there (P is an expert count: tens to hundreds of short iterations; repeating them per
// workgroup costs no time and saves a grid-wide hand-over), and the workgroups share the tile slots; workgroup 0
// also writes the table rows and the status word. Plans of more than kDynLdsProblems problems run the same
// functions on global memory (the workgroup's own scratch in the workspace).
constexpr int kDynLdsProblems = 256;
__global__ __launch_bounds__(256) void dyn_plan_kernel(DynArgs a) {
  __shared__ __attribute__((aligned(16))) DynGeom s_geom[kDynLdsProblems];
  __shared__ __attribute__((aligned(16))) DynRow s_dyn[kDynLdsProblems];
  __shared__ int32_t s_order[kDynLdsProblems], s_rows[kDynLdsProblems], s_cum[kDynLdsProblems + 1];
  const DynGeom* geom = a.geom;
  const int32_t* order = a.order;
  const DynRow* dyn = a.dyn;
  int32_t* rows = a.rows + (size_t)blockIdx.x * a.P;
  int32_t* cum = a.cum + (size_t)blockIdx.x * (a.P + 1);
  if (a.P <= kDynLdsProblems) {  // (uniform)
    const int64_t* gs = reinterpret_cast<const int64_t*>(a.geom);
    const int64_t* ds = reinterpret_cast<const int64_t*>(a.dyn);
    int64_t* gd = reinterpret_cast<int64_t*>(s_geom);
    int64_t* dd = reinterpret_cast<int64_t*>(s_dyn);
    for (int i = threadIdx.x; i < a.P * (int)(sizeof(DynGeom) / 8); i += blockDim.x) gd[i] = gs[i];
    for (int i = threadIdx.x; i < a.P * (int)(sizeof(DynRow) / 8); i += blockDim.x) dd[i] = ds[i];
    for (int i = threadIdx.x; i < a.P; i += blockDim.x) s_order[i] = a.order[i];
    __syncthreads();
    geom = s_geom, order = s_order, dyn = s_dyn, rows = s_rows, cum = s_cum;
  }
  if (threadIdx.x == 0) {
    const int32_t st = dyn_plan_rows(geom, order, a.P, *a.rows_total, a.tile_slots, dyn, rows, cum);
    if (st && blockIdx.x == 0) *a.status = *a.status | st;
  }
  __syncthreads();
  if (blockIdx.x == 0)
    for (int k = threadIdx.x; k < a.P; k += blockDim.x) {
      const int i = order[k];
      const DynGeom& q = geom[i];
      const DynRow d = dyn[i];
      const bool live = rows[i] > 0;  // (an unplanned problem keeps its base pointers: no tile reads them)
      a.meta[(size_t)i * kDynMetaWords + kDynMetaM] = rows[i];
      a.meta[(size_t)i * kDynMetaWords + kDynMetaTileBegin] = cum[k];
      a.ptr_A[i] = reinterpret_cast<const void*>(q.base_a + (live ? (uint64_t)d.a_off : 0));
      a.ptr_SA[i] = reinterpret_cast<const void*>(q.base_sa + (live && q.sa_row > 0 ? (uint64_t)d.sa_off : 0));
      a.ptr_C[i] = reinterpret_cast<void*>(q.base_c + (live ? (uint64_t)d.c_off : 0));
    }
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < a.tile_slots; s += gridDim.x * blockDim.x)
    dyn_tile_at(geom, order, a.P, rows, cum, s, a.tiles + (size_t)s * kDynTileWords);
}
#endif  // MXMOE_DYN_KERNEL

}  // namespace mxmoe
#endif  // __HIPCC__
