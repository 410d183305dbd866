// moe_decode_a16.h — the decode forward with fp16 activations on the fp16 MFMA (the _a16 entries of include/mxmoe_moe.h:
// mxmoe_moe_decode_gate_up_a16, mxmoe_moe_decode_down_a16), gfx950. Included by moe_ops.hip after moe_decode_f8g.h.
// The kinds whose A row stays fp16 — MXMOE_DECODE_FP16, MXMOE_DECODE_W4A16_MX and the eight integer weight-only kinds
// 4..11 — run a16_tile on v_mfma_f32_16x16x32_f16: a decode batch is at most 16 rows, the 16-wide side of that
// instruction, so a weight is dequantised once per workgroup pass and multiplied against every row of the batch by one
// instruction (the weight streamers of moe_decode.h multiply it once per A row on the VALU). Kinds 1 and 2 (w8a8, w4a4)
// keep expert_tile<Plain<KIND>> and its bytes in the same launch. A kernel of its own, decode_a16_kernel<DOWN>; Args,
// the grid, the id scan, the status bits, geometry()'s ct, pair-order outputs, dequant_mx, dequant_wo, load_h8 and
// glu_out are moe_decode.h's.
//
// Mapping (lp_tile's): the weights are src0 and the A rows src1 of the MFMA. Lane (r16, g), r16 = lane & 15,
// g = lane >> 4, supplies 8 K values of weight row r16 and the same 8 K values of batch row r16, and ends with the four
// f32 of batch row r16 on weight rows 4 g .. 4 g + 3 (four adjacent output columns): one 8-byte store.
//   waves     a tile of `ct` columns is cg = ct / 16 groups of 16 columns. The four waves form cl = min(cg, 4) column
//             lanes times ks = 4 / cl K slices: ct = 32 is 2 x 2 (no wave idles), ct = 64 is 4 x 1, ct = 128 is 4 x 1
//             with two column groups per wave. gate_up: a column group is its 16 gate rows and its 16 up rows — two
//             accumulators on one A fragment (both weight layouts: only the row index differs).
//   weights   from global memory straight to registers: every weight byte is loaded by one lane once. A K group is 128
//             K values; a lane's loads of a group and the K values of its four fragments j = 0..3 (one MFMA each) are
//               fp16   bytes [256 s + 64 g, + 64) of its row (4 x 16 B)           K = 128 s + 32 g + 8 j + 0..7
//               MX     bytes [64 s + 16 g, + 16) (the MX block 4 s + g), dword j  K = 128 s + 32 g + 8 j + 0..7
//               4-bit  bytes [64 s + 16 g, + 16) of the repacked row, dword j      K = 128 s + 64 (g >> 1) + 32 (j & 1)
//                                                                                      + 8 (2 (g & 1) + (j >> 1)) + 0..7
//               8-bit  bytes [128 s + 64 h + 16 g, + 16), h = 0, 1; dwords 2 kc,   K = 128 s + 64 h + 32 kc + 8 g + 0..7,
//                      2 kc + 1 of load h                                              j = 2 h + kc
//             (mxmoe_gg_repack_weightonly's layout: K value 32 kc + 8 g + e at element 16 g + 8 kc + e of a 64-K
//             segment.) A trip is kTrip groups (fp16 2, the others 4: 128 B per lane and weight row, 64 B for 4-bit
//             codes), all loaded before the first is multiplied; a group past the slice's end loads the slice's first
//             group again and is not multiplied. With a group's codes come its side data, once per group: MX the block's
//             e8m0 byte (byte 16 (s >> 2) + 4 g + (s & 3) of the row's device-layout scales, read in place; a byte
//             load, as the _ex contract gives these rows no alignment), g128 the (scale, zp) of row r16 and group s;
//             per-channel pairs are loaded once per column group. A fragment is dequantised once (dequant_mx,
//             dequant_wo: the values of the _ex / _wo entries) straight into the MFMA's 8 halves.
//   A rows    fp16, not quantised (bf16 hidden rows converted by load_h8), in K order, rows `row` bytes apart: 256 gc + 16,
//             an odd number of 16-byte slots, so the 16 rows of a fragment read lie in distinct slots of the 256-byte
//             bank row (the rule of moe_decode_mfma.h). All rows of the batch (up to 16) go in one pass over the weights:
//             where the whole rows fit the LDS budget they are staged once (gc = K / 128); otherwise in chunks of gc = 4
//             K groups (8 for batches of up to 8 rows) in two buffers — chunk c + 1 is copied (wave w rows w, w + 4, ...;
//             a lane 16 bytes) before chunk c is multiplied, one barrier per chunk. Lanes r16 >= nr read the 16 zero
//             bytes at the head instead of a row (their accumulator columns are never stored).
//   K slices  a chunk's groups are split in ks contiguous runs of ceil(groups / ks), the last what remains; slice sl
//             owns run sl of every chunk. Slices >= 1 write their accumulators to LDS; after a barrier slice 0 adds them
//             in slice order and runs the epilogue. Every barrier is reached by all four waves.
// Arithmetic: v(r) = fp16_rn(sum_k f32(x[k]) * f32(b[r][k])), accumulated in f32 by v_mfma_f32_16x16x32_f16, a slice's
// K groups ascending and within a group j ascending (inside the instruction: the hardware's order), then the slices'
// partial sums in slice order.
#pragma once

namespace mxmoe {
namespace {
namespace decode {

constexpr int kA16 = 5;  // the entry pair's number beside kFirst .. kF8g: no level of decode_kernel
constexpr int kA16Head = 16;
constexpr uint32_t kA16Plain = 1u << MXMOE_DECODE_W8A8 | 1u << MXMOE_DECODE_W4A4;  // the kinds that keep expert_tile

struct A16Lds {
  int rb;       // A rows per batch
  int gc;       // K groups per staged chunk (whole rows: all of the widest row's)
  int nbuf;     // buffers: 1 (whole rows) or 2
  int row;      // bytes between the rows of a buffer
  int cl, ks;   // column lanes and K slices of the four waves
  int part;     // byte offset of the partial sums
  int bytes;    // of the whole map (0: no kind of the mask runs a16_tile)
};
__host__ __device__ inline A16Lds a16_lds(const Args& a, bool down) {
  const int kmax = a.with_shared && a.K_shared > a.K ? a.K_shared : a.K;
  A16Lds L;
  const int cg = a.ct / 16;
  L.cl = cg < 4 ? cg : 4;
  L.ks = 4 / L.cl;
  L.rb = a.T < kBatchRows ? a.T : kBatchRows;
  const int parts = (L.ks - 1) * L.cl * 64 * (down ? 1 : 2) * 16;
  const int G = kmax >> 7;
  const bool whole = kA16Head + L.rb * (256 * G + 16) + parts <= kLdsBudget;
  L.gc = whole ? G : L.rb > 8 ? 4 : 8;
  L.nbuf = whole ? 1 : 2;
  L.row = 256 * L.gc + 16;
  L.part = kA16Head + L.nbuf * L.rb * L.row;
  L.bytes = (a.kind_mask & ~kA16Plain) ? L.part + parts : 0;
  return L;
}

// What differs between the four weight forms. kU4: 16-byte loads of a lane per K group and weight row; kGroup: bytes of
// a group in a weight row; lane_b / kStrideB: a lane's first load of a group and the distance of its loads; lane_a /
// frag_a: byte offsets of fragment j in a group of an A row (256 bytes), the lane's part and j's.
enum { kA16F16 = 0, kA16Mx = 1, kA16W4 = 2, kA16W8 = 3 };
template <int WK>
struct A16Form {
  static constexpr int kU4 = WK == kA16F16 ? 4 : WK == kA16W8 ? 2 : 1;
  static constexpr int kGroup = WK == kA16F16 ? 256 : WK == kA16W8 ? 128 : 64;
  static constexpr int kStrideB = WK == kA16W8 ? 64 : 16;
  static constexpr int kTrip = WK == kA16F16 ? 2 : 4;
  static __device__ __forceinline__ int lane_b(int g) { return WK == kA16F16 ? 64 * g : 16 * g; }
  static __device__ __forceinline__ int lane_a(int g) {
    return WK == kA16W4 ? 128 * (g >> 1) + 32 * (g & 1) : WK == kA16W8 ? 16 * g : 64 * g;
  }
  static constexpr int frag_a(int j) { return WK == kA16W4 ? 64 * (j & 1) + 16 * (j >> 1) : WK == kA16W8 ? 64 * j : 16 * j; }
  static __host__ __device__ int row_bytes(int K) { return WK == kA16F16 ? 2 * K : WK == kA16W8 ? K : K / 2; }
};

// A weight row's side data. MX: the e8m0 rows; weight-only: the fp16 (scale, zp) buffer, the group size and the symmetry
// from the record's kind (workgroup-uniform), as WeightOnly<BITS> of moe_decode.h.
struct A16Side {
  const uint8_t* SB;
  int rows, sh, sr;  // weight-only: element (grp * rows + r) << sh; MX: bytes of a scale row
  bool g128, asym;
  h2_t moff;
  __device__ __forceinline__ h2_t pair(int row, int grp) const {
    const _Float16* const s = reinterpret_cast<const _Float16*>(SB) + (((int64_t)grp * rows + row) << sh);
    return h2_t{s[0], asym ? s[1] : (_Float16)0};
  }
};

// fragment j of group u of a trip: the MFMA's 8 halves of the lane's weight row
template <int WK>
__device__ __forceinline__ h8_t a16_frag(const uint4 (&w)[A16Form<WK>::kTrip * A16Form<WK>::kU4], int u, int j, uint32_t e8,
                                         h2_t sz, h2_t moff) {
  if constexpr (WK == kA16F16) {
    return __builtin_bit_cast(h8_t, w[4 * u + j]);
  } else if constexpr (WK == kA16Mx) {
    const uint32_t d[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
    return dequant_mx(d[j], e8 << 23);
  } else if constexpr (WK == kA16W4) {
    const uint32_t d[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
    return dequant_wo<4>(d[j], 0u, moff, h2_t{sz[0], sz[0]}, h2_t{sz[1], sz[1]});
  } else {
    const uint4& v = w[2 * u + (j >> 1)];
    return (j & 1) ? dequant_wo<8>(v.z, v.w, moff, h2_t{sz[0], sz[0]}, h2_t{sz[1], sz[1]})
                   : dequant_wo<8>(v.x, v.y, moff, h2_t{sz[0], sz[0]}, h2_t{sz[1], sz[1]});
  }
}

// The K groups [g0, g1) of one column group against the staged chunk: wr the lane's weight rows, w their first bytes
// (the lane's part included), ap the lane's A bytes of the chunk's first group cg0, the groups `ainc` apart (a lane
// past the batch: the head, ainc = 0, jmask = 0).
template <bool DOWN, int WK>
__device__ __forceinline__ void a16_groups(const A16Side& sd, const int (&wr)[DOWN ? 1 : 2], const uint8_t* const (&w)[DOWN ? 1 : 2],
                                           const h2_t (&pc)[DOWN ? 1 : 2], int cg0, int g0, int g1, int g, const uint8_t* ap, int ainc,
                                           int jmask, lp_v4f (&acc)[DOWN ? 1 : 2]) {
  typedef A16Form<WK> F;
  constexpr int NW = DOWN ? 1 : 2;
  for (int s0 = g0; s0 < g1; s0 += F::kTrip) {
    uint4 wv[NW][F::kTrip * F::kU4];
    uint32_t e8[NW][F::kTrip];
    h2_t sz[NW][F::kTrip];
#pragma unroll
    for (int u = 0; u < F::kTrip; ++u) {  // the trip's loads, all in flight; a group past the slice: its first group
      const int s = s0 + u < g1 ? s0 + u : g0;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
#pragma unroll
        for (int v = 0; v < F::kU4; ++v)
          wv[i][u * F::kU4 + v] = *reinterpret_cast<const uint4*>(w[i] + (int64_t)s * F::kGroup + v * F::kStrideB);
        e8[i][u] = 0u;
        sz[i][u] = pc[i];
        if constexpr (WK == kA16Mx) e8[i][u] = sd.SB[(int64_t)wr[i] * sd.sr + (s >> 2) * 16 + 4 * g + (s & 3)];
        if constexpr (WK == kA16W4 || WK == kA16W8) {
          if (sd.g128) sz[i][u] = sd.pair(wr[i], s);  // (workgroup-uniform)
        }
      }
    }
#pragma unroll
    for (int u = 0; u < F::kTrip; ++u) {
      if (s0 + u < g1) {  // wave-uniform
        const uint8_t* const as = ap + (s0 + u - cg0) * ainc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const h8_t av = *reinterpret_cast<const h8_t*>(as + (F::frag_a(j) & jmask));
#pragma unroll
          for (int i = 0; i < NW; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16_frag<WK>(wv[i], u, j, e8[i][u], sz[i][u], sd.moff), av, acc[i],
                                                            0, 0, 0);
        }
      }
    }
  }
}

// One workgroup's work on an expert of form WK (`kind`: the record's own): per batch of rows, the A rows through LDS in
// chunks, every chunk against the slice's K groups of the wave's column groups, then the partial sums and the epilogue.
template <bool DOWN, int WK>
__device__ __forceinline__ void a16_tile(const Args& a, const mxmoe_moe_decode_expert& ex, int kind, bool shared, int tile,
                                         int nrows, uint8_t* s_a, const int* s_rows, const _Float16* brow) {
  typedef A16Form<WK> F;
  constexpr int NW = DOWN ? 1 : 2;  // weight rows per lane: down 1; gate_up the gate and the up row
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = shared ? a.K_shared : a.K, C = shared ? a.C_shared : a.C;
  const int G = K >> 7, KB = F::row_bytes(K);
  const uint8_t* const B = static_cast<const uint8_t*>(DOWN ? ex.b2 : ex.b1);
  const uint8_t* const src = static_cast<const uint8_t*>(shared ? a.src_shared : a.src);
  _Float16* const out = shared ? a.out_shared : a.out;
  const bool bf = !DOWN && a.src_bf16;
  const A16Lds L = a16_lds(a, DOWN);
  uint8_t* const s_buf = s_a + kA16Head;
  const int bufb = L.rb * L.row;
  if (tid < kA16Head / 4) reinterpret_cast<uint32_t*>(s_a)[tid] = 0u;

  A16Side sd;
  sd.SB = static_cast<const uint8_t*>(DOWN ? ex.sb2 : ex.sb1);
  sd.rows = DOWN ? C : 2 * C;
  sd.sr = ((K / 2 + 255) >> 8) * 16;
  sd.g128 = sd.asym = false;
  sd.sh = 0;
  sd.moff = h2_t{0, 0};
  if constexpr (WK == kA16W4 || WK == kA16W8) {
    sd.g128 = wo_g128(kind), sd.asym = wo_asym(kind), sd.sh = sd.asym ? 1 : 0;
    const _Float16 off = (_Float16)(sd.asym ? -1024.0f : WK == kA16W4 ? -1031.0f : -1151.0f);  // -(1024 + 2^(BITS-1) - 1), sym
    sd.moff = h2_t{off, off};
  }

  // the wave's column lane and K slice; the chunks of a row
  const int cw = wave % L.cl, sl = wave / L.cl;
  const int passes = a.ct / (16 * L.cl);  // 1, or 2 for ct = 128 (then ks = 1)
  const int nchunk = (G + L.gc - 1) / L.gc;  // (1 where the rows are staged whole: L.gc >= G)

  for (int r0 = 0; r0 < nrows; r0 += L.rb) {
    const int nr = min(L.rb, nrows - r0);
    // chunk c of the batch's rows into buffer c & 1: wave w rows w, w + 4, ..., a lane 16 bytes at a time
    auto stage = [&](int c) {
      const int k0 = c * L.gc * 128, kn = min(K - k0, L.gc * 128);
      uint8_t* const buf = s_buf + (c & 1) * bufb;
      for (int r = wave; r < nr; r += kThreadsD / 64) {
        const int p = shared ? r0 + r : s_rows[r0 + r];      // token (shared) or pair
        const int srow = (shared || DOWN) ? p : p / a.topk;  // gate_up reads the pair's token
        const uint8_t* const sp = src + (int64_t)srow * K * 2;
        for (int i = lane * 8; i < kn; i += 512) *reinterpret_cast<h8_t*>(buf + r * L.row + 2 * i) = load_h8(sp, k0 + i, bf);
      }
    };
    __syncthreads();  // s_rows and the head are complete; the previous batch's A rows and partial sums are no longer read
    stage(0);
    __syncthreads();
    const bool live = r16 < nr;  // lanes past the batch read the head: zeros
    const int orow = live ? (shared ? r0 + r16 : s_rows[r0 + r16]) : 0;
    const uint8_t* const arow = live ? s_buf + r16 * L.row + F::lane_a(g) : s_a;
    const int ainc = live ? 256 : 0, jmask = live ? ~0 : 0, abuf = live ? bufb : 0;

    // the lane's weight rows per column group: down row n + r16; gate_up the gate and the up row of column n + r16
    int wr[2][NW];
    const uint8_t* w[2][NW];
    h2_t pc[2][NW];
    lp_v4f acc[2][NW];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int n = tile * a.ct + 16 * (cw + L.cl * (ps < passes ? ps : 0));
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        wr[ps][i] = DOWN ? n + r16 : a.layout == MXMOE_DECODE_GU_INTERLEAVED ? 2 * n + r16 + 16 * i : i * C + n + r16;
        w[ps][i] = B + (int64_t)wr[ps][i] * KB + F::lane_b(g);
        pc[ps][i] = h2_t{0, 0};
        if constexpr (WK == kA16W4 || WK == kA16W8) {
          if (!sd.g128) pc[ps][i] = sd.pair(wr[ps][i], 0);
        }
        acc[ps][i] = lp_v4f{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }

    for (int c = 0; c < nchunk; ++c) {  // (workgroup-uniform)
      if (c + 1 < nchunk) stage(c + 1);
      const int cg0 = c * L.gc, cg1 = min(G, cg0 + L.gc);
      const int per = (cg1 - cg0 + L.ks - 1) / L.ks;
      const int g0 = min(cg0 + sl * per, cg1), g1 = min(g0 + per, cg1);
      const uint8_t* const ap = arow + (c & 1) * abuf;
      a16_groups<DOWN, WK>(sd, wr[0], w[0], pc[0], cg0, g0, g1, g, ap, ainc, jmask, acc[0]);
      if (passes > 1) a16_groups<DOWN, WK>(sd, wr[1], w[1], pc[1], cg0, g0, g1, g, ap, ainc, jmask, acc[1]);
      if (c + 1 < nchunk) __syncthreads();  // chunk c + 1 is staged; chunk c's buffer is no longer read
    }

    if (L.ks > 1) {  // (workgroup-uniform; then passes == 1) the K slices' partial sums through LDS, added in slice order
      lp_v4f* const part = reinterpret_cast<lp_v4f*>(s_a + L.part);
      if (sl > 0) {
#pragma unroll
        for (int i = 0; i < NW; ++i) part[(((sl - 1) * L.cl + cw) * NW + i) * 64 + lane] = acc[0][i];
      }
      __syncthreads();
      if (sl == 0) {
        for (int k = 1; k < L.ks; ++k) {
#pragma unroll
          for (int i = 0; i < NW; ++i) acc[0][i] += part[(((k - 1) * L.cl + cw) * NW + i) * 64 + lane];
        }
      }
    }

    // lane (r16, g) of slice 0: row r16 of the batch, output columns n + 4 g + 0..3 of each of the wave's column groups
    if (sl == 0 && live) {
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        if (ps < passes) {
          const int col = tile * a.ct + 16 * (cw + L.cl * ps) + 4 * g;
          typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
          h4_t o;
          if constexpr (DOWN) {
            o = h4_t{(_Float16)acc[ps][0][0], (_Float16)acc[ps][0][1], (_Float16)acc[ps][0][2], (_Float16)acc[ps][0][3]};
          } else {
            const bool has_b = brow != nullptr;  // workgroup-uniform
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const _Float16 bg = has_b ? brow[col + j] : (_Float16)0, bu = has_b ? brow[C + col + j] : (_Float16)0;
              const _Float16 gv = (_Float16)acc[ps][0][j], uv = (_Float16)acc[ps][NW - 1][j];
              o[j] = a.glu == kGluSwigluClamp ? glu_out<kGluSwigluClamp>(gv, uv, has_b, bg, bu, a.limit, a.c)
                                              : glu_out<kGluSilu>(gv, uv, has_b, bg, bu, a.limit, a.c);
            }
          }
          *reinterpret_cast<h4_t*>(out + (int64_t)orow * C + col) = o;
        }
      }
    }
  }
}

// DOWN = false: decode_gate_up_a16; true: decode_down_a16.
template <bool DOWN>
__global__ __launch_bounds__(kThreadsD) void decode_a16_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_a[];  // a16_lds's map, or expert_tile's [rb][lds_row]
  __shared__ int s_rows[kMaxPairs];
  __shared__ int s_cnt[kThreadsD / 64];
  __shared__ _Float16 s_scale[kBatchRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsh = a.with_shared ? a.tiles_shared : 0;
  const int b = blockIdx.x;
  const bool shared = b < nsh;
  const int e = shared ? a.E : (b - nsh) / a.tiles;  // in [0, E] by the grid's size
  const int tile = shared ? b : (b - nsh) % a.tiles;
  const int npairs = a.T * a.topk;

  // the rows of the workgroup's expert among the call's ids, in pair order (decode_kernel's scan)
  int nrows = a.T;
  if (!shared) {
    const int id = tid < npairs ? a.ids[tid] : -1;
    const bool hit = id == e;
    const uint64_t m = __builtin_amdgcn_ballot_w64(hit);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    if (b == nsh && a.status) {  // one workgroup reports the ids that no workgroup matches
      const bool bad = tid < npairs && (id < 0 || id >= a.E);
      if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(a.status, MXMOE_DECODE_BAD_ID);
    }
    __syncthreads();
    int base = 0;
    nrows = 0;
#pragma unroll
    for (int w = 0; w < kThreadsD / 64; ++w) {
      base += w < wave ? s_cnt[w] : 0;
      nrows += s_cnt[w];
    }
    if (nrows == 0) return;  // no token chose this expert
    if (hit) s_rows[base + __popcll(m & (((uint64_t)1 << lane) - 1))] = tid;
  }

  const mxmoe_moe_decode_expert ex = a.experts[e];
  const int kind = DOWN ? ex.kind2 : ex.kind1;
  if (kind < 0 || kind > 31 || !((a.kind_mask >> kind) & 1u)) {  // (the mask holds kinds 0..11 only: the entry's check)
    if (tid == 0 && a.status) atomicOr(a.status, MXMOE_DECODE_BAD_KIND);
    return;
  }
  // the bias row of the workgroup's own expert (e < E by the grid's size): never indexed by an id
  const _Float16* brow = nullptr;
  if constexpr (!DOWN) brow = shared ? a.bias_shared : a.bias_routed ? a.bias_routed + (int64_t)e * 2 * a.C : nullptr;
#define MXMOE_A16_PLAIN(KIND) \
  expert_tile<DOWN, Plain<KIND>, true, kA16>(a, ex, kind, shared, tile, nrows, s_a, s_rows, s_scale, brow)
#define MXMOE_A16_TILE(WK) a16_tile<DOWN, WK>(a, ex, kind, shared, tile, nrows, s_a, s_rows, brow)
  if (kind == MXMOE_DECODE_W8A8) return MXMOE_A16_PLAIN(MXMOE_DECODE_W8A8);
  if (kind == MXMOE_DECODE_W4A4) return MXMOE_A16_PLAIN(MXMOE_DECODE_W4A4);
  if (kind == MXMOE_DECODE_FP16) return MXMOE_A16_TILE(kA16F16);
  if (kind == MXMOE_DECODE_W4A16_MX) return MXMOE_A16_TILE(kA16Mx);
  if (wo_bits(kind) == 4) return MXMOE_A16_TILE(kA16W4);
  return MXMOE_A16_TILE(kA16W8);
#undef MXMOE_A16_TILE
#undef MXMOE_A16_PLAIN
}

// ---------------------------------------------------------------------------------------------
// host side: the launch. The mask check is the _wo level's (kinds 0..11), under the _a16 entries' names.

template <bool DOWN>
inline int launch_a16(Args a, void* stream) {
  // ct and the tiles; lds_row and rb as the kinds 1 and 2 of the mask size them (expert_tile's rows), the other kinds
  // their own map, and the launch takes the larger of the two
  const uint32_t mask = a.kind_mask;
  a.kind_mask = mask & kA16Plain;
  const int plain = geometry(a);
  a.kind_mask = mask;
  const A16Lds L = a16_lds(a, DOWN);
  const dim3 grid((unsigned)((int64_t)a.tiles_shared + (int64_t)a.E * a.tiles));
  hipLaunchKernelGGL((decode_a16_kernel<DOWN>), grid, dim3(kThreadsD), plain > L.bytes ? plain : L.bytes, (hipStream_t)stream, a);
  return launched(DOWN ? "decode_down_a16_kernel" : "decode_gate_up_a16_kernel");
}

}  // namespace decode
}  // namespace
}  // namespace mxmoe
