// moe_decode_f8g.h — the decode forward for block-scaled FP8 experts (the _f8g entries of include/mxmoe_moe.h:
// mxmoe_moe_decode_gate_up_f8g, mxmoe_moe_decode_down_f8g), gfx950. Included by moe_ops.hip after moe_decode_mfma.h.
//   MXMOE_DECODE_W8A8_G128_E4M3  e4m3 A codes with one f32 scale per (row, 128-element K group), e4m3 B codes with one
//                                f32 scale per 128 x 128 block — w8a8_g128_sym_E4M3, the GroupGEMM's operands in place
// A kernel of its own, decode_f8g_kernel<DOWN>: the MFMA tile without the bodies of the other fifteen kinds, so its
// register allocation is the tile's. Args, the grid, the id scan, the status bits, geometry()'s ct, pair-order outputs,
// load_h8 and glu_out are moe_decode.h's; the operand mapping is lp_tile's E4M3 mapping (moe_decode_mfma.h).
//
// Arithmetic. Every K group g is one v_mfma_scale_f32_16x16x128_f8f6f4 on a zero accumulator with unit e8m0 scales,
// acc_g, folded in f32: out = fmaf(acc_g, f32_rn(sa[row][g] * sb[g][blk]), out), plain C++ on the MFMA's result (the
// compiler places the MFMA-to-VALU wait states). Groups ascend within a wave's K slice; the slices' partial sums are
// added in slice order; v = fp16_rn(out). One slice: the GroupGEMM's contract word for word.
//
// Waves and K slices. A tile of `ct` columns is cg = ct / 16 groups of 16 columns. The four waves form cl = min(cg, 4)
// column lanes times ks = 4 / cl K slices: ct = 32 is 2 x 2 (no wave idles), ct = 64 is 4 x 1, ct = 128 is 4 x 1 with
// two passes over the column groups. Wave w is column lane w % cl of slice w / cl. A slice owns a contiguous run of
// the K / 128 groups, ceil(G / ks) each, the last what remains (none for K = 128, ks = 2). Slices >= 1 write their
// accumulators to LDS; after a barrier slice 0 adds them and runs the epilogue. Every barrier is reached by all four
// waves: the batch loop, the pass loop and ks are workgroup-uniform, and no wave leaves a loop early.
//
// Per K step a lane (r16 = lane & 15, g = lane >> 4) loads bytes [128 s + 16 g, + 16) and [128 s + 64 + 16 g, + 16)
// of weight row r16 of the group (gate_up: of the gate and of the up row) from global memory straight into the MFMA's
// registers, four steps (128 B per lane and weight row) in flight before the first is multiplied, and with them the
// trip's sb values: one f32 per weight-row block and K group, wave-uniform for a 16-column group (16 | 128; gate_up
// two: block n / 128 and block (C + n) / 128, C % 128 == 0). The lane ends with batch row r16 on columns 4 g .. 4 g + 3
// of the group: one 8-byte store.
//
// LDS (f8g_lds, one function for the host's byte count and the kernel's map):
//   [0, 32)    the head that lanes r16 >= nr read instead of a row: zero codes and the scale 0.0f (acc_g = 0 and a
//              zero scale keep their never-stored columns finite for finite sb)
//   codes      rb rows, `row` = Kmax + 16 bytes apart: an odd number of 16-byte slots, so a ds_read_b128 pass over 16
//              rows is conflict-free (as lp_tile)
//   scales     rb rows of Kmax / 128 f32, `srow` bytes apart: an odd number of dwords
//   partials   (ks - 1) * cl areas of 64 lanes x NW x 16 bytes
// rb = min(T, 16, what fits kLdsBudget); more rows than a batch re-stream the weights. Wave w quantises rows w, w + 4,
// ... of the batch as act_quant_kernel does for MXMOE_ACT_E4M3_G128, bit for bit: a 16-lane butterfly amax per group,
// s = f32(amax) / 448 (1 for a zero group), codes from the IEEE quotient clamped to +-448, an Inf / NaN group zero
// codes and a NaN scale.
#pragma once

namespace mxmoe {
namespace {
namespace decode {

constexpr int kF8g = 4;  // the entry pair's number beside kFirst .. kLp: no level of decode_kernel
constexpr int kF8gHead = 32;
struct F8gLds {
  int rb, row, srow;      // A rows per batch; bytes between code rows / between scale rows
  int cl, ks;             // column lanes and K slices of the four waves
  int code, scale, part;  // byte offsets of the three areas
  int bytes;              // of the whole map
};
__host__ __device__ inline F8gLds f8g_lds(const Args& a, bool down) {
  const int kmax = a.with_shared && a.K_shared > a.K ? a.K_shared : a.K;
  F8gLds L;
  const int cg = a.ct / 16;
  L.cl = cg < 4 ? cg : 4;
  L.ks = 4 / L.cl;
  L.row = kmax + 16;
  L.srow = 4 * ((kmax >> 7) | 1);
  const int parts = (L.ks - 1) * L.cl * 64 * (down ? 1 : 2) * 16;
  int rb = (kLdsBudget - kF8gHead - parts) / (L.row + L.srow);
  rb = rb < 1 ? 1 : rb > kBatchRows ? kBatchRows : rb;
  L.rb = rb > a.T ? a.T : rb;
  L.code = kF8gHead;
  L.scale = L.code + L.rb * L.row;
  L.part = (L.scale + L.rb * L.srow + 15) & ~15;
  L.bytes = L.part + parts;
  return L;
}

// One row (K fp16, or bf16 converted) quantised by one wave as act_quant_kernel quantises it for MXMOE_ACT_E4M3_G128
// (the same expressions): the codes to `row`, the groups' f32 scales to `sc`. A group is 16 adjacent lanes of a chunk.
__device__ __forceinline__ void f8g_quant_row(const uint8_t* __restrict__ src, int K, bool bf, uint8_t* row, float* sc) {
  const int lane = threadIdx.x & 63;
  for (int c0 = 0; c0 < K; c0 += 512) {  // (uniform: the group amax crosses lanes)
    const int idx = c0 + lane * 8;
    const bool in = idx < K;
    h8_t x = load_h8(src, in ? idx : 0, bf);
    if (!in) x = h8_t{0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t mi = amax8_bits(x);
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) mi = max(mi, (uint32_t)__shfl_xor((int)mi, d, 64));
    if (!in) continue;
    const bool bad = mi >= 0x7C00u;  // an Inf or a NaN in the group: NaN scale, zero codes
    float s = (float)__builtin_bit_cast(_Float16, (uint16_t)mi) / 448.0f;
    if (mi == 0) s = 1.0f;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = __builtin_amdgcn_fmed3f((float)x[j] / s, -448.0f, 448.0f);
    int q0 = 0, q1 = 0;  // pack_wxax's 8-bit order
    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[1], y[0], q0, false);
    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[3], y[2], q0, true);
    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[5], y[4], q1, false);
    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[7], y[6], q1, true);
    *reinterpret_cast<uint2*>(row + idx) = bad ? uint2{0u, 0u} : uint2{(uint32_t)q0, (uint32_t)q1};
    if ((lane & 15) == 0) sc[idx >> 7] = bad ? __builtin_nanf("") : s;
  }
}

// DOWN = false: decode_gate_up_f8g; true: decode_down_f8g.
template <bool DOWN>
__global__ __launch_bounds__(kThreadsD) void decode_f8g_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_a[];  // f8g_lds's map
  __shared__ int s_rows[kMaxPairs];
  __shared__ int s_cnt[kThreadsD / 64];
  constexpr int NW = DOWN ? 1 : 2;  // weight rows per lane: down 1; gate_up the gate and the up row
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
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
  if ((DOWN ? ex.kind2 : ex.kind1) != MXMOE_DECODE_W8A8_G128_E4M3) {
    if (tid == 0 && a.status) atomicOr(a.status, MXMOE_DECODE_BAD_KIND);
    return;
  }
  // the bias row of the workgroup's own expert (e < E by the grid's size): never indexed by an id
  const _Float16* brow = nullptr;
  if constexpr (!DOWN) brow = shared ? a.bias_shared : a.bias_routed ? a.bias_routed + (int64_t)e * 2 * a.C : nullptr;

  const int K = shared ? a.K_shared : a.K, C = shared ? a.C_shared : a.C;
  const int G = K >> 7;                             // K groups
  const int nblk = ((DOWN ? C : 2 * C) + 127) >> 7;  // weight-row blocks: sb is [G][nblk]
  const uint8_t* const B = static_cast<const uint8_t*>(DOWN ? ex.b2 : ex.b1);
  const float* const SB = static_cast<const float*>(DOWN ? ex.sb2 : ex.sb1);
  const uint8_t* const src = static_cast<const uint8_t*>(shared ? a.src_shared : a.src);
  _Float16* const out = shared ? a.out_shared : a.out;
  const F8gLds L = f8g_lds(a, DOWN);
  uint8_t* const s_code = s_a + L.code;
  uint8_t* const s_sc = s_a + L.scale;
  if (tid < kF8gHead / 4) reinterpret_cast<uint32_t*>(s_a)[tid] = 0u;

  // the wave's column lane and K slice, and the slice's groups [g0, g1)
  const int cw = wave % L.cl, sl = wave / L.cl;
  const int per = (G + L.ks - 1) / L.ks;
  const int g0 = sl * per < G ? sl * per : G, g1 = g0 + per < G ? g0 + per : G;
  const int passes = a.ct / (16 * L.cl);  // 1, or 2 for ct = 128

  for (int r0 = 0; r0 < nrows; r0 += L.rb) {
    const int nr = min(L.rb, nrows - r0);
    __syncthreads();  // s_rows and the head are complete; the previous batch's A rows and partial sums are no longer read
    for (int r = wave; r < nr; r += kThreadsD / 64) {
      const int p = shared ? r0 + r : s_rows[r0 + r];      // token (shared) or pair
      const int srow = (shared || DOWN) ? p : p / a.topk;  // gate_up reads the pair's token
      f8g_quant_row(src + (int64_t)srow * K * 2, K, !DOWN && a.src_bf16, s_code + r * L.row,
                    reinterpret_cast<float*>(s_sc + r * L.srow));
    }
    __syncthreads();
    const bool live = r16 < nr;  // lanes past the batch read the head: zero codes, a zero scale
    const int orow = live ? (shared ? r0 + r16 : s_rows[r0 + r16]) : 0;
    const uint8_t* const arow = live ? s_code + r16 * L.row + 16 * g : s_a;
    const float* const asc = reinterpret_cast<const float*>(live ? s_sc + r16 * L.srow : s_a + 16);
    const int ainc = live ? 128 : 0, ahalf = live ? 64 : 0, scinc = live ? 1 : 0;

    for (int pass = 0; pass < passes; ++pass) {  // (workgroup-uniform; every column group lies inside C: ct | C)
      const int n = tile * a.ct + 16 * (cw + L.cl * pass);
      // the lane's weight rows: down row n + r16; gate_up the gate and the up row of column n + r16. Their scale blocks
      // are the wave's: 16 | 128
      const uint8_t* w[NW];
      const float* ws[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        w[i] = B + (int64_t)(i * C + n + r16) * K + 16 * g;
        ws[i] = SB + ((i * C + n) >> 7);
      }
      lp_v4f acc[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) acc[i] = lp_v4f{0.0f, 0.0f, 0.0f, 0.0f};

      for (int s0 = g0; s0 < g1; s0 += 4) {
        lp_v4i lo[NW][4], hi[NW][4];
        float sb[NW][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // the trip's loads, all in flight; a step past the slice: the row's first bytes
          const int s = s0 + u < g1 ? s0 + u : 0;
#pragma unroll
          for (int i = 0; i < NW; ++i) {
            lo[i][u] = *reinterpret_cast<const lp_v4i*>(w[i] + s * 128);
            hi[i][u] = *reinterpret_cast<const lp_v4i*>(w[i] + s * 128 + 64);
            sb[i][u] = ws[i][s * nblk];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < g1) {  // wave-uniform
            const uint8_t* const ap = arow + (s0 + u) * ainc;
            const lp_v4i a0 = *reinterpret_cast<const lp_v4i*>(ap);
            const lp_v4i a1 = *reinterpret_cast<const lp_v4i*>(ap + ahalf);
            const float sa = asc[(s0 + u) * scinc];
            const lp_v8i av = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
            for (int i = 0; i < NW; ++i) {
              const lp_v8i bv = {lo[i][u][0], lo[i][u][1], lo[i][u][2], lo[i][u][3],
                                 hi[i][u][0], hi[i][u][1], hi[i][u][2], hi[i][u][3]};
              const lp_v4f t = lp_mfma<true, true>(bv, 127u, av, 127u, lp_v4f{0.0f, 0.0f, 0.0f, 0.0f});
              const float sc = sa * sb[i][u];  // f32_rn(sa * sb), rounded on its own
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(t[j], sc, acc[i][j]);
            }
          }
        }
      }

      if (L.ks > 1) {  // (workgroup-uniform) the K slices' partial sums through LDS, added in slice order
        lp_v4f* const part = reinterpret_cast<lp_v4f*>(s_a + L.part);
        if (sl > 0) {
#pragma unroll
          for (int i = 0; i < NW; ++i) part[(((sl - 1) * L.cl + cw) * NW + i) * 64 + lane] = acc[i];
        }
        __syncthreads();
        if (sl == 0) {
          for (int k = 1; k < L.ks; ++k) {
#pragma unroll
            for (int i = 0; i < NW; ++i) acc[i] += part[(((k - 1) * L.cl + cw) * NW + i) * 64 + lane];
          }
        }
      }

      // lane (r16, g) of slice 0: row r16 of the batch, output columns n + 4 g + 0..3
      if (sl == 0 && live) {
        const int col = n + 4 * g;
        typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
        h4_t o;
        if constexpr (DOWN) {
          o = h4_t{(_Float16)acc[0][0], (_Float16)acc[0][1], (_Float16)acc[0][2], (_Float16)acc[0][3]};
        } else {
          const bool has_b = brow != nullptr;  // workgroup-uniform
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const _Float16 bg = has_b ? brow[col + j] : (_Float16)0, bu = has_b ? brow[C + col + j] : (_Float16)0;
            const _Float16 gv = (_Float16)acc[0][j], uv = (_Float16)acc[NW - 1][j];
            o[j] = a.glu == kGluSwigluClamp ? glu_out<kGluSwigluClamp>(gv, uv, has_b, bg, bu, a.limit, a.c)
                                            : glu_out<kGluSilu>(gv, uv, has_b, bg, bu, a.limit, a.c);
          }
        }
        *reinterpret_cast<h4_t*>(out + (int64_t)orow * C + col) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side: the _f8g entries' own checks (before any HIP call) and the launch

inline int f8g_checks(const char* fn, uint32_t kind_mask, int layout) {
  if (kind_mask != 1u << MXMOE_DECODE_W8A8_G128_E4M3)
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "%s: kind_mask %#x must be exactly 1 << MXMOE_DECODE_W8A8_G128_E4M3 (%#x): "
                "w8a8_g128_sym_E4M3 is not mixed with other kinds in one launch", fn, kind_mask,
                1u << MXMOE_DECODE_W8A8_G128_E4M3);
  if (layout != MXMOE_DECODE_GU_PLAIN)
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "%s: layout must be MXMOE_DECODE_GU_PLAIN (got %d): w8a8_g128_sym_E4M3 has no "
                "SiLU-epilogue layout", fn, layout);
  return MXMOE_GG_OK;
}

template <bool DOWN>
inline int launch_f8g(Args a, void* stream) {
  geometry(a);  // ct and the tiles; the LDS map is this kernel's own
  const F8gLds L = f8g_lds(a, DOWN);
  const dim3 grid((unsigned)((int64_t)a.tiles_shared + (int64_t)a.E * a.tiles));
  hipLaunchKernelGGL((decode_f8g_kernel<DOWN>), grid, dim3(kThreadsD), L.bytes, (hipStream_t)stream, a);
  return launched(DOWN ? "decode_down_f8g_kernel" : "decode_gate_up_f8g_kernel");
}

}  // namespace decode
}  // namespace
}  // namespace mxmoe
