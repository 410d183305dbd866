// moe_decode.h — the decode forward's two kernels (mxmoe_moe_decode_gate_up, mxmoe_moe_decode_down of
// include/mxmoe_moe.h, and their _ex and _wo forms), gfx950. Included by moe_ops.hip after its quantiser helpers, which
// the kernels call as they are (rtn_scale, div_f16_operands, codes_i8, codes_i4, amax8, bf16x8_to_f16, glu_value): the
// quantised rows are byte for byte what act_quant_kernel writes.
//
// A forward of 1..16 tokens has at most a few hundred (token, choice) pairs, so no tile table is planned: every
// workgroup reads all T * topk ids and finds the rows of its own expert. Both kernels are weight streamers — no MFMA,
// the integer dot products on v_dot4_i32_i8 / v_dot8_i32_i4, everything else on v_fma_mix_f32.
//
// One structure: decode_kernel<DOWN, LEVEL> finds the workgroup's rows and switches once on the expert's kind to
// expert_tile<DOWN, Policy, EX> (batches of A rows into LDS, the tile's columns, the epilogue), which calls
// dot_rows<Policy> (the accumulators, the loads in flight, the row sums). A policy is what differs between kinds:
//   Plain<KIND>    fp16, w8a8, w4a4: A quantised to the weights' width, packed words multiplied as they are
//   Mx             W4A16_MX: fp16 A, e2m1 codes dequantised with a block's e8m0 byte
//   WeightOnly<B>  kinds 4..11 (w4a16 / w8a16): fp16 A, integer codes dequantised with a (scale, zp) pair
// LEVEL is the entry pair: kFirst (the plain kinds, SiLU), kEx (the _ex entries, gpt-oss layers: also Mx, and in
// gate_up the biases and the gated activation of an mxmoe_moe_glu) or kWo (the _wo entries: also WeightOnly). A
// level's kernel contains its own kinds' bodies only.
//
// Mapping. One workgroup (256 threads) per (expert, tile of `ct` output columns); the shared expert's tiles come
// first in the grid (its rows are the most: all T). A workgroup whose expert has no row returns after the id scan.
//   rows      thread i < T * topk holds id i; the pairs whose id is the workgroup's expert are listed in pair order
//             (ballot + prefix over the 4 waves). The shared expert's rows are the tokens 0..T-1.
//   A rows    wave w stages rows w, w + 4, ... of the batch into LDS by the policy (Policy::stage). A batch is `rb`
//             rows (16, or what fits the LDS budget for very wide rows; more rows than a batch — only with repeated
//             ids — re-read the weights).
//   dot       a quarter-wave (16 lanes) owns two weight rows at a time (gate_up: gate and up row of one output column;
//             down: output columns n and n + 16): lane l holds bytes [256 s + 16 l, + 16) of step s of both rows, four
//             steps (8 loads of 16 B, and what the policy loads with them) in flight, and multiplies them with the same
//             K positions of every A row of the batch (LDS, a broadcast across the 4 quarters of a wave). An
//             accumulator takes its terms step ascending, within a step run ascending, within a run element ascending.
//             The 16 partial sums of a row are added with four DPP steps inside the 16-lane row (integers: exact;
//             otherwise f32 in that order). A lane past the row's end (only inside the last step) loads the row's
//             first bytes and zeroes what it loaded: +0 weights on the A rows' zero pad.
//   epilogue  lane r of the quarter finishes row r (Policy::finish), gate_up: the activation, then a 2-byte store to
//             row `pair` of the output (pair order: no permutation).
// Nothing is indexed by an id: an id outside [0, E) matches no workgroup, its pair's rows stay as they were, and the
// first routed workgroup sets MXMOE_DECODE_BAD_ID in the status word. The expert record and the bias row are indexed by
// the workgroup's own expert number. A kind outside the call's kind_mask (which sized the LDS rows) sets
// MXMOE_DECODE_BAD_KIND and the workgroup writes nothing.
//
// The policies' A rows and K maps.
//   Plain      pack_wxax order, the K permutation of the weight rows: packed 32-bit words of A and B multiply element
//              by element. One pass for the row's amax, one for the codes (fp16: a copy); 256 LDS bytes per step.
//              finish: the GroupGEMM's scale arithmetic.
//   Mx         a step is 16 MX blocks of 16 bytes: lane l owns block 16 s + l, elements K = 512 s + 32 l + 8 j + 0..7
//              in dword (run) j, and reads one e8m0 byte of the device scale layout. A dword is dequantised with the
//              GroupGEMM's convert and reused for every A row of the batch.
//   WeightOnly mxmoe_gg_repack_weightonly's codes and the [G][rows] / [G][rows][2] fp16 scale buffer. A lane's 16 bytes
//              are whole K runs of 8 (one dword of 4-bit, two dwords of 8-bit codes):
//                4-bit  run j (0..3) of lane l: K = 512 s + 64 (l >> 1) + 32 (j & 1) + 8 (2 (l & 1) + (j >> 1)) + 0..7
//                8-bit  run j (0..1) of lane l: K = 256 s + 64 (l >> 2) + 32 j + 8 (l & 3) + 0..7
//              dequantised a run at a time, b = fp16(fma(u - off, scale, zp)) by the GroupGEMM's steps (wo_dequant of
//              gg_device.h: 0x6400 | u, an exact packed add, one packed fma). The group size and the symmetry come from
//              the record's kind as workgroup-uniform values. Per-channel: the two rows' (scale, zp), loaded once per
//              weight row; g128: one pair per lane, step and row — group 4 s + (l >> 2) (4-bit) or 2 s + (l >> 3)
//              (8-bit) — loaded with the step's codes.
//   fp16 A     (Mx, WeightOnly) the row is not quantised but permuted inside every step (256 B of 4-bit codes: 512 K =
//              1024 LDS bytes; of 8-bit codes: 256 K = 512 bytes) so that the 8 elements of run j of lane l lie at
//              LDS byte kStepLds s + 256 j + 16 l of the row: a lane's j-th ds_read_b128 of a step is the plain kinds'
//              conflict-free pattern (stage_f16).
#pragma once

namespace mxmoe {
namespace {
namespace decode {

constexpr int kThreadsD = 256;
constexpr int kMaxPairs = MXMOE_DECODE_MAX_T * 16;  // T <= 16, topk <= 16
constexpr int kBatchRows = 16;                      // A rows per batch: the accumulators a lane keeps per weight row
constexpr int kLdsBudget = 60 * 1024;               // dynamic LDS of a workgroup (the A rows of one batch)
constexpr int kMaxWidthD = 16384;

// level: which entries — kFirst, kEx (also W4A16_MX, biases, the gated activation) or kWo (also the kinds 4..11)
enum { kFirst = 0, kEx = 1, kWo = 2 };

struct Args {
  const void* src;         // gate_up: hidden [T][K] (fp16 or bf16); down: act [T * topk][K]
  const void* src_shared;  // gate_up: hidden; down: act_shared [T][K_shared]
  const int32_t* ids;      // [T][topk]
  const mxmoe_moe_decode_expert* experts;
  _Float16* out;           // gate_up: act [T * topk][C]; down: y [T * topk][C]
  _Float16* out_shared;    // [T][C_shared]
  int32_t* status;
  int T, topk, E, with_shared;
  int K, K_shared;          // elements per A row (routed / shared expert)
  int C, C_shared;          // output columns
  int tiles, tiles_shared;  // column tiles per routed expert / of the shared expert
  int ct;                   // output columns per tile (32, 64 or 128)
  int rb;                   // A rows per batch
  int lds_row;              // bytes per A row in LDS (the widest row of the kinds in kind_mask, up to 1024)
  int layout, src_bf16;
  uint32_t kind_mask;
  // kEx, kWo (gate_up): the biases and the gated activation of an mxmoe_moe_glu, as GluArgs carries them
  const _Float16* bias_routed;  // [E][2 C] ([gate | up] columns) or NULL
  const _Float16* bias_shared;  // [2 C_shared] or NULL
  int glu;                      // kGluSilu / kGluSwigluClamp
  float c, limit;               // SWIGLU_CLAMP: -(alpha log2 e), the clamp
};

// the weight-only kinds (the _wo entries): kind = 4 + (w_bits == 8) + 2 * (gsize == 128) + 4 * asym
__host__ __device__ inline bool wo_kind(int kind) { return kind >= MXMOE_DECODE_W4A16; }
__host__ __device__ inline int wo_bits(int kind) { return ((kind - MXMOE_DECODE_W4A16) & 1) ? 8 : 4; }
__host__ __device__ inline bool wo_g128(int kind) { return ((kind - MXMOE_DECODE_W4A16) & 2) != 0; }
__host__ __device__ inline bool wo_asym(int kind) { return ((kind - MXMOE_DECODE_W4A16) & 4) != 0; }

// bytes of a weight row in global memory, and of an A row in LDS: the integer kinds quantise A to the weights' width,
// W4A16_MX and the weight-only kinds keep the fp16 row
__host__ __device__ inline int b_row_bytes(int kind, int K) {
  return kind == MXMOE_DECODE_FP16 ? 2 * K : kind == MXMOE_DECODE_W8A8 ? K : K / 2;
}
__host__ __device__ inline int a_row_bytes(int kind, int K) {
  return kind == MXMOE_DECODE_W4A16_MX || wo_kind(kind) ? 2 * K : b_row_bytes(kind, K);
}

// sum over the 16 lanes of a DPP row (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror): every lane
// of the row ends with the total
template <class T>
__device__ __forceinline__ T row16_sum(T v) {
#define MXMOE_DEC_STEP(ctrl)                                                                              \
  {                                                                                                       \
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false);      \
    v = v + __builtin_bit_cast(T, o);                                                                     \
  }
  MXMOE_DEC_STEP(0xB1) MXMOE_DEC_STEP(0x4E) MXMOE_DEC_STEP(0x141) MXMOE_DEC_STEP(0x140)
#undef MXMOE_DEC_STEP
  return v;
}

// acc += f32(w) * f32(a) over 8 fp16 elements, element ascending (v_fma_mix_f32)
__device__ __forceinline__ float dot_h8(const h8_t& w, const uint4& a, float acc) {
  const h8_t av = __builtin_bit_cast(h8_t, a);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = fmaf((float)w[j], (float)av[j], acc);
  return acc;
}
// the GroupGEMM's scaled epilogue: fp16_rn(0 + f32(acc) * f32(fp16_rn(sa * sb))), the f32 product rounded on its own
// (the empty asm keeps the multiply and the conversion from fusing into one rounding)
__device__ __forceinline__ _Float16 scaled_out(int acc, _Float16 sa, _Float16 sb) {
  const _Float16 s16 = sa * sb;
  float prod = (float)acc * (float)s16;
  asm volatile("" : "+v"(prod));
  return (_Float16)(0.0f + prod);
}

// act = fp16_rn(silu(f32 g) * f32 u): act_quant_kernel's expression. The product is rounded to f32 and then to fp16, as
// there and in the GroupGEMM's SiLU epilogue (the empty asm keeps hipcc from fusing the multiply and the conversion
// into one v_fma_mixlo_f16: a single rounding, and +0 where the product is -0)
__device__ __forceinline__ _Float16 silu_mul(_Float16 g16, _Float16 u16) {
  const float g = (float)g16;
  const float sg = g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f));
  float p = sg * (float)u16;
  asm volatile("" : "+v"(p));
  return (_Float16)p;
}

// The kEx / kWo gate_up epilogue: mxmoe_moe_glu_quant's arithmetic on the fp16 g, u (the GLU builds of
// act_quant_kernel: one f32 add per bias, then glu_value — that pass's own helper), the f32 product rounded on its own
// as in silu_mul. has_b false and kGluSilu: silu_mul's value bit for bit.
template <int GLU>
__device__ __forceinline__ _Float16 glu_out(_Float16 g16, _Float16 u16, bool has_b, _Float16 bg, _Float16 bu, float limit,
                                            float c) {
  float g = (float)g16, v = (float)u16;
  if (has_b) {
    g = g + (float)bg;
    v = v + (float)bu;
  }
  float p = glu_value<GLU>(g, v, limit, c);
  asm volatile("" : "+v"(p));
  return (_Float16)p;
}

// W4A16_MX: 8 e2m1 codes (a dword, element 2i the low nibble of byte i) times 2^(byte - 127) as fp16, by the
// GroupGEMM's convert (wo_dequant_mx of gg_device.h: v_cvt_scalef32_pk_f16_fp4 on the f32 byte << 23), so b[n][k] is
// the GroupGEMM's fp16 value for every scale byte.
__device__ __forceinline__ h8_t dequant_mx(uint32_t w, uint32_t scale_bits) {
  const float sc = __builtin_bit_cast(float, scale_bits);
  const h2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 0);
  const h2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 1);
  const h2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 2);
  const h2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 3);
  return h8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// The weight-only kinds: 8 codes (K ascending: one dword of 4-bit codes, 2q and 2q + 1 at bits 4q and 16 + 4q, or two
// dwords of bytes) to b = fp16(fma(u - off, scale, zp)), the GroupGEMM's steps (wo_dequant of gg_device.h): 0x6400 | u
// is the fp16 1024 + u, moff = -(1024 + off) makes u - off exactly (v_pk_add_f16), then one v_pk_fma_f16: one rounding.
template <int BITS>
__device__ __forceinline__ h8_t dequant_wo(uint32_t w0, uint32_t w1, h2_t moff, h2_t s2, h2_t z2) {
  h8_t out;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t d;
    if constexpr (BITS == 4) d = ((w0 >> (4 * q)) & 0x000F000Fu) | 0x64006400u;
    else d = __builtin_amdgcn_perm(0x64646464u, q < 2 ? w0 : w1, (q & 1) ? 0x04030402u : 0x04010400u);
    h2_t x = __builtin_bit_cast(h2_t, d) + moff;
    x = __builtin_elementwise_fma(x, s2, z2);
    out[2 * q] = x[0];
    out[2 * q + 1] = x[1];
  }
  return out;
}

__device__ __forceinline__ h8_t load_h8(const uint8_t* __restrict__ src, int idx, bool bf) {
  const uint4 v = *reinterpret_cast<const uint4*>(src + 2 * idx);
  return bf ? bf16x8_to_f16(v) : __builtin_bit_cast(h8_t, v);
}

// Row `src` (K fp16, or bf16 converted as mxmoe_moe_gather_quant does) quantised by KIND's tag (fp16: copied) into
// `row` (LDS, pack_wxax order) by one wave, zeros behind it up to a multiple of 1024 bytes (the dot loop's group of four
// 256-byte steps reads the pad); its scale to *scale. The arithmetic and the helpers are act_quant_kernel's.
template <int KIND>
__device__ __forceinline__ void quant_row(const uint8_t* __restrict__ src, int K, bool bf, uint8_t* row, _Float16* scale) {
  const int lane = threadIdx.x & 63;
  const int KB = b_row_bytes(KIND, K);
  for (int o = KB + lane * 16; o < ((KB + 1023) & ~1023); o += 1024) *reinterpret_cast<uint4*>(row + o) = uint4{0, 0, 0, 0};
  if constexpr (KIND == MXMOE_DECODE_FP16) {
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512) *reinterpret_cast<h8_t*>(row + 2 * idx) = load_h8(src, idx, bf);
    return;
  }
  float m = 0.0f;
#pragma unroll 4
  for (int idx = lane * 8; idx < K; idx += 512) m = fmaxf(m, amax8(load_h8(src, idx, bf)));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  const float qmax = KIND == MXMOE_DECODE_W8A8 ? 127.0f : 7.0f;
  const h2_t lim = {(_Float16)qmax, (_Float16)qmax};
  const _Float16 sc = rtn_scale(m, qmax);
  const float rs = __builtin_amdgcn_rcpf((float)sc);
  if (lane == 0) *scale = sc;
  if constexpr (KIND == MXMOE_DECODE_W8A8) {
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512)
      *reinterpret_cast<uint2*>(row + idx) = codes_i8(load_h8(src, idx, bf), (float)sc, rs, lim);
  } else {
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512)
      *reinterpret_cast<uint32_t*>(row + idx / 2) = codes_i4(load_h8(src, idx, bf), (float)sc, rs, lim);
  }
}

// The fp16 row (or bf16 converted), not quantised, permuted inside every 1024 bytes for a policy's K map: 16-byte slot
// 16 j + l of a pass holds the 8 elements `src_el` of lane 16 j + l of the copying wave, counted from the pass's first
// element. So the stores are the plain copy's (consecutive lanes, consecutive slots: all 64 banks once) and only the
// global address is permuted. Pieces past the row are zeros up to a multiple of 1024 bytes.
__device__ __forceinline__ void stage_f16(const uint8_t* __restrict__ src, int K, bool bf, uint8_t* row, int src_el) {
  const int lane = threadIdx.x & 63;
  for (int o = 0; o < ((2 * K + 1023) & ~1023); o += 1024) {
    const int idx = (o >> 1) + src_el;
    h8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (idx < K) v = load_h8(src, idx, bf);
    *reinterpret_cast<h8_t*>(row + o + lane * 16) = v;
  }
}

// The policies. What dot_rows and expert_tile ask of one (SB: the weight's scale buffer; r0, r1: the quarter's two
// weight rows; KB: bytes of a weight row; rows: of the weight; kind: the record's; l: the lane of the quarter):
//   acc_t, kStepLds, kRuns   the accumulator; LDS bytes of an A row per step; 16-byte A reads per step
//   kHold                    steps whose multiplicands a lane holds while it walks the A rows: all four where they are
//                            the loaded words themselves, one where they are dequantised (8 weights of each row live)
//   row_bytes(K), stage(..)  of a weight row; an A row into LDS by one wave
//   side(which, s, in)       what is loaded with step s's 16 bytes of row `which`; neutral for a lane past the end
//   mul(w, side, j)          the multiplicands of run j of a step;  dot(m, a, acc): against 16 bytes of an A row
//   finish(acc, which, sa)   the output value; sa: the A row's scale
struct NoSide {};

template <int KIND>
struct Plain {
  typedef uint4 mul_t;
  typedef NoSide side_t;
  static constexpr bool kInt = KIND != MXMOE_DECODE_FP16;
  typedef typename std::conditional<kInt, int, float>::type acc_t;
  static constexpr int kStepLds = 256, kRuns = 1, kHold = 4;
  const _Float16* SB;
  int r[2];
  __device__ __forceinline__ Plain(const void* sb, int r0, int r1, int, int, int, int)
      : SB(static_cast<const _Float16*>(sb)), r{r0, r1} {}
  static __host__ __device__ int row_bytes(int K) { return b_row_bytes(KIND, K); }
  static __device__ __forceinline__ void stage(const uint8_t* __restrict__ src, int K, bool bf, uint8_t* row, _Float16* scale) {
    quant_row<KIND>(src, K, bf, row, scale);
  }
  __device__ __forceinline__ NoSide side(int, int, bool) const { return NoSide{}; }
  __device__ __forceinline__ const uint4& mul(const uint4& w, NoSide, int) const { return w; }
  static __device__ __forceinline__ acc_t dot(const uint4& w, const uint4& a, acc_t acc) {
    if constexpr (KIND == MXMOE_DECODE_FP16) {
      return dot_h8(__builtin_bit_cast(h8_t, w), a, acc);
    } else if constexpr (KIND == MXMOE_DECODE_W8A8) {
      acc = __builtin_amdgcn_sdot4((int)w.x, (int)a.x, acc, false);
      acc = __builtin_amdgcn_sdot4((int)w.y, (int)a.y, acc, false);
      acc = __builtin_amdgcn_sdot4((int)w.z, (int)a.z, acc, false);
      return __builtin_amdgcn_sdot4((int)w.w, (int)a.w, acc, false);
    } else {
      acc = __builtin_amdgcn_sdot8((int)w.x, (int)a.x, acc, false);
      acc = __builtin_amdgcn_sdot8((int)w.y, (int)a.y, acc, false);
      acc = __builtin_amdgcn_sdot8((int)w.z, (int)a.z, acc, false);
      return __builtin_amdgcn_sdot8((int)w.w, (int)a.w, acc, false);
    }
  }
  // fp16: fp16_rn(acc); the integer kinds: the per-row weight scale SB[row] and the A row's scale
  __device__ __forceinline__ _Float16 finish(acc_t acc, int which, const _Float16* sa) const {
    if constexpr (kInt) return scaled_out(acc, *sa, SB[r[which]]);
    else return (_Float16)acc;
  }
};

// the two dequantising policies' common part: f32 sums of fp16 products, rounded once, fp16_rn(acc)
struct F16Rows {
  typedef float acc_t;
  typedef h8_t mul_t;
  static constexpr int kHold = 1;
  static __device__ __forceinline__ float dot(const h8_t& w, const uint4& a, float acc) { return dot_h8(w, a, acc); }
  __device__ __forceinline__ _Float16 finish(float acc, int, const _Float16*) const { return (_Float16)acc; }
};

// W4A16_MX. A row's scales: 16 e8m0 bytes per step in the device layout (include/mxmoe_gg.h: dev[16 t + 4 g + i] =
// canon[16 t + 4 i + g]; pads 127), so block 16 s + l has byte 16 s + 4 (l & 3) + (l >> 2).
struct Mx : F16Rows {
  typedef uint32_t side_t;  // the block's scale as f32 bits
  static constexpr int kStepLds = 1024, kRuns = 4;
  const uint8_t* sb[2];
  int sl;
  __device__ __forceinline__ Mx(const void* SB, int r0, int r1, int KB, int, int, int l) : sl(4 * (l & 3) + (l >> 2)) {
    const int sr = ((KB + 255) >> 8) * 16;
    sb[0] = static_cast<const uint8_t*>(SB) + (int64_t)r0 * sr;
    sb[1] = static_cast<const uint8_t*>(SB) + (int64_t)r1 * sr;
  }
  static __host__ __device__ int row_bytes(int K) { return K / 2; }
  static __device__ __forceinline__ void stage(const uint8_t* __restrict__ src, int K, bool bf, uint8_t* row, _Float16*) {
    const int lane = threadIdx.x & 63;
    stage_f16(src, K, bf, row, 32 * (lane & 15) + 8 * (lane >> 4));
  }
  __device__ __forceinline__ uint32_t side(int which, int s, bool in) const {
    const uint32_t v = (uint32_t)sb[which][in ? s * 16 + sl : 0] << 23;
    return in ? v : 0u;
  }
  __device__ __forceinline__ h8_t mul(const uint4& w, uint32_t scale, int j) const {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
    return dequant_mx(d[j], scale);
  }
};

// The weight-only kinds, BITS: the code width. SB: fp16 [G][rows] or (asym) [G][rows][2] (scale, zp). A lane past the
// row's end loads group 0's pair and zeroes it: with its zeroed codes b = +0.
template <int BITS>
struct WeightOnly : F16Rows {
  typedef h2_t side_t;  // (scale, zp)
  static constexpr int kRuns = BITS == 4 ? 4 : 2;  // K runs of 8 in a lane's 16 bytes
  static constexpr int kStepLds = 256 * kRuns;
  static constexpr int kStepGroups = 16 / BITS;    // 128-K groups per step
  const _Float16* SB;
  int r[2], rows, sh, gl;  // element (g * rows + r) << sh: the scale; + 1 (asym): the zp. gl: the lane's group in a step
  bool g128, asym;
  h2_t moff, pc[2];  // -(1024 + off); per-channel: the two rows' pairs
  __device__ __forceinline__ WeightOnly(const void* sb, int r0, int r1, int, int rows_, int kind, int l)
      : SB(static_cast<const _Float16*>(sb)), r{r0, r1}, rows(rows_), sh(wo_asym(kind) ? 1 : 0),
        gl(BITS == 4 ? l >> 2 : l >> 3), g128(wo_g128(kind)), asym(wo_asym(kind)) {
    const _Float16 off = (_Float16)(asym ? -1024.0f : BITS == 4 ? -1031.0f : -1151.0f);  // -(1024 + 2^(BITS-1) - 1), sym
    moff = h2_t{off, off};
    pc[0] = pc[1] = h2_t{0, 0};
    if (!g128) {
      pc[0] = pair(r0, 0);
      pc[1] = pair(r1, 0);
    }
  }
  __device__ __forceinline__ h2_t pair(int row, int g) const {
    const int i = (g * rows + row) << sh;
    return h2_t{SB[i], asym ? SB[i + 1] : (_Float16)0};
  }
  static __host__ __device__ int row_bytes(int K) { return K * BITS / 8; }
  static __device__ __forceinline__ void stage(const uint8_t* __restrict__ src, int K, bool bf, uint8_t* row, _Float16*) {
    // 4-bit: a pass of 1024 bytes is a step; 8-bit: two steps of 512 bytes, slot 32 s' + 16 j + l for step s'
    const int lane = threadIdx.x & 63, l = lane & 15, j = lane >> 4;
    stage_f16(src, K, bf, row, BITS == 4 ? 64 * (l >> 1) + 32 * (j & 1) + 8 * (2 * (l & 1) + (j >> 1))
                                         : 256 * (j >> 1) + 64 * (l >> 2) + 32 * (j & 1) + 8 * (l & 3));
  }
  __device__ __forceinline__ h2_t side(int which, int s, bool in) const {
    const h2_t v = g128 ? pair(r[which], in ? s * kStepGroups + gl : 0) : pc[which];
    return in ? v : h2_t{0, 0};
  }
  __device__ __forceinline__ h8_t mul(const uint4& w, h2_t sz, int j) const {
    const uint32_t d[4] = {w.x, w.y, w.z, w.w};
    const int i = BITS == 4 ? j : 2 * j;
    return dequant_wo<BITS>(d[i], d[(i + 1) & 3], moff, h2_t{sz[0], sz[0]}, h2_t{sz[1], sz[1]});
  }
};

// The two weight rows w0, w1 (KB bytes each) of a quarter-wave against the nr A rows of the batch, and the rows'
// results: lane r (< nr) of the quarter returns row r's two outputs in *o0, *o1 (other lanes: unspecified). Whole
// steps past the row's end are loaded (the four steps in flight) and, where a lane holds one step at a time, not
// multiplied: the A rows are padded to a multiple of 1024 bytes.
template <class P>
__device__ __forceinline__ void dot_rows(const P& p, const uint8_t* __restrict__ w0, const uint8_t* __restrict__ w1, int KB,
                                         const uint8_t* A, int lds_row, const _Float16* s_scale, int nr, int l16,
                                         _Float16* o0, _Float16* o1) {
  typedef typename P::acc_t acc_t;
  acc_t acc0[kBatchRows], acc1[kBatchRows];
#pragma unroll
  for (int r = 0; r < kBatchRows; ++r) acc0[r] = acc1[r] = 0;
  const int S = (KB + 255) >> 8;
  for (int s0 = 0; s0 < S; s0 += 4) {
    uint4 wa[4], wb[4];
    typename P::side_t sa[4], sb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // 8 loads of 16 B and their side data in flight; past the row: the row's first bytes
      const int off = ((s0 + u) * 16 + l16) * 16;
      const bool in = off < KB;
      wa[u] = *reinterpret_cast<const uint4*>(w0 + (in ? off : 0));
      wb[u] = *reinterpret_cast<const uint4*>(w1 + (in ? off : 0));
      sa[u] = p.side(0, s0 + u, in);
      sb[u] = p.side(1, s0 + u, in);
    }
    if ((s0 + 4) * 256 > KB) {  // (uniform) the row ends inside this group: zero weights past it; the A rows' pad is zero
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t mk = ((s0 + u) * 16 + l16) * 16 < KB ? ~0u : 0u;
        wa[u].x &= mk, wa[u].y &= mk, wa[u].z &= mk, wa[u].w &= mk;
        wb[u].x &= mk, wb[u].y &= mk, wb[u].z &= mk, wb[u].w &= mk;
      }
    }
    int nrs = nr, ldr = lds_row;
    asm volatile("" : "+s"(nrs), "+s"(ldr));  // the 16 row tests and row offsets are made here, not kept in SGPRs
#pragma unroll
    for (int u0 = 0; u0 < 4; u0 += P::kHold) {
      if (s0 + u0 < S) {  // workgroup-uniform
#pragma unroll
        for (int j = 0; j < P::kRuns; ++j) {
          typename P::mul_t x0[P::kHold], x1[P::kHold];
#pragma unroll
          for (int h = 0; h < P::kHold; ++h) {
            x0[h] = p.mul(wa[u0 + h], sa[u0 + h], j);
            x1[h] = p.mul(wb[u0 + h], sb[u0 + h], j);
          }
          const uint8_t* const aj = A + (s0 + u0) * P::kStepLds + 256 * j + l16 * 16;  // (< lds_row: whole steps of the row)
#pragma unroll
          for (int r = 0; r < kBatchRows; ++r) {
            if (r < nrs) {  // workgroup-uniform
#pragma unroll
              for (int h = 0; h < P::kHold; ++h) {
                const uint4 av = *reinterpret_cast<const uint4*>(aj + r * ldr + h * P::kStepLds);
                acc0[r] = P::dot(x0[h], av, acc0[r]);
                acc1[r] = P::dot(x1[h], av, acc1[r]);
              }
            }
          }
        }
      }
    }
  }
  acc_t v0 = 0, v1 = 0;
  int lsel = l16, nrs = nr;
  asm volatile("" : "+v"(lsel), "+s"(nrs));  // the 16 lane masks and row tests below are formed here, not kept in SGPRs
#pragma unroll
  for (int r = 0; r < kBatchRows; ++r) {
    if (r < nrs) {
      const acc_t t0 = row16_sum(acc0[r]), t1 = row16_sum(acc1[r]);
      if (lsel == r) {
        v0 = t0;
        v1 = t1;
      }
    }
  }
  const _Float16* const sa = s_scale + (l16 < nr ? l16 : 0);
  *o0 = p.finish(v0, 0, sa);
  *o1 = p.finish(v1, 1, sa);
}

// One workgroup's work on an expert whose kind has policy P (`kind`: the record's own): per batch of rows, the A rows
// into LDS, then the tile's columns. EX: the kEx / kWo build — `brow`, the bias row of the workgroup's expert ([gate |
// up], or NULL), and the gated activation of Args in the gate_up epilogue. Without EX none of that code exists.
template <bool DOWN, class P, bool EX>
__device__ __forceinline__ void expert_tile(const Args& a, const mxmoe_moe_decode_expert& ex, int kind, bool shared,
                                            int tile, int nrows, uint8_t* s_a, const int* s_rows, _Float16* s_scale,
                                            const _Float16* brow) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int K = shared ? a.K_shared : a.K, C = shared ? a.C_shared : a.C;
  const int KB = P::row_bytes(K);  // of a weight row (the A row's bytes are <= lds_row: the kind is in the mask)
  const uint8_t* const B = static_cast<const uint8_t*>(DOWN ? ex.b2 : ex.b1);
  const void* const SB = DOWN ? ex.sb2 : ex.sb1;
  const uint8_t* const src = static_cast<const uint8_t*>(shared ? a.src_shared : a.src);
  _Float16* const out = shared ? a.out_shared : a.out;
  const int n0 = tile * a.ct;
  const int q = tid >> 4, l16 = tid & 15;
  const int rows = DOWN ? C : 2 * C;  // of the weight

  for (int r0 = 0; r0 < nrows; r0 += a.rb) {
    const int nr = min(a.rb, nrows - r0);
    __syncthreads();  // s_rows is complete; the previous batch's A rows are no longer read
    for (int r = wave; r < nr; r += kThreadsD / 64) {
      const int p = shared ? r0 + r : s_rows[r0 + r];      // token (shared) or pair
      const int srow = (shared || DOWN) ? p : p / a.topk;  // gate_up reads the pair's token
      P::stage(src + (int64_t)srow * K * 2, K, !DOWN && a.src_bf16, s_a + r * a.lds_row, s_scale + r);
    }
    __syncthreads();
    const int orow = l16 < nr ? (shared ? r0 + l16 : s_rows[r0 + l16]) : 0;
    for (int c = q; c < a.ct; c += DOWN ? 32 : 16) {
      // gate_up: column n, weight rows gate(n), up(n); down: columns n and n + 16, weight rows n, n + 16
      const int n = n0 + c;
      if (n + (DOWN ? 16 : 0) >= C) continue;
      int wr0, wr1;
      if constexpr (DOWN) {
        wr0 = n;
        wr1 = n + 16;
      } else if (a.layout == MXMOE_DECODE_GU_INTERLEAVED) {
        wr0 = 32 * (n >> 4) + (n & 15);
        wr1 = wr0 + 16;
      } else {
        wr0 = n;
        wr1 = C + n;
      }
      _Float16 o0, o1;
      dot_rows(P(SB, wr0, wr1, KB, rows, kind, l16), B + (int64_t)wr0 * KB, B + (int64_t)wr1 * KB, KB, s_a, a.lds_row,
               s_scale, nr, l16, &o0, &o1);
      if (l16 < nr) {
        _Float16* const orp = out + (int64_t)orow * C;
        if constexpr (DOWN) {
          orp[n] = o0;
          orp[n + 16] = o1;
        } else if constexpr (EX) {
          // the bias by column, whatever the weight layout: bg[n], bu[C + n] of the workgroup's own expert
          const bool has_b = brow != nullptr;  // workgroup-uniform
          const _Float16 bg = has_b ? brow[n] : (_Float16)0, bu = has_b ? brow[C + n] : (_Float16)0;
          orp[n] = a.glu == kGluSwigluClamp ? glu_out<kGluSwigluClamp>(o0, o1, has_b, bg, bu, a.limit, a.c)
                                            : glu_out<kGluSilu>(o0, o1, has_b, bg, bu, a.limit, a.c);
        } else {
          orp[n] = silu_mul(o0, o1);
        }
      }
    }
  }
}

// The kernel. DOWN = false: decode_gate_up; true: decode_down. It finds the workgroup's expert and column tile, the
// rows of that expert among the call's ids (in pair order, into s_rows), reports the ids that no workgroup matches, and
// runs the tile of the expert's kind: the kind is chosen once, outside the loops — one body per policy, one switch,
// and only the bodies of LEVEL's kinds.
template <bool DOWN, int LEVEL>
__global__ __launch_bounds__(kThreadsD) void decode_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_a[];  // [rb][lds_row]
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
  if (kind < 0 || kind > 31 || !((a.kind_mask >> kind) & 1u)) {  // (the mask holds LEVEL's kinds only: the entry's check)
    if (tid == 0 && a.status) atomicOr(a.status, MXMOE_DECODE_BAD_KIND);
    return;
  }
  constexpr bool EX = LEVEL != kFirst;
  // the bias row of the workgroup's own expert (e < E by the grid's size): never indexed by an id
  const _Float16* brow = nullptr;
  if constexpr (EX && !DOWN) brow = shared ? a.bias_shared : a.bias_routed ? a.bias_routed + (int64_t)e * 2 * a.C : nullptr;
#define MXMOE_DEC_TILE(...) expert_tile<DOWN, __VA_ARGS__, EX>(a, ex, kind, shared, tile, nrows, s_a, s_rows, s_scale, brow)
  if (kind == MXMOE_DECODE_FP16) return MXMOE_DEC_TILE(Plain<MXMOE_DECODE_FP16>);
  if (kind == MXMOE_DECODE_W8A8) return MXMOE_DEC_TILE(Plain<MXMOE_DECODE_W8A8>);
  if (LEVEL == kFirst || kind == MXMOE_DECODE_W4A4) return MXMOE_DEC_TILE(Plain<MXMOE_DECODE_W4A4>);
  if constexpr (LEVEL >= kEx) {
    if (LEVEL == kEx || kind == MXMOE_DECODE_W4A16_MX) return MXMOE_DEC_TILE(Mx);
    if constexpr (LEVEL == kWo) {
      if (wo_bits(kind) == 4) return MXMOE_DEC_TILE(WeightOnly<4>);
      return MXMOE_DEC_TILE(WeightOnly<8>);
    }
  }
#undef MXMOE_DEC_TILE
}

// ---------------------------------------------------------------------------------------------
// host side: the entries' checks (before any HIP call) and the launch geometry

inline int kind_mask_check(const char* fn, uint32_t kind_mask, int level = kFirst) {
  if (level == kWo) {
    if (kind_mask >> (MXMOE_DECODE_W8A16_G128_ASYM + 1))
      return fail(MXMOE_GG_ERR_UNSUPPORTED, "%s: unknown expert kind in kind_mask %#x (kinds 0 to %d only)", fn, kind_mask,
                  (int)MXMOE_DECODE_W8A16_G128_ASYM);
  } else {
    const bool ex = level == kEx;
    const uint32_t known = 1u << MXMOE_DECODE_FP16 | 1u << MXMOE_DECODE_W8A8 | 1u << MXMOE_DECODE_W4A4 |
                           (ex ? 1u << MXMOE_DECODE_W4A16_MX : 0u);
    if (kind_mask & ~known)
      return fail(MXMOE_GG_ERR_UNSUPPORTED, "%s: unknown expert kind in kind_mask %#x (fp16, w8a8_g-1_sym%s w4a4_g-1_sym%s "
                  "only)", fn, kind_mask, ex ? "," : " and", ex ? " and w4a16_g32_sym_MXFP4" : "");
  }
  if (!kind_mask) return fail(MXMOE_GG_ERR_INVALID, "%s: kind_mask names no kind", fn);
  return MXMOE_GG_OK;
}
inline bool width_ok(int w) { return w > 0 && w % 128 == 0 && w <= kMaxWidthD; }

inline int sizes_check(const char* fn, int64_t T, int topk, int E, int with_shared, int H, int N, int N_shared) {
  if (T < 0 || T > MXMOE_DECODE_MAX_T || E < 1 || topk < 1 || topk > 16 || topk > E)
    return fail(MXMOE_GG_ERR_INVALID, "%s: need 0 <= T <= %d, E >= 1, 1 <= topk <= min(E, 16) (T=%lld E=%d topk=%d)", fn,
                (int)MXMOE_DECODE_MAX_T, (long long)T, E, topk);
  if (!width_ok(H) || !width_ok(N) || (with_shared && !width_ok(N_shared)))
    return fail(MXMOE_GG_ERR_INVALID, "%s: H, N and N_shared must be multiples of 128 and <= %d (H=%d N=%d N_shared=%d)",
                fn, kMaxWidthD, H, N, N_shared);
  return MXMOE_GG_OK;
}

// tiles, batch rows and LDS bytes of a launch whose other fields are set; returns the dynamic LDS bytes
inline int geometry(Args& a) {
  int kb = 0;
  const int kmax = a.with_shared && a.K_shared > a.K ? a.K_shared : a.K;
  for (int k = 0; k <= MXMOE_DECODE_W8A16_G128_ASYM; ++k)
    if ((a.kind_mask >> k) & 1u) {
      const int ab = a_row_bytes(k, kmax);
      kb = ab > kb ? ab : kb;
    }
  a.lds_row = kb = (kb + 1023) & ~1023;  // (rows are zero-padded to the dot loop's group of four 256-byte steps)
  int rb = kLdsBudget / kb;
  rb = rb < 1 ? 1 : rb > kBatchRows ? kBatchRows : rb;
  a.rb = rb > a.T ? a.T : rb;
  // columns of the experts that can have rows; tiles of 128 columns, halved while the grid would not fill the CUs
  const int npairs = a.T * a.topk;
  const int64_t cols = (int64_t)(a.E < npairs ? a.E : npairs) * a.C + (a.with_shared ? a.C_shared : 0);
  int ct = 128;
  while (ct > 32 && cols / ct < 1024) ct >>= 1;
  a.ct = ct;
  a.tiles = a.C / ct;
  a.tiles_shared = a.with_shared ? a.C_shared / ct : 0;
  return a.rb * a.lds_row;
}

template <bool DOWN>
inline int launch(Args a, int level, void* stream) {
  const int lds = geometry(a);
  const dim3 grid((unsigned)((int64_t)a.tiles_shared + (int64_t)a.E * a.tiles));
  switch (level) {
    case kWo:
      hipLaunchKernelGGL((decode_kernel<DOWN, kWo>), grid, dim3(kThreadsD), lds, (hipStream_t)stream, a);
      return launched(DOWN ? "decode_down_wo_kernel" : "decode_gate_up_wo_kernel");
    case kEx:
      hipLaunchKernelGGL((decode_kernel<DOWN, kEx>), grid, dim3(kThreadsD), lds, (hipStream_t)stream, a);
      return launched(DOWN ? "decode_down_ex_kernel" : "decode_gate_up_ex_kernel");
    default:
      hipLaunchKernelGGL((decode_kernel<DOWN, kFirst>), grid, dim3(kThreadsD), lds, (hipStream_t)stream, a);
      return launched(DOWN ? "decode_down_kernel" : "decode_gate_up_kernel");
  }
}

}  // namespace decode
}  // namespace
}  // namespace mxmoe
