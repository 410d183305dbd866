// moe_decode.h — the decode forward's two kernels (mxmoe_moe_decode_gate_up, mxmoe_moe_decode_down of
// include/mxmoe_moe.h), gfx950. Included by moe_ops.hip after its quantiser helpers, which the kernels call as they
// are (rtn_scale, div_f16_operands, codes_i8, codes_i4, amax8, bf16x8_to_f16): the quantised rows are byte for byte
// what act_quant_kernel writes.
//
// A forward of 1..16 tokens has at most a few hundred (token, choice) pairs, so no tile table is planned: every
// workgroup reads all T * topk ids and finds the rows of its own expert. Both kernels are weight streamers — no MFMA,
// the integer dot products on v_dot4_i32_i8 / v_dot8_i32_i4, fp16 on v_fma_mix_f32.
//
// Mapping. One workgroup (256 threads) per (expert, tile of `ct` output columns); the shared expert's tiles come
// first in the grid (its rows are the most: all T). A workgroup whose expert has no row returns after the id scan.
//   rows      thread i < T * topk holds id i; the pairs whose id is the workgroup's expert are listed in pair order
//             (ballot + prefix over the 4 waves). The shared expert's rows are the tokens 0..T-1.
//   A rows    wave w quantises rows w, w + 4, ... of the batch into LDS by the tag of the expert's kind (one pass for
//             the row's amax, one for the codes; fp16: a copy), in pack_wxax order, the K permutation of the weight
//             rows: packed 32-bit words of A and B multiply element by element. A batch is `rb` rows (16, or what
//             fits the LDS budget for very wide rows; more rows than a batch — only with repeated ids — re-read the
//             weights).
//   dot       a quarter-wave (16 lanes) owns two weight rows at a time (gate_up: gate and up row of one output column;
//             down: output columns n and n + 16): lane l holds bytes [256 s + 16 l, + 16) of step s of both rows, four
//             steps (8 loads of 16 B) in flight, and multiplies them with the same bytes of every A row of the batch
//             (LDS, a broadcast across the 4 quarters of a wave). The 16 partial sums of a row are added with four
//             DPP steps inside the 16-lane row (integers: exact; fp16 experts: f32 in that order).
//   epilogue  lane r of the quarter finishes row r: the GroupGEMM's scale arithmetic, gate_up: the SiLU, then a 2-byte
//             store to row `pair` of the output (pair order: no permutation).
// Nothing is indexed by an id: an id outside [0, E) matches no workgroup, its pair's rows stay as they were, and the
// first routed workgroup sets MXMOE_DECODE_BAD_ID in the status word. The expert record is indexed by the workgroup's
// own expert number. A kind outside the call's kind_mask (which sized the LDS rows) sets MXMOE_DECODE_BAD_KIND and the
// workgroup writes nothing.
//
// The _ex entries (mxmoe_moe_decode_gate_up_ex, mxmoe_moe_decode_down_ex: gpt-oss layers) run kernels of their own,
// decode_ex_kernel<DOWN>, which begin with the same statements (moe_decode_body.inc) and instantiate expert_tile with
// EX, a template parameter; without it none of the following exists:
//   W4A16_MX  w4a16_g32_sym_MXFP4: the A row stays fp16 (4 LDS bytes per weight byte), stored permuted inside every
//             1024 bytes so that a lane's four 16-byte reads of its MX block are the other kinds' conflict-free pattern
//             (quant_row); lane l at step s owns block 16 s + l, reads one e8m0 byte of the device scale layout,
//             dequantises a dword of codes at a time with the GroupGEMM's convert and reuses it for every A row of the
//             batch, accumulating in f32 (dot_rows_mx).
//   epilogue  gate_up: the bias row of the workgroup's own expert and the gated activation of an mxmoe_moe_glu, by the
//             activation pass's own helper (glu_value of moe_ops.hip); glu_out.
//
// The _wo entries (mxmoe_moe_decode_gate_up_wo, mxmoe_moe_decode_down_wo) run a third pair, decode_wo_kernel<DOWN>: the
// _ex kernels' four kinds and epilogue, and the integer weight-only kinds 4..11 (w4a16 / w8a16, per-channel or g128,
// sym or asym) on mxmoe_gg_repack_weightonly's codes and the [G][rows] / [G][rows][2] fp16 scale buffer. One body per
// code width (expert_tile_wo<DOWN, 4 or 8>); the group size and the symmetry come from the record's kind as
// workgroup-uniform values.
//   codes     a lane's 16 bytes of step s are whole K runs of 8 (one dword of 4-bit, two dwords of 8-bit codes):
//             4-bit  run j (0..3) of lane l: K = 512 s + 64 (l >> 1) + 32 (j & 1) + 8 (2 (l & 1) + (j >> 1)) + 0..7
//             8-bit  run j (0..1) of lane l: K = 256 s + 64 (l >> 2) + 32 j + 8 (l & 3) + 0..7
//   A rows    fp16, not quantised, permuted inside every step (4-bit: 512 K = 1024 bytes; 8-bit: 256 K = 512 bytes) so
//             that the 8 elements of run j of lane l lie at LDS byte
//               4-bit: 1024 s + 256 j + 16 l        8-bit: 512 s + 256 j + 16 l
//             of the row: a lane's j-th ds_read_b128 of a step is the other kinds' conflict-free pattern (quant_row_wo).
//   dequant   a run at a time, b = fp16(fma(u - off, scale, zp)) by the GroupGEMM's steps (wo_dequant of gg_device.h:
//             0x6400 | u, an exact packed add, one packed fma), reused for every A row of the batch; f32 accumulation
//             as the MX kind (dot_rows_wo).
//   scales    per-channel: the two rows' (scale, zp), loaded once per weight row; g128: one pair per lane, step and
//             row — group 4 s + (l >> 2) (4-bit) or 2 s + (l >> 3) (8-bit) — loaded with the step's codes.
#pragma once

namespace mxmoe {
namespace {
namespace decode {

constexpr int kThreadsD = 256;
constexpr int kMaxPairs = MXMOE_DECODE_MAX_T * 16;  // T <= 16, topk <= 16
constexpr int kBatchRows = 16;                      // A rows per batch: the accumulators a lane keeps per weight row
constexpr int kLdsBudget = 60 * 1024;               // dynamic LDS of a workgroup (the A rows of one batch)
constexpr int kMaxWidthD = 16384;

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
};

// the _ex entries' arguments: the gate_up biases and the gated activation of an mxmoe_moe_glu, as GluArgs carries them
struct ArgsEx : Args {
  const _Float16* bias_routed;  // gate_up: [E][2 C] ([gate | up] columns) or NULL
  const _Float16* bias_shared;  // gate_up: [2 C_shared] or NULL
  int glu;                      // gate_up: kGluSilu / kGluSwigluClamp
  float c, limit;               // SWIGLU_CLAMP: -(alpha log2 e), the clamp
};
template <bool EX> struct ArgsOf { typedef Args type; };
template <> struct ArgsOf<true> { typedef ArgsEx type; };

// bytes of a weight row in global memory, and of an A row in LDS: the integer kinds quantise A to the weights' width,
// W4A16_MX keeps the fp16 row (four times its weight row)
// the weight-only kinds (the _wo entries): kind = 4 + (w_bits == 8) + 2 * (gsize == 128) + 4 * asym
__host__ __device__ inline bool wo_kind(int kind) { return kind >= MXMOE_DECODE_W4A16; }
__host__ __device__ inline int wo_bits(int kind) { return ((kind - MXMOE_DECODE_W4A16) & 1) ? 8 : 4; }
__host__ __device__ inline bool wo_g128(int kind) { return ((kind - MXMOE_DECODE_W4A16) & 2) != 0; }
__host__ __device__ inline bool wo_asym(int kind) { return ((kind - MXMOE_DECODE_W4A16) & 4) != 0; }

__host__ __device__ inline int b_row_bytes(int kind, int K) {
  return kind == MXMOE_DECODE_FP16 ? 2 * K : kind == MXMOE_DECODE_W8A8 ? K : K / 2;
}
__host__ __device__ inline int a_row_bytes(int kind, int K) {
  return kind == MXMOE_DECODE_W4A16_MX ? 2 * K : b_row_bytes(kind, K);
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

// One kind's dequant-and-dot: acc += dot of 16 packed bytes of a weight row with the same 16 bytes of an A row.
template <int KIND> struct Dot;
template <> struct Dot<MXMOE_DECODE_FP16> {
  typedef float acc_t;
  static __device__ __forceinline__ float dot(const uint4& w, const uint4& a, float acc) {
    const h8_t wv = __builtin_bit_cast(h8_t, w), av = __builtin_bit_cast(h8_t, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf((float)wv[j], (float)av[j], acc);
    return acc;
  }
  // fp16_rn(acc)
  static __device__ __forceinline__ _Float16 finish(float acc, _Float16, _Float16) { return (_Float16)acc; }
};
// the GroupGEMM's scaled epilogue: fp16_rn(0 + f32(acc) * f32(fp16_rn(sa * sb))), the f32 product rounded on its own
// (the empty asm keeps the multiply and the conversion from fusing into one rounding)
__device__ __forceinline__ _Float16 scaled_out(int acc, _Float16 sa, _Float16 sb) {
  const _Float16 s16 = sa * sb;
  float prod = (float)acc * (float)s16;
  asm volatile("" : "+v"(prod));
  return (_Float16)(0.0f + prod);
}
template <> struct Dot<MXMOE_DECODE_W8A8> {
  typedef int acc_t;
  static __device__ __forceinline__ int dot(const uint4& w, const uint4& a, int acc) {
    acc = __builtin_amdgcn_sdot4((int)w.x, (int)a.x, acc, false);
    acc = __builtin_amdgcn_sdot4((int)w.y, (int)a.y, acc, false);
    acc = __builtin_amdgcn_sdot4((int)w.z, (int)a.z, acc, false);
    return __builtin_amdgcn_sdot4((int)w.w, (int)a.w, acc, false);
  }
  static __device__ __forceinline__ _Float16 finish(int acc, _Float16 sa, _Float16 sb) { return scaled_out(acc, sa, sb); }
};
template <> struct Dot<MXMOE_DECODE_W4A4> {
  typedef int acc_t;
  static __device__ __forceinline__ int dot(const uint4& w, const uint4& a, int acc) {
    acc = __builtin_amdgcn_sdot8((int)w.x, (int)a.x, acc, false);
    acc = __builtin_amdgcn_sdot8((int)w.y, (int)a.y, acc, false);
    acc = __builtin_amdgcn_sdot8((int)w.z, (int)a.z, acc, false);
    return __builtin_amdgcn_sdot8((int)w.w, (int)a.w, acc, false);
  }
  static __device__ __forceinline__ _Float16 finish(int acc, _Float16 sa, _Float16 sb) { return scaled_out(acc, sa, sb); }
};

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

// The _ex gate_up epilogue: mxmoe_moe_glu_quant's arithmetic on the fp16 g, u (the GLU builds of act_quant_kernel:
// one f32 add per bias, then glu_value — that pass's own helper), the f32 product rounded on its own as in silu_mul.
// has_b false and kGluSilu: silu_mul's value bit for bit.
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

// W4A16_MX: the 32 e2m1 codes of one MX block (16 bytes, element 2i the low nibble of byte i) times 2^(byte - 127) as
// fp16, by the GroupGEMM's convert (wo_dequant_mx of gg_device.h: v_cvt_scalef32_pk_f16_fp4 on the f32 byte << 23), so
// b[n][k] is the GroupGEMM's fp16 value for every scale byte. Dword j of the block's 16 bytes: elements 8 j .. 8 j + 7.
__device__ __forceinline__ h8_t dequant_mx(uint32_t w, uint32_t scale_bits) {
  const float sc = __builtin_bit_cast(float, scale_bits);
  const h2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 0);
  const h2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 1);
  const h2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 2);
  const h2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 3);
  return h8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
// its dot: 8 dequantised weights against the same 8 fp16 elements of an A row, accumulated in f32
// (acc += f32(b) * f32(a), v_fma_mix_f32 as the fp16 kind); a row's sum is rounded once, fp16_rn(acc)
template <> struct Dot<MXMOE_DECODE_W4A16_MX> {
  typedef float acc_t;
  static __device__ __forceinline__ float dot(const h8_t& w, const uint4& a, float acc) {
    const h8_t av = __builtin_bit_cast(h8_t, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf((float)w[j], (float)av[j], acc);
    return acc;
  }
  static __device__ __forceinline__ _Float16 finish(float acc, _Float16, _Float16) { return (_Float16)acc; }
};

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

// Row `src` (K fp16, or bf16 converted as mxmoe_moe_gather_quant does) quantised by kind's tag into `row` (LDS,
// pack_wxax order) by one wave, zeros behind it up to a multiple of 1024 bytes (the dot loop's group of four 256-byte
// steps reads the pad); its scale to *scale. The arithmetic and the helpers are act_quant_kernel's.
__device__ __forceinline__ void quant_row(const uint8_t* __restrict__ src, int K, int kind, bool bf, uint8_t* row,
                                          _Float16* scale) {
  const int lane = threadIdx.x & 63;
  const int KB = a_row_bytes(kind, K);
  auto ld = [&](int idx) -> h8_t {
    const uint4 v = *reinterpret_cast<const uint4*>(src + 2 * idx);
    return bf ? bf16x8_to_f16(v) : __builtin_bit_cast(h8_t, v);
  };
  if (kind == MXMOE_DECODE_W4A16_MX) {
    // The fp16 row, permuted inside every 1024 bytes (a step: 16 MX blocks of 64 bytes): piece j (16 bytes) of block l
    // goes to byte 256 j + 16 l, so that the dot loop's j-th read of lane l is the plain kinds' conflict-free pattern
    // (16 lanes, 16 consecutive 16-byte slots: all 64 banks once). Lane 16 j + l copies that piece, so the stores are
    // the plain copy's (consecutive lanes, consecutive slots) and only the global address is permuted. Pieces past the
    // row are zeros up to the step's end.
    const int src_piece = 4 * (lane & 15) + (lane >> 4);
    for (int o = 0; o < ((KB + 1023) & ~1023); o += 1024) {
      const int idx = (o >> 1) + 8 * src_piece;
      h8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (idx < K) v = ld(idx);
      *reinterpret_cast<h8_t*>(row + o + lane * 16) = v;
    }
    return;
  }
  for (int o = KB + lane * 16; o < ((KB + 1023) & ~1023); o += 1024) *reinterpret_cast<uint4*>(row + o) = uint4{0, 0, 0, 0};
  if (kind == MXMOE_DECODE_FP16) {
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512) *reinterpret_cast<h8_t*>(row + 2 * idx) = ld(idx);
    return;
  }
  float m = 0.0f;
#pragma unroll 4
  for (int idx = lane * 8; idx < K; idx += 512) m = fmaxf(m, amax8(ld(idx)));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  const float qmax = kind == MXMOE_DECODE_W8A8 ? 127.0f : 7.0f;
  const h2_t lim = {(_Float16)qmax, (_Float16)qmax};
  const _Float16 sc = rtn_scale(m, qmax);
  const float rs = __builtin_amdgcn_rcpf((float)sc);
  if (lane == 0) *scale = sc;
  if (kind == MXMOE_DECODE_W8A8) {
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512) *reinterpret_cast<uint2*>(row + idx) = codes_i8(ld(idx), (float)sc, rs, lim);
  } else {
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512)
      *reinterpret_cast<uint32_t*>(row + idx / 2) = codes_i4(ld(idx), (float)sc, rs, lim);
  }
}

// quant_row for the weight-only kinds (bits: the code width): the fp16 row (or bf16 converted), not quantised, as the
// permuted copy the MX kind makes, with these kinds' source element (the K map at the head of this file). 4-bit: slot
// 16 j + l of a step's 1024 bytes holds run j of lane l. 8-bit: two steps of 512 bytes per pass of 1024, slot
// 32 s' + 16 j + l holds run j of lane l of step 2 (o / 1024) + s'. Lane 16 j' + l of the copying wave stores slot
// 16 j' + l: consecutive lanes, consecutive slots. Pieces past the row are zeros up to a multiple of 1024 bytes.
__device__ __forceinline__ void quant_row_wo(const uint8_t* __restrict__ src, int K, int bits, bool bf, uint8_t* row) {
  const int lane = threadIdx.x & 63;
  const int l = lane & 15, j = lane >> 4;
  const int src_el = bits == 4 ? 64 * (l >> 1) + 32 * (j & 1) + 8 * (2 * (l & 1) + (j >> 1))
                               : 256 * (j >> 1) + 64 * (l >> 2) + 32 * (j & 1) + 8 * (l & 3);
  for (int o = 0; o < ((2 * K + 1023) & ~1023); o += 1024) {
    const int idx = (o >> 1) + src_el;
    h8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (idx < K) {
      const uint4 x = *reinterpret_cast<const uint4*>(src + 2 * idx);
      v = bf ? bf16x8_to_f16(x) : __builtin_bit_cast(h8_t, x);
    }
    *reinterpret_cast<h8_t*>(row + o + lane * 16) = v;
  }
}

// The two weight rows w0, w1 (KB bytes each) of a quarter-wave against the nr A rows of the batch, and the rows'
// results: lane r (< nr) of the quarter returns row r's two outputs in *o0, *o1 (other lanes: unspecified).
template <int KIND>
__device__ __forceinline__ void dot_rows(const uint8_t* __restrict__ w0, const uint8_t* __restrict__ w1,
                                         const _Float16* __restrict__ SB, int sb0, int sb1, int KB,
                                         const uint8_t* A, int lds_row, const _Float16* s_scale, int nr, int l16,
                                         _Float16* o0, _Float16* o1) {
  typedef typename Dot<KIND>::acc_t acc_t;
  acc_t acc0[kBatchRows], acc1[kBatchRows];
#pragma unroll
  for (int r = 0; r < kBatchRows; ++r) acc0[r] = acc1[r] = 0;
  const int S = (KB + 255) >> 8;
  for (int s0 = 0; s0 < S; s0 += 4) {
    uint4 wa[4], wb[4];
    int off[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // 8 loads of 16 B in flight; past the row: the row's first bytes (zeroed below)
      off[u] = ((s0 + u) * 16 + l16) * 16;
      const int wo = off[u] < KB ? off[u] : 0;
      wa[u] = *reinterpret_cast<const uint4*>(w0 + wo);
      wb[u] = *reinterpret_cast<const uint4*>(w1 + wo);
    }
    if ((s0 + 4) * 256 > KB) {  // (uniform) the row ends inside this group: zero weights past it; the A rows' pad is zero
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t mk = off[u] < KB ? ~0u : 0u;
        wa[u].x &= mk, wa[u].y &= mk, wa[u].z &= mk, wa[u].w &= mk;
        wb[u].x &= mk, wb[u].y &= mk, wb[u].z &= mk, wb[u].w &= mk;
      }
    }
    int nrs = nr, ldr = lds_row;
    asm volatile("" : "+s"(nrs), "+s"(ldr));  // the 16 row tests and row offsets are made here, not kept in SGPRs
#pragma unroll
    for (int r = 0; r < kBatchRows; ++r) {
      if (r < nrs) {  // workgroup-uniform
        const uint8_t* ar = A + r * ldr;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint4 av = *reinterpret_cast<const uint4*>(ar + off[u]);  // (off < lds_row: a multiple of 1024)
          acc0[r] = Dot<KIND>::dot(wa[u], av, acc0[r]);
          acc1[r] = Dot<KIND>::dot(wb[u], av, acc1[r]);
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
  _Float16 sa = (_Float16)0, b0 = (_Float16)0, b1 = (_Float16)0;
  if constexpr (KIND != MXMOE_DECODE_FP16) {
    sa = s_scale[l16 < nr ? l16 : 0];
    b0 = SB[sb0];
    b1 = SB[sb1];
  }
  *o0 = Dot<KIND>::finish(v0, sa, b0);
  *o1 = Dot<KIND>::finish(v1, sa, b1);
}

// dot_rows for W4A16_MX. A step is 256 bytes of codes = 16 MX blocks: lane l holds block 16 s + l of both weight rows
// and its scale byte — device byte 16 s + 4 (l & 3) + (l >> 2) of the row's scales (include/mxmoe_gg.h:
// dev[16 t + 4 g + i] = canon[16 t + 4 i + g]; a row has 16 bytes per step, pads 127). The block is dequantised once
// (a quarter at a time) and multiplied with the 64 bytes of the block in every A row of the batch (quant_row's
// permuted copy: four 16-byte reads at 1024 s + 256 j + 16 l). SB0 / SB1: the two rows' scale bytes. A lane past the row's end (only inside its
// last step) loads the row's first bytes, codes and scale alike, and both are zeroed: +0 weights on the A rows' zero
// pad. Whole steps past the end are loaded the same way (the four steps in flight) but not multiplied: the A rows end
// with the last step.
__device__ __forceinline__ void dot_rows_mx(const uint8_t* __restrict__ w0, const uint8_t* __restrict__ w1,
                                            const uint8_t* __restrict__ SB0, const uint8_t* __restrict__ SB1, int KB,
                                            const uint8_t* A, int lds_row, int nr, int l16, _Float16* o0, _Float16* o1) {
  typedef Dot<MXMOE_DECODE_W4A16_MX> D;
  float acc0[kBatchRows], acc1[kBatchRows];
#pragma unroll
  for (int r = 0; r < kBatchRows; ++r) acc0[r] = acc1[r] = 0;
  const int S = (KB + 255) >> 8;
  const int sl = 4 * (l16 & 3) + (l16 >> 2);
  for (int s0 = 0; s0 < S; s0 += 4) {
    uint4 wa[4], wb[4];
    uint32_t sa[4], sb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // 8 loads of 16 B and 8 scale bytes in flight
      const bool in = ((s0 + u) * 16 + l16) * 16 < KB;
      const int wo = in ? ((s0 + u) * 16 + l16) * 16 : 0;
      const int so = in ? (s0 + u) * 16 + sl : 0;
      wa[u] = *reinterpret_cast<const uint4*>(w0 + wo);
      wb[u] = *reinterpret_cast<const uint4*>(w1 + wo);
      sa[u] = (uint32_t)SB0[so] << 23;
      sb[u] = (uint32_t)SB1[so] << 23;
      if (!in) {
        wa[u] = wb[u] = uint4{0, 0, 0, 0};
        sa[u] = sb[u] = 0;
      }
    }
    int nrs = nr, ldr = lds_row;
    asm volatile("" : "+s"(nrs), "+s"(ldr));  // (as in dot_rows)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s0 + u < S) {  // workgroup-uniform
        const uint32_t da[4] = {wa[u].x, wa[u].y, wa[u].z, wa[u].w}, db[4] = {wb[u].x, wb[u].y, wb[u].z, wb[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // a quarter of the block at a time: 8 weights of each row live, not 32
          const h8_t x0 = dequant_mx(da[j], sa[u]), x1 = dequant_mx(db[j], sb[u]);
          const uint8_t* const aj = A + (s0 + u) * 1024 + 256 * j + l16 * 16;  // (< lds_row: whole steps of the padded row)
#pragma unroll
          for (int r = 0; r < kBatchRows; ++r) {
            if (r < nrs) {  // workgroup-uniform
              const uint4 av = *reinterpret_cast<const uint4*>(aj + r * ldr);
              acc0[r] = D::dot(x0, av, acc0[r]);
              acc1[r] = D::dot(x1, av, acc1[r]);
            }
          }
        }
      }
    }
  }
  float v0 = 0, v1 = 0;
  int lsel = l16, nrs = nr;
  asm volatile("" : "+v"(lsel), "+s"(nrs));
#pragma unroll
  for (int r = 0; r < kBatchRows; ++r) {
    if (r < nrs) {
      const float t0 = row16_sum(acc0[r]), t1 = row16_sum(acc1[r]);
      if (lsel == r) {
        v0 = t0;
        v1 = t1;
      }
    }
  }
  *o0 = D::finish(v0, (_Float16)0, (_Float16)0);
  *o1 = D::finish(v1, (_Float16)0, (_Float16)0);
}

// dot_rows for the weight-only kinds (BITS: the code width; g128, asym: of the expert's kind, workgroup-uniform). SB:
// the weight's scale buffer, fp16 [G][rows] or (asym) [G][rows][2] (scale, zp); sr0 / sr1: the two weight rows. Lane l
// holds 16 bytes of codes of step s of both rows: 4 (4-bit) or 2 (8-bit) runs of 8 K, each dequantised once and
// multiplied with the run's 16 bytes of every A row of the batch (quant_row_wo's permuted copy). Per-channel scales are
// loaded once here; g128 scales with the step's codes, one pair per lane and row. A lane past the row's end (only
// inside its last step) loads the row's first bytes and group 0's scales, and codes, scale and zp are zeroed: b = +0
// on the A rows' zero pad. Whole steps past the end are loaded the same way but not multiplied.
template <int BITS>
__device__ __forceinline__ void dot_rows_wo(const uint8_t* __restrict__ w0, const uint8_t* __restrict__ w1,
                                            const _Float16* __restrict__ SB, int sr0, int sr1, int rows, bool g128,
                                            bool asym, int KB, const uint8_t* A, int lds_row, int nr, int l16,
                                            _Float16* o0, _Float16* o1) {
  typedef Dot<MXMOE_DECODE_W4A16_MX> D;  // (the fp16-times-fp16 f32 dot of 8 elements)
  constexpr int kRuns = BITS == 4 ? 4 : 2;           // K runs of 8 in a lane's 16 bytes
  constexpr int kStepLds = BITS == 4 ? 1024 : 512;   // LDS bytes of an A row per step
  constexpr int kStepGroups = BITS == 4 ? 4 : 2;     // 128-K groups per step
  float acc0[kBatchRows], acc1[kBatchRows];
#pragma unroll
  for (int r = 0; r < kBatchRows; ++r) acc0[r] = acc1[r] = 0;
  const int S = (KB + 255) >> 8;
  const int gl = BITS == 4 ? l16 >> 2 : l16 >> 3;
  const int sh = asym ? 1 : 0;  // element (g * rows + r) << sh: the scale; + 1 (asym): the zp
  const _Float16 off = (_Float16)(asym ? -1024.0f : BITS == 4 ? -1031.0f : -1151.0f);  // -(1024 + 2^(BITS-1) - 1), sym
  const h2_t moff = {off, off};
  // (scale, zp) of a row's group as one register
  auto pair = [&](int row, int g) -> h2_t {
    const int i = (g * rows + row) << sh;
    return h2_t{SB[i], asym ? SB[i + 1] : (_Float16)0};
  };
  h2_t pc0 = {0, 0}, pc1 = {0, 0};
  if (!g128) {
    pc0 = pair(sr0, 0);
    pc1 = pair(sr1, 0);
  }
  for (int s0 = 0; s0 < S; s0 += 4) {
    uint4 wa[4], wb[4];
    h2_t sa[4], sb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // 8 loads of 16 B (and, g128, the 2 or 4 scale halves of each) in flight
      const bool in = ((s0 + u) * 16 + l16) * 16 < KB;
      const int wo = in ? ((s0 + u) * 16 + l16) * 16 : 0;
      wa[u] = *reinterpret_cast<const uint4*>(w0 + wo);
      wb[u] = *reinterpret_cast<const uint4*>(w1 + wo);
      if (g128) {
        const int g = in ? (s0 + u) * kStepGroups + gl : 0;
        sa[u] = pair(sr0, g);
        sb[u] = pair(sr1, g);
      } else {
        sa[u] = pc0;
        sb[u] = pc1;
      }
      if (!in) {
        wa[u] = wb[u] = uint4{0, 0, 0, 0};
        sa[u] = sb[u] = h2_t{0, 0};
      }
    }
    int nrs = nr, ldr = lds_row;
    asm volatile("" : "+s"(nrs), "+s"(ldr));  // (as in dot_rows)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s0 + u < S) {  // workgroup-uniform
        const uint32_t da[4] = {wa[u].x, wa[u].y, wa[u].z, wa[u].w}, db[4] = {wb[u].x, wb[u].y, wb[u].z, wb[u].w};
        const h2_t as2 = {sa[u][0], sa[u][0]}, az2 = {sa[u][1], sa[u][1]};
        const h2_t bs2 = {sb[u][0], sb[u][0]}, bz2 = {sb[u][1], sb[u][1]};
#pragma unroll
        for (int j = 0; j < kRuns; ++j) {  // a run at a time: 8 weights of each row live
          const int d = BITS == 4 ? j : 2 * j;
          const h8_t x0 = dequant_wo<BITS>(da[d], da[(d + 1) & 3], moff, as2, az2);
          const h8_t x1 = dequant_wo<BITS>(db[d], db[(d + 1) & 3], moff, bs2, bz2);
          const uint8_t* const aj = A + (s0 + u) * kStepLds + 256 * j + l16 * 16;  // (< lds_row: whole steps of the row)
#pragma unroll
          for (int r = 0; r < kBatchRows; ++r) {
            if (r < nrs) {  // workgroup-uniform
              const uint4 av = *reinterpret_cast<const uint4*>(aj + r * ldr);
              acc0[r] = D::dot(x0, av, acc0[r]);
              acc1[r] = D::dot(x1, av, acc1[r]);
            }
          }
        }
      }
    }
  }
  float v0 = 0, v1 = 0;
  int lsel = l16, nrs = nr;
  asm volatile("" : "+v"(lsel), "+s"(nrs));
#pragma unroll
  for (int r = 0; r < kBatchRows; ++r) {
    if (r < nrs) {
      const float t0 = row16_sum(acc0[r]), t1 = row16_sum(acc1[r]);
      if (lsel == r) {
        v0 = t0;
        v1 = t1;
      }
    }
  }
  *o0 = D::finish(v0, (_Float16)0, (_Float16)0);
  *o1 = D::finish(v1, (_Float16)0, (_Float16)0);
}

// One workgroup's work on an expert of kind KIND: per batch of rows, the A rows into LDS, then the tile's columns.
// EX: the _ex entries' build — `brow`, the bias row of the workgroup's expert ([gate | up], or NULL), and the gated
// activation of ArgsEx in the gate_up epilogue. Without EX none of that code exists. WO: a tag that changes no code and
// gives the _wo kernels instantiations of their own — when they shared the _ex kernels', those kernels' register
// allocation changed (DESIGN.md §4 "Decode forward: weight-only experts").
template <bool DOWN, int KIND, bool EX = false, int WO = 0>
__device__ __forceinline__ void expert_tile(const typename ArgsOf<EX>::type& a, const mxmoe_moe_decode_expert& ex,
                                            bool shared, int tile, int nrows, uint8_t* s_a, const int* s_rows,
                                            _Float16* s_scale, const _Float16* brow = nullptr) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int K = shared ? a.K_shared : a.K, C = shared ? a.C_shared : a.C;
  const int KB = b_row_bytes(KIND, K);  // of a weight row (the A row's bytes are <= lds_row: the kind is in the mask)
  const uint8_t* const B = static_cast<const uint8_t*>(DOWN ? ex.b2 : ex.b1);
  const _Float16* const SB = static_cast<const _Float16*>(DOWN ? ex.sb2 : ex.sb1);
  const uint8_t* const src = static_cast<const uint8_t*>(shared ? a.src_shared : a.src);
  _Float16* const out = shared ? a.out_shared : a.out;
  const int n0 = tile * a.ct;
  const int q = tid >> 4, l16 = tid & 15;

  for (int r0 = 0; r0 < nrows; r0 += a.rb) {
    const int nr = min(a.rb, nrows - r0);
    __syncthreads();  // s_rows is complete; the previous batch's A rows are no longer read
    for (int r = wave; r < nr; r += kThreadsD / 64) {
      const int p = shared ? r0 + r : s_rows[r0 + r];      // token (shared) or pair
      const int srow = (shared || DOWN) ? p : p / a.topk;  // gate_up reads the pair's token
      quant_row(src + (int64_t)srow * K * 2, K, KIND, !DOWN && a.src_bf16, s_a + r * a.lds_row, s_scale + r);
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
      if constexpr (KIND == MXMOE_DECODE_W4A16_MX) {
        const uint8_t* const SB8 = reinterpret_cast<const uint8_t*>(SB);  // e8m0 rows of 16 bytes per step
        const int sr = ((KB + 255) >> 8) * 16;
        dot_rows_mx(B + (int64_t)wr0 * KB, B + (int64_t)wr1 * KB, SB8 + (int64_t)wr0 * sr, SB8 + (int64_t)wr1 * sr, KB, s_a,
                    a.lds_row, nr, l16, &o0, &o1);
      } else {
        dot_rows<KIND>(B + (int64_t)wr0 * KB, B + (int64_t)wr1 * KB, SB, wr0, wr1, KB, s_a, a.lds_row, s_scale, nr, l16, &o0,
                       &o1);
      }
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

// expert_tile for the weight-only kinds 4..11 (the _wo kernels; BITS: the code width, `kind`: the record's own, which
// gives the group size and the symmetry as workgroup-uniform values): the same batches, columns, weight rows and
// gate_up epilogue, with the fp16 A rows of quant_row_wo and the dot of dot_rows_wo.
template <bool DOWN, int BITS>
__device__ __forceinline__ void expert_tile_wo(const ArgsEx& a, const mxmoe_moe_decode_expert& ex, int kind, bool shared,
                                               int tile, int nrows, uint8_t* s_a, const int* s_rows,
                                               const _Float16* brow) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int K = shared ? a.K_shared : a.K, C = shared ? a.C_shared : a.C;
  const int KB = K * BITS / 8;  // of a weight row (the fp16 A row's 2 K bytes are <= lds_row: the kind is in the mask)
  const uint8_t* const B = static_cast<const uint8_t*>(DOWN ? ex.b2 : ex.b1);
  const _Float16* const SB = static_cast<const _Float16*>(DOWN ? ex.sb2 : ex.sb1);
  const uint8_t* const src = static_cast<const uint8_t*>(shared ? a.src_shared : a.src);
  _Float16* const out = shared ? a.out_shared : a.out;
  const int n0 = tile * a.ct;
  const int q = tid >> 4, l16 = tid & 15;
  const int rows = DOWN ? C : 2 * C;  // of the weight: the scale buffer is [G][rows] or [G][rows][2]
  const bool g128 = wo_g128(kind), asym = wo_asym(kind);

  for (int r0 = 0; r0 < nrows; r0 += a.rb) {
    const int nr = min(a.rb, nrows - r0);
    __syncthreads();  // s_rows is complete; the previous batch's A rows are no longer read
    for (int r = wave; r < nr; r += kThreadsD / 64) {
      const int p = shared ? r0 + r : s_rows[r0 + r];      // token (shared) or pair
      const int srow = (shared || DOWN) ? p : p / a.topk;  // gate_up reads the pair's token
      quant_row_wo(src + (int64_t)srow * K * 2, K, BITS, !DOWN && a.src_bf16, s_a + r * a.lds_row);
    }
    __syncthreads();
    const int orow = l16 < nr ? (shared ? r0 + l16 : s_rows[r0 + l16]) : 0;
    for (int c = q; c < a.ct; c += DOWN ? 32 : 16) {
      const int n = n0 + c;
      if (n + (DOWN ? 16 : 0) >= C) continue;
      int wr0, wr1;  // (as in expert_tile)
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
      dot_rows_wo<BITS>(B + (int64_t)wr0 * KB, B + (int64_t)wr1 * KB, SB, wr0, wr1, rows, g128, asym, KB, s_a, a.lds_row,
                        nr, l16, &o0, &o1);
      if (l16 < nr) {
        _Float16* const orp = out + (int64_t)orow * C;
        if constexpr (DOWN) {
          orp[n] = o0;
          orp[n + 16] = o1;
        } else {
          const bool has_b = brow != nullptr;  // workgroup-uniform
          const _Float16 bg = has_b ? brow[n] : (_Float16)0, bu = has_b ? brow[C + n] : (_Float16)0;
          orp[n] = a.glu == kGluSwigluClamp ? glu_out<kGluSwigluClamp>(o0, o1, has_b, bg, bu, a.limit, a.c)
                                            : glu_out<kGluSilu>(o0, o1, has_b, bg, bu, a.limit, a.c);
        }
      }
    }
  }
}

// The kernels. DOWN = false: decode_gate_up; true: decode_down. Both begin with the statements of
// moe_decode_body.inc; decode_ex_kernel (the _ex entries) also carries the W4A16_MX kind and (gate_up) the biases and the
// gated activation, through expert_tile's EX parameter: without it that code does not exist.
template <bool DOWN>
__global__ __launch_bounds__(kThreadsD) void decode_kernel(Args a) {
#include "moe_decode_body.inc"
  // the kind is chosen once, outside the loops: one dequant-and-dot body per kind, one switch
  if (kind == MXMOE_DECODE_FP16) expert_tile<DOWN, MXMOE_DECODE_FP16>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale);
  else if (kind == MXMOE_DECODE_W8A8) expert_tile<DOWN, MXMOE_DECODE_W8A8>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale);
  else expert_tile<DOWN, MXMOE_DECODE_W4A4>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale);
}
template <bool DOWN>
__global__ __launch_bounds__(kThreadsD) void decode_ex_kernel(ArgsEx a) {
#include "moe_decode_body.inc"
  // the bias row of the workgroup's own expert (e < E by the grid's size): never indexed by an id
  const _Float16* brow = nullptr;
  if constexpr (!DOWN) brow = shared ? a.bias_shared : a.bias_routed ? a.bias_routed + (int64_t)e * 2 * a.C : nullptr;
  if (kind == MXMOE_DECODE_FP16)
    expert_tile<DOWN, MXMOE_DECODE_FP16, true>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
  else if (kind == MXMOE_DECODE_W8A8)
    expert_tile<DOWN, MXMOE_DECODE_W8A8, true>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
  else if (kind == MXMOE_DECODE_W4A4)
    expert_tile<DOWN, MXMOE_DECODE_W4A4, true>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
  else
    expert_tile<DOWN, MXMOE_DECODE_W4A16_MX, true>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
}

// the _wo entries: the _ex kernel's kinds and, per code width, one body for the weight-only kinds 4..11
struct ArgsWo : ArgsEx {};
template <bool DOWN>
__global__ __launch_bounds__(kThreadsD) void decode_wo_kernel(ArgsWo a) {
#include "moe_decode_body.inc"
  const _Float16* brow = nullptr;
  if constexpr (!DOWN) brow = shared ? a.bias_shared : a.bias_routed ? a.bias_routed + (int64_t)e * 2 * a.C : nullptr;
  if (kind == MXMOE_DECODE_FP16)
    expert_tile<DOWN, MXMOE_DECODE_FP16, true, 1>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
  else if (kind == MXMOE_DECODE_W8A8)
    expert_tile<DOWN, MXMOE_DECODE_W8A8, true, 1>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
  else if (kind == MXMOE_DECODE_W4A4)
    expert_tile<DOWN, MXMOE_DECODE_W4A4, true, 1>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
  else if (kind == MXMOE_DECODE_W4A16_MX)
    expert_tile<DOWN, MXMOE_DECODE_W4A16_MX, true, 1>(a, ex, shared, tile, nrows, s_a, s_rows, s_scale, brow);
  else if (wo_bits(kind) == 4)  // (kind <= 11: it is in the mask, which the entry checked)
    expert_tile_wo<DOWN, 4>(a, ex, kind, shared, tile, nrows, s_a, s_rows, brow);
  else
    expert_tile_wo<DOWN, 8>(a, ex, kind, shared, tile, nrows, s_a, s_rows, brow);
}

// ---------------------------------------------------------------------------------------------
// host side: the entries' checks (before any HIP call) and the launch geometry

// level: which entries — kFirst, kEx (also W4A16_MX) or kWo (also the weight-only kinds 4..11)
enum { kFirst = 0, kEx = 1, kWo = 2 };
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
      const int ab = wo_kind(k) ? 2 * kmax : a_row_bytes(k, kmax);  // (the weight-only kinds keep the fp16 row)
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

// ArgsWo: the _wo kernels; ArgsEx: the _ex kernels; Args: the kernels of the first two entries
template <bool DOWN, class ARGS>
inline int launch(ARGS a, void* stream) {
  const int lds = geometry(a);
  const int64_t blocks = (int64_t)a.tiles_shared + (int64_t)a.E * a.tiles;
  if constexpr (std::is_same<ARGS, ArgsWo>::value) {
    hipLaunchKernelGGL(decode_wo_kernel<DOWN>, dim3((unsigned)blocks), dim3(kThreadsD), lds, (hipStream_t)stream, a);
    return launched(DOWN ? "decode_down_wo_kernel" : "decode_gate_up_wo_kernel");
  } else if constexpr (std::is_same<ARGS, ArgsEx>::value) {
    hipLaunchKernelGGL(decode_ex_kernel<DOWN>, dim3((unsigned)blocks), dim3(kThreadsD), lds, (hipStream_t)stream, a);
    return launched(DOWN ? "decode_down_ex_kernel" : "decode_gate_up_ex_kernel");
  } else {
    hipLaunchKernelGGL(decode_kernel<DOWN>, dim3((unsigned)blocks), dim3(kThreadsD), lds, (hipStream_t)stream, a);
    return launched(DOWN ? "decode_down_kernel" : "decode_gate_up_kernel");
  }
}

}  // namespace decode
}  // namespace
}  // namespace mxmoe
