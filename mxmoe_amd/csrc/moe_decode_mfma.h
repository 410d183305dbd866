// moe_decode_mfma.h — the decode forward's MFMA tile (the _lp entries of include/mxmoe_moe.h: mxmoe_moe_decode_gate_up_lp,
// mxmoe_moe_decode_down_lp), gfx950. Included by moe_ops.hip after moe_decode.h, whose decode_kernel<DOWN, kLp> calls
// lp_tile for the kinds with low-precision floating-point activations:
//   MXMOE_DECODE_W8A8_E4M3   e4m3 A codes with one fp16 scale per row, e4m3 B codes with one fp16 scale per row
//   MXMOE_DECODE_W4A8_MXFP8  OCP MXFP8 A (e4m3 codes, an e8m0 byte per 32), OCP MXFP4 B (e2m1 codes, e8m0 bytes)
//   MXMOE_DECODE_W4A4_MXFP4  OCP MXFP4 A and B
// gfx950 has no VALU dot product for fp8 or fp4 codes; it has v_mfma_scale_f32_16x16x128_f8f6f4, which takes them as
// they are, block scales included, and a decode batch is at most 16 rows: the M of that instruction. Everything around
// the tile (Args, the grid, the id scan, the status bits, geometry()'s ct, pair-order outputs) is moe_decode.h's.
//
// Mapping. The weights are src0 and the A rows src1 of the MFMA, as in the GroupGEMM (gg_tile_v2): lane (r16, g),
// r16 = lane & 15, g = lane >> 4, supplies weight row r16 and A row r16 of K group g, and ends with the four f32 of A
// row r16 (a row of the batch) on weight rows 4 g .. 4 g + 3 (four adjacent output columns).
//   groups    a workgroup's tile of `ct` columns is ct / 16 groups of 16 output columns, taken round-robin by the four
//             waves. down: the group's 16 weight rows; gate_up: its 16 gate rows and its 16 up rows — two accumulators
//             on one A fragment (both weight layouts: only the row index differs).
//   weights   from global memory straight to registers: every weight byte is used by one lane once. Per K = 128 step s
//             a lane loads, with the K assignment of the GroupGEMM's bodies (QT_F8, QT_MXF8A, QT_MXF4),
//               fp8 B: bytes [128 s + 16 g, + 16) and [128 s + 64 + 16 g, + 16) of its row (32 B),
//               fp4 B: bytes [64 s + 16 g, + 16) of its row (16 B: the MX block 4 s + g),
//             so the 16 rows x 4 K groups of a wave consume whole 128-B / 64-B runs of every row. kSteps steps (4 for
//             fp8, 8 for fp4 weights: 128 B per lane and weight row) are loaded before the first is multiplied. The row
//             is a whole number of steps (the widths are multiples of 128); a step past the row's end inside the last
//             group loads the row's first bytes and is not multiplied. MX: the e8m0 bytes of four steps are one dword
//             of the device scale layout (include/mxmoe_gg.h: dword g of the row's 16-byte group t holds K group g's
//             bytes of steps 4 t .. 4 t + 3), read in place; a step's byte is shifted down to byte 0.
//   A rows    wave w quantises rows w, w + 4, ... of the batch into LDS with the activation pass's helpers, byte for
//             byte what act_quant_kernel writes for MXMOE_ACT_E4M3 / _MXFP8 / _MXFP4 (an Inf / NaN row or block: zero
//             codes and a NaN scale; a zero block: e8m0 byte 0). bf16 hidden rows are converted by bf16x8_to_f16.
//   LDS       [0, 16) zeros, [16, 20) four e8m0 bytes 127: what lanes r16 >= nr read instead of a row (zero codes, a
//             neutral scale; their accumulator columns are never stored). From byte 32: rb rows of codes, `row` bytes
//             apart (the widest A row of the call's lp kinds + 16: an odd number of 16-byte slots, so the 16 rows a
//             ds_read_b128 pass touches lie in the 16 slots of the 256-byte bank row once), then rb rows of e8m0 bytes
//             in the device scale layout, `srow` bytes apart (+ 4: an odd number of dwords). A lane's A fragment of a
//             step is bytes [128 s + 16 g, + 16) and [128 s + 64 + 16 g, + 16) of its row (fp8: two ds_read_b128) or
//             [64 s + 16 g, + 16) (fp4: one), its scale byte comes with a ds_read_b32 per four steps.
//   epilogue  E4M3: fp16_rn(f32 acc * f32(fp16_rn(sa * sb))), the product rounded on its own (the GroupGEMM's
//             scale_pack4f); MX: fp16_rn(acc). gate_up: glu_out, as the _wo level's epilogue. One 8-byte store per lane.
#pragma once

namespace mxmoe {
namespace {
namespace decode {

typedef int lp_v4i __attribute__((ext_vector_type(4)));
typedef int lp_v8i __attribute__((ext_vector_type(8)));
typedef float lp_v4f __attribute__((ext_vector_type(4)));

// src0 = weights, src1 = A rows; format code 0: fp8 e4m3, 4: fp4 e2m1 (16 B in the low half of the operand). The scale
// operands' byte 0 is the e8m0 byte of the lane's MX block (op_sel 0); 127 = 2^0.
template <bool B8, bool A8>
__device__ __forceinline__ lp_v4f lp_mfma(const lp_v8i& b, uint32_t sb, const lp_v8i& a, uint32_t sa, const lp_v4f& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, c, B8 ? 0 : 4, A8 ? 0 : 4, 0, (int)sb, 0, (int)sa);
}

// One row (K fp16, or bf16 converted) quantised by one wave as act_quant_kernel quantises it for KIND's tag: the codes
// to `row`, E4M3: the row's fp16 scale to *scale, MX: the blocks' e8m0 bytes to `sc` (device layout).
template <int KIND>
__device__ __forceinline__ void lp_quant_row(const uint8_t* __restrict__ src, int K, bool bf, uint8_t* row, uint8_t* sc,
                                             _Float16* scale) {
  const int lane = threadIdx.x & 63;
  if constexpr (KIND == MXMOE_DECODE_W8A8_E4M3) {
    uint32_t mi = 0;
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512) mi = max(mi, amax8_bits(load_h8(src, idx, bf)));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mi = max(mi, (uint32_t)__shfl_xor((int)mi, d, 64));
    const bool bad = mi >= 0x7C00u;  // an Inf or a NaN in the row: NaN scale, zero codes
    // s = fp16_rn(amax / 448), at least 2^-14, 1 for a zero row
    _Float16 s16 = (_Float16)((float)__builtin_bit_cast(_Float16, (uint16_t)mi) / 448.0f);
    if (__builtin_bit_cast(uint16_t, s16) < 0x0400u) s16 = __builtin_bit_cast(_Float16, (uint16_t)0x0400u);
    if (mi == 0) s16 = (_Float16)1;
    if (bad) s16 = __builtin_bit_cast(_Float16, (uint16_t)0x7E00u);
    if (lane == 0) *scale = s16;
    const float s = (float)s16, r = 1.0f / s;
#pragma unroll 4
    for (int idx = lane * 8; idx < K; idx += 512) {
      const uint2 q = codes_e4m3(load_h8(src, idx, bf), s, r);
      *reinterpret_cast<uint2*>(row + idx) = bad ? uint2{0u, 0u} : q;
    }
  } else {
    constexpr bool A8 = KIND == MXMOE_DECODE_W4A8_MXFP8;
    for (int c0 = 0; c0 < K; c0 += 512) {  // (uniform: the block amax crosses lanes)
      const int idx = c0 + lane * 8;
      const bool in = idx < K;
      h8_t x = load_h8(src, in ? idx : 0, bf);
      if (!in) x = h8_t{0, 0, 0, 0, 0, 0, 0, 0};
      const uint32_t m2 = mx_block_amax(x);
      if (!in) continue;
      const bool bad = m2 >= 0x7C00u;  // an Inf or a NaN in the block: NaN scale, zero codes
      float inv;
      const int e = mx_exponent<A8 ? 8 : 2>(m2, inv);
      if constexpr (A8) {  // the MXMOE_ACT_MXFP8 tag's codes
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = __builtin_amdgcn_fmed3f((float)x[j] * inv, -448.0f, 448.0f);  // product exact
        int q0 = 0, q1 = 0;
        q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], q0, false);
        q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], q0, true);
        q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], q1, false);
        q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], q1, true);
        *reinterpret_cast<uint2*>(row + idx) = bad ? uint2{0u, 0u} : uint2{(uint32_t)q0, (uint32_t)q1};
      } else {  // the MXMOE_ACT_MXFP4 tag's codes
        uint32_t q = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float y = (float)x[j] * inv;  // exact
          const float ay = fminf(fabsf(y), 6.0f);
          const float r = ay < 2.0f ? __builtin_rintf(ay * 2.0f)
                        : ay < 4.0f ? 2.0f + __builtin_rintf(ay) : 4.0f + __builtin_rintf(ay * 0.5f);
          q |= ((uint32_t)r | ((__builtin_bit_cast(uint32_t, y) >> 28) & 8u)) << (4 * j);
        }
        *reinterpret_cast<uint32_t*>(row + idx / 2) = bad ? 0u : q;
      }
      if ((lane & 3) == 0) {  // the block's first lane: its byte at mx_store_scale's place in the 16-byte group
        const int blk = idx >> 5, c16 = blk & 15;
        sc[(blk & ~15) + 4 * (c16 & 3) + (c16 >> 2)] = bad ? (uint8_t)255 : (uint8_t)(e + 127);
      }
    }
  }
}

// the E4M3 epilogue: scaled_out's arithmetic on an f32 accumulator (scale_pack4f of gg_device.h)
__device__ __forceinline__ _Float16 lp_scaled_out(float acc, _Float16 sa, _Float16 sb) {
  const _Float16 s16 = sa * sb;
  float prod = acc * (float)s16;
  asm volatile("" : "+v"(prod));
  return (_Float16)(0.0f + prod);
}

// One workgroup's work on an expert of an lp kind: per batch of rows, the A rows into LDS, then the tile's groups.
template <bool DOWN, int KIND>
__device__ __forceinline__ void lp_tile(const Args& a, const mxmoe_moe_decode_expert& ex, bool shared, int tile, int nrows,
                                        uint8_t* s_a, const int* s_rows, _Float16* s_scale, const _Float16* brow) {
  constexpr bool B8 = KIND == MXMOE_DECODE_W8A8_E4M3;    // fp8 weight codes
  constexpr bool A8 = KIND != MXMOE_DECODE_W4A4_MXFP4;   // fp8 A codes
  constexpr bool MX = KIND != MXMOE_DECODE_W8A8_E4M3;    // block scales on both operands
  constexpr int kSteps = B8 ? 4 : 8;                     // K = 128 steps in flight: 128 B per lane and weight row
  constexpr int kBStep = B8 ? 128 : 64, kAStep = A8 ? 128 : 64;  // bytes of a step in a weight row / an A row
  constexpr int NW = DOWN ? 1 : 2;                       // weight rows per lane: down 1; gate_up the gate and the up row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int K = shared ? a.K_shared : a.K, C = shared ? a.C_shared : a.C;
  const int KB = lp_b_row_bytes(KIND, K), S = K >> 7;
  const int sbrow = lp_scale_row_bytes(K);  // e8m0 bytes of a weight row
  const uint8_t* const B = static_cast<const uint8_t*>(DOWN ? ex.b2 : ex.b1);
  const uint8_t* const SB = static_cast<const uint8_t*>(DOWN ? ex.sb2 : ex.sb1);
  const uint8_t* const src = static_cast<const uint8_t*>(shared ? a.src_shared : a.src);
  _Float16* const out = shared ? a.out_shared : a.out;
  const LpLds L = lp_lds(a);
  uint8_t* const s_code = s_a + kLpHead;
  uint8_t* const s_sc = s_code + L.rb * L.row;
  if (tid < kLpHead / 4) reinterpret_cast<uint32_t*>(s_a)[tid] = tid == 4 ? 0x7F7F7F7Fu : 0u;

  for (int r0 = 0; r0 < nrows; r0 += L.rb) {
    const int nr = min(L.rb, nrows - r0);
    __syncthreads();  // s_rows and the head are complete; the previous batch's A rows are no longer read
    for (int r = wave; r < nr; r += kThreadsD / 64) {
      const int p = shared ? r0 + r : s_rows[r0 + r];      // token (shared) or pair
      const int srow = (shared || DOWN) ? p : p / a.topk;  // gate_up reads the pair's token
      lp_quant_row<KIND>(src + (int64_t)srow * K * 2, K, !DOWN && a.src_bf16, s_code + r * L.row, s_sc + r * L.srow,
                         s_scale + r);
    }
    __syncthreads();
    const bool live = r16 < nr;  // lanes past the batch read the head: zero codes, scale bytes 127
    const int orow = live ? (shared ? r0 + r16 : s_rows[r0 + r16]) : 0;
    const uint8_t* const arow = live ? s_code + r16 * L.row + 16 * g : s_a;
    const uint8_t* const asc = live ? s_sc + r16 * L.srow + 4 * g : s_a + 16;
    const int ainc = live ? kAStep : 0, ahalf = live ? 64 : 0, scinc = live ? 16 : 0;

    for (int n = tile * a.ct + 16 * wave; n < min((tile + 1) * a.ct, C); n += 16 * (kThreadsD / 64)) {
      // the lane's weight rows: down row n + r16; gate_up the gate and the up row of column n + r16
      int wr[NW];
      if constexpr (DOWN) {
        wr[0] = n + r16;
      } else if (a.layout == MXMOE_DECODE_GU_INTERLEAVED) {
        wr[0] = 2 * n + r16;
        wr[1] = wr[0] + 16;
      } else {
        wr[0] = n + r16;
        wr[1] = C + n + r16;
      }
      const uint8_t* w[NW];
      const uint8_t* ws[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        w[i] = B + (int64_t)wr[i] * KB + 16 * g;
        ws[i] = MX ? SB + (int64_t)wr[i] * sbrow + 4 * g : nullptr;
      }
      lp_v4f acc[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) acc[i] = lp_v4f{0.0f, 0.0f, 0.0f, 0.0f};

      for (int s0 = 0; s0 < S; s0 += kSteps) {
        lp_v4i lo[NW][kSteps], hi[NW][B8 ? kSteps : 1];
        uint32_t sw[NW][kSteps / 4];
#pragma unroll
        for (int u = 0; u < kSteps; ++u) {  // the group's loads, all in flight; a step past the row: its first bytes
          const int off = s0 + u < S ? (s0 + u) * kBStep : 0;
#pragma unroll
          for (int i = 0; i < NW; ++i) {
            lo[i][u] = *reinterpret_cast<const lp_v4i*>(w[i] + off);
            if constexpr (B8) hi[i][u] = *reinterpret_cast<const lp_v4i*>(w[i] + off + 64);
          }
        }
        if constexpr (MX) {
#pragma unroll
          for (int t = 0; t < kSteps / 4; ++t) {
            const int so = s0 + 4 * t < S ? ((s0 >> 2) + t) * 16 : 0;
#pragma unroll
            for (int i = 0; i < NW; ++i) sw[i][t] = *reinterpret_cast<const uint32_t*>(ws[i] + so);
          }
        }
#pragma unroll
        for (int u = 0; u < kSteps; ++u) {
          if (s0 + u < S) {  // workgroup-uniform
            const uint8_t* const ap = arow + (s0 + u) * ainc;
            const lp_v4i a0 = *reinterpret_cast<const lp_v4i*>(ap);
            lp_v4i a1 = {0, 0, 0, 0};
            if constexpr (A8) a1 = *reinterpret_cast<const lp_v4i*>(ap + ahalf);
            uint32_t sa = 127u;
            if constexpr (MX) sa = *reinterpret_cast<const uint32_t*>(asc + ((s0 + u) >> 2) * scinc) >> (8 * (u & 3));
            const lp_v8i av = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
            for (int i = 0; i < NW; ++i) {
              lp_v8i bv = {lo[i][u][0], lo[i][u][1], lo[i][u][2], lo[i][u][3], 0, 0, 0, 0};
              if constexpr (B8) bv = lp_v8i{lo[i][u][0], lo[i][u][1], lo[i][u][2], lo[i][u][3],
                                            hi[i][u][0], hi[i][u][1], hi[i][u][2], hi[i][u][3]};
              uint32_t sb = 127u;
              if constexpr (MX) sb = sw[i][u >> 2] >> (8 * (u & 3));
              acc[i] = lp_mfma<B8, A8>(bv, sb, av, sa, acc[i]);
            }
          }
        }
      }

      // lane (r16, g): row r16 of the batch, output columns n + 4 g + 0..3
      const int col = n + 4 * g;
      _Float16 v[NW][4];
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        // (the weight rows of the lane's four columns: those of lanes 4 g .. 4 g + 3)
        const int wrow = DOWN ? col : a.layout == MXMOE_DECODE_GU_INTERLEAVED ? 2 * n + 4 * g + 16 * i : i * C + col;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (MX) v[i][j] = (_Float16)acc[i][j];
          else v[i][j] = lp_scaled_out(acc[i][j], s_scale[live ? r16 : 0], reinterpret_cast<const _Float16*>(SB)[wrow + j]);
        }
      }
      if (live) {
        typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
        h4_t o;
        if constexpr (DOWN) {
          o = h4_t{v[0][0], v[0][1], v[0][2], v[0][3]};
        } else {
          const bool has_b = brow != nullptr;  // workgroup-uniform
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const _Float16 bg = has_b ? brow[col + j] : (_Float16)0, bu = has_b ? brow[C + col + j] : (_Float16)0;
            o[j] = a.glu == kGluSwigluClamp ? glu_out<kGluSwigluClamp>(v[0][j], v[1][j], has_b, bg, bu, a.limit, a.c)
                                            : glu_out<kGluSilu>(v[0][j], v[1][j], has_b, bg, bu, a.limit, a.c);
          }
        }
        *reinterpret_cast<h4_t*>(out + (int64_t)orow * C + col) = o;
      }
    }
  }
}

}  // namespace decode
}  // namespace
}  // namespace mxmoe
