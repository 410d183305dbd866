// gg_mxf6.h — w6a6_g32_sym_MXFP6 (QT_MXF6): OCP MXFP6 operands (e2m3 codes, one e8m0 scale per 32-K block) on
// v_mfma_scale_f32_16x16x128_f8f6f4, the block scales as the instruction's scale operands, f32 accumulate,
// C = fp16_rn(acc). A tile body of gg_v2_kernel (512 threads, 2 x 4 waves, 128 x 64 or 64 x 64 wave tiles);
// included by gg_device.h in front of that kernel.
//
// Operand image (include/mxmoe_gg.h, quantize.pack_mxfp6; the same for A and B rows): per K = 128 step 96 bytes,
//   bytes [0, 64)  P: 16 B per MX block g (g < 4) = dwords 0-3 of the block's 192-bit value (code j at bit 6 j)
//   bytes [64, 96) Q:  8 B per block               = dwords 4-5
// MFMA lane map: lane l holds row l & 15 and block g = l >> 4 of the step: its fragment is P chunk g + Q piece g,
// six dwords, padded to the builtin's eight with zeros (format code 2 reads six).
//
// LDS: two A stages, then three B stages, 96 B per row each (256-row tile: 2 x 24 + 3 x 24 = 120 KiB). A stage of R
// rows is P | Q:
//   P  64-B rows, 16-B chunk c of row r at chunk c ^ swz64(r): a fragment's 16-row ds_read_b128 spreads over the banks.
//      Filled by 16-row x 64-B pieces (one wave instruction = one fragment's P).
//   Q  512 B per 16-row fragment, block pair c = g >> 1 of row r at (16 c + r) * 16, block g's 8 B at + 8 (g & 1): a
//      fragment's ds_read_b64 covers 256 contiguous bytes per half wave. Filled by ONE wave instruction per two
//      fragments (lanes 0-31 the first, 32-63 the second); the 128-row class, one A fragment per wave, uses a
//      half-wave piece.
// (Measured, DESIGN.md §4 "MXFP6": a third of the body's LDS-active cycles are bank conflicts all the same; which
// accesses cause them has not been found.)
// Pieces are buffer-form LDS-DMA: the resource starts at the tile's first row and ends after its last valid one, the
// lane offset holds row and chunk (the range check covers it), the stage's 96 s bytes go in the scalar offset. Rows
// past M or N read as zero codes; K is whole steps (the planner checks), so the loop has no tail code.
//
// Ring: A is fetched one stage ahead, B two. Iteration s: wait for A(s) and B(s) (vmcnt leaves B(s + 1), issued last,
// in flight), barrier, issue A(s + 1) into the A buffer compute(s - 1) read and B(s + 2) into the B buffer it read,
// compute(s) with the six or five pieces spread through its MFMAs (sched_group_barrier).
//
// Scales never pass LDS: dword g of 16-byte group t of a row's device-layout scales (pack_mxfp4_scales) holds
// block g's scale bytes of steps 4 t .. 4 t + 3. Every fourth step a lane loads one dword per fragment row (A) and
// column (B) for the NEXT four steps, by range-checked buffer loads issued in front of that step's pieces (so the
// ring's own waits land them); a step's MFMAs select its byte of the dwords (the loop runs groups of four steps
// unrolled, so the byte index is an immediate). A row past M / N
// reads scale code 0 on zero codes: a zero product, never stored.
#pragma once

namespace mxmoe {

// fp6 e2m3 x e2m3 over K = 128 (format code 2 for both operands); byte SEL of sb / sa is the e8m0 scale of the
// lane's block
template <int SEL>
__device__ __forceinline__ v4f mfma_mxf6_k128(const v8i& b, uint32_t sb, const v8i& a, uint32_t sa, const v4f& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, c, 2, 2, SEL, (int)sb, SEL, (int)sa);
}

template <class Cfg>
__device__ __forceinline__ void gg_tile_mxf6(const GGMeta& mt, const uint8_t* __restrict__ A,
                                             const uint8_t* __restrict__ B, const uint8_t* __restrict__ SA,
                                             const uint8_t* __restrict__ SB, _Float16* __restrict__ C, int m0, int n0,
                                             uint8_t* lds) {
  constexpr int FM = Cfg::FM, FN = Cfg::FN, BM = Cfg::BM, BN = Cfg::BN;
  constexpr int SKB = 96, NW = Cfg::WM * Cfg::WN;
  constexpr int A_STAGE = BM * SKB, B_STAGE = BN * SKB, A_Q = BM * 64, B_Q = BN * 64, B_RING = 2 * A_STAGE;
  constexpr int GA = BM / (16 * NW), GB = BN / (16 * NW);  // fragments (P pieces) per wave and stage
  constexpr int QA = (GA + 1) / 2, QB = (GB + 1) / 2;      // Q pieces: full-wave over two fragments, or a half wave
  constexpr int DA = GA + QA, DB = GB + QB;
  static_assert(NW == 8 && Cfg::NT == 512 && Cfg::WTN == 64, "2 x 4 waves, 128-B staged epilogue rows");
  static_assert(GA * 16 * NW == BM && GB * 16 * NW == BN && (GA == 1 || GA % 2 == 0) && GB % 2 == 0, "whole pieces");
  static_assert(B_RING + 3 * B_STAGE <= 120 * 1024 && Cfg::EPI_BYTES <= V2Cfg<256>::LDS_BYTES, "inside either v2 LDS image");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / Cfg::WN, wn = wave % Cfg::WN;
  const int r16 = lane & 15, g = lane >> 4;
  const int M = mt.M, N = mt.N;
  const int lda = (int)mt.lda_b, ldb = (int)mt.ldb_b;  // below 8 MiB (the planner checks): 256 rows stay below 2^31
  const int nst = mt.kbytes / SKB;
  const int rowsA = min(M - m0, BM), rowsB = min(N - n0, BN);

  auto rsrc = [](const uint8_t* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), (short)0, bytes, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rsA = rsrc(A + (int64_t)m0 * lda, rowsA * lda);
  const __amdgpu_buffer_rsrc_t rsB = rsrc(B + (int64_t)n0 * ldb, rowsB * ldb);
  uint32_t voAP[GA], voAQ[QA], voBP[GB], voBQ[QB];
  {
    const int rsub = lane >> 2, p = lane & 3;        // P piece: lane -> row rsub, physical chunk p
    const uint32_t qo = 64u + ((lane >> 4) & 1) * 16u;  // Q piece: lane -> row r16 (+ 16 in the upper half wave), block pair
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      const int rp = (wave * GA + j) * 16 + rsub;
      voAP[j] = (uint32_t)(rp * lda) + (uint32_t)((p ^ swz64(rp)) << 4);
    }
#pragma unroll
    for (int j = 0; j < QA; ++j) voAQ[j] = (uint32_t)(((wave * GA + 2 * j) * 16 + (GA > 1 ? (lane >> 5) * 16 : 0) + r16) * lda) + qo;
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const int rp = (wave * GB + j) * 16 + rsub;
      voBP[j] = (uint32_t)(rp * ldb) + (uint32_t)((p ^ swz64(rp)) << 4);
    }
#pragma unroll
    for (int j = 0; j < QB; ++j) voBQ[j] = (uint32_t)(((wave * GB + 2 * j) * 16 + (lane >> 5) * 16 + r16) * ldb) + qo;
  }
  auto issue_a = [&](int s, int buf) {
    uint8_t* st = lds + buf * A_STAGE;
#pragma unroll
    for (int j = 0; j < GA; ++j) v3_bdma(rsA, st + (wave * GA + j) * 1024, voAP[j], s * SKB);
    if constexpr (GA > 1) {
#pragma unroll
      for (int j = 0; j < QA; ++j) v3_bdma(rsA, st + A_Q + (wave * GA + 2 * j) * 512, voAQ[j], s * SKB);
    } else {
      if (lane < 32) v3_bdma(rsA, st + A_Q + wave * 512, voAQ[0], s * SKB);
    }
  };
  auto issue_b = [&](int s, int buf) {
    uint8_t* st = lds + B_RING + buf * B_STAGE;
#pragma unroll
    for (int j = 0; j < GB; ++j) v3_bdma(rsB, st + (wave * GB + j) * 1024, voBP[j], s * SKB);
#pragma unroll
    for (int j = 0; j < QB; ++j) v3_bdma(rsB, st + B_Q + (wave * GB + 2 * j) * 512, voBQ[j], s * SKB);
  };

  // block scales: `nsa` / `nsb` the dwords of the next four steps, `gsa` / `gsb` those of the current four
  const int srow = ((mt.K / 32 + 15) >> 4) << 4;  // scale bytes per row (device layout)
  const __amdgpu_buffer_rsrc_t rsSA = rsrc(SA + (int64_t)m0 * srow, rowsA * srow);
  const __amdgpu_buffer_rsrc_t rsSB = rsrc(SB + (int64_t)n0 * srow, rowsB * srow);
  const int vsa = (wm * Cfg::WTM + r16) * srow + 4 * g, vsb = (wn * Cfg::WTN + r16) * srow + 4 * g;
  uint32_t gsa[FM], gsb[FN], nsa[FM], nsb[FN];
  auto load_scales = [&](int t) {
#pragma unroll
    for (int i = 0; i < FM; ++i) nsa[i] = __builtin_amdgcn_raw_buffer_load_b32(rsSA, vsa + i * 16 * srow + t * 16, 0, 0);
#pragma unroll
    for (int j = 0; j < FN; ++j) nsb[j] = __builtin_amdgcn_raw_buffer_load_b32(rsSB, vsb + j * 16 * srow + t * 16, 0, 0);
  };

  v4f acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = v4f{0, 0, 0, 0};

  // a wave whose rows all lie past M reads no fragment and runs no MFMA; it still issues its pieces
  const bool live = m0 + wm * Cfg::WTM < M;
  const uint32_t offP = (uint32_t)(((g ^ swz64(r16)) << 4) + r16 * 64);
  const uint32_t offQ = (uint32_t)((((g >> 1) * 16 + r16) << 4) + (g & 1) * 8);
  auto frag = [&](const uint8_t* P, const uint8_t* Q) {
    const v4i p = *reinterpret_cast<const v4i*>(P + offP);
    const v2i q = *reinterpret_cast<const v2i*>(Q + offQ);
    return v8i{p[0], p[1], p[2], p[3], q[0], q[1], 0, 0};
  };
  auto compute = [&](int bufa, int bufb, auto U) {
    constexpr int u = decltype(U)::value;  // the step's place in its group of four: the scale byte the MFMA selects
    const uint8_t* sa = lds + bufa * A_STAGE;
    const uint8_t* sb = lds + B_RING + bufb * B_STAGE;
    const uint8_t* AP = sa + wm * Cfg::WTM * 64;
    const uint8_t* AQ = sa + A_Q + wm * Cfg::WTM * 32;
    const uint8_t* BP = sb + wn * Cfg::WTN * 64;
    const uint8_t* BQ = sb + B_Q + wn * Cfg::WTN * 32;
    v8i b[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) b[j] = frag(BP + j * 1024, BQ + j * 512);
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const v8i a = frag(AP + i * 1024, AQ + i * 512);
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = mfma_mxf6_k128<u>(b[j], gsb[j], a, gsa[i], acc[i][j]);
    }
  };

  int bufa = 0, bufb = 0;
  // One K = 128 step. FULL: steps s + 1 and s + 2 exist (no test); U: the step's place in its group of four — a
  // group's first step comes right after the next group's FM + FN scale loads, which its wait leaves in flight too
  auto stage = [&](int s, auto U, auto FULL) {
    constexpr int u = decltype(U)::value;
    constexpr bool full = decltype(FULL)::value;
    if (full || s + 1 < nst) wait_vmcnt<DB + (u == 0 ? FM + FN : 0)>();  // everything but B(s + 1), the last stage issued
    else wait_vmcnt<0>();
    lds_barrier();  // A(s), B(s) landed for every wave; every wave is done with the buffers of stage s - 1
    if (full || s + 1 < nst) issue_a(s + 1, bufa ^ 1);
    if (full || s + 2 < nst) issue_b(s + 2, bufb == 0 ? 2 : bufb - 1);
    if (live) {
      compute(bufa, bufb, U);
      constexpr int KS = FM * FN / (DA + DB);
#pragma unroll
      for (int q = 0; q < DA + DB; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, KS, 0);  // KS MFMAs
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // one VMEM read (an LDS-DMA piece)
      }
    }
    bufa ^= 1;
    bufb = bufb == 2 ? 0 : bufb + 1;
  };
  // (the copy below is ordered by the compiler's own vmcnt wait on nsa / nsb, ahead of the hand-written one: 24 pieces
  // lie behind those loads in steady state, so it waits for nothing; the first group's copy sits right behind the
  // prologue's load_scales(0) and does wait for it, once per tile)
  auto take_scales = [&](int s) {  // at a group's first step s: its scales have landed; fetch the next group's
#pragma unroll
    for (int i = 0; i < FM; ++i) gsa[i] = nsa[i];
#pragma unroll
    for (int j = 0; j < FN; ++j) gsb[j] = nsb[j];
    load_scales(min((s >> 2) + 1, (nst - 1) >> 2));  // (the last group: itself again, unused)
  };
  typedef std::integral_constant<int, 0> U0;
  typedef std::integral_constant<int, 1> U1;
  typedef std::integral_constant<int, 2> U2;
  typedef std::integral_constant<int, 3> U3;
  int s = 0;
  if (nst > 0) {
    load_scales(0);
    issue_a(0, 0);
    issue_b(0, 0);
    if (nst > 1) issue_b(1, 1);
  }
  for (; s + 6 <= nst; s += 4) {  // whole groups whose every step fetches ahead: nothing conditional between the waits
    take_scales(s);
    stage(s, U0{}, std::true_type{});
    stage(s + 1, U1{}, std::true_type{});
    stage(s + 2, U2{}, std::true_type{});
    stage(s + 3, U3{}, std::true_type{});
  }
  for (; s < nst; s += 4) {  // the last one or two groups
    take_scales(s);
    stage(s, U0{}, std::false_type{});
    if (s + 1 < nst) stage(s + 1, U1{}, std::false_type{});
    if (s + 2 < nst) stage(s + 2, U2{}, std::false_type{});
    if (s + 3 < nst) stage(s + 3, U3{}, std::false_type{});
  }
  wait_vmcnt<0>();
  lds_barrier();  // ring -> epilogue staging

  // ---- epilogue (as gg_tile_f8g128): fp16, per-wave LDS staging, 16-B stores ----
  if (!live) return;
  uint8_t* reg = lds + wave * (Cfg::WTM * Cfg::WTN * 2);
  const int mrow0 = m0 + wm * Cfg::WTM, ncol0 = n0 + wn * Cfg::WTN;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int ml = i * 16 + r16;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const uint2 pk = pack4_f16(acc[i][j]);
      const int q = 2 * j + (g >> 1);
      *reinterpret_cast<uint2*>(reg + ml * 128 + ((q ^ (ml & 7)) << 4) + (g & 1) * 8) = pk;
    }
  }
  _Float16* const cbase = C + (int64_t)mrow0 * mt.ldc + ncol0;  // wave-uniform
  const bool narrow = (int64_t)Cfg::WTM * mt.ldc < (int64_t)1 << 29;  // byte offsets < 2^30
#pragma unroll 4
  for (int it = 0; it < Cfg::WTM / 8; ++it) {
    const int row = it * 8 + (lane >> 3), q = lane & 7;
    const uint4 v = *reinterpret_cast<const uint4*>(reg + row * 128 + ((q ^ (row & 7)) << 4));
    const int m = mrow0 + row, n = ncol0 + q * 8;
    if (m < M && n < N) store_c16(cbase, (int64_t)row * mt.ldc + q * 8, narrow, v);
  }
}

}  // namespace mxmoe
