// moe_gate_wide.h — the router for 257 .. 512 experts (mxmoe_moe_gate_wide, include/mxmoe_moe.h), gfx950: one
// launch, mxmoe_moe_gate_ex2's rules without the group stage. No reference counterpart (the reference has no router
// kernel); the semantics are the models' public routing code (Kimi-K2: 384 experts, sigmoid + bias; Qwen3-Next:
// 512 experts + a shared-expert gate, softmax over the chosen ones).
//
// Why another kernel: moe_gate.h's body keeps every column block of a token block in every wave (4 NB accumulator
// registers, then x[NB] and key[NB][4] in the finishing wave) and hands 3 NB KiB of partial sums through LDS; at the
// 33 blocks of 513 columns that is ~400 live registers and 99 KiB.
//
// Form. A workgroup owns 16 MR token rows and every column (E experts, + 1 for the shared gate, padded to NB <= 33
// blocks of 16), split into CS column slices of SB <= 9 blocks. Its CS * KS waves are CS slices times a K split
// of KS: wave (slice c, part ks) runs moe_gate.h's K loop (16-B K-contiguous global fragment loads, no LDS staging,
// two register groups in flight, D = W * X^T so a token sits on lane & 15) over the groups of U K-32 steps
// (q KS + ks) U .. + U - 1 of the slice's SB blocks. The partial sums of a slice meet in LDS in a fixed order,
// CS * (KS / 2) * SB KiB <= 36 KiB: MR = 1, a tree towards part 0 (KS = 4: (p0 + p2) + (p1 + p3)); MR = 2 (KS = 2,
// from 256 workgroups of 32 rows on: half the w_gate re-reads from L2 per token, measured 1.77x at T = 8192), part 1
// hands its sums of token block 0 to part 0 and then part 0 its sums of block 1 to part 1 through the one buffer, so
// both parts finish a token block each. The owner of a (slice, token block) then finishes its columns in registers: bias, logits store, shared-gate column, scores, keys (order_key of moe_gate.h), and topk
// local rounds of (largest key, lowest index), whose winners lane group kk & 3 keeps in registers and writes, as
// (key, id), to the slice's sorted candidate list in LDS (8 KiB per token block).
// Merge: the global choice kk of a token is the candidate that exactly kk candidates of all lists beat in
// (key descending, id ascending) — the single-wave kernel's tie rule over the whole row. An owner's lane counts, for
// each candidate it kept, the entries of the other slices' lists that beat it (every read serves the lane's 4
// candidates); its rank is its place in its own list plus those counts, and a rank below topk is written to the
// token's final list. The global top-k lies in the union of the slices' top-k, so the final list is complete.
// Softmax over all E experts (no renormalize): the row maximum is the first final choice; every owner sums
// exp(x - max) over its columns, the CS sums are added in slice order. The owner of slice 0 writes ids and weights
// with the arithmetic of moe_gate_body.inc. Static LDS: at most 58 KiB (4 slices of 9, 32 rows); no scratch.
#pragma once

#include "moe_gate.h"

namespace mxmoe {
namespace gate {

constexpr int kGateWideMaxExperts = 512;  // 32 column blocks, 33 with the shared gate
constexpr int kGateWideMaxTopk = 16;

// K-32 steps per load group (two groups of SB + 1 fragments beside 4 SB accumulators): moe_gate.h's rule
constexpr int gate_wide_group_steps(int sb, int mr) { return sb <= 8 && mr == 1 ? 2 : 1; }

// CS slices of SB column blocks, K split KS, 16 MR token rows (MR = 2 with KS = 2 only: part ks finishes token
// block ks); SIGMOID: mxmoe_moe_gate_ex's sigmoid scoring (else softmax on the logits).
// The logit bias is a run-time pointer (one wave-uniform branch per workgroup). BF: the bf16 builds (the `if constexpr` in mma below)
template <int CS, int SB, int KS, int MR, int U, bool SIGMOID, bool BF = false>
__global__ __launch_bounds__(64 * CS * KS) void gate_wide_kernel(GateBiasArgs bb) {
  static_assert(MR == 1 || (MR == 2 && KS == 2), "32 rows: one token block per K part");
  static_assert(CS >= 2 && CS <= 4 && SB <= 9 && CS * SB >= 17 && CS * SB <= 36, "17 .. 33 blocks in <= 4 slices of <= 9");
  static_assert(KS == 2 || KS == 4, "K split of 2 or 4");
  constexpr int kRedSlots = KS / 2;
  static_assert(CS * kRedSlots * SB <= 36, "partial sums: at most 36 KiB of LDS");
  constexpr int KMAX = kGateWideMaxTopk;
  __shared__ gf4_t red[CS * kRedSlots * SB * 64];
  __shared__ uint2 cand[MR * CS * KMAX * 16];  // [token block][slice][choice][token]: (key, expert)
  __shared__ uint2 fin[MR * KMAX * 16];        // [token block][choice][token]: the merged list
  __shared__ float fin_score[MR * KMAX * 16];  // (sigmoid: the chosen experts' unbiased scores)
  __shared__ float part[MR * CS * 16];         // [token block][slice][token]: sum of exp(x - max) over the slice's columns

  const GateModeArgs& m = bb.m;
  const GateArgs& a = m.g;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slice = wave % CS, ks = wave / CS;  // waves 0 .. CS - 1 are the slice owners
  const int c16 = lane & 15, g = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * (16 * MR);
  const int E = a.E;
  const int col0 = 16 * SB * slice;  // the slice's first column

  // fragment rows: tokens past T and columns past E (+ 1) read a clamped, existing row; what they produce is never
  // used (masked by index below) and never stored
  const _Float16* hp[MR];
  const _Float16* wp[SB];
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    int64_t r = row0 + 16 * i + c16;
    r = r < a.T ? r : a.T - 1;
    hp[i] = a.hidden + r * a.H + 8 * g;
  }
#pragma unroll
  for (int j = 0; j < SB; ++j) {
    const int c = col0 + 16 * j + c16;
    const _Float16* p = c < E ? a.w_gate + (int64_t)c * a.H : (c == E && a.w_shared) ? a.w_shared : a.w_gate;
    wp[j] = p + 8 * g;
  }

  gf4_t acc[MR][SB];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < SB; ++j) acc[i][j] = gf4_t{0.0f, 0.0f, 0.0f, 0.0f};

  const int nsteps = a.H >> 5;
  // (moe_gate_body.inc's loop: a step past H loads step 0 and is skipped by mma, wave-uniformly)
  auto load = [&](int s0, gh8_t(&h)[U][MR], gh8_t(&w)[U][SB]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int off = s0 + u < nsteps ? (s0 + u) * 32 : 0;
#pragma unroll
      for (int i = 0; i < MR; ++i) h[u][i] = *reinterpret_cast<const gh8_t*>(hp[i] + off);
#pragma unroll
      for (int j = 0; j < SB; ++j) w[u][j] = *reinterpret_cast<const gh8_t*>(wp[j] + off);
    }
  };
  auto mma = [&](int s0, const gh8_t(&h)[U][MR], const gh8_t(&w)[U][SB]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < nsteps) {
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < SB; ++j)
            if constexpr (BF)  // (in place, not through a helper: moe_gate.h, above gate_kernel)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gb8_t, w[u][j]),
                                                                  __builtin_bit_cast(gb8_t, h[u][i]), acc[i][j], 0, 0, 0);
            else
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[u][j], h[u][i], acc[i][j], 0, 0, 0);
      }
    }
  };
  {
    constexpr int kStride = KS * U;
    gh8_t hA[U][MR], wA[U][SB], hB[U][MR], wB[U][SB];
    int s = ks * U;
    if (s < nsteps) {
      load(s, hA, wA);
      for (;;) {
        const bool more1 = s + kStride < nsteps;
        if (more1) load(s + kStride, hB, wB);
        mma(s, hA, wA);
        if (!more1) break;
        const bool more2 = s + 2 * kStride < nsteps;
        if (more2) load(s + 2 * kStride, hA, wA);
        mma(s + kStride, hB, wB);
        if (!more2) break;
        s += 2 * kStride;
      }
    }
  }

  // split-K reduction of every slice, in a fixed order
  if constexpr (MR == 1) {
    // a tree: parts [step, 2 step) hand theirs to parts [0, step)
#pragma unroll
    for (int step = KS / 2; step >= 1; step >>= 1) {
      if (ks >= step && ks < 2 * step) {
#pragma unroll
        for (int j = 0; j < SB; ++j) red[((slice * kRedSlots + ks - step) * SB + j) * 64 + lane] = acc[0][j];
      }
      __syncthreads();
      if (ks < step) {
#pragma unroll
        for (int j = 0; j < SB; ++j) acc[0][j] += red[((slice * kRedSlots + ks) * SB + j) * 64 + lane];
      }
      if (step > 1) __syncthreads();
    }
  } else {
    // two parts, two token blocks: part 1 hands its sums of block 0 to part 0, then part 0 its sums of block 1 to
    // part 1, through the one buffer (p0 + p1 and p1 + p0: the same f32 sum)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (ks != i) {
#pragma unroll
        for (int j = 0; j < SB; ++j) red[(slice * SB + j) * 64 + lane] = acc[i][j];
      }
      __syncthreads();
      if (ks == i) {
#pragma unroll
        for (int j = 0; j < SB; ++j) acc[i][j] += red[(slice * SB + j) * 64 + lane];
      }
      if (i == 0) __syncthreads();
    }
  }

  // Every wave stays for the barriers below; only the owners (part ks < MR: token block ks) work between them.
  const bool owner = ks < MR;
  const int tb = MR == 1 ? 0 : (ks & 1);  // the owner's token block
  // this lane: token t, experts col0 + 16 j + 4 g + r
  const int64_t t = row0 + 16 * tb + c16;
  const bool live = t < a.T;
  const bool vec = (E & 3) == 0;  // a row of an f32 [T][E] output in 16-B pieces (and the buffer 16-byte aligned)

  gf4_t x[SB];
  uint32_t sk[4] = {0, 0, 0, 0};
  int se[4] = {0, 0, 0, 0};
  float ss[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (owner) {
#pragma unroll
    for (int j = 0; j < SB; ++j) {
      x[j] = acc[0][j];
      if constexpr (MR == 2) {
        if (tb == 1) x[j] = acc[1][j];  // wave-uniform
      }
    }
    if (bb.logit_bias) {  // x[e] += logit_bias[e], e < E: one add, before everything that reads x (not the shared column)
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = col0 + 16 * j + 4 * g + r;
          const float b = bb.logit_bias[e < E ? e : E - 1];
          x[j][r] = e < E ? x[j][r] + b : x[j][r];
        }
    }
    auto store_row = [&](float* out) {
      float* row = out + t * E;
      const bool v16 = vec && ((uintptr_t)out & 15) == 0;
#pragma unroll
      for (int j = 0; j < SB; ++j) {
        const int e0 = col0 + 16 * j + 4 * g;
        if (v16) {
          if (e0 < E) *reinterpret_cast<gf4_t*>(row + e0) = x[j];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (e0 + r < E) row[e0 + r] = x[j][r];
        }
      }
    };
    if (a.logits && live) store_row(a.logits);

    if (a.w_shared) {  // column E (in one slice only): one more output column, outside the softmax and the selection
      float s = 0.0f;
      bool mine = false;
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col0 + 16 * j + 4 * g + r == E) {
            s = x[j][r];
            mine = true;
          }
      if (live && mine) a.shared_w[t] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s * -kLog2e));
    }

    uint32_t key[SB][4];
    if constexpr (SIGMOID) {
      // x becomes the scores s (the logits are stored by then), key = the keys of v = s + e_bias
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[j][r] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x[j][r] * -kLog2e));
      if (m.scores && live) store_row(m.scores);
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = col0 + 16 * j + 4 * g + r;
          const float b = m.e_bias ? m.e_bias[e < E ? e : E - 1] : 0.0f;
          key[j][r] = e < E ? order_key(m.e_bias ? x[j][r] + b : x[j][r]) : 0u;
        }
    } else {
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) key[j][r] = col0 + 16 * j + 4 * g + r < E ? order_key(x[j][r]) : 0u;
    }

    // the slice's top-k: moe_gate_body.inc's rounds over the slice's registers and the token's 4 lane groups. Choice
    // kk is kept by lane group kk & 3 in slot kk >> 2 and written to the slice's list. (A slice with fewer than topk
    // columns fills up with key 0, which every real candidate beats.)
    for (int kk = 0; kk < a.topk; ++kk) {
      uint32_t bk = 0;
      int be = 0x7fffffff;
      float bs = 0.0f;
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key[j][r] > bk) {
            bk = key[j][r];
            be = col0 + 16 * j + 4 * g + r;
            if constexpr (SIGMOID) bs = x[j][r];
          }
#pragma unroll
      for (int d = 16; d <= 32; d <<= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)bk, d, 64);
        const int oe = __shfl_xor(be, d, 64);
        float os = 0.0f;
        if constexpr (SIGMOID) os = __shfl_xor(bs, d, 64);
        if (ok > bk || (ok == bk && oe < be)) {
          bk = ok;
          be = oe;
          bs = os;
        }
      }
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col0 + 16 * j + 4 * g + r == be) key[j][r] = 0u;
      if ((kk & 3) == g) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q == (kk >> 2)) {
            sk[q] = bk;
            se[q] = be;
            ss[q] = bs;
          }
        cand[((tb * CS + slice) * KMAX + kk) * 16 + c16] = uint2{bk, (uint32_t)be};
      }
    }
  }
  __syncthreads();

  if (owner) {
    // merge: rank of the lane's candidate 4 q + g = its place in its own list + the other lists' entries that beat it
    int rank[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rank[q] = 4 * q + g;
#pragma unroll
    for (int c = 0; c < CS; ++c) {
      if (c != slice) {  // wave-uniform
        for (int i = 0; i < a.topk; ++i) {
          const uint2 o = cand[((tb * CS + c) * KMAX + i) * 16 + c16];
#pragma unroll
          for (int q = 0; q < 4; ++q) rank[q] += (o.x > sk[q] || (o.x == sk[q] && (int)o.y < se[q])) ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (4 * q + g < a.topk && rank[q] < a.topk) {
        fin[(tb * KMAX + rank[q]) * 16 + c16] = uint2{sk[q], (uint32_t)se[q]};
        if constexpr (SIGMOID) fin_score[(tb * KMAX + rank[q]) * 16 + c16] = ss[q];
      }
    }
  }
  __syncthreads();

  const bool full_softmax = !SIGMOID && !a.renorm;  // workgroup-uniform
  if (full_softmax) {
    if (owner) {
      const float mx = key_value(fin[tb * KMAX * 16 + c16].x);  // the first choice is the row's maximum
      float sum = 0.0f;
#pragma unroll
      for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) sum += col0 + 16 * j + 4 * g + r < E ? exp_rel(x[j][r], mx) : 0.0f;
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      if (g == 0) part[(tb * CS + slice) * 16 + c16] = sum;
    }
    __syncthreads();
  }

  if (slice != 0 || !owner || !live) return;
  // the owner of slice 0, lane (token, g): choices 4 q + g, moe_gate_body.inc's arithmetic
  uint2 f[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) f[q] = 4 * q + g < a.topk ? fin[(tb * KMAX + 4 * q + g) * 16 + c16] : uint2{0u, 0u};
  if constexpr (SIGMOID) {
    float sc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sc[q] = 4 * q + g < a.topk ? fin_score[(tb * KMAX + 4 * q + g) * 16 + c16] : 0.0f;
    float sum = 1.0f;
    if (a.renorm) {
      sum = ((sc[0] + sc[1]) + sc[2]) + sc[3];
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      sum += 1e-20f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kk = 4 * q + g;
      if (kk < a.topk) {
        a.ids[t * a.topk + kk] = (int)f[q].y;
        a.weights[t * a.topk + kk] = (a.renorm ? sc[q] / sum : sc[q]) * m.routed_scale;
      }
    }
  } else {
    const float mx = key_value(fin[tb * KMAX * 16 + c16].x);
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = 4 * q + g < a.topk ? exp_rel(key_value(f[q].x), mx) : 0.0f;
    float sum;
    if (a.renorm) {
      sum = ((p[0] + p[1]) + p[2]) + p[3];
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
    } else {
      sum = part[tb * CS * 16 + c16];
#pragma unroll
      for (int c = 1; c < CS; ++c) sum += part[(tb * CS + c) * 16 + c16];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kk = 4 * q + g;
      if (kk < a.topk) {
        a.ids[t * a.topk + kk] = (int)f[q].y;
        a.weights[t * a.topk + kk] = p[q] / sum * m.routed_scale;
      }
    }
  }
}

template <int CS, int SB, int KS, int MR, bool BF>
inline void gate_wide_launch_mr(const GateBiasArgs& b, bool sigmoid, hipStream_t st) {
  constexpr int U = gate_wide_group_steps(SB, MR);
  const dim3 blocks((unsigned)((b.m.g.T + 16 * MR - 1) / (16 * MR))), threads(64 * CS * KS);
  if (sigmoid) hipLaunchKernelGGL((gate_wide_kernel<CS, SB, KS, MR, U, true, BF>), blocks, threads, 0, st, b);
  else hipLaunchKernelGGL((gate_wide_kernel<CS, SB, KS, MR, U, false, BF>), blocks, threads, 0, st, b);
}
// 32 rows per workgroup (half the w_gate re-reads per token) once the grid still has a workgroup per CU
// (gate_rows_per_wg of moe_gate.h); the K split of 4 keeps 16
template <int CS, int SB, int KS, bool BF>
inline void gate_wide_launch_one(const GateBiasArgs& b, bool sigmoid, hipStream_t st) {
  if constexpr (KS == 2) {
    if (gate_rows_per_wg(b.m.g.T, 2) == 2) return gate_wide_launch_mr<CS, SB, KS, 2, BF>(b, sigmoid, st);
  }
  gate_wide_launch_mr<CS, SB, KS, 1, BF>(b, sigmoid, st);
}
// one launch; the caller has validated the arguments (T > 0, 256 < E <= 512, no groups). The fewest slices of at most
// 9 blocks, then the fewest blocks per slice; 8 waves (6 for three slices)
template <bool BF = false>
inline void gate_wide_launch(const GateBiasArgs& b, bool sigmoid, hipStream_t st) {
  const int nb = (b.m.g.E + (b.m.g.w_shared ? 1 : 0) + 15) / 16;  // 17 .. 33
  if (nb <= 18) gate_wide_launch_one<2, 9, 4, BF>(b, sigmoid, st);
  else if (nb <= 21) gate_wide_launch_one<3, 7, 2, BF>(b, sigmoid, st);
  else if (nb <= 24) gate_wide_launch_one<3, 8, 2, BF>(b, sigmoid, st);
  else if (nb <= 27) gate_wide_launch_one<3, 9, 2, BF>(b, sigmoid, st);
  else if (nb <= 28) gate_wide_launch_one<4, 7, 2, BF>(b, sigmoid, st);
  else if (nb <= 32) gate_wide_launch_one<4, 8, 2, BF>(b, sigmoid, st);
  else gate_wide_launch_one<4, 9, 2, BF>(b, sigmoid, st);
}

}  // namespace gate
}  // namespace mxmoe
