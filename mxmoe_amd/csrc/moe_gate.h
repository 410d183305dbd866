// moe_gate.h — the MoE router as one launch (mxmoe_moe_gate, include/mxmoe_moe.h), gfx950:
// gate logits (fp16 x fp16 -> f32 on v_mfma_f32_16x16x32_f16), top-k selection on the logits,
// softmax weights and the optional shared-expert gate. No reference counterpart: the reference has no
// router kernel; the semantics are the models' own softmax -> topk code (qwen2_moe, DeepSeek-V2-Lite,
// Mixtral) and qwen2_moe's sigmoid(shared_expert_gate(hidden)).
//
// Form. A workgroup of NW = 8 waves (4 beyond 192 columns) owns 16 * MR token rows and every column
// (E experts, + 1 for the shared gate, padded to NB blocks of 16). Both operands are K-contiguous,
// which is the MFMA operand layout itself (lane l: row l & 15, k = 8 (l >> 4) + j), so fragments are
// 16-B global loads — no LDS staging. The K loop is split over the waves: wave w takes the groups of
// U K-32 steps (q NW + w) U .. + U - 1 (U * 64 contiguous bytes of each row), two groups in
// registers, so the kernel's dependent memory round trips are H / (32 NW U) — 2 at H = 2048 — and
// even one workgroup keeps 8 waves' loads in flight (bs 128 is 8 workgroups). w_gate (240 - 256 KiB
// at H = 2048) is re-read from L2 once per workgroup, i.e. per 16 * MR rows; MR grows with T
// (gate_rows_per_wg).
// The MFMA is issued as D = W * X^T (experts on the A side): the accumulator then has the TOKEN on
// lane & 15 and expert 16 j + 4 (lane >> 4) + reg in lane group / register, so a token's reduction
// over experts is in-lane over 4 NB registers plus two cross-lane steps (lane ^ 16, lane ^ 32).
// The waves' partial sums meet in LDS in a fixed order (at most 4 MR NB KiB <= 64 KiB); wave i then
// finishes token block i entirely in registers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mxmoe {
namespace gate {

typedef _Float16 gh8_t __attribute__((ext_vector_type(8)));
typedef float gf4_t __attribute__((ext_vector_type(4)));

struct GateArgs {
  const _Float16* hidden;    // [T][H]
  const _Float16* w_gate;    // [E][H]
  const _Float16* w_shared;  // [H] or NULL
  int64_t T;
  int H, E, topk, renorm;
  int32_t* ids;      // [T][topk]
  float* weights;    // [T][topk]
  float* shared_w;   // [T] or NULL
  float* logits;     // [T][E] or NULL
};

constexpr int kGateMaxBlocks = 17;  // 256 experts + the shared gate
constexpr float kLog2e = 1.4426950408889634f;

// f32 -> uint32 whose unsigned order is the float order (-0 first made +0, so equal logits get equal
// keys; NaNs sort above +Inf / below -Inf by their sign). Valid columns have keys >= 1; 0 marks a
// padded or already selected column, so a row of NaN / Inf logits still selects distinct experts.
__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t b = __builtin_bit_cast(uint32_t, x + 0.0f);
  const uint32_t k = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  return k ? k : 1u;
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
__device__ __forceinline__ float exp_rel(float x, float m) { return __builtin_amdgcn_exp2f((x - m) * kLog2e); }

template <int NB, int MR, int NW, int U>
__global__ __launch_bounds__(64 * NW) void gate_kernel(GateArgs a) {
  constexpr int kSlots = NW == 8 ? 4 : 3;  // partial-sum tiles in LDS at a time, per (token block, column block)
  static_assert(NW == 4 || NW == 8, "4 or 8 waves");
  static_assert(MR >= 1 && MR <= 4 && MR * kSlots * NB * 1024 <= 64 * 1024, "partial sums must fit 64 KiB of LDS");
  __shared__ gf4_t red[MR * kSlots * NB * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * (16 * MR);
  const int E = a.E;

  // fragment rows: tokens past T and columns past E (+ 1) read a clamped, existing row; what they
  // produce is never used (masked by index below) and never stored
  const _Float16* hp[MR];
  const _Float16* wp[NB];
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    int64_t r = row0 + 16 * i + c16;
    r = r < a.T ? r : a.T - 1;
    hp[i] = a.hidden + r * a.H + 8 * g;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int c = 16 * j + c16;
    const _Float16* p = c < E ? a.w_gate + (int64_t)c * a.H : (c == E && a.w_shared) ? a.w_shared : a.w_gate;
    wp[j] = p + 8 * g;
  }

  gf4_t acc[MR][NB];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = gf4_t{0.0f, 0.0f, 0.0f, 0.0f};

  const int nsteps = a.H >> 5;
  // U consecutive K-32 steps s0 .. s0 + U - 1 of every fragment row (U * 64 contiguous bytes of each
  // row). A step past H loads step 0 instead and is skipped by mma (wave-uniform): nothing here
  // consumes a loaded register, so a prefetched group stays in flight across the previous one's MFMAs
  auto load = [&](int s0, gh8_t(&h)[U][MR], gh8_t(&w)[U][NB]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int off = s0 + u < nsteps ? (s0 + u) * 32 : 0;
#pragma unroll
      for (int i = 0; i < MR; ++i) h[u][i] = *reinterpret_cast<const gh8_t*>(hp[i] + off);
#pragma unroll
      for (int j = 0; j < NB; ++j) w[u][j] = *reinterpret_cast<const gh8_t*>(wp[j] + off);
    }
  };
  auto mma = [&](int s0, const gh8_t(&h)[U][MR], const gh8_t(&w)[U][NB]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s0 + u < nsteps) {
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[u][j], h[u][i], acc[i][j], 0, 0, 0);
      }
    }
  };
  {
    // wave w: groups (q NW + w) U, q = 0, 1, ...; two register buffers, the next group's loads issued
    // before the current group's MFMAs
    constexpr int kStride = NW * U;
    gh8_t hA[U][MR], wA[U][NB], hB[U][MR], wB[U][NB];
    int s = wave * U;
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

  // split-K reduction, in a fixed order. 8 waves: waves 4-7 first hand everything to waves 0-3
  if constexpr (NW == 8) {
    if (wave >= 4) {
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) red[(((wave - 4) * MR + i) * NB + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] += red[((wave * MR + i) * NB + j) * 64 + lane];
    }
    __syncthreads();
  }
  // then wave w < 4 hands its partial of token block i != w to wave i (slot (w - i - 1) & 3)
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    if (i != wave && wave < 4) {
      const int slot = (wave - i - 1) & 3;
#pragma unroll
      for (int j = 0; j < NB; ++j) red[((i * 3 + slot) * NB + j) * 64 + lane] = acc[i][j];
    }
  }
  __syncthreads();
  if (wave >= MR || row0 + 16 * wave >= a.T) return;  // wave-uniform
  gf4_t x[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    x[j] = acc[0][j];
#pragma unroll
    for (int i = 1; i < MR; ++i)
      if (i == wave) x[j] = acc[i][j];
#pragma unroll
    for (int sl = 0; sl < 3; ++sl) x[j] += red[((wave * 3 + sl) * NB + j) * 64 + lane];
  }

  // this lane: token t, experts 16 j + 4 g + r
  const int64_t t = row0 + 16 * wave + c16;
  const bool live = t < a.T;

  if (a.logits && live) {
    float* lrow = a.logits + t * E;
    const bool vec = (E & 3) == 0 && ((uintptr_t)a.logits & 15) == 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int e0 = 16 * j + 4 * g;
      if (vec) {
        if (e0 < E) *reinterpret_cast<gf4_t*>(lrow + e0) = x[j];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (e0 + r < E) lrow[e0 + r] = x[j][r];
      }
    }
  }

  if (a.w_shared) {  // column E: one more output column, outside the softmax and the selection
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * j + 4 * g + r == E) s = x[j][r];
    if (live && g == ((E & 15) >> 2)) a.shared_w[t] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(s * -kLog2e));
  }

  uint32_t key[NB][4];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) key[j][r] = 16 * j + 4 * g + r < E ? order_key(x[j][r]) : 0u;

  // top-k: k rounds of (largest key, lowest index) over the lane's registers and the token's 4 lane
  // groups; choice kk is kept by lane group kk & 3 in slot kk >> 2
  uint32_t sk[4] = {0, 0, 0, 0}, mkey = 0;
  int se[4] = {0, 0, 0, 0};
  for (int kk = 0; kk < a.topk; ++kk) {
    uint32_t bk = 0;
    int be = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (key[j][r] > bk) {
          bk = key[j][r];
          be = 16 * j + 4 * g + r;
        }
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {
      const uint32_t ok = (uint32_t)__shfl_xor((int)bk, d, 64);
      const int oe = __shfl_xor(be, d, 64);
      if (ok > bk || (ok == bk && oe < be)) {
        bk = ok;
        be = oe;
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * j + 4 * g + r == be) key[j][r] = 0u;
    if (kk == 0) mkey = bk;
    if ((kk & 3) == g) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q == (kk >> 2)) {
          sk[q] = bk;
          se[q] = be;
        }
    }
  }

  const float m = key_value(mkey);  // the first choice is the row's maximum
  float p[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) p[q] = 4 * q + g < a.topk ? exp_rel(key_value(sk[q]), m) : 0.0f;
  float sum = 0.0f;
  if (a.renorm) {
    sum = ((p[0] + p[1]) + p[2]) + p[3];
  } else {
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += 16 * j + 4 * g + r < E ? exp_rel(x[j][r], m) : 0.0f;
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if (!live) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kk = 4 * q + g;
    if (kk < a.topk) {
      a.ids[t * a.topk + kk] = se[q];
      a.weights[t * a.topk + kk] = p[q] / sum;
    }
  }
}

// A/B build knobs (-D; DESIGN.md §4 "Router", profiles/r07/gate/ab_builds.jsonl): waves per workgroup
// (8 or 4), the cap on K-32 steps per load group, and MXMOE_GATE_FORCE_MR = 1 | 2 | 4 rows / 16 per
// workgroup whatever T is
#ifndef MXMOE_GATE_NW
#define MXMOE_GATE_NW 8
#endif
#ifndef MXMOE_GATE_U
#define MXMOE_GATE_U 4
#endif
// K-32 steps per load group: as many (4, 2, 1) as two groups of (MR + NB) fragments fit the 256
// registers of a wave beside the accumulators without spilling (checked with
// -Rpass-analysis=kernel-resource-usage)
constexpr int gate_group_steps(int nb, int mr) {
  const int u = nb <= 4 ? (mr == 4 ? 2 : 4) : nb == 5 ? (mr == 2 ? 2 : 4) : nb <= 8 ? (mr == 2 ? 1 : 2) : 1;
  return u < MXMOE_GATE_U ? u : MXMOE_GATE_U;
}
// 16 * MR token rows per workgroup: as many as the accumulators and the LDS allow (max_mr) while the
// grid still has a workgroup per CU: the w_gate re-reads per token shrink with MR, but a CU's own
// load rate is the bound, so idle CUs cost more (measured: DESIGN.md §4 "Router")
inline int gate_rows_per_wg(int64_t T, int max_mr) {
#ifdef MXMOE_GATE_FORCE_MR
  const int cap = MXMOE_GATE_FORCE_MR;
  const int64_t want = 0;
#else
  const int cap = 4;
  const int64_t want = 256;
#endif
  int mr = max_mr < cap ? max_mr : cap;
  while (mr > 1 && (T + 16 * mr - 1) / (16 * mr) < want) mr >>= 1;
  return mr;
}

template <int NB, int MR, int NW, int U>
inline void gate_launch_one(const GateArgs& a, hipStream_t st) {
  const unsigned blocks = (unsigned)((a.T + 16 * MR - 1) / (16 * MR));
  hipLaunchKernelGGL((gate_kernel<NB, MR, NW, U>), dim3(blocks), dim3(64 * NW), 0, st, a);
}
// NB column blocks: 8 waves split K while 4 partial tiles per (token, column) block fit the LDS
// (NB <= 12), else 4; MR up to 64 / NB accumulator registers' worth
template <int NB>
inline void gate_launch_nb(const GateArgs& a, hipStream_t st) {
  constexpr int NW = NB <= 12 ? MXMOE_GATE_NW : 4;
  constexpr int MAXMR = NB <= 4 ? 4 : NB <= 8 ? 2 : 1;
  const int mr = gate_rows_per_wg(a.T, MAXMR);
  if constexpr (MAXMR >= 4) {
    if (mr == 4) return gate_launch_one<NB, 4, NW, gate_group_steps(NB, 4)>(a, st);
  }
  if constexpr (MAXMR >= 2) {
    if (mr == 2) return gate_launch_one<NB, 2, NW, gate_group_steps(NB, 2)>(a, st);
  }
  gate_launch_one<NB, 1, NW, gate_group_steps(NB, 1)>(a, st);
}
// one launch; the caller has validated the arguments (T > 0)
inline void gate_launch(const GateArgs& a, hipStream_t st) {
  const int nb = (a.E + (a.w_shared ? 1 : 0) + 15) / 16;
  if (nb <= 1) gate_launch_nb<1>(a, st);
  else if (nb <= 2) gate_launch_nb<2>(a, st);
  else if (nb <= 4) gate_launch_nb<4>(a, st);
  else if (nb <= 5) gate_launch_nb<5>(a, st);
  else if (nb <= 8) gate_launch_nb<8>(a, st);
  else if (nb <= 12) gate_launch_nb<12>(a, st);
  else gate_launch_nb<kGateMaxBlocks>(a, st);
}

}  // namespace gate
}  // namespace mxmoe
