// moe_gate.h — the MoE router as one launch (mxmoe_moe_gate, include/mxmoe_moe.h), gfx950:
// gate logits (fp16 x fp16 -> f32 on v_mfma_f32_16x16x32_f16), top-k selection on the logits,
// softmax weights and the optional shared-expert gate. No reference counterpart: the reference has no
// router kernel; the semantics are the models' own softmax -> topk code (qwen2_moe, DeepSeek-V2-Lite,
// Mixtral) and qwen2_moe's sigmoid(shared_expert_gate(hidden)). mxmoe_moe_gate_ex (gate_modes_kernel)
// adds, behind a compile-time mode of the same body, sigmoid scores with a selection bias,
// group-limited top-k and a scaling factor (DeepSeek-V3 / R1, DeepSeek-V2, GLM-4.5-style).
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
typedef __bf16 gb8_t __attribute__((ext_vector_type(8)));

// The bf16 builds (BF, mxmoe_moe_gate_dt): the 16 bytes of each fragment are 8 bf16 values — the builds keep the
// fp16-typed pointers and fragment registers, so their loads and address arithmetic are the fp16 builds' own — and go
// to v_mfma_f32_16x16x32_bf16, whose operand and accumulator layout is the f16 form's. A product of two bf16 values
// (8-bit significands) is exact in f32; the accumulation is the MFMA's f32.

struct GateArgs {
  const _Float16* hidden;    // [T][H]   (the bf16 builds: bf16 bit patterns, all three operands alike)
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

// mxmoe_moe_gate_ex's routing rules (include/mxmoe_moe.h) on top of GateArgs: sigmoid scores with a
// selection bias, group-limited top-k and a scaling factor on the weights
struct GateModeArgs {
  GateArgs g;
  const float* e_bias;  // [E] or NULL (sigmoid only)
  float* scores;        // [T][E] or NULL (sigmoid only)
  int n_group, topk_group, group_top;
  float routed_scale;
};

// mxmoe_moe_gate_ex2: a bias on the logits themselves (gpt-oss: F.linear(hidden, w, bias)), added once after
// the split-K reduction; everything after it (the logits output, selection, scoring, groups) sees the sum
struct GateBiasArgs {
  GateModeArgs m;
  const float* logit_bias;  // [E]
};
inline const GateArgs& gate_args_of(const GateModeArgs& m) { return m.g; }
inline const GateArgs& gate_args_of(const GateBiasArgs& b) { return b.m.g; }

// what a kernel is compiled for: mxmoe_moe_gate's rule (gate_kernel, which gets no GateModeArgs), or
// mxmoe_moe_gate_ex's with softmax / sigmoid scoring (gate_modes_kernel)
enum GateMode { kGatePlain = 0, kGateSoftmaxEx = 1, kGateSigmoidEx = 2 };

// Row t of an f32 [T][E] output from the lane's registers (experts 16 j + 4 g + r): 16-B stores when
// E % 4 == 0 and the buffer is 16-byte aligned
template <int NB>
__device__ __forceinline__ void gate_store_row(float* out, int64_t t, int E, int g, const gf4_t (&x)[NB]) {
  float* row = out + t * E;
  const bool vec = (E & 3) == 0 && ((uintptr_t)out & 15) == 0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int e0 = 16 * j + 4 * g;
    if (vec) {
      if (e0 < E) *reinterpret_cast<gf4_t*>(row + e0) = x[j];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (e0 + r < E) row[e0 + r] = x[j][r];
    }
  }
}

// Sigmoid scoring: x becomes the scores s (the logits are stored by then), key = the keys of the
// selection values v = s + bias
template <int NB>
__device__ __forceinline__ void gate_sigmoid_keys(const GateModeArgs& m, int64_t t, bool live, int g, gf4_t (&x)[NB],
                                                  uint32_t (&key)[NB][4]) {
  const int E = m.g.E;
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) x[j][r] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x[j][r] * -kLog2e));
  if (m.scores && live) gate_store_row<NB>(m.scores, t, E, g, x);
  const bool vec = (E & 3) == 0 && ((uintptr_t)m.e_bias & 15) == 0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int e0 = 16 * j + 4 * g;
    gf4_t b{0.0f, 0.0f, 0.0f, 0.0f};
    if (m.e_bias) {
      if (vec) {
        if (e0 < E) b = *reinterpret_cast<const gf4_t*>(m.e_bias + e0);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (e0 + r < E) b[r] = m.e_bias[e0 + r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) key[j][r] = e0 + r < E ? order_key(x[j][r] + b[r]) : 0u;
  }
}

// Group stage: the two largest keys of every group (in-lane, then over the token's 4 lane groups),
// topk_group rounds of (largest group key, lowest group) over at most 8 groups, and the keys of the
// other groups' experts zeroed, which is how a padded column is never chosen either. gs % 4 == 0: a
// lane's 4 registers of a block share a group; a group of 20 straddles 16-column blocks, so the
// group of block j is (16 j + 4 g) / gs and not a function of j alone
template <int NB>
__device__ __forceinline__ void gate_group_limit(const GateModeArgs& m, int g, uint32_t (&key)[NB][4]) {
  const int gs = m.g.E / m.n_group;
  uint32_t gkey[8];
#pragma unroll
  for (int G = 0; G < 8; ++G) {
    gkey[G] = 0u;
    if (G < m.n_group) {  // wave-uniform
      const int lo = G * gs, hi = lo + gs;
      uint32_t t1 = 0, t2 = 0;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int e0 = 16 * j + 4 * g;
        const bool in = e0 >= lo && e0 < hi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t k = in ? key[j][r] : 0u;
          t2 = max(t2, min(t1, k));
          t1 = max(t1, k);
        }
      }
#pragma unroll
      for (int d = 16; d <= 32; d <<= 1) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)t1, d, 64), o2 = (uint32_t)__shfl_xor((int)t2, d, 64);
        t2 = max(min(t1, o1), max(t2, o2));
        t1 = max(t1, o1);
      }
      gkey[G] = m.group_top == 2 ? order_key(key_value(t1) + key_value(t2)) : t1;
    }
  }
  uint32_t keep = 0;
  for (int q = 0; q < m.topk_group; ++q) {
    uint32_t bk = 0;
    int bg = 0;
#pragma unroll
    for (int G = 0; G < 8; ++G)
      if (gkey[G] > bk) {
        bk = gkey[G];
        bg = G;
      }
#pragma unroll
    for (int G = 0; G < 8; ++G)
      if (G == bg) gkey[G] = 0u;
    keep |= 1u << bg;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int e0 = 16 * j + 4 * g;
    int grp = 0;
#pragma unroll
    for (int G = 1; G < 8; ++G) grp += e0 >= G * gs;
    if (!((keep >> grp) & 1u)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) key[j][r] = 0u;
    }
  }
}

// Both kernels are the one body of moe_gate_body.inc (K loop, split-K reduction, logits, shared gate,
// top-k rounds, weights), which reads `a`, `ex` and MODE; the mxmoe_moe_gate_ex stages in it are
// `if constexpr (MODE ...)`. It is shared as text and not as a function on purpose: through a
// __forceinline__ function taking the arguments by reference or by value the compiler allocated
// 1-2 registers differently in most gate_kernel instantiations, and mxmoe_moe_gate's kernels are to
// stay the ones measured in DESIGN.md §4 "Router", bit for bit.
template <int NB, int MR, int NW, int U>
__global__ __launch_bounds__(64 * NW) void gate_kernel(GateArgs a) {
  constexpr int MODE = kGatePlain;
  const GateModeArgs* const ex = nullptr;
  constexpr bool LB = false;
  constexpr bool BF = false;  // (a bf16 call with every rule at its default runs gate_modes_kernel: mxmoe_moe_gate_dt)
  const float* const lbias = nullptr;
#include "moe_gate_body.inc"
}
// BF (here and in gate_bias_kernel): the bf16 builds (mxmoe_moe_gate_dt); BF = false is the fp16 kernel as it was
template <int NB, int MR, int NW, int U, int MODE, bool BF = false>
__global__ __launch_bounds__(64 * NW) void gate_modes_kernel(GateModeArgs mm) {
  static_assert(MODE == kGateSoftmaxEx || MODE == kGateSigmoidEx, "an mxmoe_moe_gate_ex mode");
  const GateArgs& a = mm.g;
  const GateModeArgs* const ex = &mm;
  constexpr bool LB = false;
  const float* const lbias = nullptr;
#include "moe_gate_body.inc"
}
// gate_modes_kernel with the logit bias (mxmoe_moe_gate_ex2 with a non-NULL logit_bias): builds of their own, so
// the two kernels above keep their code and registers
template <int NB, int MR, int NW, int U, int MODE, bool BF = false>
__global__ __launch_bounds__(64 * NW) void gate_bias_kernel(GateBiasArgs bb) {
  static_assert(MODE == kGateSoftmaxEx || MODE == kGateSigmoidEx, "an mxmoe_moe_gate_ex mode");
  const GateArgs& a = bb.m.g;
  const GateModeArgs* const ex = &bb.m;
  constexpr bool LB = true;
  const float* const lbias = bb.logit_bias;
#include "moe_gate_body.inc"
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

// gate_modes_kernel: gate_kernel's forms (the same NW, U and rows per workgroup by T), and a 16-block
// form for 256 experts without a shared gate
template <int NB, int MR, int NW, int U, bool BF>
inline void gate_modes_launch_one(const GateModeArgs& m, bool sigmoid, hipStream_t st) {
  const dim3 blocks((unsigned)((m.g.T + 16 * MR - 1) / (16 * MR))), threads(64 * NW);
  if (sigmoid) hipLaunchKernelGGL((gate_modes_kernel<NB, MR, NW, U, kGateSigmoidEx, BF>), blocks, threads, 0, st, m);
  else hipLaunchKernelGGL((gate_modes_kernel<NB, MR, NW, U, kGateSoftmaxEx, BF>), blocks, threads, 0, st, m);
}
template <int NB, int MR, int NW, int U, bool BF>
inline void gate_modes_launch_one(const GateBiasArgs& b, bool sigmoid, hipStream_t st) {
  const dim3 blocks((unsigned)((b.m.g.T + 16 * MR - 1) / (16 * MR))), threads(64 * NW);
  if (sigmoid) hipLaunchKernelGGL((gate_bias_kernel<NB, MR, NW, U, kGateSigmoidEx, BF>), blocks, threads, 0, st, b);
  else hipLaunchKernelGGL((gate_bias_kernel<NB, MR, NW, U, kGateSoftmaxEx, BF>), blocks, threads, 0, st, b);
}
// (16 blocks would fit 8 waves - 64 KiB of partial sums, 241 VGPRs - and ran no faster than 4 at
// H = 7168: DESIGN.md §4 "Router: the other routing rules")
template <int NB, bool BF, class ARGS>
inline void gate_modes_launch_nb(const ARGS& m, bool sigmoid, hipStream_t st) {
  constexpr int NW = NB <= 12 ? MXMOE_GATE_NW : 4;
  constexpr int MAXMR = NB <= 4 ? 4 : NB <= 8 ? 2 : 1;
  const int mr = gate_rows_per_wg(gate_args_of(m).T, MAXMR);
  if constexpr (MAXMR >= 4) {
    if (mr == 4) return gate_modes_launch_one<NB, 4, NW, gate_group_steps(NB, 4), BF>(m, sigmoid, st);
  }
  if constexpr (MAXMR >= 2) {
    if (mr == 2) return gate_modes_launch_one<NB, 2, NW, gate_group_steps(NB, 2), BF>(m, sigmoid, st);
  }
  gate_modes_launch_one<NB, 1, NW, gate_group_steps(NB, 1), BF>(m, sigmoid, st);
}
// one launch; the caller has validated the arguments (T > 0). ARGS: GateModeArgs, or GateBiasArgs (gate_bias_kernel);
// BF: the bf16 builds
template <bool BF = false, class ARGS>
inline void gate_modes_launch(const ARGS& m, bool sigmoid, hipStream_t st) {
  const int nb = (gate_args_of(m).E + (gate_args_of(m).w_shared ? 1 : 0) + 15) / 16;
  if (nb <= 1) gate_modes_launch_nb<1, BF>(m, sigmoid, st);
  else if (nb <= 2) gate_modes_launch_nb<2, BF>(m, sigmoid, st);
  else if (nb <= 4) gate_modes_launch_nb<4, BF>(m, sigmoid, st);
  else if (nb <= 5) gate_modes_launch_nb<5, BF>(m, sigmoid, st);
  else if (nb <= 8) gate_modes_launch_nb<8, BF>(m, sigmoid, st);
  else if (nb <= 12) gate_modes_launch_nb<12, BF>(m, sigmoid, st);
  else if (nb <= 16) gate_modes_launch_nb<16, BF>(m, sigmoid, st);
  else gate_modes_launch_nb<kGateMaxBlocks, BF>(m, sigmoid, st);
}

}  // namespace gate
}  // namespace mxmoe
