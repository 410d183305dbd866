// moe_ops.hip — MoE-layer plumbing around the GroupGEMM (include/mxmoe_moe.h), gfx950.
//
// Reference (SeaCatComplexes/MxMoE, mxmoe/kernels/src/ref_bind.cu; read as text only):
//   gg_permute_inp: sort(topk_ids) / floor_divide(topk) / bincount ......... ref_bind.cu:47-64, 452-456
//   quant_inp_act -> quant_act_kernel (per-expert activation quantisation) .. :434-592
//   silu_mul_then_quant -> silu_mul_then_quant_kernel ....................... :595-757
//   gg_unpermute_out (empty stub) ........................................... :66
// The reference's device kernels (act_kernel.cuh) are absent from its tree; the quantiser here is
// its quant_weight (quantize.cuh:218-279) per token row / 128-element group + pack_wxax
// (quantize.cuh:425-475), i.e. exactly the operand format of the GroupGEMM.
//
// All four kernels are HBM-bound byte movers: one workgroup per row (token or slot), 16-B
// coalesced loads of 8 fp16 per lane, reductions in registers / lane shuffles, stores of the packed
// codes as one 4-B (int4) / 8-B (int8) / 16-B (fp16) word per lane — no LDS tiling, no MFMA.
// gpt-oss layers: the activation pass also comes with a bias row per expert and the clamped SwiGLU
// (mxmoe_moe_glu_quant: the GLU builds of act_quant_kernel), the combine with a bias row per expert
// (mxmoe_moe_combine_bias: combine_bias_kernel, the BIAS build of the combine's one loop), the router with a bias on
// its logits (mxmoe_moe_gate_ex2); no reference counterpart.
// The router in front of them (mxmoe_moe_gate: logits on the MFMA, top-k, softmax; mxmoe_moe_gate_ex:
// sigmoid scores, selection bias, group-limited top-k) is moe_gate.h; beyond 256 experts (mxmoe_moe_gate_wide),
// moe_gate_wide.h. The decode forward (mxmoe_moe_decode_gate_up, mxmoe_moe_decode_down: a layer call of up to 16 tokens
// as two weight-streaming launches with no planner; their _ex forms for gpt-oss layers: MXFP4 weights, gate_up biases,
// the clamped SwiGLU) is moe_decode.h.
// bf16 layers (mxmoe_moe_gate_dt, mxmoe_moe_gather_quant, mxmoe_moe_combine_dt): the element type of the router's
// operands, of the gather's source rows and of the combine's output is a template parameter of the kernels above;
// the fp16 instantiations are the kernels as they were. No reference counterpart (the reference is fp16 only).
// What builds share exists once: the two block-scaled tags' amax, exponent and scale store (mx_block_amax, mx_exponent,
// mx_store_scale), the two combine kernels' loop (combine_row), the choice of an activation build (launch_act_any) and
// the entry points' post-launch and element-type checks (launched, dtype_check).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <type_traits>

#include "../../include/mxmoe_gg.h"
#include "../../include/mxmoe_moe.h"
#include "gg_error.h"  // fail(): the library's error channel (mxmoe_gg_last_error)
#include "moe_gate.h"
#include "moe_gate_wide.h"
#define MXMOE_DYN_KERNEL  // gg_dyn.h: the GroupGEMM's device tile planner kernel is compiled here
#include "gg_dyn.h"

namespace mxmoe {
namespace detail {
void launch_dyn_plan(const DynArgs& a, hipStream_t stream) {
  const int want = (a.tile_slots + kDynSlotsPerBlock - 1) / kDynSlotsPerBlock;
  const int blocks = want < 1 ? 1 : want > kDynMaxBlocks ? kDynMaxBlocks : want;
  hipLaunchKernelGGL(dyn_plan_kernel, dim3(blocks), dim3(256), 0, stream, a);
}
}  // namespace detail

namespace {

// after a launch: the runtime's verdict on it, under the kernel's name
int launched(const char* kernel) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MXMOE_GG_ERR_HIP, "%s launch failed: %s", kernel, hipGetErrorString(e));
  return MXMOE_GG_OK;
}
// an element-type argument (what: its name in the entry point fn) must be one of the two MXMOE_DT_*
int dtype_check(const char* fn, const char* what, int dtype) {
  if (dtype != MXMOE_DT_FP16 && dtype != MXMOE_DT_BF16)
    return fail(MXMOE_GG_ERR_INVALID, "%s: %s must be MXMOE_DT_FP16 or MXMOE_DT_BF16 (got %d)", fn, what, dtype);
  return MXMOE_GG_OK;
}

constexpr int kThreads = 256;
constexpr int kRouteThreads = 1024;
constexpr int kChunk = kThreads * 8;     // fp16 elements one pass of the workgroup covers
constexpr int kMaxChunks = 8;            // rows up to 16384 elements
constexpr int kMaxWidth = kChunk * kMaxChunks;

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// exclusive block prefix of v (NT threads) and the block total
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* total, int* lds4) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int incl = wave_incl_scan(v);
  if (lane == 63) lds4[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    base += w < wave ? lds4[w] : 0;
    tot += lds4[w];
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// ---------------------------------------------------------------------------------------------
// route: workgroup e finds every id == e in flattened order (stable), its slot base = #ids < e.
// Each thread scans a contiguous run of the ids twice (count, then place); the runs' counts are
// prefix-summed across the workgroup so the placement keeps the flattened order.
__global__ __launch_bounds__(kRouteThreads) void route_kernel(const int32_t* __restrict__ ids, int n, int topk,
                                                              int32_t* __restrict__ sorted, int32_t* __restrict__ perm,
                                                              int32_t* __restrict__ inv, int32_t* __restrict__ counts) {
  __shared__ int lds[kRouteThreads / 64];
  const int e = blockIdx.x;
  // run of 4*q ids per thread (q int4 words, read as independent 16-B loads); ids past n read as -1
  const int q = (n + 4 * kRouteThreads - 1) / (4 * kRouteThreads);
  const int b = threadIdx.x * q * 4;
  auto id4 = [&](int w) -> int4 {
    const int i = b + 4 * w;
    if (i + 4 <= n && (n & 3) == 0) return *reinterpret_cast<const int4*>(ids + i);
    int4 v;
    v.x = i < n ? ids[i] : -1;
    v.y = i + 1 < n ? ids[i + 1] : -1;
    v.z = i + 2 < n ? ids[i + 2] : -1;
    v.w = i + 3 < n ? ids[i + 3] : -1;
    return v;
  };
  int less = 0, eq = 0;
#pragma unroll 8
  for (int w = 0; w < q; ++w) {
    const int4 v = id4(w);
    less += (v.x >= 0 && v.x < e) + (v.y >= 0 && v.y < e) + (v.z >= 0 && v.z < e) + (v.w >= 0 && v.w < e);
    eq += (v.x == e) + (v.y == e) + (v.z == e) + (v.w == e);
  }
  int eq_total, less_total;
  const int rank = block_excl_scan<kRouteThreads>(eq, &eq_total, lds);
  block_excl_scan<kRouteThreads>(less, &less_total, lds);
  if (threadIdx.x == 0) counts[e] = eq_total;
  if (eq == 0) return;
  int pos = less_total + rank;
  for (int w = 0; w < q && eq > 0; ++w) {
    const int4 v = id4(w);
    const int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (vv[j] == e) {
        const int i = b + 4 * w + j;
        sorted[pos] = e;
        perm[pos] = i / topk;
        inv[i] = pos;
        ++pos;
        --eq;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
struct ActArgs {
  const _Float16* src;         // quant: hidden [T][K]; silu: routed gate_up [T*topk][2N]
  const _Float16* src_shared;  // silu: shared gate_up [T][2Ns] (quant: = src)
  int64_t ntk;                 // T * topk routed slots
  int64_t nslots;              // end of the launch's slot range (ntk, + T shared slots)
  int64_t s0;                  // first slot of the launch
  int K;                       // quant: row width of hidden
  int N, Ns;                   // silu: routed / shared intermediate width
  const int32_t* sorted;
  const int32_t* perm;
  const mxmoe_moe_seg* segs;
  int nseg;
  uint8_t* out;
  _Float16* scales;
  int64_t blk_shared;          // parts > 1: first workgroup of the shared rows (one row per workgroup)
  int parts;                   // 1, or 4: a shared row is split over the 4 waves of its workgroup
};
// mxmoe_moe_glu_quant (GLU builds of act_quant_kernel): the biases of the gate_up output and the gated activation
struct GluArgs : ActArgs {
  const _Float16* bias_routed;  // [nexp][2N] ([gate | up] columns) or NULL
  const _Float16* bias_shared;  // [2Ns] or NULL
  int nexp;                     // routed experts (rows of bias_routed)
  float c, limit;               // SWIGLU_CLAMP: -(alpha log2 e), the clamp
};
enum { kGluNone = 0, kGluSilu = 1, kGluSwigluClamp = 2 };
template <int GLU> struct ActArgsOf { typedef GluArgs type; };
template <> struct ActArgsOf<kGluNone> { typedef ActArgs type; };
// The gated activation of mxmoe_moe_glu (include/mxmoe_moe.h) on the f32 gate and up values, biases added: the f32
// value `a` that its caller rounds to fp16. One definition for the GLU builds of act_quant_kernel and the decode
// forward's _ex gate_up epilogue (moe_decode.h).
template <int GLU>
__device__ __forceinline__ float glu_value(float g, float v, float limit, float c) {
  static_assert(GLU == kGluSilu || GLU == kGluSwigluClamp, "a gated activation");
  if constexpr (GLU == kGluSilu) {  // the SiLU pass's own expression
    const float sg = g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f));
    return sg * v;
  } else {  // (u + 1) * g * sigmoid(alpha g) on g clamped from above, u from both sides
    const float gc = fminf(g, limit);
    const float uc = fminf(fmaxf(v, -limit), limit);
    const float sg = gc * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gc * c));
    return sg * (uc + 1.0f);
  }
}

// quant_weight arithmetic (quantize.cuh:218-279): scale = fp16(amax / qmax), 0 -> 1;
// q = rint_even(clamp(fp16(x / scale), -qmax, qmax))
__device__ __forceinline__ _Float16 rtn_scale(float amax, float qmax) {
  _Float16 s = (_Float16)(amax / qmax);
  return s == (_Float16)0 ? (_Float16)1 : s;
}
// fp16(f32(x) / f32(s)) without the IEEE divide sequence (~10 VALU, which made these kernels
// VALU-bound): q = x * r, one Newton step q' = q + (x - q s) r with r = v_rcp_f32(s) (<= 1 ulp).
// q' is within 0.5 ulp (+ 2^-46 relative) of x / s. For fp16 x and s (11-bit significands) x / s is
// at least 1 / ((2^11 - 1)(2^12 - 1)) > 2^-23 (relative) away from every fp16 rounding midpoint
// (a 12-bit odd significand M with |x - M s| > 0 is at least one unit of the 23-bit product M s),
// so q' and the correctly rounded quotient lie on the same side of every midpoint and round to the
// same fp16 — bit-exact with the IEEE division the oracle uses.
__device__ __forceinline__ float div_f16_operands(float x, float s, float r) {
  const float q = x * r;
  return fmaf(fmaf(-q, s, x), r, q);
}
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

// Codes of elements 2p, 2p+1 of x: d = fp16(x / s) clamped to +-qmax in fp16 (exact), then
// d + 1536 in fp16: for |d| <= 127 the sum lies in [1024, 2048) where the fp16 spacing is 1, so
// the add rounds d to an integer with ties to even (1536 is even: rint's tie rule), and the low
// byte of the sum's bits (mantissa 512 + rint(d)) is rint(d)'s two's-complement byte. Returns the
// pair's bits: code(2p) in byte 0, code(2p+1) in byte 2.
__device__ __forceinline__ uint32_t pair_codes(const h8_t& x, int p, float s, float r, h2_t lim) {
  h2_t d = {(_Float16)div_f16_operands((float)x[2 * p], s, r), (_Float16)div_f16_operands((float)x[2 * p + 1], s, r)};
  d = __builtin_elementwise_min(__builtin_elementwise_max(d, -lim), lim);
  d = d + h2_t{(_Float16)1536, (_Float16)1536};
  return __builtin_bit_cast(uint32_t, d);
}
// pack_wxax (quantize.cuh:425-475) stores element j+x of a 16-bit word at bits (PACK-1-x)*bits:
// int8 word j = q[2j] << 8 | q[2j+1] (little-endian bytes q[2j+1], q[2j]); int4 word j =
// q[4j] << 12 | q[4j+1] << 8 | q[4j+2] << 4 | q[4j+3].
// order4: 4 codes from two pair words as bytes [q1, q0, q3, q2] (v_perm_b32: selectors 0-3 take
// the second operand's bytes, 4-7 the first's)
__device__ __forceinline__ uint32_t order4(uint32_t p01, uint32_t p23) { return __builtin_amdgcn_perm(p23, p01, 0x04060002u); }
// int8: 8 codes -> 8 packed bytes
__device__ __forceinline__ uint2 codes_i8(const h8_t& x, float s, float r, h2_t lim) {
  return uint2{order4(pair_codes(x, 0, s, r, lim), pair_codes(x, 1, s, r, lim)),
               order4(pair_codes(x, 2, s, r, lim), pair_codes(x, 3, s, r, lim))};
}
// int4: from [q1, q0, q3, q2] nibbles, t = a | a >> 4 puts (q0 << 4 | q1) in byte 0 and
// (q2 << 4 | q3) in byte 2; the word is bytes [t.2, t.0, u.2, u.0] (pack_i4x8 order)
__device__ __forceinline__ uint32_t codes_i4(const h8_t& x, float s, float r, h2_t lim) {
  const uint32_t a = order4(pair_codes(x, 0, s, r, lim), pair_codes(x, 1, s, r, lim)) & 0x0F0F0F0Fu;
  const uint32_t b = order4(pair_codes(x, 2, s, r, lim), pair_codes(x, 3, s, r, lim)) & 0x0F0F0F0Fu;
  return __builtin_amdgcn_perm(b | (b >> 4), a | (a >> 4), 0x04060002u);
}
// max |x| over 8 fp16 (exact in fp16: v_pk_max_f16 on sign-cleared pairs)
__device__ __forceinline__ float amax8(const h8_t& x) {
  const uint4 w = __builtin_bit_cast(uint4, x);
  const uint32_t m = 0x7FFF7FFFu;
  const h2_t a = __builtin_elementwise_max(__builtin_bit_cast(h2_t, w.x & m), __builtin_bit_cast(h2_t, w.y & m));
  const h2_t b = __builtin_elementwise_max(__builtin_bit_cast(h2_t, w.z & m), __builtin_bit_cast(h2_t, w.w & m));
  const h2_t c = __builtin_elementwise_max(a, b);
  return fmaxf((float)c[0], (float)c[1]);
}

// 8 bf16 (one 16-B load) -> 8 fp16: each element widened to f32 (its bits << 16, exact) and rounded once to fp16 by
// v_cvt_f16_f32 — to nearest even, overflow to +-Inf, the fp16-subnormal range rounded and not flushed (the fp16
// denormal mode of these kernels is IEEE): the value hidden.to(torch.float16) holds.
__device__ __forceinline__ h8_t bf16x8_to_f16(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  h8_t r;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    r[2 * p] = (_Float16)__builtin_bit_cast(float, w[p] << 16);
    r[2 * p + 1] = (_Float16)__builtin_bit_cast(float, w[p] & 0xFFFF0000u);
  }
  return r;
}

// The block-scaled tags (OCP MXFP4 / MXFP8, include/mxmoe_gg.h): what the two share. A 32-element block is 4 adjacent
// lanes of one chunk.
// mx_block_amax: the block amax on the sign-cleared fp16 bit patterns as integers (their order is the values', with
// Inf / NaN on top: a result >= 0x7C00 means an Inf or a NaN in the block)
__device__ __forceinline__ uint32_t mx_block_amax(const h8_t& x) {
  const uint4 w = __builtin_bit_cast(uint4, x);
  const uint32_t cm = 0x7FFF7FFFu;
  uint32_t m2 = max(max((w.x & cm) & 0xFFFFu, (w.x & cm) >> 16), max((w.y & cm) & 0xFFFFu, (w.y & cm) >> 16));
  m2 = max(m2, max(max((w.z & cm) & 0xFFFFu, (w.z & cm) >> 16), max((w.w & cm) & 0xFFFFu, (w.w & cm) >> 16)));
  m2 = max(m2, (uint32_t)__shfl_xor((int)m2, 1, 64));
  m2 = max(m2, (uint32_t)__shfl_xor((int)m2, 2, 64));
  return m2;
}
// mx_exponent: e = floor(log2 amax) - EOFF from the exponent field of f32(amax) (the conversion normalises fp16
// subnormals; EOFF: the exponent of the element format's largest binade, 2 for e2m1 and 8 for e4m3), -127 for a
// zero block, and inv = 2^-e (e in [-127, 15 - EOFF]), by which the elements are scaled exactly
template <int EOFF>
__device__ __forceinline__ int mx_exponent(uint32_t m2, float& inv) {
  const float am = (float)__builtin_bit_cast(_Float16, (uint16_t)m2);
  const int e = m2 == 0 ? -127 : (int)((__builtin_bit_cast(uint32_t, am) >> 23) & 0xFF) - 127 - EOFF;
  inv = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);
  return e;
}
// mx_store_scale (the block's first lane): the e8m0 byte of block blk of a row of nblk blocks whose scale bytes start
// at so, at its permuted place in the row's 16-byte group (device layout); bad: a NaN scale
__device__ __forceinline__ void mx_store_scale(uint8_t* so, int blk, int nblk, bool bad, int e) {
  const int c16 = blk & 15;
  so[(blk & ~15) + 4 * (c16 & 3) + (c16 >> 2)] = bad ? (uint8_t)255 : (uint8_t)(e + 127);
  if (blk == nblk - 1) {  // the row's last block: the pads of its 16-byte group are 2^0
#pragma clang loop unroll(disable) vectorize(disable)
    for (int pc = c16 + 1; pc < 16; ++pc) so[(blk & ~15) + 4 * (pc & 3) + (pc >> 2)] = 127;
  }
}

// The per-token e4m3 tag (MXMOE_ACT_E4M3, include/mxmoe_moe.h).
// amax8_bits: max |x| over 8 fp16 as the largest sign-cleared bit pattern (v_pk_max_u16; the patterns' order is the
// values', with Inf / NaN on top: a result >= 0x7C00 means an Inf or a NaN among them)
typedef uint16_t us2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t amax8_bits(const h8_t& x) {
  const uint4 w = __builtin_bit_cast(uint4, x);
  const uint32_t m = 0x7FFF7FFFu;
  const us2_t a = __builtin_elementwise_max(__builtin_bit_cast(us2_t, w.x & m), __builtin_bit_cast(us2_t, w.y & m));
  const us2_t b = __builtin_elementwise_max(__builtin_bit_cast(us2_t, w.z & m), __builtin_bit_cast(us2_t, w.w & m));
  const us2_t c = __builtin_elementwise_max(a, b);
  return max((uint32_t)c[0], (uint32_t)c[1]);
}
// codes_e4m3: 8 elements -> 8 code bytes in pack_wxax's 8-bit order (bytes [q1, q0, q3, q2, ...]).
// The tag's contract is e4m3_rn_sat of the correctly rounded f32 quotient x / s. The IEEE divide sequence costs ~10
// VALU per element; here r = the correctly rounded 1 / s (once per row), q = x * r and one residual step
// q' = q + (x - q s) r, which is within 0.5 ulp (+ 2^-46 relative) of x / s in f32. Both q' and the IEEE quotient
// round to the same code: a point where the e4m3 rounding (or the clamp at 448) changes is a value of at most 5
// significant bits, x and s have 11, so x / s either IS such a point — then it is an f32 and both sequences return it
// exactly — or is more than 2^-16 (relative) away from it (x - P s is a non-zero multiple of the finer of x's and
// P s's grids, P s having at most 16 bits): over a hundred f32 ulps. tests/test_e4m3_layer.py checks this over every
// pair of fp16 significands. x = -0 leaves q' = +0 (the residual is +0), so the sign is copied from x (s > 0).
// The clamp at +-448 (v_med3_f32) precedes the hardware convert, which rounds once to OCP e4m3, to nearest even.
__device__ __forceinline__ uint2 codes_e4m3(const h8_t& x, float s, float r) {
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xf = (float)x[j];
    const float q = xf * r;
    y[j] = __builtin_amdgcn_fmed3f(__builtin_copysignf(fmaf(fmaf(-q, s, xf), r, q), xf), -448.0f, 448.0f);
  }
  int q0 = 0, q1 = 0;
  q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[1], y[0], q0, false);
  q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[3], y[2], q0, true);
  q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[5], y[4], q1, false);
  q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[7], y[6], q1, true);
  return uint2{(uint32_t)q0, (uint32_t)q1};
}

// One WAVE per slot row (4 rows per 256-thread workgroup): lane l holds elements c*512 + 8l .. +7
// of chunk c in registers (MAXC chunks: rows up to MAXC*512 elements, MAXC = the launch's widest
// row in 512-element chunks), so every lane has MAXC independent 16-B loads in flight, the
// per-token amax is a wave butterfly and a 128-element group is 16 adjacent lanes — no LDS, no
// barrier. Loads and the SiLU are straight-line over all MAXC chunks (lanes past the row read the
// row's first 16 B and zero them by a select): per-chunk branches kept the scheduler from
// interleaving the chunks' dependency chains (v_exp / v_rcp latency, packed-math wait states). parts == 4: the workgroups from blk_shared on take one
// wide shared row each, wave w its w-th run of 128-aligned columns (the per-token amax then crosses
// the 4 waves through LDS), so routed and shared rows share one launch and one register budget.
// MODE 0: quant_act (routed slot s gathers hidden[perm[s]], width K); 1: silu_mul_quant (slot rows
// [gate | up] of the gate_up output); 2: quant_slots (slot rows already activated: the gate_up
// GroupGEMM's fused SiLU epilogue, routed [T*topk][N], shared [T][Ns]); 3: silu_mul_quant on a
// gate_up output whose gate / up columns alternate in 16-column blocks (the interleaved weights of
// the fused epilogue, run through the plain epilogue: small-batch calls on wo3)
// MX: the build that also carries the MXMOE_ACT_MXFP4 and MXMOE_ACT_MXFP8 tags (launched only for calls whose segments hold
// one, mxmoe_moe_act_quant: the other tags' builds stay as they are without it)
// GLU (MODE 1 only; mxmoe_moe_glu_quant): kGluSilu / kGluSwigluClamp builds take GluArgs, add the expert's bias
// row to the gate and up values as they are read (one f32 add each; a NULL bias: no add) and apply the named
// gated activation. kGluNone: none of that code exists and the builds are the ones above.
// SRCBF (MODE 0 only; mxmoe_moe_gather_quant): hidden holds bf16; every 16-B load is converted to fp16 as it arrives
// (bf16x8_to_f16) and nothing after the loads differs. SRCBF = false: the builds above, as they were.
// kActF8 (a flag on the MODE argument, MODEF = MODE | kActF8): the builds that also carry the MXMOE_ACT_E4M3 tag,
// launched only for calls whose tag_mask has bit 8. They carry the block-scaled tags too (MX = true), so one family
// serves an E4M3 layer and a layer that mixes E4M3 with MX experts (a second family without the MX code would be 63
// more kernels to compile). The flag rides on MODE so that the template's parameter list, and with it the name and
// the code of every build without the flag, stay what they were before the tag existed: in those none of its code
// exists.
constexpr int kActF8 = 8;
template <int MODEF, int MAXC, bool MX = false, int GLU = kGluNone, bool SRCBF = false>
__global__ __launch_bounds__(kThreads) void act_quant_kernel(typename ActArgsOf<GLU>::type a) {
  constexpr int MODE = MODEF & ~kActF8;
  constexpr bool F8 = (MODEF & kActF8) != 0;
  static_assert(!F8 || MX, "the E4M3 builds carry the MX tags too");
  constexpr bool SILU = MODE == 1 || MODE == 3;
  static_assert(GLU == kGluNone || MODE == 1, "the GLU builds read [gate | up] columns");
  static_assert(!SRCBF || MODE == 0, "only the gather reads bf16 rows: the gate_up output stays fp16");
  __shared__ float wave_amax[kThreads / 64];
  const int lane = threadIdx.x & 63;
  const bool split_row = a.parts > 1 && (int64_t)blockIdx.x >= a.blk_shared;  // workgroup-uniform
  const int part = split_row ? (int)(threadIdx.x >> 6) : 0;
  const int64_t s = split_row ? a.ntk + ((int64_t)blockIdx.x - a.blk_shared)
                              : a.s0 + (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (s >= (a.parts > 1 && !split_row ? a.ntk : a.nslots)) return;  // split_row: uniform
  int e;
  const _Float16* row_src;
  if (s < a.ntk) {
    e = a.sorted[s];
    row_src = (MODE == 1 || MODE == 3) ? a.src + s * 2 * (int64_t)a.N
            : MODE == 2 ? a.src + s * (int64_t)a.N
                        : a.src + (int64_t)a.perm[s] * a.K;
  } else {
    e = a.nseg - 1;
    const int64_t t = s - a.ntk;
    row_src = (MODE == 1 || MODE == 3) ? a.src_shared + t * 2 * (int64_t)a.Ns
            : MODE == 2 ? a.src_shared + t * (int64_t)a.Ns
                        : a.src + t * a.K;
  }
  if (e < 0 || e >= a.nseg) return;  // invalid id: the slot was never routed (route ignores it)
  const mxmoe_moe_seg sg = a.segs[e];
  const int64_t row = s - sg.first_slot;
  if (row < 0 || row >= sg.rows) return;  // slot outside its segment (inconsistent table): never write
  const int upoff = SILU ? (s < a.ntk ? a.N : a.Ns) : 0;  // column of the "up" half
  // this wave's columns [col0, col0 + width) of the row (split rows: 128-aligned quarter runs)
  const int qw = split_row ? ((sg.width / 4 + 127) & ~127) : sg.width;
  const int col0 = part * qw;
  const int width = split_row ? max(0, min(qw, sg.width - col0)) : sg.width;
  // (a wave whose quarter of a split row is empty keeps a valid address: the row's start)
  const _Float16* const base = width > 0 ? row_src + (MODE == 3 ? 2 * col0 : col0) : row_src;

  // every load of the row first (all in flight together), then the arithmetic
  h8_t x[MAXC];
  h8_t u[SILU ? MAXC : 1];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    const int idx = c * 512 + lane * 8;
    const bool in = idx < width;
    const int li = in ? idx : 0;
    // (MODE 3: element e of the row sits at 2 (e & ~15) + (e & 15), its up value 16 further)
    const int gi = MODE == 3 ? 2 * (li & ~15) + (li & 15) : li;
    const uint4 xv = *reinterpret_cast<const uint4*>(base + gi);
    const uint4 z = {0, 0, 0, 0};
    if constexpr (SRCBF) x[c] = bf16x8_to_f16(in ? xv : z);
    else x[c] = __builtin_bit_cast(h8_t, in ? xv : z);
    if constexpr (SILU) {
      const uint4 uv = *reinterpret_cast<const uint4*>(base + (MODE == 3 ? gi + 16 : upoff + li));
      u[c] = __builtin_bit_cast(h8_t, in ? uv : z);
    }
  }
  if constexpr (GLU != kGluNone) {
    // the bias row of this slot's expert ([gate | up], the input row's layout; split rows: from col0), loaded
    // like the row itself; a routed id that is no routed expert's (inconsistent table) gets no bias
    const _Float16* brow = s >= a.ntk ? a.bias_shared
                           : (a.bias_routed && e < a.nexp) ? a.bias_routed + (int64_t)e * 2 * a.N : nullptr;
    const bool has_b = brow != nullptr;  // wave-uniform
    const _Float16* const bbase = has_b ? (width > 0 ? brow + col0 : brow) : row_src;  // (always a valid address)
    h8_t bg[MAXC], bu[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int idx = c * 512 + lane * 8;
      const bool in = has_b && idx < width;
      const int li = in ? idx : 0;
      const uint4 gv = *reinterpret_cast<const uint4*>(bbase + li);
      const uint4 uv = *reinterpret_cast<const uint4*>(bbase + (has_b ? upoff : 0) + li);
      const uint4 z = {0, 0, 0, 0};
      bg[c] = __builtin_bit_cast(h8_t, in ? gv : z);
      bu[c] = __builtin_bit_cast(h8_t, in ? uv : z);
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {  // (zeros past the row: both activations give 0 * ... = 0)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float g = (float)x[c][j], v = (float)u[c][j];
        if (has_b) {
          g = g + (float)bg[c][j];
          v = v + (float)bu[c][j];
        }
        x[c][j] = (_Float16)glu_value<GLU>(g, v, a.limit, a.c);
      }
    }
  } else if constexpr (SILU) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {  // (zeros past the row: silu(0) * 0 = 0)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // silu(g) = g / (1 + e^-g) with the hardware exp2 / reciprocal (v_exp_f32, v_rcp_f32: the
        // reference kernel is absent, so this is our definition; oracle/moe_ref.py allows 1 ulp)
        const float g = (float)x[c][j];
        const float sg = g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f));
        x[c][j] = (_Float16)(sg * (float)u[c][j]);
      }
    }
  }

  if (sg.qtag == MXMOE_ACT_FP16) {
    _Float16* o = reinterpret_cast<_Float16*>(a.out + sg.out_off) + row * sg.width + col0;  // (width 0: no store)
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      const int idx = c * 512 + lane * 8;
      if (idx < width) *reinterpret_cast<h8_t*>(o + idx) = x[c];
    }
    return;
  }
  if constexpr (MX) if (sg.qtag == MXMOE_ACT_MXFP4) {
    // OCP MXFP4 (include/mxmoe_gg.h): block amax, e = floor(log2 amax) - 2 and scale bytes by the mx_* helpers
    // above, elements scaled by 2^-e exactly and rounded to the e2m1 grid with v_rndne (an even
    // multiple of the grid step is an even code in each of the three segments).
    const int srow = ((sg.width / 32 + 15) >> 4) << 4;  // scale bytes per row (device layout)
    uint8_t* const o4 = a.out + sg.out_off + (row * (int64_t)sg.width + col0) / 2;
    uint8_t* const so = reinterpret_cast<uint8_t*>(a.scales + sg.scale_off) + row * (int64_t)srow;
    const int nblk = sg.width / 32;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c * 512 >= width) break;  // uniform
      const int idx = c * 512 + lane * 8;
      const uint32_t m2 = mx_block_amax(x[c]);
      if (idx >= width) continue;
      const bool bad = m2 >= 0x7C00u;  // an Inf or a NaN in the block: NaN scale, zero codes
      float inv;
      const int e = mx_exponent<2>(m2, inv);
      uint32_t q = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float y = (float)x[c][j] * inv;  // exact
        const float ay = fminf(fabsf(y), 6.0f);
        const float r = ay < 2.0f ? __builtin_rintf(ay * 2.0f)
                      : ay < 4.0f ? 2.0f + __builtin_rintf(ay) : 4.0f + __builtin_rintf(ay * 0.5f);
        const uint32_t nib = (uint32_t)r | ((__builtin_bit_cast(uint32_t, y) >> 28) & 8u);
        q |= nib << (4 * j);
      }
      *reinterpret_cast<uint32_t*>(o4 + idx / 2) = bad ? 0u : q;
      if ((lane & 3) == 0) mx_store_scale(so, (col0 + idx) >> 5, nblk, bad, e);
    }
    return;
  }
  if constexpr (MX) if (sg.qtag == MXMOE_ACT_MXFP8) {
    // OCP MXFP8, e4m3 elements (include/mxmoe_gg.h, w4a8_g32_sym_MXFP8): blocks, amax and scale bytes
    // as the MXFP4 tag's with e = floor(log2 amax) - 8 (e4m3's largest binade); elements scaled by
    // 2^-e exactly, clamped to +-448 (v_med3_f32 keeps the sign of -0) and rounded ONCE to e4m3, to
    // nearest even, by the hardware convert (OCP e4m3 on gfx950). One code byte per element.
    const int srow = ((sg.width / 32 + 15) >> 4) << 4;  // scale bytes per row (device layout)
    uint8_t* const o8 = a.out + sg.out_off + row * (int64_t)sg.width + col0;
    uint8_t* const so = reinterpret_cast<uint8_t*>(a.scales + sg.scale_off) + row * (int64_t)srow;
    const int nblk = sg.width / 32;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c * 512 >= width) break;  // uniform
      const int idx = c * 512 + lane * 8;
      const uint32_t m2 = mx_block_amax(x[c]);
      if (idx >= width) continue;
      const bool bad = m2 >= 0x7C00u;  // an Inf or a NaN in the block: NaN scale, zero codes
      float inv;
      const int e = mx_exponent<8>(m2, inv);
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = __builtin_amdgcn_fmed3f((float)x[c][j] * inv, -448.0f, 448.0f);  // product exact
      int q0 = 0, q1 = 0;
      q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], q0, false);
      q0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], q0, true);
      q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], q1, false);
      q1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], q1, true);
      *reinterpret_cast<uint2*>(o8 + idx) = bad ? uint2{0u, 0u} : uint2{(uint32_t)q0, (uint32_t)q1};
      if ((lane & 3) == 0) mx_store_scale(so, (col0 + idx) >> 5, nblk, bad, e);
    }
    return;
  }
  if constexpr (F8) if (sg.qtag == MXMOE_ACT_E4M3) {
    // per-token e4m3 (include/mxmoe_moe.h): the row amax as a bit pattern (chunks past the row are zeros), across the
    // wave by a butterfly and, for a split row, across its 4 waves through LDS as the INT8 tag's
    uint32_t mi = 0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) mi = max(mi, amax8_bits(x[c]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mi = max(mi, (uint32_t)__shfl_xor((int)mi, d, 64));
    if (split_row) {  // every wave of the workgroup reaches here (its row's checks are uniform)
      if (lane == 0) wave_amax[part] = __builtin_bit_cast(float, mi);
      __syncthreads();
      mi = max(max(__builtin_bit_cast(uint32_t, wave_amax[0]), __builtin_bit_cast(uint32_t, wave_amax[1])),
               max(__builtin_bit_cast(uint32_t, wave_amax[2]), __builtin_bit_cast(uint32_t, wave_amax[3])));
    }
    const bool bad = mi >= 0x7C00u;  // an Inf or a NaN in the row: NaN scale, zero codes
    // s = fp16_rn(amax / 448) (the f32 quotient correctly rounded), at least 2^-14, 1 for a zero row
    _Float16 sc = (_Float16)((float)__builtin_bit_cast(_Float16, (uint16_t)mi) / 448.0f);
    if (__builtin_bit_cast(uint16_t, sc) < 0x0400u) sc = __builtin_bit_cast(_Float16, (uint16_t)0x0400u);
    if (mi == 0) sc = (_Float16)1;
    if (bad) sc = __builtin_bit_cast(_Float16, (uint16_t)0x7E00u);
    if (lane == 0 && part == 0) a.scales[sg.scale_off + row] = sc;
    const float s = (float)sc, r = 1.0f / s;  // (the IEEE division: once per row)
    uint8_t* const o8 = a.out + sg.out_off + row * (int64_t)sg.width + col0;
    uint2 q[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) q[c] = codes_e4m3(x[c], s, r);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c * 512 + lane * 8 < width) *reinterpret_cast<uint2*>(o8 + c * 512 + lane * 8) = bad ? uint2{0u, 0u} : q[c];
    return;
  }
  const int bits = sg.qtag == MXMOE_ACT_INT8 ? 8 : 4;
  const float qmax = bits == 8 ? 127.0f : 7.0f;
  const h2_t lim = {(_Float16)qmax, (_Float16)qmax};
  uint8_t* o = a.out + sg.out_off + (row * (int64_t)sg.width + col0) * bits / 8;
  if (sg.qtag == MXMOE_ACT_INT4_G128) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c * 512 >= width) break;  // uniform
      const int idx = c * 512 + lane * 8;
      float m = amax8(x[c]);
#pragma unroll
      for (int d = 8; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
      if (idx < width) {
        const _Float16 sc = rtn_scale(m, qmax);
        const float rs = __builtin_amdgcn_rcpf((float)sc);
        *reinterpret_cast<uint32_t*>(o + idx / 2) = codes_i4(x[c], (float)sc, rs, lim);
        if ((lane & 15) == 0) a.scales[sg.scale_off + (int64_t)((col0 + idx) / 128) * sg.rows + row] = sc;
      }
    }
    return;
  }
  float m = 0.0f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) m = fmaxf(m, amax8(x[c]));  // chunks past the row are zeros
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  if (split_row) {  // every wave of the workgroup reaches here (its row's checks are uniform)
    if (lane == 0) wave_amax[part] = m;
    __syncthreads();
    m = fmaxf(fmaxf(wave_amax[0], wave_amax[1]), fmaxf(wave_amax[2], wave_amax[3]));
  }
  const _Float16 sc = rtn_scale(m, qmax);
  const float rs = __builtin_amdgcn_rcpf((float)sc);
  if (lane == 0 && part == 0) a.scales[sg.scale_off + row] = sc;
  // every chunk's codes first (straight-line: the chunks' packed-math chains interleave), then the
  // predicated stores
  if (bits == 8) {
    uint2 q[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) q[c] = codes_i8(x[c], (float)sc, rs, lim);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c * 512 + lane * 8 < width) *reinterpret_cast<uint2*>(o + c * 512 + lane * 8) = q[c];
  } else {
    uint32_t q[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) q[c] = codes_i4(x[c], (float)sc, rs, lim);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c * 512 + lane * 8 < width) *reinterpret_cast<uint32_t*>(o + (c * 512 + lane * 8) / 2) = q[c];
  }
}

// ---------------------------------------------------------------------------------------------
// combine: one workgroup per token, 8 fp16 columns per lane and pass. OT: the output element, _Float16 (the kernel
// as it was) or __bf16 (mxmoe_moe_combine_dt: the f32 accumulator rounded to bf16 to nearest even, v_cvt_pk_bf16_f32).
// BIAS: the build with a bias row per expert on the down output (mxmoe_moe_combine_bias): the term of choice k is
// f32(y) + f32(bias[e]) (one add), e = sorted[slot] — an id outside [0, E) (a stale slot) adds nothing — and the
// shared term f32(shared) + f32(shared_bias); either pointer may be NULL. BIAS = false: none of that code exists and
// sorted, bias, shared_bias and E are not read.
// One body under two kernels, each with the arguments its build reads: one argument list for both moved the
// kernel-argument loads of whichever build did not keep its own layout (profiles/r16/plumbing_dedupe/).
template <class OT, bool BIAS>
__device__ __forceinline__ void combine_row(const _Float16* __restrict__ y, const int32_t* __restrict__ inv,
                                            const int32_t* __restrict__ sorted, const float* __restrict__ w,
                                            const _Float16* __restrict__ bias, const _Float16* __restrict__ shared,
                                            const float* __restrict__ shared_w, const _Float16* __restrict__ shared_bias,
                                            int topk, int E, int H, OT* __restrict__ out) {
  typedef OT o8_t __attribute__((ext_vector_type(8)));
  const int64_t t = blockIdx.x;
  for (int idx = threadIdx.x * 8; idx < H; idx += kChunk) {
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < topk; ++k) {
      const int64_t slot = inv[t * topk + k];
      const float wk = w[t * topk + k];
      const h8_t v = *reinterpret_cast<const h8_t*>(y + slot * H + idx);
      int e = -1;  // the expert whose bias row the term takes
      if constexpr (BIAS) e = bias ? sorted[slot] : -1;
      if (e >= 0 && e < E) {  // workgroup-uniform
        const h8_t b = *reinterpret_cast<const h8_t*>(bias + (int64_t)e * H + idx);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(wk, (float)v[j] + (float)b[j], acc[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(wk, (float)v[j], acc[j]);
      }
    }
    if (shared) {
      const float ws = shared_w ? shared_w[t] : 1.0f;
      const h8_t v = *reinterpret_cast<const h8_t*>(shared + t * H + idx);
      bool sb = false;
      if constexpr (BIAS) sb = shared_bias != nullptr;
      if (sb) {
        const h8_t b = *reinterpret_cast<const h8_t*>(shared_bias + idx);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(ws, (float)v[j] + (float)b[j], acc[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(ws, (float)v[j], acc[j]);
      }
    }
    o8_t r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (OT)acc[j];
    *reinterpret_cast<o8_t*>(out + t * H + idx) = r;
  }
}
template <class OT>
__global__ __launch_bounds__(kThreads) void combine_kernel(const _Float16* __restrict__ y, const int32_t* __restrict__ inv,
                                                           const float* __restrict__ w, const _Float16* __restrict__ shared,
                                                           const float* __restrict__ shared_w, int topk, int H,
                                                           OT* __restrict__ out) {
  combine_row<OT, false>(y, inv, nullptr, w, nullptr, shared, shared_w, nullptr, topk, 0, H, out);
}
template <class OT>
__global__ __launch_bounds__(kThreads) void combine_bias_kernel(const _Float16* __restrict__ y, const int32_t* __restrict__ inv,
                                                                const int32_t* __restrict__ sorted, const float* __restrict__ w,
                                                                const _Float16* __restrict__ bias,
                                                                const _Float16* __restrict__ shared,
                                                                const float* __restrict__ shared_w,
                                                                const _Float16* __restrict__ shared_bias, int topk, int E, int H,
                                                                OT* __restrict__ out) {
  combine_row<OT, true>(y, inv, sorted, w, bias, shared, shared_w, shared_bias, topk, E, H, out);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------
// segments: the segment table (and the next GroupGEMM's row table) from the routing counts. One function
// for the kernel and the host diagnostic. Offsets as mxmoe_amd/moe.py's _make_segments lays them out: 16-B
// aligned out_off, even scale_off for the block-scaled tags, the shared segment last with rows = T.
// A count is clamped so the routed rows never exceed T * topk (route counts every id at most once, so a
// clamp means the counts are not route's); a clamp or a sum below T * topk (ids outside [0, E)) sets bit 0
// of the returned status.
__host__ __device__ inline int act_bits(int tag) {
  return tag == MXMOE_ACT_INT8 || tag == MXMOE_ACT_MXFP8 || tag == MXMOE_ACT_E4M3 ? 8
         : tag == MXMOE_ACT_INT4 || tag == MXMOE_ACT_INT4_G128 || tag == MXMOE_ACT_MXFP4 ? 4 : 16;
}
__host__ __device__ inline int32_t fill_segments(const int32_t* counts, int E, int64_t T, int topk, bool with_shared,
                                                 const mxmoe_moe_seg_table& tb) {
  const int64_t ntk = T * topk;
  int64_t off = 0, soff = 0, first = 0;
  int32_t status = 0;
  mxmoe_gg_dyn_row* dyn = static_cast<mxmoe_gg_dyn_row*>(tb.dyn);
  for (int e = 0; e < E + (with_shared ? 1 : 0); ++e) {
    const bool shared = e == E;
    int64_t r = shared ? T : counts[e];
    if (!shared && (r < 0 || r > ntk - first)) {
      status |= MXMOE_MOE_SEG_COUNT_MISMATCH;
      r = r < 0 ? 0 : ntk - first;
    }
    const int tag = tb.qtags[e], w = shared ? tb.width_shared : tb.width;
    const bool mx = tag == MXMOE_ACT_MXFP4 || tag == MXMOE_ACT_MXFP8;
    if (mx) soff += soff & 1;  // its scale bytes are read as dwords: a 4-byte aligned block
    const int64_t f = shared ? ntk : first;
    tb.segs[e] = mxmoe_moe_seg{tag, (int32_t)f, (int32_t)r, w, off, soff};
    if (dyn) dyn[e] = mxmoe_gg_dyn_row{(int32_t)r, 0, off, soff * 2, shared ? 0 : f * tb.ldc * 2};
    off += (r * w * act_bits(tag) / 8 + 15) / 16 * 16;
    if (mx) soff += r * (16 * ((w / 32 + 15) / 16)) / 2;  // (fp16 elements: two e8m0 bytes each)
    else soff += tag == MXMOE_ACT_FP16 ? 0 : r * (tag == MXMOE_ACT_INT4_G128 ? w / 128 : 1);
    if (!shared) first += r;
  }
  if (first != ntk) status |= MXMOE_MOE_SEG_COUNT_MISMATCH;
  return status;
}
struct SegArgs {
  const int32_t* counts;
  int E, topk, with_shared, n_tables;
  int64_t T;
  int32_t* status;
  mxmoe_moe_seg_table tables[2];
};
// thread t fills table t (a layer has two: the gate_up and the down GEMM's inputs). The counts and tags are first
// copied into LDS by the whole workgroup: the sequential walk then waits on no global load (from global memory
// it took 41 us for 61 segments, profiles/r12/graph_forward/). More than kSegLdsExperts experts: from global.
constexpr int kSegLdsExperts = 1024;
__global__ __launch_bounds__(kThreads) void segments_kernel(SegArgs a) {
  __shared__ int32_t s_counts[kSegLdsExperts];
  __shared__ int32_t s_tags[2][kSegLdsExperts + 1];
  const int nseg = a.E + (a.with_shared ? 1 : 0);
  const bool lds = a.E <= kSegLdsExperts;  // (uniform)
  if (lds) {
    for (int i = threadIdx.x; i < a.E; i += blockDim.x) s_counts[i] = a.counts[i];
    for (int t = 0; t < a.n_tables; ++t)
      for (int i = threadIdx.x; i < nseg; i += blockDim.x) s_tags[t][i] = a.tables[t].qtags[i];
    __syncthreads();
  }
  if ((int)threadIdx.x >= a.n_tables) return;
  mxmoe_moe_seg_table tb = a.tables[threadIdx.x];
  if (lds) tb.qtags = s_tags[threadIdx.x];
  const int32_t st = fill_segments(lds ? s_counts : a.counts, a.E, a.T, a.topk, a.with_shared != 0, tb);
  if (st && a.status && threadIdx.x == 0) *a.status = *a.status | st;  // (every table sees the same counts)
}

int segments_check(const int32_t* counts, int E, int64_t T, int topk, const mxmoe_moe_seg_table* tables, int n_tables) {
  if (!counts || E < 1 || E > 4096 || T < 0 || topk < 1 || T * topk > (int64_t)1 << 30 || !tables || n_tables < 1 ||
      n_tables > 2)
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_segments: need counts, 1 <= E <= 4096, T >= 0, topk >= 1, 1 or 2 tables");
  for (int t = 0; t < n_tables; ++t)
    if (!tables[t].qtags || !tables[t].segs || tables[t].width <= 0 || tables[t].width % 128 || tables[t].width_shared < 0 ||
        tables[t].width_shared % 128 || tables[t].ldc < 0 || tables[t].ldc % 8)
      return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_segments: table %d: NULL pointer, a width that is no multiple of 128 "
                  "or an ldc that is no multiple of 8", t);
  return MXMOE_GG_OK;
}

}  // namespace
}  // namespace mxmoe

#include "moe_decode.h"  // the decode forward's kernels (after the quantiser helpers above, which they call)

using namespace mxmoe;

// registers sized to the widest row of the launch, in 512-element chunks (1408 -> 3, 2048 -> 4)
// F8: the kActF8 builds (the MXMOE_ACT_E4M3 tag and the MX tags; MX is then not read)
template <int MODE, bool MX, bool F8, int GLU = kGluNone, bool SRCBF = false>
static void launch_act_w(const typename ActArgsOf<GLU>::type& a, int maxw, hipStream_t st) {
  const int64_t blocks = a.parts > 1 ? a.blk_shared + (a.nslots - a.ntk)
                                     : (a.nslots - a.s0 + kThreads / 64 - 1) / (kThreads / 64);
  const dim3 grid((unsigned)blocks), block(kThreads);
  const int nc = (maxw + 511) / 512;
  const auto go = [&](auto maxc) {
    constexpr int C = decltype(maxc)::value;
    if constexpr (F8) hipLaunchKernelGGL((act_quant_kernel<MODE | kActF8, C, true, GLU, SRCBF>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((act_quant_kernel<MODE, C, MX, GLU, SRCBF>), grid, block, 0, st, a);
  };
  if (nc <= 1) go(std::integral_constant<int, 1>{});
  else if (nc <= 2) go(std::integral_constant<int, 2>{});
  else if (nc <= 3) go(std::integral_constant<int, 3>{});
  else if (nc <= 4) go(std::integral_constant<int, 4>{});
  else if (nc <= 6) go(std::integral_constant<int, 6>{});
  else if (nc <= 8) go(std::integral_constant<int, 8>{});
  else if (nc <= 12) go(std::integral_constant<int, 12>{});
  else if (nc <= 16) go(std::integral_constant<int, 16>{});
  else go(std::integral_constant<int, 32>{});
}

constexpr int kModeGatherBf16 = 4;  // launch_act_any's number for mode 0 on bf16 rows (no mode of the C interface)
// The tags a call's tag_mask names beyond the integer ones: which builds of the kernel run it
struct ActTags {
  bool mx = false;  // MXMOE_ACT_MXFP4 or MXMOE_ACT_MXFP8 (the MX builds)
  bool f8 = false;  // MXMOE_ACT_E4M3 (the kActF8 builds, which carry the MX tags as well)
};
// (mode, tags): which build of the kernel; ActArgs: the four passes, GluArgs: mxmoe_moe_glu_quant's (mode = MXMOE_GLU_*)
template <class ARGS>
static void launch_act_any(int mode, const ARGS& a, int maxw, ActTags tags, hipStream_t st) {
  const auto go = [&](auto mx_build, auto f8_build) {
    constexpr bool MX = decltype(mx_build)::value, F8 = decltype(f8_build)::value;
    if constexpr (std::is_same<ARGS, GluArgs>::value) {
      if (mode == MXMOE_GLU_SWIGLU_CLAMP) launch_act_w<1, MX, F8, kGluSwigluClamp>(a, maxw, st);
      else launch_act_w<1, MX, F8, kGluSilu>(a, maxw, st);
    } else if (mode == 1) launch_act_w<1, MX, F8>(a, maxw, st);
    else if (mode == 2) launch_act_w<2, MX, F8>(a, maxw, st);
    else if (mode == 3) launch_act_w<3, MX, F8>(a, maxw, st);
    else if (mode == kModeGatherBf16) launch_act_w<0, MX, F8, kGluNone, true>(a, maxw, st);
    else launch_act_w<0, MX, F8>(a, maxw, st);
  };
  if (tags.f8) go(std::true_type{}, std::true_type{});
  else if (tags.mx) go(std::true_type{}, std::false_type{});
  else go(std::false_type{}, std::false_type{});
}
// slots [0, nslots): one launch; rows of different widths (routed [0, ntk), shared [ntk, nslots)):
// one launch with each shared row split over a workgroup's 4 waves when a quarter of the shared row
// fits the routed rows' register width, else two launches, each with the register row of its width
// tags: the call's segments may carry the MX tags / MXMOE_ACT_E4M3 (the builds of the kernel that hold their code)
template <class ARGS>
static int launch_act(int mode, ARGS a, int64_t nslots, int w_routed, int w_shared, void* stream, ActTags tags = {}) {
  if (nslots == 0) return MXMOE_GG_OK;
  a.parts = 1;
  a.blk_shared = 0;
  a.s0 = 0;
  const int qw = (w_shared / 4 + 127) & ~127;
  if (nslots > a.ntk && a.ntk > 0 && w_shared > w_routed && qw <= w_routed) {
    a.parts = 4;
    a.blk_shared = (a.ntk + kThreads / 64 - 1) / (kThreads / 64);
    a.nslots = nslots;
    launch_act_any(mode, a, w_routed, tags, (hipStream_t)stream);
  } else {
    const bool split = nslots > a.ntk && w_routed != w_shared && a.ntk > 0;
    a.nslots = split ? a.ntk : nslots;
    const int w0 = split ? w_routed : (nslots > a.ntk ? (w_routed > w_shared ? w_routed : w_shared) : w_routed);
    launch_act_any(mode, a, w0, tags, (hipStream_t)stream);
    if (split) {
      a.s0 = a.ntk;
      a.nslots = nslots;
      launch_act_any(mode, a, w_shared, tags, (hipStream_t)stream);
    }
  }
  return launched("act_quant_kernel");
}

// the activation entry points' bodies; tags: what the call's tag_mask names (the four older entries: nothing)
static int quant_act_impl(const char* fn, const void* hidden, int64_t T, int K, int topk, int with_shared,
                          const int32_t* sorted_expert, const int32_t* perm_token, const mxmoe_moe_seg* segs, int nseg,
                          void* out, void* scales, void* stream, ActTags tags, bool src_bf16 = false) {
  if (T < 0 || topk <= 0 || nseg <= 0 || K <= 0 || K % 128 || K > kMaxWidth)
    return fail(MXMOE_GG_ERR_INVALID, "%s: need K %% 128 == 0, K <= %d, topk > 0, nseg > 0 (K=%d)", fn, kMaxWidth, K);
  if (T > 0 && (!hidden || !sorted_expert || !perm_token || !segs || !out || !aligned16(hidden) || !aligned16(out)))
    return fail(MXMOE_GG_ERR_INVALID, "%s: NULL or misaligned pointer (hidden / out need 16 B)", fn);
  const ActArgs a{static_cast<const _Float16*>(hidden), static_cast<const _Float16*>(hidden), T * topk, 0, 0, K, 0, 0,
                  sorted_expert, perm_token, segs, nseg, static_cast<uint8_t*>(out), static_cast<_Float16*>(scales)};
  return launch_act(src_bf16 ? kModeGatherBf16 : 0, a, T * topk + (with_shared ? T : 0), K, K, stream, tags);
}
static int slots_check(const char* fn, const void* routed_in, const void* shared_in, int64_t T, int topk, int N,
                       int N_shared, const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, void* out) {
  if (T < 0 || topk <= 0 || nseg <= 0 || N <= 0 || N % 128 || N > kMaxWidth ||
      (shared_in && (N_shared <= 0 || N_shared % 128 || N_shared > kMaxWidth)))
    return fail(MXMOE_GG_ERR_INVALID, "%s: widths must be multiples of 128 and <= %d (N=%d, N_shared=%d)", fn, kMaxWidth,
                N, N_shared);
  if (T > 0 && (!routed_in || !sorted_expert || !segs || !out || !aligned16(routed_in) || !aligned16(out) ||
                (shared_in && !aligned16(shared_in))))
    return fail(MXMOE_GG_ERR_INVALID, "%s: NULL or misaligned pointer (16 B)", fn);
  return MXMOE_GG_OK;
}
// the kernel arguments of a pass over slot-ordered inputs (modes 1..3 and mxmoe_moe_glu_quant)
static ActArgs slot_args(const void* routed_in, const void* shared_in, int64_t T, int topk, int N, int N_shared,
                         const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, void* out, void* scales) {
  return ActArgs{static_cast<const _Float16*>(routed_in), static_cast<const _Float16*>(shared_in), T * topk, 0, 0, 0,
                 N, N_shared, sorted_expert, nullptr, segs, nseg, static_cast<uint8_t*>(out),
                 static_cast<_Float16*>(scales)};
}
static int slots_impl(const char* fn, int mode, const void* routed_in, const void* shared_in, int64_t T, int topk, int N,
                      int N_shared, const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, void* out,
                      void* scales, void* stream, ActTags tags) {
  if (int st = slots_check(fn, routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs, nseg, out)) return st;
  const ActArgs a = slot_args(routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs, nseg, out, scales);
  return launch_act(mode, a, T * topk + (shared_in ? T : 0), N, shared_in ? N_shared : N, stream, tags);
}
// a tag_mask's check (MXMOE_GG_OK or the failure, under the entry point's name) and which builds' tags it names
static int tag_mask_tags(const char* fn, uint32_t tag_mask, ActTags* tags) {
  // (tags 5 and 7 are not assigned)
  if (tag_mask & ~((2u << MXMOE_ACT_MXFP4) - 1u | 1u << MXMOE_ACT_MXFP8 | 1u << MXMOE_ACT_E4M3))
    return fail(MXMOE_GG_ERR_UNSUPPORTED, "%s: unknown activation tag in mask %#x", fn, tag_mask);
  tags->mx = ((tag_mask >> MXMOE_ACT_MXFP4) & 1) || ((tag_mask >> MXMOE_ACT_MXFP8) & 1);
  tags->f8 = (tag_mask >> MXMOE_ACT_E4M3) & 1;
  return MXMOE_GG_OK;
}
// what mxmoe_moe_combine and mxmoe_moe_combine_bias check alike once T > 0
// (missing: an entry point's own required pointer is NULL)
static int combine_check(const char* fn, const void* y, const int32_t* inv_slot, const float* weights, const void* shared,
                         const void* out, bool missing = false) {
  if (!y || !inv_slot || !weights || !out || missing || !aligned16(y) || !aligned16(out) || (shared && !aligned16(shared)))
    return fail(MXMOE_GG_ERR_INVALID, "%s: NULL or misaligned pointer (16 B)", fn);
  return MXMOE_GG_OK;
}

// the combine's launch (T > 0, arguments checked) on the output type OT. plain: combine_kernel, which takes neither
// sorted_expert nor the bias pointers nor E; else combine_bias_kernel
template <class OT>
static int launch_combine(const void* y, const int32_t* inv_slot, const int32_t* sorted_expert, const float* weights,
                          const void* bias, const void* shared, const float* shared_w, const void* shared_bias, int64_t T,
                          int topk, int E, int H, void* out, bool plain, void* stream) {
  if (plain)
    hipLaunchKernelGGL(combine_kernel<OT>, dim3((unsigned)T), dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const _Float16*>(y), inv_slot, weights, static_cast<const _Float16*>(shared), shared_w,
                       topk, H, static_cast<OT*>(out));
  else
    hipLaunchKernelGGL(combine_bias_kernel<OT>, dim3((unsigned)T), dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const _Float16*>(y), inv_slot, sorted_expert, weights, static_cast<const _Float16*>(bias),
                       static_cast<const _Float16*>(shared), shared_w, static_cast<const _Float16*>(shared_bias), topk, E, H,
                       static_cast<OT*>(out));
  return launched(plain ? "combine_kernel" : "combine_bias_kernel");
}
// mxmoe_moe_combine_bias and mxmoe_moe_combine_dt: the checks, then the launch. dt_entry: mxmoe_moe_combine_dt (a call
// without any bias runs the build without, the arithmetic of mxmoe_moe_combine; mxmoe_moe_combine_bias always the
// bias build)
static int combine_bias_impl(const char* fn, bool dt_entry, int out_dtype, const void* y, const int32_t* inv_slot,
                             const int32_t* sorted_expert, const float* weights, const void* bias, const void* shared,
                             const float* shared_w, const void* shared_bias, int64_t T, int topk, int E, int H, void* out,
                             void* stream) {
  if (int st = dtype_check(fn, "out_dtype", out_dtype)) return st;
  if (T < 0 || topk <= 0 || H <= 0 || H % 8 || E < 1)
    return fail(MXMOE_GG_ERR_INVALID, "%s: need H %% 8 == 0, topk > 0, E >= 1 (H=%d E=%d)", fn, H, E);
  if (!aligned16(bias) || !aligned16(shared_bias) || (shared_bias && !shared))
    return fail(MXMOE_GG_ERR_INVALID, "%s: misaligned bias pointer (16 B), or a shared_bias without shared", fn);
  if (T == 0) return MXMOE_GG_OK;
  if (int st = combine_check(fn, y, inv_slot, weights, shared, out, bias && !sorted_expert)) return st;
  const bool plain = dt_entry && !bias && !shared_bias;
  const auto launch = out_dtype == MXMOE_DT_BF16 ? launch_combine<__bf16> : launch_combine<_Float16>;
  return launch(y, inv_slot, sorted_expert, weights, bias, shared, shared_w, shared_bias, T, topk, E, H, out, plain, stream);
}

// what mxmoe_moe_gate and mxmoe_moe_gate_ex check alike, before any HIP call
static int gate_check(const char* fn, const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H,
                      int E, int topk, const int32_t* topk_ids, const float* topk_weights, const float* shared_w,
                      int max_e = 256) {
  if (T < 0 || E < 1 || E > max_e || topk < 1 || topk > 16 || topk > E || H <= 0 || H % 32 ||
      T * topk > (int64_t)1 << 30)
    return fail(MXMOE_GG_ERR_INVALID, "%s: need T >= 0, 1 <= E <= %d, 1 <= topk <= min(E, 16), H %% 32 == 0, "
                "T * topk <= 2^30 (T=%lld H=%d E=%d topk=%d)", fn, max_e, (long long)T, H, E, topk);
  if ((w_shared_gate != nullptr) != (shared_w != nullptr))
    return fail(MXMOE_GG_ERR_INVALID, "%s: w_shared_gate and shared_w must be given together", fn);
  if (!aligned16(hidden) || !aligned16(w_gate) || !aligned16(w_shared_gate))
    return fail(MXMOE_GG_ERR_INVALID, "%s: misaligned pointer (hidden / w_gate / w_shared_gate need 16 B)", fn);
  if (T > 0 && (!hidden || !w_gate || !topk_ids || !topk_weights)) return fail(MXMOE_GG_ERR_INVALID, "%s: NULL pointer", fn);
  return MXMOE_GG_OK;
}

static int gate_ex_impl(const char* fn, const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H,
                        int E, int topk, int renormalize, int scoring, const float* e_bias, int n_group, int topk_group,
                        int group_top, float routed_scale, const float* logit_bias, int32_t* topk_ids, float* topk_weights,
                        float* shared_w, float* logits, float* scores, void* stream, int max_e = 256,
                        int dtype = MXMOE_DT_FP16) {
  if (int st = dtype_check(fn, "dtype", dtype)) return st;
  if (scoring != MXMOE_GATE_SOFTMAX && scoring != MXMOE_GATE_SIGMOID)
    return fail(MXMOE_GG_ERR_INVALID, "%s: scoring must be MXMOE_GATE_SOFTMAX or MXMOE_GATE_SIGMOID (got %d)", fn, scoring);
  const int st = gate_check(fn, hidden, w_gate, w_shared_gate, T, H, E, topk, topk_ids, topk_weights, shared_w, max_e);
  if (st != MXMOE_GG_OK) return st;
  if (E > 256 && (n_group != 1 || topk_group != 1 || group_top != 1))  // (mxmoe_moe_gate_wide only: max_e)
    return fail(MXMOE_GG_ERR_INVALID, "%s: E > 256 routes without groups: n_group, topk_group and group_top must be 1 "
                "(E=%d n_group=%d topk_group=%d group_top=%d)", fn, E, n_group, topk_group, group_top);
  // ((E / n_group) % 4 serves the group stage's register layout; the kernel for E > 256 has none and takes any E)
  if (n_group < 1 || n_group > 8 || E % n_group || (E <= 256 && (E / n_group) % 4) || topk_group < 1 ||
      topk_group > n_group || (int64_t)topk > (int64_t)topk_group * (E / n_group))
    return fail(MXMOE_GG_ERR_INVALID, "%s: need 1 <= n_group <= 8, E %% n_group == 0, (E / n_group) %% 4 == 0, "
                "1 <= topk_group <= n_group (1 without groups), topk <= topk_group * E / n_group "
                "(E=%d topk=%d n_group=%d topk_group=%d)", fn, E, topk, n_group, topk_group);
  if (group_top < 1 || group_top > 2 || group_top > E / n_group)
    return fail(MXMOE_GG_ERR_INVALID, "%s: group_top must be 1 or 2 and at most E / n_group (got %d)", fn, group_top);
  if (scoring == MXMOE_GATE_SOFTMAX && (e_bias || scores || group_top != 1))
    return fail(MXMOE_GG_ERR_INVALID, "%s: softmax scoring takes no e_bias, no scores output and group_top == 1", fn);
  if (!std::isfinite(routed_scale)) return fail(MXMOE_GG_ERR_INVALID, "%s: routed_scale must be finite", fn);
  if (((uintptr_t)e_bias | (uintptr_t)scores | (uintptr_t)logit_bias) & 3)
    return fail(MXMOE_GG_ERR_INVALID, "%s: misaligned pointer (e_bias / scores / logit_bias need 4 B)", fn);
  if (T == 0) return MXMOE_GG_OK;
  const gate::GateModeArgs m{{static_cast<const _Float16*>(hidden), static_cast<const _Float16*>(w_gate),
                              static_cast<const _Float16*>(w_shared_gate), T, H, E, topk, renormalize != 0, topk_ids,
                              topk_weights, shared_w, logits},
                             e_bias, scores, n_group, topk_group, group_top, routed_scale};
  const bool sigmoid = scoring == MXMOE_GATE_SIGMOID;
  hipStream_t const hs = (hipStream_t)stream;
  if (dtype == MXMOE_DT_BF16) {  // the same launch forms on the bf16 builds (the pointers carry bf16 bit patterns)
    if (E > 256) gate::gate_wide_launch<true>(gate::GateBiasArgs{m, logit_bias}, sigmoid, hs);
    else if (logit_bias) gate::gate_modes_launch<true>(gate::GateBiasArgs{m, logit_bias}, sigmoid, hs);
    else gate::gate_modes_launch<true>(m, sigmoid, hs);
  } else if (E > 256) gate::gate_wide_launch(gate::GateBiasArgs{m, logit_bias}, sigmoid, hs);
  else if (logit_bias) gate::gate_modes_launch(gate::GateBiasArgs{m, logit_bias}, sigmoid, hs);
  else gate::gate_modes_launch(m, sigmoid, hs);
  return launched(E > 256 ? "gate_wide_kernel" : "gate_modes_kernel");
}

// the checks of an mxmoe_moe_glu (mxmoe_moe_glu_quant and the decode forward's _ex gate_up), under the entry's name
static int glu_check(const char* fn, const mxmoe_moe_glu* glu) {
  if (!glu || (glu->act != MXMOE_GLU_SILU && glu->act != MXMOE_GLU_SWIGLU_CLAMP))
    return fail(MXMOE_GG_ERR_INVALID, "%s: glu->act must be MXMOE_GLU_SILU or MXMOE_GLU_SWIGLU_CLAMP (got %d)", fn,
                glu ? glu->act : -1);
  if (glu->act == MXMOE_GLU_SWIGLU_CLAMP && (!std::isfinite(glu->alpha) || !std::isfinite(glu->limit) || !(glu->limit > 0.0f)))
    return fail(MXMOE_GG_ERR_INVALID, "%s: SWIGLU_CLAMP needs a finite alpha and a finite limit > 0 (alpha=%g limit=%g)", fn,
                (double)glu->alpha, (double)glu->limit);
  if (!aligned16(glu->bias_routed) || !aligned16(glu->bias_shared))
    return fail(MXMOE_GG_ERR_INVALID, "%s: misaligned bias pointer (16 B)", fn);
  return MXMOE_GG_OK;
}

// The two decode entries and their _ex and _wo forms: one body of checks and one launcher each. level: decode::kEx, the
// _ex entry (kind bit 3, the _ex kernels; glu may be NULL: SiLU and no bias), decode::kWo, the _wo entry (kind bits up
// to 11, the _wo kernels, glu likewise); decode::kFirst: glu is NULL and the first entries' kernels run.
static int decode_gate_up_impl(const char* fn, int level, const mxmoe_moe_glu* glu, int dtype, const void* hidden, int64_t T,
                               int topk, int E, int with_shared, const int32_t* topk_ids,
                               const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                               int layout, void* act, void* act_shared, int32_t* status, void* stream) {
  if (int st = dtype_check(fn, "dtype", dtype)) return st;
  if (int st = decode::kind_mask_check(fn, kind_mask, level)) return st;
  if (int st = decode::sizes_check(fn, T, topk, E, with_shared, H, N, N_shared)) return st;
  if (layout != MXMOE_DECODE_GU_PLAIN && layout != MXMOE_DECODE_GU_INTERLEAVED)
    return fail(MXMOE_GG_ERR_INVALID, "%s: layout must be MXMOE_DECODE_GU_PLAIN or MXMOE_DECODE_GU_INTERLEAVED (got %d)", fn,
                layout);
  if (glu) {
    if (int st = glu_check(fn, glu)) return st;
    if (glu->bias_shared && !with_shared)
      return fail(MXMOE_GG_ERR_INVALID, "%s: glu->bias_shared given without a shared expert", fn);
  }
  if (!aligned16(hidden) || !aligned16(act) || !aligned16(act_shared) || ((uintptr_t)topk_ids & 3) ||
      ((uintptr_t)experts & 7) || ((uintptr_t)status & 3))
    return fail(MXMOE_GG_ERR_INVALID, "%s: misaligned pointer (hidden / act / act_shared need 16 B)", fn);
  if (T == 0) return MXMOE_GG_OK;
  if (!hidden || !topk_ids || !experts || !act || (with_shared && !act_shared))
    return fail(MXMOE_GG_ERR_INVALID, "%s: NULL pointer", fn);
  decode::Args a{};
  a.src = a.src_shared = hidden;
  a.ids = topk_ids;
  a.experts = experts;
  a.out = static_cast<_Float16*>(act);
  a.out_shared = static_cast<_Float16*>(act_shared);
  a.status = status;
  a.T = (int)T, a.topk = topk, a.E = E, a.with_shared = with_shared != 0;
  a.K = a.K_shared = H;
  a.C = N, a.C_shared = with_shared ? N_shared : 0;
  a.layout = layout, a.src_bf16 = dtype == MXMOE_DT_BF16, a.kind_mask = kind_mask;
  a.glu = glu && glu->act == MXMOE_GLU_SWIGLU_CLAMP ? kGluSwigluClamp : kGluSilu;
  if (glu) {
    a.bias_routed = static_cast<const _Float16*>(glu->bias_routed);
    a.bias_shared = static_cast<const _Float16*>(glu->bias_shared);
    a.c = -(glu->alpha * 1.4426950408889634f);
    a.limit = glu->limit;
  }
  return decode::launch<false>(a, level, stream);
}

static int decode_down_impl(const char* fn, int level, int64_t T, int topk, int E, int with_shared, const int32_t* topk_ids,
                            const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                            const void* act, const void* act_shared, void* y, void* ys, int32_t* status, void* stream) {
  if (int st = decode::kind_mask_check(fn, kind_mask, level)) return st;
  if (int st = decode::sizes_check(fn, T, topk, E, with_shared, H, N, N_shared)) return st;
  if (!aligned16(act) || !aligned16(act_shared) || !aligned16(y) || !aligned16(ys) || ((uintptr_t)topk_ids & 3) ||
      ((uintptr_t)experts & 7) || ((uintptr_t)status & 3))
    return fail(MXMOE_GG_ERR_INVALID, "%s: misaligned pointer (act / act_shared / y / ys need 16 B)", fn);
  if (T == 0) return MXMOE_GG_OK;
  if (!act || !topk_ids || !experts || !y || (with_shared && (!act_shared || !ys)))
    return fail(MXMOE_GG_ERR_INVALID, "%s: NULL pointer", fn);
  decode::Args a{};
  a.src = act;
  a.src_shared = act_shared;
  a.ids = topk_ids;
  a.experts = experts;
  a.out = static_cast<_Float16*>(y);
  a.out_shared = static_cast<_Float16*>(ys);
  a.status = status;
  a.T = (int)T, a.topk = topk, a.E = E, a.with_shared = with_shared != 0;
  a.K = N, a.K_shared = with_shared ? N_shared : N;
  a.C = a.C_shared = H;
  a.kind_mask = kind_mask;
  return decode::launch<true>(a, level, stream);
}

extern "C" {

int mxmoe_moe_gate(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                   int renormalize, int32_t* topk_ids, float* topk_weights, float* shared_w, float* logits,
                   void* stream) {
  const int st = gate_check("mxmoe_moe_gate", hidden, w_gate, w_shared_gate, T, H, E, topk, topk_ids, topk_weights, shared_w);
  if (st != MXMOE_GG_OK || T == 0) return st;
  const gate::GateArgs a{static_cast<const _Float16*>(hidden), static_cast<const _Float16*>(w_gate),
                         static_cast<const _Float16*>(w_shared_gate), T, H, E, topk, renormalize != 0, topk_ids,
                         topk_weights, shared_w, logits};
  gate::gate_launch(a, (hipStream_t)stream);
  return launched("gate_kernel");
}

int mxmoe_moe_gate_ex(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                      int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                      float routed_scale, int32_t* topk_ids, float* topk_weights, float* shared_w, float* logits,
                      float* scores, void* stream) {
  return gate_ex_impl("mxmoe_moe_gate_ex", hidden, w_gate, w_shared_gate, T, H, E, topk, renormalize, scoring, e_bias, n_group,
                      topk_group, group_top, routed_scale, nullptr, topk_ids, topk_weights, shared_w, logits, scores, stream);
}

int mxmoe_moe_gate_ex2(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                       int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                       float routed_scale, const float* logit_bias, int32_t* topk_ids, float* topk_weights, float* shared_w,
                       float* logits, float* scores, void* stream) {
  return gate_ex_impl("mxmoe_moe_gate_ex2", hidden, w_gate, w_shared_gate, T, H, E, topk, renormalize, scoring, e_bias,
                      n_group, topk_group, group_top, routed_scale, logit_bias, topk_ids, topk_weights, shared_w, logits,
                      scores, stream);
}

int mxmoe_moe_gate_wide(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                        int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                        float routed_scale, const float* logit_bias, int32_t* topk_ids, float* topk_weights, float* shared_w,
                        float* logits, float* scores, void* stream) {
  // E <= 256: mxmoe_moe_gate_ex2's path and kernels; beyond, gate_wide_kernel (moe_gate_wide.h)
  return gate_ex_impl("mxmoe_moe_gate_wide", hidden, w_gate, w_shared_gate, T, H, E, topk, renormalize, scoring, e_bias,
                      n_group, topk_group, group_top, routed_scale, logit_bias, topk_ids, topk_weights, shared_w, logits,
                      scores, stream, gate::kGateWideMaxExperts);
}

int mxmoe_moe_gate_dt(int dtype, const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E,
                      int topk, int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                      float routed_scale, const float* logit_bias, int32_t* topk_ids, float* topk_weights, float* shared_w,
                      float* logits, float* scores, void* stream) {
  // MXMOE_DT_FP16: mxmoe_moe_gate_wide's call; MXMOE_DT_BF16: the same launch forms on the kernels' bf16 builds
  return gate_ex_impl("mxmoe_moe_gate_dt", hidden, w_gate, w_shared_gate, T, H, E, topk, renormalize, scoring, e_bias,
                      n_group, topk_group, group_top, routed_scale, logit_bias, topk_ids, topk_weights, shared_w, logits,
                      scores, stream, gate::kGateWideMaxExperts, dtype);
}

int mxmoe_moe_route(const int32_t* topk_ids, int64_t T, int topk, int E, int32_t* sorted_expert,
                    int32_t* perm_token, int32_t* inv_slot, int32_t* counts, void* stream) {
  if (T < 0 || topk <= 0 || E <= 0 || E > 4096 || T * topk > (int64_t)1 << 30)
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_route: bad sizes (T=%lld topk=%d E=%d)", (long long)T, topk, E);
  if (T > 0 && (!topk_ids || !sorted_expert || !perm_token || !inv_slot))
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_route: NULL pointer");
  if (!counts) return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_route: NULL counts");
  hipLaunchKernelGGL(route_kernel, dim3(E), dim3(kRouteThreads), 0, (hipStream_t)stream, topk_ids, (int)(T * topk), topk,
                     sorted_expert, perm_token, inv_slot, counts);
  return launched("route_kernel");
}

int mxmoe_moe_segments(const int32_t* counts, int E, int64_t T, int topk, int with_shared,
                       const mxmoe_moe_seg_table* tables, int n_tables, int32_t* status, void* stream) {
  if (int st = segments_check(counts, E, T, topk, tables, n_tables)) return st;
  SegArgs a{counts, E, topk, with_shared, n_tables, T, status, {}};
  for (int t = 0; t < n_tables; ++t) {
    if (with_shared && tables[t].width_shared == 0)
      return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_segments: table %d: with_shared needs width_shared", t);
    a.tables[t] = tables[t];
  }
  hipLaunchKernelGGL(segments_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a);
  return launched("segments_kernel");
}

int mxmoe_moe_segments_host(const int32_t* counts, int E, int64_t T, int topk, int with_shared,
                            const mxmoe_moe_seg_table* table, int32_t* status) {
  if (int st = segments_check(counts, E, T, topk, table, 1)) return st;
  if (with_shared && table->width_shared == 0)
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_segments_host: with_shared needs width_shared");
  const int32_t st = fill_segments(counts, E, T, topk, with_shared != 0, *table);
  if (status) *status = st;
  return MXMOE_GG_OK;
}

int mxmoe_moe_quant_act(const void* hidden, int64_t T, int K, int topk, int with_shared,
                        const int32_t* sorted_expert, const int32_t* perm_token, const mxmoe_moe_seg* segs, int nseg,
                        void* out, void* scales, void* stream) {
  return quant_act_impl("mxmoe_moe_quant_act", hidden, T, K, topk, with_shared, sorted_expert, perm_token, segs, nseg, out,
                        scales, stream, ActTags{});
}

int mxmoe_moe_gather_quant(int dtype, const void* hidden, int64_t T, int K, int topk, int with_shared,
                           const int32_t* sorted_expert, const int32_t* perm_token, const mxmoe_moe_seg* segs, int nseg,
                           uint32_t tag_mask, void* out, void* scales, void* stream) {
  const char* fn = "mxmoe_moe_gather_quant";
  if (int st = dtype_check(fn, "dtype", dtype)) return st;
  ActTags tags;
  if (int st = tag_mask_tags(fn, tag_mask, &tags)) return st;
  return quant_act_impl(fn, hidden, T, K, topk, with_shared, sorted_expert, perm_token, segs, nseg, out, scales, stream, tags,
                        dtype == MXMOE_DT_BF16);
}

int mxmoe_moe_silu_mul_quant(const void* routed_in, const void* shared_in, int64_t T, int topk, int N, int N_shared,
                             const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, void* out,
                             void* scales, void* stream) {
  return slots_impl("mxmoe_moe_silu_mul_quant", 1, routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs, nseg,
                    out, scales, stream, ActTags{});
}

int mxmoe_moe_silu_mul_quant_il(const void* routed_in, const void* shared_in, int64_t T, int topk, int N,
                                int N_shared, const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg,
                                void* out, void* scales, void* stream) {
  return slots_impl("mxmoe_moe_silu_mul_quant_il", 3, routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs,
                    nseg, out, scales, stream, ActTags{});
}

int mxmoe_moe_quant_slots(const void* routed_in, const void* shared_in, int64_t T, int topk, int N, int N_shared,
                          const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, void* out, void* scales,
                          void* stream) {
  return slots_impl("mxmoe_moe_quant_slots", 2, routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs, nseg, out,
                    scales, stream, ActTags{});
}

int mxmoe_moe_act_quant(int mode, const void* routed_in, const void* shared_in, int64_t T, int topk, int N, int N_shared,
                        const int32_t* sorted_expert, const int32_t* perm_token, const mxmoe_moe_seg* segs, int nseg,
                        uint32_t tag_mask, void* out, void* scales, void* stream) {
  if (mode < 0 || mode > 3) return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_act_quant: mode must be 0..3 (mode=%d)", mode);
  ActTags tags;
  if (int st = tag_mask_tags("mxmoe_moe_act_quant", tag_mask, &tags)) return st;
  if (mode == 0)
    return quant_act_impl("mxmoe_moe_act_quant", routed_in, T, N, topk, shared_in != nullptr, sorted_expert, perm_token,
                          segs, nseg, out, scales, stream, tags);
  return slots_impl("mxmoe_moe_act_quant", mode, routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs, nseg, out,
                    scales, stream, tags);
}

int mxmoe_moe_glu_quant(const mxmoe_moe_glu* glu, const void* routed_in, const void* shared_in, int64_t T, int topk, int N,
                        int N_shared, const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, uint32_t tag_mask,
                        void* out, void* scales, void* stream) {
  const char* fn = "mxmoe_moe_glu_quant";
  if (int st = glu_check(fn, glu)) return st;
  ActTags tags;
  if (int st = tag_mask_tags(fn, tag_mask, &tags)) return st;
  if (int st = slots_check(fn, routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs, nseg, out)) return st;
  GluArgs a{};
  static_cast<ActArgs&>(a) = slot_args(routed_in, shared_in, T, topk, N, N_shared, sorted_expert, segs, nseg, out, scales);
  a.bias_routed = static_cast<const _Float16*>(glu->bias_routed);
  a.bias_shared = static_cast<const _Float16*>(glu->bias_shared);
  a.nexp = nseg - (shared_in ? 1 : 0);
  a.c = -(glu->alpha * 1.4426950408889634f);
  a.limit = glu->limit;
  return launch_act(glu->act, a, T * topk + (shared_in ? T : 0), N, shared_in ? N_shared : N, stream, tags);
}

int mxmoe_moe_combine_bias(const void* y, const int32_t* inv_slot, const int32_t* sorted_expert, const float* weights,
                           const void* bias, const void* shared, const float* shared_w, const void* shared_bias, int64_t T,
                           int topk, int E, int H, void* out, void* stream) {
  return combine_bias_impl("mxmoe_moe_combine_bias", false, MXMOE_DT_FP16, y, inv_slot, sorted_expert, weights, bias, shared,
                           shared_w, shared_bias, T, topk, E, H, out, stream);
}

int mxmoe_moe_combine_dt(int out_dtype, const void* y, const int32_t* inv_slot, const int32_t* sorted_expert,
                         const float* weights, const void* bias, const void* shared, const float* shared_w,
                         const void* shared_bias, int64_t T, int topk, int E, int H, void* out, void* stream) {
  return combine_bias_impl("mxmoe_moe_combine_dt", true, out_dtype, y, inv_slot, sorted_expert, weights, bias, shared,
                           shared_w, shared_bias, T, topk, E, H, out, stream);
}

int mxmoe_moe_combine(const void* y, const int32_t* inv_slot, const float* weights, const void* shared,
                      const float* shared_w, int64_t T, int topk, int H, void* out, void* stream) {
  if (T < 0 || topk <= 0 || H <= 0 || H % 8)
    return fail(MXMOE_GG_ERR_INVALID, "mxmoe_moe_combine: need H %% 8 == 0, topk > 0 (H=%d)", H);
  if (T == 0) return MXMOE_GG_OK;
  if (int st = combine_check("mxmoe_moe_combine", y, inv_slot, weights, shared, out)) return st;
  return launch_combine<_Float16>(y, inv_slot, nullptr, weights, nullptr, shared, shared_w, nullptr, T, topk, 0, H, out, true,
                                  stream);
}

int mxmoe_moe_decode_gate_up(int dtype, const void* hidden, int64_t T, int topk, int E, int with_shared,
                             const int32_t* topk_ids, const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H,
                             int N, int N_shared, int layout, void* act, void* act_shared, int32_t* status, void* stream) {
  return decode_gate_up_impl("mxmoe_moe_decode_gate_up", decode::kFirst, nullptr, dtype, hidden, T, topk, E, with_shared, topk_ids,
                             experts, kind_mask, H, N, N_shared, layout, act, act_shared, status, stream);
}

int mxmoe_moe_decode_down(int64_t T, int topk, int E, int with_shared, const int32_t* topk_ids,
                          const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                          const void* act, const void* act_shared, void* y, void* ys, int32_t* status, void* stream) {
  return decode_down_impl("mxmoe_moe_decode_down", decode::kFirst, T, topk, E, with_shared, topk_ids, experts, kind_mask, H, N,
                          N_shared, act, act_shared, y, ys, status, stream);
}

int mxmoe_moe_decode_gate_up_ex(const mxmoe_moe_glu* glu, int dtype, const void* hidden, int64_t T, int topk, int E,
                                int with_shared, const int32_t* topk_ids, const mxmoe_moe_decode_expert* experts,
                                uint32_t kind_mask, int H, int N, int N_shared, int layout, void* act, void* act_shared,
                                int32_t* status, void* stream) {
  return decode_gate_up_impl("mxmoe_moe_decode_gate_up_ex", decode::kEx, glu, dtype, hidden, T, topk, E, with_shared, topk_ids,
                             experts, kind_mask, H, N, N_shared, layout, act, act_shared, status, stream);
}

int mxmoe_moe_decode_down_ex(int64_t T, int topk, int E, int with_shared, const int32_t* topk_ids,
                             const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                             const void* act, const void* act_shared, void* y, void* ys, int32_t* status, void* stream) {
  return decode_down_impl("mxmoe_moe_decode_down_ex", decode::kEx, T, topk, E, with_shared, topk_ids, experts, kind_mask, H, N,
                          N_shared, act, act_shared, y, ys, status, stream);
}

int mxmoe_moe_decode_gate_up_wo(const mxmoe_moe_glu* glu, int dtype, const void* hidden, int64_t T, int topk, int E,
                                int with_shared, const int32_t* topk_ids, const mxmoe_moe_decode_expert* experts,
                                uint32_t kind_mask, int H, int N, int N_shared, int layout, void* act, void* act_shared,
                                int32_t* status, void* stream) {
  return decode_gate_up_impl("mxmoe_moe_decode_gate_up_wo", decode::kWo, glu, dtype, hidden, T, topk, E, with_shared,
                             topk_ids, experts, kind_mask, H, N, N_shared, layout, act, act_shared, status, stream);
}

int mxmoe_moe_decode_down_wo(int64_t T, int topk, int E, int with_shared, const int32_t* topk_ids,
                             const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                             const void* act, const void* act_shared, void* y, void* ys, int32_t* status, void* stream) {
  return decode_down_impl("mxmoe_moe_decode_down_wo", decode::kWo, T, topk, E, with_shared, topk_ids, experts, kind_mask,
                          H, N, N_shared, act, act_shared, y, ys, status, stream);
}

}  // extern "C"
