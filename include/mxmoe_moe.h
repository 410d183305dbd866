/*
 * mxmoe_moe.h — C-ABI of the MoE-layer plumbing around the GroupGEMM (MI355X / gfx950):
 * token routing (permute), per-expert activation quantisation, SiLU·mul + quantisation of the
 * gate_up output, and the weighted combine (unpermute). SURVEY.md §8(f) rank 2.
 *
 * Reference interface each entry point replaces (SeaCatComplexes/MxMoE, mxmoe/kernels/src/ref_bind.cu,
 * the torch extension `mxmoe_ops`):
 *   mxmoe_moe_route ............ gg_permute_inp (ref_bind.cu:47-64) and the sort / bincount at the
 *                                head of quant_inp_act (:452-456): values_sorted, perm_indices,
 *                                recv_tokens_per_exp
 *   mxmoe_moe_quant_act ........ quant_act_kernel launched by quant_inp_act (:434-592)
 *   mxmoe_moe_silu_mul_quant ... silu_mul_then_quant_kernel launched by silu_mul_then_quant (:595-757)
 *   mxmoe_moe_combine .......... gg_unpermute_out (:66, an empty stub in the reference)
 * The reference's device kernels (act_kernel.cuh) are not in its tree; the arithmetic here is the
 * reference's quant_weight (quantize.cuh:218-279) applied per token row (or 128-element group) and
 * pack_wxax (quantize.cuh:425-475), producing exactly the A operands the GroupGEMM consumes.
 *
 * Conventions: all pointers are DEVICE pointers unless stated; every call is one or two kernel
 * launches on `stream` (hipStream_t as void*), no allocation, no synchronisation; int status
 * (MXMOE_GG_OK == 0; messages via mxmoe_gg_last_error()).
 */
#ifndef MXMOE_MOE_H_
#define MXMOE_MOE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Quantisation tag of one expert's activation (the reference's cvt_qparams_to_tag, ref_bind.cu:467-479). */
enum {
  MXMOE_ACT_FP16 = 0,    /* a_bits 16: the row is copied                                  */
  MXMOE_ACT_INT8 = 1,    /* a_bits 8, one scale per token                                 */
  MXMOE_ACT_INT4 = 2,    /* a_bits 4, one scale per token                                 */
  MXMOE_ACT_INT4_G128 = 3, /* a_bits 4, one scale per (token, 128-element group)          */
  MXMOE_ACT_MXFP4 = 4,   /* OCP MXFP4 (w4a4_g32_sym_MXFP4): e2m1 codes, one e8m0 scale per (token,
                          * 32-element block), quantised as include/mxmoe_gg.h defines; codes in the
                          * canonical nibble order, scale bytes in the GroupGEMM's device layout;
                          * through mxmoe_moe_act_quant with bit 4 of tag_mask only               */
  /* 5 is NOT assigned: a tag_mask with bit 5 stays "unknown activation tag" */
  MXMOE_ACT_MXFP8 = 6,   /* OCP MXFP8, e4m3 elements (w4a8_g32_sym_MXFP8): one code byte per element
                          * (torch.float8_e4m3fn's bit patterns), one e8m0 scale per (token, 32-element
                          * block) in the device layout, as MXFP4's. Per block: e = floor(log2 amax) - 8
                          * clamped to [-127, 127], scale code e + 127; an all-zero block: scale code 0
                          * and zero codes; a block holding Inf or NaN: scale 255 and zero codes; each
                          * element is multiplied by 2^-e exactly, saturated at +-448 and rounded to
                          * e4m3 once, to nearest even (-0 keeps its sign). quantize.quant_mxfp8 is
                          * the same rule. Through mxmoe_moe_act_quant with bit 6 of tag_mask only  */
  /* 7 is NOT assigned: a tag_mask with bit 7 stays "unknown activation tag" */
  MXMOE_ACT_E4M3 = 8     /* per-token OCP e4m3 (w8a8_g-1_sym_E4M3): one code byte per element (torch.float8_e4m3fn's
                          * bit patterns) in MXMOE_ACT_INT8's byte order (pack_wxax 8-bit: element 2j in the high byte
                          * of its 16-bit word), one fp16 scale per row at scales[scale_off + row]: the A operand of
                          * the E4M3 GroupGEMM tile as it reads it. A row whose values are all finite: amax = the
                          * row's largest |x| (the fp16 values as f32); s = fp16_rn(amax / 448), 1.0 for an all-zero
                          * row, clamped from below to 0x0400 (2^-14: never subnormal); code =
                          * e4m3_rn_sat(f32(x) / f32(s)) — the correctly rounded f32 quotient, rounded ONCE to e4m3
                          * to nearest even and saturated at +-448; -0 and values that round to zero keep their
                          * sign (-0 -> 0x80). quantize.quant_e4m3 and the oracle's oracle_quant_e4m3 are the same
                          * rule. A row holding +-Inf or NaN (a bf16 hidden value beyond 65504 becomes one in the
                          * gather): every code 0x00 and the scale fp16 NaN 0x7E00, so the GroupGEMM's outputs of
                          * that slot are NaN and the fault stays visible (neither the oracle's nor torch's answer
                          * for such a row is kept). Through mxmoe_moe_act_quant, mxmoe_moe_gather_quant and
                          * mxmoe_moe_glu_quant with bit 8 of tag_mask only */
};

/* One expert's segment of a permuted activation buffer. Slots (rows of the permuted batch) are
 * sorted by expert; segment e holds slots [first_slot, first_slot + rows). The shared expert, if
 * any, is segment E, fed by every token once (slots T*topk + t). */
typedef struct mxmoe_moe_seg {
  int32_t qtag;        /* MXMOE_ACT_*                                                          */
  int32_t first_slot;  /* first slot of the segment                                           */
  int32_t rows;        /* tokens routed to this expert                                        */
  int32_t width;       /* elements per row of this segment's output (K of the next GEMM)      */
  int64_t out_off;     /* byte offset of the segment's [rows][width * bits / 8] block in `out` */
  int64_t scale_off;   /* fp16-element offset of its scales: [rows] (INT8, INT4, E4M3) or [width/128][rows];
                        * MXFP4 / MXFP8: of its [rows][16 ceil(width/32 / 16)] e8m0 bytes (even offset: the
                        * block is 4-byte aligned)                                              */
} mxmoe_moe_seg;

/* The router in front of the layer, one launch: gate logits, top-k selection, softmax weights and
 * (optionally) the shared expert's gate, from one pass over `hidden`.
 * Replaces: nothing in the reference, which has no router kernel (its bench draws topk_ids). The
 * semantics are the models' own `softmax(hidden @ w_gate.T) -> topk` routing code (qwen2_moe,
 * DeepSeek-V2-Lite, Mixtral) and qwen2_moe's `sigmoid(shared_expert_gate(hidden))`.
 *   hidden fp16 [T][H], w_gate fp16 [E][H], w_shared_gate fp16 [H] or NULL (all row-major).
 *   logits   x[e] = sum_h f32(hidden[t][h]) * f32(w_gate[e][h]), f32 accumulation on the MFMA
 *            (v_mfma_f32_16x16x32_f16; the summation order is the kernel's own).
 *   selection: the topk largest x[e]; among equal logits (-0 == +0) the lower index wins.
 *            topk_ids[t][k] (int32) in descending order of logit, ties by ascending index. The
 *            selection is made on the logits, not on the probabilities.
 *   weights  m = max_e x[e], p[e] = exp2((x[e] - m) * log2 e) (hardware exp2), f32 [T][topk] as
 *            mxmoe_moe_combine reads them:
 *            renormalize == 0: p[id_k] / sum_{e<E} p[e]       (qwen2_moe, DeepSeek-V2-Lite)
 *            renormalize != 0: p[id_k] / sum_{j<topk} p[id_j] (Mixtral)
 *   shared_w[t] = rcp(1 + exp2(-s * log2 e)), s = hidden[t] . w_shared_gate (f32 [T], the shared_w
 *            of mxmoe_moe_combine): one more output column of the same pass, outside the softmax,
 *            the max and the selection. shared_w must be non-NULL exactly when w_shared_gate is.
 *   logits   NULL, or f32 [T][E]: receives the very x[e] the selection and the softmax used.
 * A row whose logits hold NaN or +-Inf still gets topk distinct ids in [0, E) (its weights may be
 * anything, NaN included). Rows past T and columns past E (E + 1 with the shared gate) pad the last
 * MFMA block through clamped addresses: nothing outside the operands is read, nothing outside
 * [T] rows written. No workspace, no allocation.
 * Limits: T >= 0 (T == 0: OK, no launch), T * topk <= 2^30, 1 <= E <= 256, 1 <= topk <= min(E, 16),
 * H % 32 == 0; hidden, w_gate and w_shared_gate 16-byte aligned. Anything else: MXMOE_GG_ERR_INVALID
 * (checked before any HIP call). */
int mxmoe_moe_gate(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                   int renormalize, int32_t* topk_ids, float* topk_weights, float* shared_w, float* logits,
                   void* stream);

/* mxmoe_moe_gate with the routing rules of DeepSeek-V3 / R1 (sigmoid scores, e_score_correction_bias,
 * group-limited top-k, routed_scaling_factor), DeepSeek-V2 (softmax, group_limited_greedy) and
 * GLM-4.5-style layers (sigmoid + bias, one group): the same single launch and the same K loop.
 * Replaces: nothing in the reference (no router kernel); the semantics are the models' public routing
 * code, with the two deviations named below (tie rule, -inf fill).
 *   hidden, w_gate, w_shared_gate, T, H, E, topk, renormalize, shared_w, logits: as mxmoe_moe_gate; the
 *            logits x[e] and the shared gate column are computed exactly as there, under both scorings.
 *   scoring  MXMOE_GATE_SOFTMAX: selection values v[e] = x[e] (the selection stays on the logits).
 *            e_bias and scores must be NULL and group_top 1.
 *            MXMOE_GATE_SIGMOID: s[e] = rcp(1 + exp2(-x[e] * log2 e)) in f32 (the shared gate's
 *            arithmetic), v[e] = s[e] + e_bias[e] (one f32 add; e_bias f32 [E] or NULL: v = s).
 *   scores   NULL, or f32 [T][E] (sigmoid only): receives the very s[e] used.
 *   groups   n_group == 1: no group stage. Otherwise group G holds experts [G gs, (G + 1) gs),
 *            gs = E / n_group; its score is max v (group_top == 1) or the f32 sum (one add) of its two
 *            largest v (group_top == 2: DeepSeek-V3). The topk_group groups with the largest score are
 *            kept; among equal scores (-0 == +0) the lower group index wins. Experts of the other
 *            groups are never selected: the -inf fill of serving stacks. (The HF DeepSeek-V3 code fills
 *            dropped groups with 0.0 instead, which can select a masked expert when a kept v is
 *            negative; that is not reproduced.)
 *   selection: the topk largest v among the kept experts; topk_ids in descending order of v, ties
 *            (-0 == +0) to the lower index. A row whose values hold NaN or +-Inf still gets topk
 *            distinct ids in [0, E).
 *   weights  SOFTMAX: mxmoe_moe_gate's weights (softmax over all E experts, or over the chosen ones with
 *            renormalize), then one f32 multiply by routed_scale.
 *            SIGMOID: s[id_k] (the unbiased score), or with renormalize s[id_k] / (sum_j s[id_j] + 1e-20),
 *            then one f32 multiply by routed_scale.
 *            routed_scale == 1.0 multiplies by one: the weights are unchanged bit for bit.
 * Limits: mxmoe_moe_gate's, and 1 <= n_group <= 8, E % n_group == 0, gs % 4 == 0 (gs = 20 works),
 * 1 <= topk_group <= n_group (so 1 when n_group is 1), topk <= topk_group * gs, group_top 1 or 2 and
 * <= gs, routed_scale finite, e_bias and scores 4-byte aligned. Anything else: MXMOE_GG_ERR_INVALID
 * (checked before any HIP call). E > 256: mxmoe_moe_gate_wide (without groups). */
enum { MXMOE_GATE_SOFTMAX = 0, MXMOE_GATE_SIGMOID = 1 };
int mxmoe_moe_gate_ex(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                      int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                      float routed_scale, int32_t* topk_ids, float* topk_weights, float* shared_w, float* logits,
                      float* scores, void* stream);

/* mxmoe_moe_gate_ex with a bias on the logits (gpt-oss's router: F.linear(hidden, w, bias) -> top-k on the
 * logits -> softmax over the chosen ones, i.e. scoring = MXMOE_GATE_SOFTMAX, renormalize = 1, logit_bias).
 * Replaces: nothing in the reference (no router kernel); the semantics are GptOssTopKRouter's public code.
 *   logit_bias f32 [E] or NULL (4-byte aligned): x[e] = acc[e] + logit_bias[e], one f32 add after the MFMA
 *            reduction and before everything else. The `logits` output, the selection, the softmax / sigmoid
 *            scores and the group stage all see the biased x. The shared-gate column gets no bias.
 *   Every other argument, rule and limit: mxmoe_moe_gate_ex's. With logit_bias == NULL the call IS
 *   mxmoe_moe_gate_ex (the same kernels), bit for bit; a non-NULL bias runs builds of their own, so
 *   mxmoe_moe_gate's and mxmoe_moe_gate_ex's kernels are untouched by it.
 * e_bias (sigmoid scoring's selection bias on the scores) and logit_bias are independent and may be combined. */
int mxmoe_moe_gate_ex2(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                       int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                       float routed_scale, const float* logit_bias, int32_t* topk_ids, float* topk_weights, float* shared_w,
                       float* logits, float* scores, void* stream);

/* mxmoe_moe_gate_ex2 for layers with up to 512 experts (Kimi-K2: 384 experts, top-8, sigmoid scores + e_bias,
 * renormalize, routed_scale; Qwen3-Next: 512 experts, top-10, softmax over the chosen ones, a shared-expert gate,
 * i.e. 513 columns). One launch, no workspace, no allocation, no synchronisation; graph-capturable like the others.
 * Replaces: nothing in the reference (no router kernel); the semantics are the models' public routing code.
 *   Every argument and rule: mxmoe_moe_gate_ex2's — logits by fp16 MFMA with f32 accumulation, logit_bias, e_bias, the
 *   scores and logits outputs, the shared-gate column outside the softmax and the selection, renormalize,
 *   routed_scale. Selection: descending value over the whole row, ties (-0 == +0) to the lower expert index over the
 *   whole row; a row of NaN or +-Inf still gets topk distinct ids in [0, E); rows past T are never written.
 *   E <= 256: the call IS mxmoe_moe_gate_ex2 (the same kernels, byte-identical outputs; groups allowed).
 *   E > 256: a kernel of another form (mxmoe_amd/csrc/moe_gate_wide.h): the columns are split into slices that
 *   different waves finish, and the slices' sorted candidates are merged by (value descending, index ascending).
 *   The f32 sum of the softmax over all E experts (renormalize == 0) adds per-slice sums in slice order, so weights
 *   may differ from a single-slice sum in the last bits (never from run to run).
 * Limits: mxmoe_moe_gate_ex2's with 1 <= E <= 512. For E > 256, n_group, topk_group and group_top must all be 1:
 * group-limited routing across column slices is deliberately left out (no known model with more than 256 experts
 * routes group-limited); E need then be no multiple of 4 (that rule serves the group stage). E > 512 and topk > 16 are out
 * of scope; bf16 operands: mxmoe_moe_gate_dt. Anything else:
 * MXMOE_GG_ERR_INVALID under this entry point's name (checked before any HIP call). T == 0: OK, no launch.
 * mxmoe_moe_gate, mxmoe_moe_gate_ex and mxmoe_moe_gate_ex2 keep their E <= 256 limit and their kernels. */
int mxmoe_moe_gate_wide(const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E, int topk,
                        int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                        float routed_scale, const float* logit_bias, int32_t* topk_ids, float* topk_weights, float* shared_w,
                        float* logits, float* scores, void* stream);

/* Element types of the entry points that take one (the *_dt / gather entries below). Every other entry is fp16. */
enum { MXMOE_DT_FP16 = 0, MXMOE_DT_BF16 = 1 };

/* mxmoe_moe_gate_wide with the operands' element type as an argument: the router of a bf16 model, with no cast pass.
 * Replaces: nothing in the reference (no router kernel, fp16 only).
 *   dtype    MXMOE_DT_FP16: the call IS mxmoe_moe_gate_wide (the same kernels, byte-identical outputs).
 *            MXMOE_DT_BF16: hidden, w_gate and w_shared_gate are bf16 (all three: one dtype per call). The logits are
 *            x[e] = sum_h f32(hidden[t][h]) * f32(w_gate[e][h]) on v_mfma_f32_16x16x32_bf16: every product of two bf16
 *            values is exact in f32, the accumulation is f32 in the kernel's own order. The operands are NOT converted
 *            to fp16 on the way: a weight below 2^-14 or a hidden value above 65504 keeps its value. Everything after
 *            the logits — logit_bias, selection, softmax / sigmoid, groups, e_bias, renormalize, routed_scale, the
 *            shared-expert gate, the logits / scores outputs — is the fp16 kernels' code, unchanged; so are the launch
 *            forms (rows per workgroup, K split, column slices beyond 256 experts).
 *   Every other argument, rule and limit: mxmoe_moe_gate_wide's (1 <= E <= 512; groups up to 256 experts), checked
 *   before any HIP call and reported under this entry point's name; an unknown dtype: MXMOE_GG_ERR_INVALID.
 * A call with every rule at its default (mxmoe_moe_gate's) runs the softmax build of mxmoe_moe_gate_ex's kernel with
 * routed_scale 1.0: there is no bf16 build of mxmoe_moe_gate's own kernel. */
int mxmoe_moe_gate_dt(int dtype, const void* hidden, const void* w_gate, const void* w_shared_gate, int64_t T, int H, int E,
                      int topk, int renormalize, int scoring, const float* e_bias, int n_group, int topk_group, int group_top,
                      float routed_scale, const float* logit_bias, int32_t* topk_ids, float* topk_weights, float* shared_w,
                      float* logits, float* scores, void* stream);

/* Stable counting sort of the T*topk expert ids (int32, row-major [T][topk], values in [0, E)):
 *   sorted_expert[s] = expert of slot s (non-decreasing), perm_token[s] = source token of slot s,
 *   inv_slot[t*topk + k] = slot of (token t, choice k), counts[e] = tokens routed to expert e.
 * Equal to torch.sort(topk_ids.view(-1), stable=True) + floor_divide(topk) + bincount(E).
 * One workgroup per expert; E <= 4096. */
int mxmoe_moe_route(const int32_t* topk_ids, int64_t T, int topk, int E, int32_t* sorted_expert,
                    int32_t* perm_token, int32_t* inv_slot, int32_t* counts, void* stream);

/* The segment table on the device: what a host builds from the routing counts after copying them back
 * (mxmoe_amd/moe.py, _make_segments), from the DEVICE counts[E] of mxmoe_moe_route, in one small launch — the
 * piece that lets a whole layer run without the host ("Device planning / graph forward").
 * No reference counterpart: the reference moves the counts to the host (ref_bind.cu:456).
 * A table describes one activation buffer: qtags DEVICE int32 [nseg] (MXMOE_ACT_*, nseg = E + 1 with the
 * shared expert), the routed segments' width and the shared one's. Written, per segment in expert order:
 *   segs[e]   {qtag, first_slot = rows before e (shared: T * topk), rows = counts[e] (shared: T), width,
 *              out_off, scale_off}: out_off advances by the segment's bytes rounded up to 16, scale_off by its
 *              scale elements ([rows] for INT8 / INT4 / E4M3, g128 [width/128][rows], MXFP4 / MXFP8 rows * 16 ceil(width/32 / 16) / 2
 *              after rounding scale_off up to even, fp16 none);
 *   dyn[e]    (optional, mxmoe_gg_dyn_row of include/mxmoe_gg.h: the row table of the GroupGEMM that reads the
 *              buffer) {rows, a_off = out_off, sa_off = 2 * scale_off, c_off = 2 * first_slot * ldc; shared: 0}.
 * status (DEVICE int32, optional): bit MXMOE_MOE_SEG_COUNT_MISMATCH is OR-ed in when the counts do not sum to
 * T * topk (ids outside [0, E) were dropped by the routing) or a count had to be clamped to keep the routed rows
 * within T * topk. One launch fills up to two tables (a layer's gate_up and down inputs). */
typedef struct mxmoe_moe_seg_table {
  const int32_t* qtags;  /* DEVICE int32 [nseg] */
  int32_t width;         /* elements per row of a routed segment (multiple of 128) */
  int32_t width_shared;  /* ... of the shared segment (with_shared) */
  int64_t ldc;           /* row stride, in fp16 elements, of the routed experts' C in the next GroupGEMM */
  mxmoe_moe_seg* segs;   /* DEVICE out [nseg] */
  void* dyn;             /* DEVICE out mxmoe_gg_dyn_row [nseg], or NULL */
} mxmoe_moe_seg_table;
enum { MXMOE_MOE_SEG_COUNT_MISMATCH = 1 };
int mxmoe_moe_segments(const int32_t* counts, int E, int64_t T, int topk, int with_shared,
                       const mxmoe_moe_seg_table* tables, int n_tables, int32_t* status, void* stream);

/* Diagnostics: mxmoe_moe_segments' function run on the host. Every pointer (counts, the one table's qtags, segs,
 * dyn, status) is HOST memory; no device is touched. */
int mxmoe_moe_segments_host(const int32_t* counts, int E, int64_t T, int topk, int with_shared,
                            const mxmoe_moe_seg_table* table, int32_t* status);

/* Gather + quantise the permuted activations: slot s < T*topk reads hidden[perm_token[s]] and is
 * written to segment sorted_expert[s]; with_shared != 0 adds slots T*topk + t, which read hidden[t]
 * into the last segment (nseg - 1: the shared expert). hidden: fp16 [T][K]; segs: DEVICE array of nseg segments, every
 * width == K. Quantised rows: RTN sym in fp16 (scale = fp16(amax / qmax), 0 -> 1;
 * q = rint_even(clamp(fp16(x / scale), +-qmax))), packed per pack_wxax.
 * K % 128 == 0 and K <= 16384. */
int mxmoe_moe_quant_act(const void* hidden, int64_t T, int K, int topk, int with_shared,
                        const int32_t* sorted_expert, const int32_t* perm_token, const mxmoe_moe_seg* segs, int nseg,
                        void* out, void* scales, void* stream);

/* mxmoe_moe_quant_act with the element type of hidden as an argument and mxmoe_moe_act_quant's tag_mask (bits 4 / 6 / 8
 * select the builds that carry MXMOE_ACT_MXFP4 / MXMOE_ACT_MXFP8 / MXMOE_ACT_E4M3; an unknown bit:
 * MXMOE_GG_ERR_UNSUPPORTED).
 * Replaces: nothing in the reference (fp16 only).
 *   dtype    MXMOE_DT_FP16: mxmoe_moe_quant_act's (mxmoe_moe_act_quant mode 0's) kernels and bytes.
 *            MXMOE_DT_BF16: hidden is bf16 [T][K]. Each element is converted to fp16 as it is loaded — widened to f32
 *            (exact), then rounded once to fp16 to nearest even; beyond fp16's range +-Inf; the fp16-subnormal range
 *            is rounded, not flushed: the value hidden.to(torch.float16) holds — and from there the pass is the fp16
 *            one for every tag: out and scales equal, byte for byte, what the fp16 pass writes for the converted
 *            hidden. The experts therefore still compute on fp16 values: bf16's range is not kept past this pass.
 *            NaN payloads are unspecified.
 * Only the gather reads bf16: the gate_up output the other activation passes read stays fp16.
 * Other arguments and limits: mxmoe_moe_quant_act's; an unknown dtype: MXMOE_GG_ERR_INVALID. */
int mxmoe_moe_gather_quant(int dtype, const void* hidden, int64_t T, int K, int topk, int with_shared,
                           const int32_t* sorted_expert, const int32_t* perm_token, const mxmoe_moe_seg* segs, int nseg,
                           uint32_t tag_mask, void* out, void* scales, void* stream);

/* act = fp16_rn(silu(f32 g) * f32 u) of the gate_up output (silu(g) = g * rcp(1 + exp2(-g log2 e)) with
 * the hardware exp2 / reciprocal), then quantised as mxmoe_moe_quant_act.
 * routed_in: fp16 [T*topk][2*N] (slot order; gate = columns [0, N), up = [N, 2N));
 * shared_in: fp16 [T][2*N_shared] or NULL (non-NULL: slots T*topk + t, segment nseg - 1). Segment widths: N for routed experts,
 * N_shared for the shared one (both multiples of 128, <= 16384). */
int mxmoe_moe_silu_mul_quant(const void* routed_in, const void* shared_in, int64_t T, int topk, int N, int N_shared,
                             const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, void* out,
                             void* scales, void* stream);

/* mxmoe_moe_silu_mul_quant on a gate_up output computed with gate / up rows interleaved in 16-row
 * blocks (MXMOE_GG_EPI_SILU_MUL's weight layout) but the plain epilogue: routed_in [T*topk][2 N],
 * shared_in [T][2 N_shared], columns [32 b, 32 b + 16) = gate columns [16 b, 16 b + 16) and
 * [32 b + 16, 32 b + 32) the matching up columns. Same arithmetic and outputs as
 * mxmoe_moe_silu_mul_quant on the de-interleaved input (the small-batch form of a fused layer). */
int mxmoe_moe_silu_mul_quant_il(const void* routed_in, const void* shared_in, int64_t T, int topk, int N,
                                int N_shared, const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg,
                                void* out, void* scales, void* stream);

/* mxmoe_moe_silu_mul_quant's quantisation alone, for activations the gate_up GroupGEMM already
 * produced with its fused SiLU epilogue (MXMOE_GG_EPI_SILU_MUL, include/mxmoe_gg.h): routed_in fp16
 * [T*topk][N] in slot order, shared_in fp16 [T][N_shared] or NULL; same segments, outputs and limits.
 * (No reference counterpart: the reference's silu_mul_then_quant, ref_bind.cu:595-757, does both.) */
int mxmoe_moe_quant_slots(const void* routed_in, const void* shared_in, int64_t T, int topk, int N, int N_shared,
                          const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, void* out, void* scales,
                          void* stream);

/* The four activation launches above behind one entry point that is told which tags the segments
 * carry: tag_mask bit t is set when some segment has qtag t. REQUIRED for segments tagged
 * MXMOE_ACT_MXFP4: the kernel builds with the MXFP4 code run only when bit 4 is set, so the four named
 * entry points (and any call here without the bit) keep the builds they had before the tag existed
 * and must not be given such a segment — they would treat it as int4. MXMOE_ACT_MXFP8 segments
 * likewise need bit 6, MXMOE_ACT_E4M3 segments bit 8 (builds of their own, which carry the MX tags too: a call may
 * set bit 8 together with bit 4 or 6, a mixed layer). A mask with bit 5, bit 7 or a bit above 8 is MXMOE_GG_ERR_UNSUPPORTED.
 *   mode 0: mxmoe_moe_quant_act      (routed_in = hidden [T][N], N = K; shared_in != NULL <=> with_shared,
 *                                     its value is ignored; perm_token required)
 *   mode 1: mxmoe_moe_silu_mul_quant, 2: mxmoe_moe_quant_slots, 3: mxmoe_moe_silu_mul_quant_il
 *           (arguments as there; perm_token unused)
 * (No reference counterpart.) */
int mxmoe_moe_act_quant(int mode, const void* routed_in, const void* shared_in, int64_t T, int topk, int N, int N_shared,
                        const int32_t* sorted_expert, const int32_t* perm_token, const mxmoe_moe_seg* segs, int nseg,
                        uint32_t tag_mask, void* out, void* scales, void* stream);

/* The activation pass of a layer whose gate_up projection has a bias and / or whose gated activation is not
 * SiLU (gpt-oss): mxmoe_moe_silu_mul_quant's inputs, segments, outputs and limits (mode 1: [gate | up] columns),
 * tag_mask as in mxmoe_moe_act_quant (every tag; MXFP4, MXFP8 and E4M3 with their bits).
 * Replaces: nothing in the reference; the clamped activation is GptOssExperts._apply_gate's public code.
 * For slot s of expert e = sorted_expert[s] (the shared segment: bias_shared) and column n, all in f32:
 *   g = f32(in[s][n]) + f32(bg[e][n]),  u = f32(in[s][N + n]) + f32(bu[e][n])   (one IEEE add each; a NULL bias:
 *                                                                                no add), bias row = [bg | bu]
 *   MXMOE_GLU_SILU:         a = g * rcp(1 + exp2(g * -log2 e)) * u              (mxmoe_moe_silu_mul_quant's expression)
 *   MXMOE_GLU_SWIGLU_CLAMP: gc = min(g, limit), uc = min(max(u, -limit), limit), c = -(alpha * 1.4426950408889634f)
 *                           (computed once on the host in f32), a = (gc * rcp(1 + exp2(gc * c))) * (uc + 1.0f)
 *   act = fp16_rn(a), then quantised by the segment's tag as mxmoe_moe_quant_act does. NaN inputs: unspecified.
 * With act = SILU and both biases NULL the outputs are mxmoe_moe_silu_mul_quant's byte for byte. A routed slot
 * whose id is no routed expert's gets no bias (and, as everywhere, is never written).
 * Limits: mxmoe_moe_silu_mul_quant's; bias pointers 16-byte aligned; SWIGLU_CLAMP: alpha finite, limit finite and
 * > 0 (gpt-oss: 1.702, 7.0; both ignored by SILU). An unknown act, a bad limit or a misaligned bias:
 * MXMOE_GG_ERR_INVALID; an unknown tag bit: MXMOE_GG_ERR_UNSUPPORTED (both checked before any HIP call). */
enum { MXMOE_GLU_SILU = 0, MXMOE_GLU_SWIGLU_CLAMP = 1 };
typedef struct mxmoe_moe_glu {
  int32_t act;              /* MXMOE_GLU_*                                                 */
  float alpha, limit;       /* SWIGLU_CLAMP only (gpt-oss: 1.702, 7.0); limit > 0, finite  */
  const void* bias_routed;  /* fp16 [E][2N]  ([gate | up] columns, as routed_in) or NULL   */
  const void* bias_shared;  /* fp16 [2 N_shared] or NULL                                   */
} mxmoe_moe_glu;
int mxmoe_moe_glu_quant(const mxmoe_moe_glu* glu, const void* routed_in, const void* shared_in, int64_t T, int topk, int N,
                        int N_shared, const int32_t* sorted_expert, const mxmoe_moe_seg* segs, int nseg, uint32_t tag_mask,
                        void* out, void* scales, void* stream);

/* mxmoe_moe_combine for a down projection with a bias per expert: out[t][h] = fp16_rn(acc), acc = +0 then, for
 * k = 0..topk-1 in order, slot = inv_slot[t*topk + k], e = sorted_expert[slot],
 *   acc = fma(weights[t][k], f32(y[slot][h]) + f32(bias[e][h]), acc)      (the inner add: one IEEE f32 add),
 * then, if shared != NULL, acc = fma(shared_w ? shared_w[t] : 1, f32(shared[t][h]) + f32(shared_bias[h]), acc).
 * bias fp16 [E][H] or NULL, shared_bias fp16 [H] or NULL (NULL: no add; shared_bias needs shared); both 16-byte
 * aligned. An e outside [0, E) adds no bias (stale slots of an invalid id in a graph forward): bias is never
 * indexed with an unchecked id. sorted_expert: mxmoe_moe_route's (required with a bias). Other arguments and
 * limits: mxmoe_moe_combine's, and E >= 1. With both biases NULL the output is mxmoe_moe_combine's bit for bit.
 * (No reference counterpart: gg_unpermute_out is an empty stub.) */
int mxmoe_moe_combine_bias(const void* y, const int32_t* inv_slot, const int32_t* sorted_expert, const float* weights,
                           const void* bias, const void* shared, const float* shared_w, const void* shared_bias, int64_t T,
                           int topk, int E, int H, void* out, void* stream);

/* mxmoe_moe_combine_bias with the output's element type as an argument: the f32 accumulator of the same fma chain
 * (y, bias, shared and shared_bias stay fp16) is rounded once to out_dtype, to nearest even — MXMOE_DT_BF16: out is
 * bf16 [T][H] (v_cvt_pk_bf16_f32); MXMOE_DT_FP16: mxmoe_moe_combine_bias's output bit for bit.
 * sorted_expert, bias and shared_bias may be NULL (sorted_expert is required with a bias); with bias and shared_bias
 * both NULL the arithmetic is mxmoe_moe_combine's (and its kernel runs). Other arguments and limits:
 * mxmoe_moe_combine_bias's; an unknown out_dtype: MXMOE_GG_ERR_INVALID. (No reference counterpart.) */
int mxmoe_moe_combine_dt(int out_dtype, const void* y, const int32_t* inv_slot, const int32_t* sorted_expert,
                         const float* weights, const void* bias, const void* shared, const float* shared_w,
                         const void* shared_bias, int64_t T, int topk, int E, int H, void* out, void* stream);

/* out[t][h] = fp16_rn(acc), acc = +0 then, for k = 0..topk-1 in order,
 *   acc = fma(weights[t][k], f32(y[inv_slot[t*topk + k]][h]), acc),
 * then, if shared != NULL, acc = fma(shared_w ? shared_w[t] : 1, f32(shared[t][h]), acc).
 * y: fp16 [T*topk][H] in slot order; weights: f32 [T][topk]; shared: fp16 [T][H]; H % 8 == 0. */
int mxmoe_moe_combine(const void* y, const int32_t* inv_slot, const float* weights, const void* shared,
                      const float* shared_w, int64_t T, int topk, int H, void* out, void* stream);

/* The decode forward: a layer call of 1..16 tokens as two weight-streaming launches, with no sort, no segment table,
 * no tile table and no planner — every workgroup reads the T * topk ids and finds the rows of its own expert
 * (mxmoe_amd/csrc/moe_decode.h). mxmoe_moe_decode_gate_up writes the activations, mxmoe_moe_decode_down the down
 * projections, both in PAIR order (row p = t * topk + k, no permutation); mxmoe_moe_combine / mxmoe_moe_combine_dt
 * with inv_slot[p] = p then give the layer's output.
 * Replaces: nothing in the reference (which plans a GroupGEMM whatever the batch). The arithmetic is the one the
 * entries above and the GroupGEMM (include/mxmoe_gg.h) compute, so for the integer kinds act, y and out equal the
 * planned layer's bit for bit.
 *   experts  DEVICE array of E records (E + 1 with_shared: the shared expert last). Per linear a kind:
 *            MXMOE_DECODE_FP16 (B fp16 [rows][K], no scale), MXMOE_DECODE_W8A8 (w8a8_g-1_sym: B pack_wxax int8
 *            [rows][K], scale_b fp16 [rows]), MXMOE_DECODE_W4A4 (w4a4_g-1_sym: B pack_wxax int4 [rows][K / 2], scale_b
 *            fp16 [rows]); the kinds may differ per expert and between an expert's two linears. b1: the gate_up weight,
 *            2N rows (2 N_shared for the shared expert), K = H; b2: the down weight, H rows, K = N (N_shared).
 *   kind_mask bit k set when some record carries kind k on the call's linear (kind1 for gate_up, kind2 for down): it
 *            sizes the workgroups' LDS rows. A bit of a kind that does not exist: MXMOE_GG_ERR_UNSUPPORTED. A record
 *            whose kind is not in the mask sets MXMOE_DECODE_BAD_KIND in *status and its rows are not written.
 *   layout   of every gate_up weight: MXMOE_DECODE_GU_PLAIN (gate rows [0, N), up rows [N, 2N)) or
 *            MXMOE_DECODE_GU_INTERLEAVED (16-row blocks alternating gate, up — MXMOE_GG_EPI_SILU_MUL's layout: gate
 *            row n at 32 (n / 16) + n % 16, its up row 16 further); scale_b follows its rows. The layout changes only
 *            the row index.
 * mxmoe_moe_decode_gate_up, for every pair p = t * topk + k with e = topk_ids[t][k] in [0, E) (and, with_shared, for
 * every token t on the shared expert), with the expert's kind1:
 *   x        hidden[t], fp16; dtype MXMOE_DT_BF16: each bf16 element converted to fp16 as mxmoe_moe_gather_quant does
 *            (to nearest even, +-Inf beyond fp16's range, subnormals rounded).
 *   A row    FP16: x. W8A8 / W4A4 (qmax 127 / 7): mxmoe_moe_quant_act's rule over the whole row,
 *            scale_a = fp16(amax / qmax), 0 -> 1; q = rint_even(clamp(fp16(x / scale_a), +-qmax)).
 *   dot      row r of B against the A row: integers exactly in int32 (v_dot4_i32_i8 / v_dot8_i32_i4; int4 codes are
 *            two's-complement nibbles; A and B share pack_wxax's K permutation), fp16 in f32 (fma, the kernel's order).
 *   v(r)     FP16: fp16_rn(acc); W8A8 / W4A4: fp16_rn(0 + f32(acc) * f32(fp16_rn(scale_a * scale_b[r]))), the f32
 *            product rounded on its own — the GroupGEMM's epilogue.
 *   act      column n: g = v(gate row of n), u = v(up row of n), act[p][n] = fp16_rn(silu(f32 g) * f32 u),
 *            silu(g) = g * rcp(1 + exp2(g * -log2 e)) on the hardware exp2 / rcp (mxmoe_moe_silu_mul_quant's).
 *            act fp16 [T * topk][N]; act_shared fp16 [T][N_shared] (row t).
 * mxmoe_moe_decode_down, for the same pairs and tokens, with the expert's kind2: the A row is act[p] (act_shared[t])
 *   quantised by the same rule (amax over the whole row of N / N_shared elements; every workgroup re-derives the rows
 *   it needs), dot and v(r) as above on b2 / sb2: y[p][h] = v(h), fp16 [T * topk][H]; ys[t][h], fp16 [T][H].
 * Safety: nothing is indexed by an id. An id outside [0, E) is matched by no workgroup: its pair's act / y rows keep
 * what they held, and MXMOE_DECODE_BAD_ID is OR-ed into *status (DEVICE int32, optional). Rows past T are never
 * written. NaN inputs: unspecified.
 * Limits: 1 <= T <= MXMOE_DECODE_MAX_T (T == 0: OK, no launch), E >= 1, 1 <= topk <= min(E, 16); H, N and (with_shared)
 * N_shared multiples of 128 and <= 16384; hidden, act, act_shared, y, ys and every B 16-byte aligned, topk_ids 4-byte;
 * layout and dtype known. Anything else: MXMOE_GG_ERR_INVALID (an unknown kind bit: MXMOE_GG_ERR_UNSUPPORTED), checked
 * before any HIP call and reported under the entry point's name. Each entry is one launch on `stream`, no allocation,
 * no synchronisation: graph-capturable. */
enum { MXMOE_DECODE_MAX_T = 16 };
enum { MXMOE_DECODE_FP16 = 0, MXMOE_DECODE_W8A8 = 1, MXMOE_DECODE_W4A4 = 2,
       MXMOE_DECODE_W4A16_MX = 3 /* the _ex and _wo entries only */,
       /* the _wo entries only: kind = 4 + (w_bits == 8) + 2 * (gsize == 128) + 4 * asym */
       MXMOE_DECODE_W4A16 = 4, MXMOE_DECODE_W8A16 = 5, MXMOE_DECODE_W4A16_G128 = 6, MXMOE_DECODE_W8A16_G128 = 7,
       MXMOE_DECODE_W4A16_ASYM = 8, MXMOE_DECODE_W8A16_ASYM = 9, MXMOE_DECODE_W4A16_G128_ASYM = 10,
       MXMOE_DECODE_W8A16_G128_ASYM = 11 };                                    /* per linear */
enum { MXMOE_DECODE_GU_PLAIN = 0, MXMOE_DECODE_GU_INTERLEAVED = 1 };
enum { MXMOE_DECODE_BAD_ID = 1, MXMOE_DECODE_BAD_KIND = 2 };                   /* bits of *status */
typedef struct mxmoe_moe_decode_expert {
  const void* b1;  /* gate_up B [2N][K bits / 8]           */
  const void* sb1; /* its fp16 scale_b [2N] (FP16: NULL; W4A16_MX: the e8m0 rows, uint8 [2N][16 ceil(K / 512)]) */
  const void* b2;  /* down B [H][N bits / 8]               */
  const void* sb2; /* its fp16 scale_b [H] (FP16: NULL; W4A16_MX: the e8m0 rows, uint8 [H][16 ceil(N / 512)])    */
  int32_t kind1, kind2;
} mxmoe_moe_decode_expert;
int mxmoe_moe_decode_gate_up(int dtype, const void* hidden, int64_t T, int topk, int E, int with_shared,
                             const int32_t* topk_ids, const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H,
                             int N, int N_shared, int layout, void* act, void* act_shared, int32_t* status, void* stream);
int mxmoe_moe_decode_down(int64_t T, int topk, int E, int with_shared, const int32_t* topk_ids,
                          const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                          const void* act, const void* act_shared, void* y, void* ys, int32_t* status, void* stream);

/* The decode forward for gpt-oss layers (added to ABI 7 without a version bump): the two entries above with one more
 * kind and, in gate_up, the biases and the gated activation of an mxmoe_moe_glu. Arguments, pair order, safety and
 * limits are those of mxmoe_moe_decode_gate_up / mxmoe_moe_decode_down; the expert record is unchanged. The first two
 * entries keep their kernels and refuse kind bit 3; these run kernels of their own.
 *   MXMOE_DECODE_W4A16_MX (w4a16_g32_sym_MXFP4): B the canonical e2m1 codes, uint8 [rows][K / 2] (element 2i the low
 *            nibble of byte i); sb1 / sb2 the e8m0 scale bytes in the device layout of include/mxmoe_gg.h, uint8
 *            [rows][16 ceil(K / 512)], pads 127 — byte for byte the GroupGEMM's operands of that type, used in place.
 *            K % 64 == 0 (the widths' multiple of 128 gives it).
 *   A row    x (gate_up: hidden[t], bf16 converted as above; down: act[p]) as fp16: not quantised.
 *   b[r][k]  = fp16(e2m1(code) * 2^(byte - 127)) by v_cvt_scalef32_pk_f16_fp4 on the f32 byte << 23, the GroupGEMM's
 *            convert: the same fp16 value as there for every scale byte (exact for bytes 104..140, include/mxmoe_gg.h).
 *   v(r)     = fp16_rn(sum_k f32(x[k]) * f32(b[r][k])), accumulated in f32 (fma; the order of the sum is the
 *            kernel's) — the contract of the GroupGEMM's w4a16_g32_sym_MXFP4 tile.
 * mxmoe_moe_decode_gate_up_ex, every kind: with g = v(gate row of n), u = v(up row of n) (fp16), expert e of the pair
 *   (the shared expert: bias_shared) and bias rows [bg | bu] = glu->bias_routed[e] (fp16 [E][2N], indexed by column
 *   whatever the weight layout), mxmoe_moe_glu_quant's arithmetic in f32:
 *     g' = f32 g + f32 bg[n], u' = f32 u + f32 bu[n]  (one IEEE add each; a NULL bias: no add),
 *     MXMOE_GLU_SILU: a = g' * rcp(1 + exp2(g' * -log2 e)) * u';  MXMOE_GLU_SWIGLU_CLAMP: gc = min(g', limit),
 *     uc = min(max(u', -limit), limit), a = (gc * rcp(1 + exp2(gc * c))) * (uc + 1.0f), c = -(alpha * 1.4426950408889634f)
 *     computed once on the host in f32;  act[p][n] = fp16_rn(a), the f32 product rounded on its own.
 *   The bias row is that of the workgroup's own expert, never indexed by an id. glu == NULL, or SILU with both biases
 *   NULL: mxmoe_moe_decode_gate_up's output byte for byte.
 * mxmoe_moe_decode_down_ex: y[p][h] = v(h) with kind2 on b2 / sb2. A down bias is not added here: it stays in the
 *   combine (mxmoe_moe_combine_bias / _dt with inv_slot[p] = p and sorted_expert[p] = topk_ids[p]: an id outside
 *   [0, E) gets no bias there).
 * Refusals, before any HIP call and under the entry's name: everything the first two entries check; glu's checks
 * as in mxmoe_moe_glu_quant (an unknown act, a non-finite alpha, a limit that is not finite and > 0, a bias that is
 * not 16-byte aligned) and bias_shared without with_shared: MXMOE_GG_ERR_INVALID; a kind bit >= 4:
 * MXMOE_GG_ERR_UNSUPPORTED. One launch each, no allocation, no synchronisation: graph-capturable. */
int mxmoe_moe_decode_gate_up_ex(const mxmoe_moe_glu* glu, int dtype, const void* hidden, int64_t T, int topk, int E,
                                int with_shared, const int32_t* topk_ids, const mxmoe_moe_decode_expert* experts,
                                uint32_t kind_mask, int H, int N, int N_shared, int layout, void* act, void* act_shared,
                                int32_t* status, void* stream);
int mxmoe_moe_decode_down_ex(int64_t T, int topk, int E, int with_shared, const int32_t* topk_ids,
                             const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                             const void* act, const void* act_shared, void* y, void* ys, int32_t* status, void* stream);

/* The decode forward with integer weight-only experts (added to ABI 7 without a version bump): the two _ex entries
 * with eight more kinds, w4a16 and w8a16, per-channel or g128, sym or asym — the reference's small-batch scheme
 * w4a16 + w8a8 among them. Arguments (glu included), pair order, safety, limits and refusals are those of
 * mxmoe_moe_decode_gate_up_ex / mxmoe_moe_decode_down_ex; the expert record is unchanged (40 bytes). The four entries
 * above keep their kernels and their mask checks; these run kernels of their own and take kinds 0 to 11.
 *   kinds    the record has no room for a group size or a symmetry flag, so the kind carries them:
 *            kind = 4 + (w_bits == 8) + 2 * (gsize == 128) + 4 * asym, MXMOE_DECODE_W4A16 .. _W8A16_G128_ASYM (4..11).
 *   b1 / b2  mxmoe_gg_repack_weightonly's layout (include/mxmoe_gg.h), uint8 [rows][K bits / 8], used in place: per
 *            64-K segment, K value 32 kc + 8 g + e at element position 16 g + 8 kc + e; 4-bit: one 32-bit word per
 *            (g, kc), codes 2q, 2q + 1 at bits 4q and 16 + 4q. Sym codes are stored with the offset 2^(bits-1) - 1.
 *   sb1 / sb2 the fp16 scale buffer in the reference's permute_scale layout, used in place: sym [G][rows], asym
 *            [G][rows][2] (scale, zp); G = 1 per-channel, K / 128 for g128; rows the weight's own row count (2N, or
 *            2 N_shared, for gate_up; H for down). 2-byte aligned. With MXMOE_DECODE_GU_INTERLEAVED the scales follow
 *            their rows.
 *   A row    x (gate_up: hidden[t], bf16 converted as mxmoe_moe_gather_quant does; down: act[p]) as fp16: not quantised.
 *   b[r][k]  = fp16(fma(u - off, scale, zp)), one fp16 rounding (v_pk_fma_f16), scale / zp those of row r and of group
 *            k / 128 (g128); off = 2^(bits-1) - 1 for sym codes, 0 for asym; zp = +0 for sym; u - off exact (0x6400 | u
 *            as fp16, then an exact v_pk_add_f16): the GroupGEMM's weight-only value (DESIGN.md §4 "Weight-only WxA16").
 *   v(r)     = fp16_rn(sum_k f32(x[k]) * f32(b[r][k])), accumulated in f32 (v_fma_mix_f32; the order of the sum is the
 *            kernel's), as the FP16 and W4A16_MX kinds.
 *   The gate_up epilogue (SiLU, or glu's biases and clamp) and everything behind it are the _ex entries'. On kinds 0..3
 *   the outputs are those entries' byte for byte.
 * Refusals, before any HIP call and under these entries' names: everything the _ex entries check; a kind bit >= 12:
 * MXMOE_GG_ERR_UNSUPPORTED. A record whose kind is outside the mask: MXMOE_DECODE_BAD_KIND and nothing written. Scale
 * and zp values that are not finite: unspecified. One launch each, no allocation, no synchronisation: graph-capturable. */
int mxmoe_moe_decode_gate_up_wo(const mxmoe_moe_glu* glu, int dtype, const void* hidden, int64_t T, int topk, int E,
                                int with_shared, const int32_t* topk_ids, const mxmoe_moe_decode_expert* experts,
                                uint32_t kind_mask, int H, int N, int N_shared, int layout, void* act, void* act_shared,
                                int32_t* status, void* stream);
int mxmoe_moe_decode_down_wo(int64_t T, int topk, int E, int with_shared, const int32_t* topk_ids,
                             const mxmoe_moe_decode_expert* experts, uint32_t kind_mask, int H, int N, int N_shared,
                             const void* act, const void* act_shared, void* y, void* ys, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MXMOE_MOE_H_ */
