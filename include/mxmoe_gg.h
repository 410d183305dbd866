/*
 * mxmoe_gg.h — C-ABI of the MI355X (gfx950) mixed-precision MoE GroupGEMM.
 *
 * One call computes P independent problems  C_i[M_i,N_i] = A_i[M_i,K_i] . B_i[N_i,K_i]^T
 * (RCR layout: A row-major, B "column-major" = [N][K] with K contiguous, C row-major fp16),
 * each problem with its own quantisation type:
 *
 *   fp16 : A,B fp16, fp32 accumulate, C = fp16_rn(acc)
 *   w8a8 : A,B int8  per-channel sym (gsize -1), exact int32 accumulate,
 *          C = fp16_rn(0.f + f32(acc) * f32(fp16_rn(sa[m] * sb[n])))
 *   w4a4 : A,B int4  per-channel sym (gsize -1), same epilogue
 *   w4a4_g128, WxA16 weight-only: see DESIGN.md §4 / mxmoe_gg_repack_weightonly below
 *   w8a8_g-1_sym_E4M3 (fmt MXMOE_GG_FMT_E4M3): A,B OCP fp8 e4m3 codes (one byte each, pack_wxax
 *          8-bit byte order), per-channel fp16 scales, f32 accumulate (products exact, sum order
 *          unspecified), C = fp16_rn(0.f + acc * f32(fp16_rn(sa[m] * sb[n])))
 *   bf16 (fmt MXMOE_GG_FMT_BF16): A,B bf16, fp32 accumulate, C = fp16_rn(acc) (C is fp16 for every
 *          type, as the reference's `half** ptr_Cs`)
 *   w4a4_g32_sym_MXFP4 (fmt MXMOE_GG_FMT_MXFP4): A,B OCP MXFP4 (e2m1 codes, e8m0 scale per 32-K block),
 *          f32 accumulate on the block-scaled fp4 MFMA, C = fp16_rn(acc); layouts at MXMOE_GG_FMT_MXFP4
 *
 * Data layout is byte-identical to the reference bench (SeaCatComplexes/MxMoE):
 *   - packed A/B words follow pack_wxax        (mxmoe/kernels/src/include/quantize.cuh:425-475)
 *   - QParams {int2 qbits(x=a_bits,y=w_bits); int gsize; bool sym}  (quantize.cuh:14-25)
 *   - scale_a[M], scale_b[N] fp16 per problem  (test.cu:301-313, 522-523)
 *   - epilogue arithmetic                      (mm_tile.cuh:469-496, 610-662; cta_gemm.cuh:599-607)
 *
 * Conventions (differences from the reference ABI):
 *   - every entry point returns an int status (MXMOE_GG_OK == 0); nothing calls exit();
 *     mxmoe_gg_last_error() returns a thread-local message for the last failure;
 *   - the caller owns all device memory, including the workspace; no call allocates
 *     device memory except the reference-compatible shim groupgemm_mxmoe();
 *   - explicit stream argument (hipStream_t passed as void*); mxmoe_gg_launch() does no host
 *     synchronisation and no allocation, so it can be captured into a hipGraph;
 *   - mutable global state: the thread-local error string, the reference shim's per-device
 *     workspaces (mxmoe_gg_release_shim_workspaces) and mxmoe_gg_rebind's per-workspace plan keys
 *     (mutex-guarded, host memory only).
 */
#ifndef MXMOE_GG_H_
#define MXMOE_GG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MXMOE_GG_ABI_VERSION 7  /* 5: QParams padding ignored, groupgemm_mxmoe_fmt; 6: MXMOE_GG_EPI_SILU_MUL;
                                 * 7: mxmoe_gg_variant_caps */

enum {
  MXMOE_GG_OK = 0,
  MXMOE_GG_ERR_INVALID = 1,     /* bad argument / shape / alignment */
  MXMOE_GG_ERR_UNSUPPORTED = 2, /* quantisation type or variant not compiled */
  MXMOE_GG_ERR_WORKSPACE = 3,   /* workspace too small */
  MXMOE_GG_ERR_HIP = 4          /* a HIP runtime call failed */
};

/* Element format of a problem's A / B beyond the bit widths (the reference's QConfig USE_FP flag,
 * tile_config.py:192, and its MMA_BF16_FP32 / MMA_E4M3_K32 strategies, tile_config.py:87-106). */
enum {
  MXMOE_GG_FMT_DEFAULT = 0, /* fp16 for 16-bit operands, two's-complement integers otherwise */
  MXMOE_GG_FMT_E4M3 = 1,    /* w8a8_g-1_sym_E4M3: OCP fp8 e4m3 codes                         */
  MXMOE_GG_FMT_BF16 = 2,    /* bf16: 16-bit operands are bfloat16                              */
  /* 3: fp6 images of int4 codes (tools-only lab library) */
  MXMOE_GG_FMT_MXFP4 = 4,   /* w4a4_g32_sym_MXFP4 and w4a16_g32_sym_MXFP4: OCP MXFP4, e2m1 codes + e8m0
                             * block scales (a_bits selects: 4 = both operands, 16 = fp16 A, weights only) */
  MXMOE_GG_FMT_MXFP8 = 5    /* w4a8_g32_sym_MXFP8: OCP MXFP8 (e4m3) activations on MXFP4 weights; w_bits = 8
                             * under this format is reserved (a later w8a8_g32_sym_MXFP8) and UNSUPPORTED */
};

/* MXFP4 operands (fmt MXMOE_GG_FMT_MXFP4; a_bits = w_bits = 4, gsize = 32, sym; K % 32 == 0).
 *   codes : A uint8 [M][K/2], B uint8 [N][K/2] (lda / ldb in 16-bit words as for every type). Element
 *           2i of a row is the low nibble of byte i, element 2i+1 the high nibble; a nibble is the OCP
 *           e2m1 code: bit 3 the sign, bits 2..0 an index into {0, .5, 1, 1.5, 2, 3, 4, 6}.
 *   scales: one OCP e8m0 byte per 32-element block, value 2^(code - 127), code 255 = NaN.
 *           The CANONICAL layout (what the Python helpers quant_mxfp4 / dequant_mxfp4 speak) is
 *           uint8 [rows][K/32]. scale_a / scale_b take the DEVICE layout (pack_mxfp4_scales):
 *           uint8 [rows][G * 16] with G = ceil(K/32 / 16), 4-byte aligned; every 16-byte group of a row
 *           is the canonical group transposed 4 x 4, dev[16 t + 4 g + i] = canon[16 t + 4 i + g]
 *           (i, g < 4), and bytes for blocks past K/32 hold 127 (2^0) — never 255: the zero-filled
 *           codes of a K tail times a NaN scale would poison the sum. Dword g of group t then holds,
 *           for K group g of the MFMA (K = [32 g, 32 g + 32) of each 128), the scales of four
 *           consecutive MFMAs: two 128-byte (K = 256) stages.
 *   result: C[m][n] = fp16_rn(sum over blocks b of 2^(sa[m][b]-127) 2^(sb[n][b]-127)
 *           sum_{k in b} a[m][k] b[n][k]), accumulated in f32 by the block-scaled MFMA (summation order
 *           unspecified); no per-channel fp16 scales. Runs on the v2x variant only (AUTO picks it for
 *           every call that holds an MXFP4 problem); no SiLU epilogue. */

/* Weight-only MXFP4 (fmt MXMOE_GG_FMT_MXFP4 with a_bits = 16, w_bits = 4, gsize = 32, sym: w4a16_g32_sym_MXFP4;
 * plan-info qtype_mask bit 11). fp16 activations on MXFP4 weights, on the fp16 MFMA.
 *   A      : fp16 [M][K]; scale_a unused (may be NULL).
 *   B      : uint8 [N][K/2] CANONICAL e2m1 codes (element 2i the low nibble of byte i) and scale_b the e8m0
 *            bytes in the DEVICE layout above ([N][16 ceil(K/32 / 16)], 4-byte aligned, pads 127): byte for
 *            byte the B operand of a w4a4_g32_sym_MXFP4 problem, so one copy of a layer's MXFP4 weights
 *            serves both types. NOT the K-interleaved mxmoe_gg_repack_weightonly layout: there is no repack.
 *   limits : K % 64 == 0 (the weight-only stage), N % 8 == 0, K <= 2^20; lda / ldb / ldc as for the other
 *            weight-only types.
 *   result : b[n][k] = e2m1(code) * 2^(sb[n][k/32] - 127) as an fp16 value (the hardware convert
 *            v_cvt_scalef32_pk_f16_fp4 with the f32 scale `byte << 23`); C[m][n] = fp16_rn(sum_k f32(A[m][k])
 *            * f32(b[n][k])), accumulated in f32 by v_mfma_f32_16x16x32_f16 (summation order unspecified).
 *            b is exact for every code whenever the scale byte is in [104, 140]. Outside that range the
 *            result is RECORDED, NOT SPECIFIED: bytes 1..103 underflow (values below fp16's
 *            subnormal grid round to it or to zero), byte 0 is taken as a zero scale (b = +-0, not 2^-127),
 *            bytes 141..254 overflow to +-inf for the larger codes and byte 255 gives inf / NaN — an inf
 *            times a zero of A is NaN, so such a scale poisons its whole output column and no other.
 *            quantize.quant_mxfp4 of fp16 weights yields bytes 101..140, 0 (all-zero block) or 255.
 *   runs on: the small-batch kernel wo3 (AUTO picks it under the weight-only rule: mean M <= 512) and v2x;
 *            a call that also holds a w4a4_g32_sym_MXFP4 problem stays on v2x. MXMOE_GG_EPI_SILU_MUL: on wo3
 *            only, as for the other weight-only types (scale_b rows permuted with the B rows). */

/* MXFP8 activations on MXFP4 weights (fmt MXMOE_GG_FMT_MXFP8 with a_bits = 8, w_bits = 4, gsize = 32, sym:
 * w4a8_g32_sym_MXFP8; plan-info qtype_mask bit 12). One block-scaled MFMA with a format per operand
 * (e4m3 x e2m1), no dequantisation.
 *   A      : uint8 [M][K] OCP e4m3 codes (torch.float8_e4m3fn's bit patterns) in logical K order, lda in 16-bit
 *            words; scale_a one e8m0 byte per 32 elements in the DEVICE layout above ([M][16 ceil(K/32 / 16)],
 *            4-byte aligned, pads 127) — the layout is indexed by (K = 128 MFMA, K group of 32), which means the
 *            same for an 8-bit operand.
 *   B      : uint8 [N][K/2] canonical e2m1 codes and scale_b in the device layout: byte for byte the B operand
 *            of a w4a4_g32_sym_MXFP4 problem (no repack, no second layout).
 *   limits : K % 32 == 0, N % 8 == 0; alignment as for w4a4_g32_sym_MXFP4.
 *   result : C[m][n] = fp16_rn(sum over blocks b of 2^(sa[m][b]-127) 2^(sb[n][b]-127) sum_{k in b} e4m3(a[m][k])
 *            e2m1(b[n][k])), accumulated in f32 by the block-scaled MFMA (summation order unspecified); no
 *            per-channel fp16 scales. A scale byte 255 is NaN and poisons its output row / column only.
 *   runs on: v2x (256 / 128-row tiles, ring of K = 128 stages) and the small-batch kernel wo3 (64 x 128 tiles;
 *            AUTO picks it below a weighted mean M of its own); a call that also holds a
 *            w4a4_g32_sym_MXFP4 problem stays on v2x. MXMOE_GG_EPI_SILU_MUL is accepted on both (the fp16
 *            body's epilogue path: f32 accumulators rounded to fp16, then the SiLU arithmetic below). */

/* Epilogue flag, OR-ed into mxmoe_gg_problem.fmt (fp16, w8a8_g-1_sym, w4a4_g-1_sym and w4a8_g32_sym_MXFP8
 * problems on the v2x, v3 (not the MX type) and wo3 variants; weight-only WxA16 problems on wo3, whose scale_b is permuted with the rows;
 * no reference counterpart — it fuses the MoE layer's silu_mul_then_quant
 * activation, ref_bind.cu:595-757, into the gate_up GroupGEMM). B holds N = 2 Nh rows interleaved
 * in 16-row blocks: rows [32 b, 32 b + 16) are gate rows [16 b, 16 b + 16) and rows
 * [32 b + 16, 32 b + 32) the matching up rows (scale_b permuted alike; N % 32 == 0). C is [M][Nh]
 * (ldc >= Nh, 0 = Nh): C[m][n] = fp16_rn(silu(f32 g) * f32 u) with g, u the fp16 outputs the call
 * would have written for gate column n and up column n, silu(g) = g * rcp(1 + exp2(-g log2 e)) —
 * the arithmetic of mxmoe_moe_silu_mul_quant, bit for bit. */
#define MXMOE_GG_EPI_SILU_MUL 0x100

/* Same memory layout as the reference's mxmoe::QParams (quantize.cuh:14-25):
 * int2 qbits {x = a_bits, y = w_bits}; int gsize; bool sym; padded to 16 bytes, 8-byte aligned.
 * The three bytes after `sym` are the reference's padding: its QParams constructors
 * (quantize.cuh:19-20) leave them uninitialised, so nothing in this library reads them. Operand
 * formats other than the default travel in mxmoe_gg_problem.fmt or groupgemm_mxmoe_fmt's array. */
typedef struct mxmoe_qparams {
  int32_t a_bits;
  int32_t w_bits;
  int32_t gsize;
  uint8_t sym;
  uint8_t pad_[3];
} __attribute__((aligned(8))) mxmoe_qparams;

/* Same memory layout as CUDA/HIP dim3 (x = M, y = N, z = K), as used in registry.cuh:28-39. */
typedef struct mxmoe_dim3 {
  uint32_t x, y, z;
} mxmoe_dim3;

/* One GroupGEMM problem (host-side descriptor). Pointers are DEVICE pointers.
 * lda/ldb/ldc are row strides in 16-bit words (the reference's `half` unit); 0 = dense. */
typedef struct mxmoe_gg_problem {
  const void* A;       /* fp16 [M][K]  or packed [M][K*a_bits/16] words            */
  const void* B;       /* fp16 [N][K]  or packed [N][K*w_bits/16] words            */
  const void* scale_a; /* fp16 [M] (quantised problems only, else may be NULL)     */
  const void* scale_b; /* fp16 [N] (quantised problems only, else may be NULL)     */
  void* C;             /* fp16 [M][ldc]                                            */
  int32_t M, N, K;
  int32_t a_bits, w_bits, gsize, sym;
  int32_t fmt; /* MXMOE_GG_FMT_* */
  int64_t lda, ldb, ldc;
} mxmoe_gg_problem;

/* Result of planning: what mxmoe_gg_launch needs on the host side. */
typedef struct mxmoe_gg_plan_info {
  int32_t variant;
  int32_t problem_count;
  int32_t total_tiles;
  int32_t grid;
  int32_t block;
  int32_t lds_bytes;
  int32_t qtype_mask;      /* bit q set if a planned problem has quant type q (0 fp16, 1 w8a8, 2 w4a4,
                            * 3 w4a16, 4 w8a16, 5 w4a4_g128, 6 w2a16, 7 w8a8 E4M3, 8 bf16, 10 MXFP4, 11 weight-only MXFP4,
                            * 12 w4a8 MXFP8); bit 16:
                            * a weight-only problem carries MXMOE_GG_EPI_SILU_MUL (small-batch kernel);
                            * selects the kernel specialisation at launch */
  int32_t splitk_slabs;    /* 256-KiB partial-sum slabs the plan's split-K tiles use (0: no split) */
  int64_t workspace_bytes; /* bytes of the workspace actually used by the plan */
  void* workspace;         /* device workspace the plan was written to */
  uint64_t signature;      /* hash of the plan table and tile table (shapes, quant params, strides) */
  int32_t tile_slots;      /* entries of the device tile table (= grid, except for persistent variants,
                            * whose workgroups walk [k][grid]-ordered tile lists) */
  int32_t reserved;
} mxmoe_gg_plan_info;

int mxmoe_gg_abi_version(void);

/* Thread-local message describing the last failed call on this thread ("" if none). */
const char* mxmoe_gg_last_error(void);

/* Number of compiled kernel variants. */
int mxmoe_gg_variant_count(void);

/* The variant AUTO resolves to for long-K calls that are not w4a4-only (mxmoe_gg_resolve_variant). */
int mxmoe_gg_default_variant(void);

/* Writes a newline-separated description of every compiled variant into buf (truncated,
 * always NUL-terminated when n > 0). Line i describes variant i in the reference TileConfig
 * repr form per qcfg, e.g. "0 fused fp16=TileConfig(BM=128, BN=128, ...) w8a8_g-1_sym=...".
 * Returns the number of variants, or a negative status on error. */
int mxmoe_gg_list_variants(char* buf, size_t n);

/* Tile geometry of variant `variant` for a quantisation type (a_bits, w_bits):
 * writes BM, BN, K-bytes-per-stage and threads per workgroup. */
int mxmoe_gg_variant_tile(int variant, int a_bits, int w_bits, int32_t* bm, int32_t* bn, int32_t* bk_bytes,
                          int32_t* threads);

/* Capability bits of a compiled variant (mxmoe_gg_variant_caps). */
#define MXMOE_GG_CAP_SILU_MUL 1u /* plans problems carrying MXMOE_GG_EPI_SILU_MUL (the fused SiLU epilogue) */

/* Capabilities of variant `variant` (an index, not AUTO): *caps = OR of MXMOE_GG_CAP_* bits. Lets a
 * caller ask whether the kernel AUTO resolved to supports an epilogue before planning with it
 * (the MoE layer routes small-batch gate_up calls, whose kernel has no SiLU epilogue, through the
 * interleaved SiLU pass). No reference counterpart: the reference compiles one epilogue per kernel. */
int mxmoe_gg_variant_caps(int variant, uint32_t* caps);

/* Pass as `variant` to mxmoe_gg_workspace_size / _plan / _run: the library picks the variant
 * from the quant types present (the plan info records the concrete one). groupgemm_mxmoe uses it. */
#define MXMOE_GG_VARIANT_AUTO (-1)

/* The concrete variant `variant` (MXMOE_GG_VARIANT_AUTO or an index) resolves to for these
 * problems, written to *out. Host only (no GPU). AUTO: small-batch calls (mean rows per weight
 * byte under the DESIGN.md §4 cuts) -> the 3-WG/CU 64-row kernel (wo3); w4a4-only sets -> the
 * 256x128 2-WG/CU kernel (unless the plan needs split-K); otherwise mxmoe_gg_default_variant(). */
int mxmoe_gg_resolve_variant(const mxmoe_gg_problem* problems, int problem_count, int variant, int* out);

/* Device workspace bytes the plan of these problems needs with this variant
 * (plan table + pointer arrays + tile table). Validates the problems like mxmoe_gg_plan. */
int mxmoe_gg_workspace_size(const mxmoe_gg_problem* problems, int problem_count, int variant, size_t* bytes);

/* Validate problems, build the tile table and upload it into the workspace (hipMemcpyAsync on
 * `stream`, then a stream synchronisation: planning is done once, outside the hot loop).
 * The host problem array may be freed after return. */
int mxmoe_gg_plan(const mxmoe_gg_problem* problems, int problem_count, int variant, void* workspace,
                  size_t workspace_bytes, void* stream, mxmoe_gg_plan_info* info);

/* Re-point a plan at new operand buffers: `problems` must describe the same shapes, quant params
 * and strides as the planned call (checked through the plan signature, MXMOE_GG_ERR_INVALID
 * otherwise); only the 5 pointer columns of the workspace are uploaded (one copy on `stream` and a
 * stream synchronisation). The pointers get mxmoe_gg_plan's NULL / alignment checks.
 * BLOCKING and NOT graph-capturable (unlike mxmoe_gg_launch): the call ends with
 * hipStreamSynchronize(stream). The library remembers, per workspace, a key over the planned
 * shapes / quant params / strides: a rebind with the same key skips the host planner (pointers are
 * still checked); otherwise the planner re-runs to compare the plan signature. A plan must be
 * rebound on the stream its launches run on: the upload is ordered behind that stream's work only. */
int mxmoe_gg_rebind(const mxmoe_gg_problem* problems, int problem_count, const mxmoe_gg_plan_info* info, void* stream);

/* Drop mxmoe_gg_rebind's remembered plan key for `workspace` (call before freeing a workspace that
 * held a plan; host only, no device access). A later plan into the same address re-registers it.
 * Returns MXMOE_GG_OK whether or not an entry existed. */
int mxmoe_gg_forget_workspace(const void* workspace);

/* Launch a planned GroupGEMM on `stream`. No allocation, no synchronisation. */
int mxmoe_gg_launch(const mxmoe_gg_plan_info* info, void* stream);

/* plan + launch. */
int mxmoe_gg_run(const mxmoe_gg_problem* problems, int problem_count, int variant, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Drop-in for the reference registry FuncType (mxmoe/kernels/src/include/registry.cuh:28-39;
 * generated host API groupgemm_hz_fused_<i>, kernel_sketch.py:25-46, 82-145).
 * ptr_* / problem_sizes / qbits_list are DEVICE arrays, h_problem_sizes / h_qbits_list host
 * copies; ptr_Ds and the ld* arrays are accepted and ignored exactly as in the reference.
 * Runs the AUTO variant on the legacy default stream. Unlike the reference it reports errors
 * through the return value (and mxmoe_gg_last_error) instead of exit(), and validates the gathered
 * device pointers (NULL, 16-B alignment) like mxmoe_gg_plan. It keeps one workspace and one pinned
 * staging buffer per device (grown on demand, one host synchronisation per call); release them with
 * mxmoe_gg_release_shim_workspaces(). */
int groupgemm_mxmoe(void** ptr_As, void** ptr_Bs, void** ptr_scale_a, void** ptr_scale_b, void** ptr_Cs,
                    void** ptr_Ds, int64_t* ldas, int64_t* ldbs, int64_t* ldcs, int64_t* ldds,
                    mxmoe_dim3* problem_sizes, mxmoe_dim3* h_problem_sizes, mxmoe_qparams* qbits_list,
                    mxmoe_qparams* h_qbits_list, int problem_count);

/* groupgemm_mxmoe with an explicit operand format per problem (h_fmts[i] = MXMOE_GG_FMT_*, host
 * array; NULL = MXMOE_GG_FMT_DEFAULT for every problem, i.e. exactly groupgemm_mxmoe). The opt-in
 * for the E4M3 / bf16 strategies, which the reference's QParams cannot express. */
int groupgemm_mxmoe_fmt(void** ptr_As, void** ptr_Bs, void** ptr_scale_a, void** ptr_scale_b, void** ptr_Cs,
                        void** ptr_Ds, int64_t* ldas, int64_t* ldbs, int64_t* ldcs, int64_t* ldds,
                        mxmoe_dim3* problem_sizes, mxmoe_dim3* h_problem_sizes, mxmoe_qparams* qbits_list,
                        mxmoe_qparams* h_qbits_list, int problem_count, const int32_t* h_fmts);

/* Free groupgemm_mxmoe's per-device workspaces and staging buffers (waits for each device to be
 * idle first). Safe to call at any time; the next shim call re-allocates. */
int mxmoe_gg_release_shim_workspaces(void);

/* Weight-only (WxA16) B, host-side and once per weight: converts the reference's packed words
 * (pack_weightonly after permute_weight(Row), quantize.cuh:318-421: uint16 [N / (16/w_bits)][K],
 * sym codes stored with the +2^(w_bits-1)-1 offset) into the layout the kernels read:
 * uint8 [N][K * w_bits / 8], per 64-K segment of a row the K values {kc*32 + g*8 + e} at element
 * position g*16 + kc*8 + e (kc < 2, g < 4, e < 8); 4-bit: e at nibble (e >> 1) | (e & 1) << 2 of
 * the unit's 32-bit word (codes 2q, 2q+1 at bits 4q and 16 + 4q), low nibble first; 2-bit: the
 * unit (g) of a segment's 16-B row is one little-endian 32-bit word at byte 4 g holding both K
 * halves, code (kc, e) at bit 16 (e & 1) + 2 (4 kc + e / 2). Code values are
 * unchanged. Needs N % (8 * 16 / w_bits) == 0 and K % 64 == 0; w_bits 2, 4 or 8. The scale / zero
 * buffer is used as the reference lays it out (permute_scale: [K/gsize][N] sym, [K/gsize][N][2]
 * scale/zp pairs asym). */
int mxmoe_gg_repack_weightonly(const uint16_t* ref_words, int N, int K, int w_bits, uint8_t* out);

/* Diagnostics (no reference counterpart): the tile timeline the "abl_v2s_trace" variant records,
 * 4 uint64 per block {start, mainloop end, end after its stores drained (s_memrealtime, 100 MHz
 * ticks), K stages << 48 | height class << 40 | qtype << 36 | XCC_ID << 32 | HW_ID} for the first
 * 32768 blocks of the last traced launch. Copies
 * min(bytes, 1 MiB) into host memory `dst` (synchronous); reset != 0 then zeroes the record. */
int mxmoe_gg_debug_trace(void* dst, size_t bytes, int reset);

/* Diagnostics (no reference counterpart): the host tile table mxmoe_gg_plan would upload, without
 * touching a device — 8 int32 per workgroup slot {table row (-1 = empty slot), m0, n0, class
 * (bits 8-15 split-K slice, 16-23 slices), first K stage, end K stage, split-K slab, split-K group},
 * blockIdx order (XCD x runs slots x, x + 8, ...); `rows` (optional, problem_count int32) receives
 * the caller's problem index of every table row. Writes min(*slots, needed) slots and sets *slots
 * to the number needed. */
int mxmoe_gg_plan_tiles(const mxmoe_gg_problem* problems, int problem_count, int variant, int32_t* tiles,
                        int32_t* rows, int* slots);

/* ---- Device planning: a fixed-capacity plan whose row counts live in device memory ("Device
 * planning / graph forward"). No reference counterpart: the reference plans on the host every call.
 *
 * mxmoe_gg_plan_dynamic runs once, on the host. problems[i].M is the CAPACITY of problem i, A / scale_a / C are
 * BASE pointers; the problems listed in joint_idx (distinct indices: a MoE layer's routed experts) also share the
 * bound sum rows <= rows_total. Each launch then reads one mxmoe_gg_dyn_row per problem from device memory:
 * a small planner kernel turns the rows into the plan table's M, the A / scale_a / C pointer columns and the
 * tile table, and the variant's unchanged GEMM kernel runs at the fixed grid `tile_slots` (unused slots exit at
 * once). Nothing in a launch depends on the host, so it can be captured into a hipGraph and replayed while the
 * row table changes.
 *   validation  as mxmoe_gg_plan (same errors from the same type tables), at the capacities.
 *   variant     v2x, v3 and wo3 (the product's kernels); persistent and lab variants: MXMOE_GG_ERR_UNSUPPORTED.
 *               MXMOE_GG_VARIANT_AUTO resolves ONCE, as mxmoe_gg_resolve_variant does for the balanced call: every
 *               joint problem with min(M, ceil(rows_total / n_joint)) rows, the others with their M. The kernel
 *               does not follow the routing afterwards.
 *   tiles       the host planner's rule (256-row tiles while more than 128 rows remain, then one 128-row or, for
 *               the types that take it, 64-row tile; wo3: 64-row tiles), tiles_n = cdiv(N, BN); problems in a
 *               fixed order, longest K stages first; no split-K (splitk_slabs = 0) and no XCD packing.
 *   capacity    info.grid = info.tile_slots = info.total_tiles = the capacity bound: with tn_i = tiles_n and
 *               bm the tile height, slots = sum_{i not joint} tn_i cdiv(M_i, bm)
 *                 + min( sum_{joint} tn_i cdiv(M_i, bm),
 *                        max over n in [1, min(n_joint, rows_total)] of
 *                          [sum of the n largest tn_i] + max tn_i * floor((rows_total - n) / bm) )
 *               (an expert with r > 0 rows has floor((r - 1) / bm) + 1 m-tiles; n counts the non-empty experts,
 *               whose first rows cannot also fill tiles; derivation at dyn_capacity_slots, mxmoe_amd/csrc/gg_dyn.h).
 *   extents     NULL, or per problem the bytes behind its A / scale_a / C base pointers. NULL: the problem's own
 *               capacity (M rows at its strides), so an offset can only move rows inside [base, base + M rows).
 *   safety      whatever the row table holds, no tile is planned outside the capacities: rows are clamped to
 *               [0, M_i] and the joint sum to rows_total (in problem order), an offset that is negative,
 *               misaligned (A / C 16 B, scale_a 2 B, block scales 4 B) or would put a row outside its extent
 *               gives the problem 0 rows, and tile emission stops at tile_slots. Each case ORs a
 *               MXMOE_GG_DYN_* bit into a status word in the workspace (mxmoe_gg_dynamic_status).
 * The workspace holds mxmoe_gg_dynamic_workspace_size bytes and belongs to this plan alone; mxmoe_gg_rebind
 * and mxmoe_gg_launch are not for dynamic plans. */
typedef struct mxmoe_gg_dyn_row {
  int32_t rows;     /* rows of the problem in this launch */
  int32_t reserved; /* 0 */
  int64_t a_off;    /* byte offsets added to the planned A / scale_a / C base pointers */
  int64_t sa_off;
  int64_t c_off;
} mxmoe_gg_dyn_row;

typedef struct mxmoe_gg_dyn_extent {
  int64_t a_bytes, sa_bytes, c_bytes; /* bytes addressable behind the A / scale_a / C base pointers */
} mxmoe_gg_dyn_extent;

enum {
  MXMOE_GG_DYN_ROWS_CLAMPED = 1,  /* a row count was negative or above its capacity */
  MXMOE_GG_DYN_JOINT_CLAMPED = 2, /* the joint problems' rows exceeded rows_total */
  MXMOE_GG_DYN_SLOTS_CUT = 4,     /* more tiles than tile_slots (cannot happen with admissible rows) */
  MXMOE_GG_DYN_BAD_OFFSET = 8     /* an offset was refused: that problem ran with 0 rows */
};

int mxmoe_gg_dynamic_workspace_size(const mxmoe_gg_problem* problems, int problem_count, int variant,
                                    const int32_t* joint_idx, int n_joint, int64_t rows_total, size_t* bytes);

int mxmoe_gg_plan_dynamic(const mxmoe_gg_problem* problems, int problem_count, int variant, const int32_t* joint_idx,
                          int n_joint, int64_t rows_total, const mxmoe_gg_dyn_extent* extents, void* workspace,
                          size_t workspace_bytes, void* stream, mxmoe_gg_plan_info* info);

/* Two launches on `stream` (the planner kernel, then the GEMM kernel at grid tile_slots); no allocation, no
 * synchronisation. dyn: DEVICE array of problem_count rows, read by the planner kernel when it runs. */
int mxmoe_gg_launch_dynamic(const mxmoe_gg_plan_info* info, const mxmoe_gg_dyn_row* dyn, void* stream);

/* The plan's status word (OR of MXMOE_GG_DYN_* since the plan or the last reset) into *status: synchronises
 * `stream`, so not for use under capture. reset != 0 zeroes the word afterwards. */
int mxmoe_gg_dynamic_status(const mxmoe_gg_plan_info* info, void* stream, int32_t* status, int reset);

/* Diagnostics: the tile table the planner kernel would write for the HOST row table `dyn`, computed on the
 * host by the very functions the kernel runs, without touching a device (pointers are not checked) — in
 * mxmoe_gg_plan_tiles' format, 8 int32 per slot, prob = the caller's problem index. slot_limit > 0 plans with
 * that many tile slots instead of the capacity bound. planned_rows (optional, problem_count int32) receives
 * the rows each problem was planned with, *status the MXMOE_GG_DYN_* bits. Writes min(*slots, tile_slots)
 * slots and sets *slots to tile_slots. */
int mxmoe_gg_dynamic_tiles(const mxmoe_gg_problem* problems, int problem_count, int variant, const int32_t* joint_idx,
                           int n_joint, int64_t rows_total, const mxmoe_gg_dyn_extent* extents,
                           const mxmoe_gg_dyn_row* dyn, int slot_limit, int32_t* tiles, int32_t* planned_rows,
                           int* slots, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* MXMOE_GG_H_ */
