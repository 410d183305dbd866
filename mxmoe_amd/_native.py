"""ctypes binding of ``libmxmoe_gg.so`` (the C-ABI in ``include/mxmoe_gg.h``).

The library is the product path: if it is missing or does not load, every GPU entry point raises
``NativeLibraryError`` — there is no CPU or PyTorch fallback anywhere in the package.

torch is imported before the library is opened so that ``libamdhip64.so.7`` resolves to the HIP
runtime torch already loaded (one runtime per process; streams and device pointers are shared).
"""
from __future__ import annotations

import atexit
import ctypes
import os
from pathlib import Path

import torch  # noqa: F401  (must precede the CDLL: binds the shared HIP runtime)

LIB_DIR = Path(__file__).resolve().parent / "lib"
LIB_PATH = LIB_DIR / "libmxmoe_gg.so"

MXMOE_GG_OK = 0
MXMOE_GG_ERR_INVALID = 1
MXMOE_GG_ERR_UNSUPPORTED = 2
MXMOE_GG_ERR_WORKSPACE = 3
MXMOE_GG_ERR_HIP = 4

# operand formats (MXMOE_GG_FMT_*): fp16 / integer, OCP fp8 e4m3, bfloat16; FMT_F6 (w4a4 as fp6
# images, gg_f6.h) is understood by the lab library only (measured slower)
FMT_DEFAULT, FMT_E4M3, FMT_BF16, FMT_F6 = 0, 1, 2, 3
FMT_MXFP4 = 4  # MXMOE_GG_FMT_MXFP4: w4a4_g32_sym_MXFP4 (OCP e2m1 codes, e8m0 scale per 32-K block)
FMT_MXFP8 = 5  # MXMOE_GG_FMT_MXFP8: w4a8_g32_sym_MXFP8 (OCP e4m3 activation codes on MXFP4 weights)
EPI_SILU_MUL = 0x100  # MXMOE_GG_EPI_SILU_MUL: fmt flag, C = silu(gate) * up (include/mxmoe_gg.h)


def f6_row_bytes(K: int) -> int:
    """Bytes of one fp6-image row of K int4 codes (96 per K-128 block; lab library)."""
    return (K + 127) // 128 * 96


class NativeLibraryError(RuntimeError):
    """libmxmoe_gg.so is missing or failed to load."""


class GGError(RuntimeError):
    """A C-ABI call returned a non-zero status."""

    def __init__(self, status: int, message: str):
        super().__init__(f"mxmoe_gg status {status}: {message}")
        self.status = status


class MxmoeQParams(ctypes.Structure):
    """Layout of the reference's mxmoe::QParams (quantize.cuh:14-25): int2 qbits; int gsize; bool sym."""

    _fields_ = [("a_bits", ctypes.c_int32), ("w_bits", ctypes.c_int32), ("gsize", ctypes.c_int32),
                ("sym", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 3)]


class MxmoeDim3(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("z", ctypes.c_uint32)]


class GGProblemC(ctypes.Structure):
    _fields_ = [
        ("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("scale_a", ctypes.c_void_p),
        ("scale_b", ctypes.c_void_p), ("C", ctypes.c_void_p),
        ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
        ("a_bits", ctypes.c_int32), ("w_bits", ctypes.c_int32), ("gsize", ctypes.c_int32),
        ("sym", ctypes.c_int32), ("fmt", ctypes.c_int32),
        ("lda", ctypes.c_int64), ("ldb", ctypes.c_int64), ("ldc", ctypes.c_int64),
    ]


VARIANT_AUTO = -1  # MXMOE_GG_VARIANT_AUTO
CAP_SILU_MUL = 1  # MXMOE_GG_CAP_SILU_MUL (mxmoe_gg_variant_caps)
ABI_VERSION = 7  # MXMOE_GG_ABI_VERSION this binding is written for (include/mxmoe_gg.h)


class GGPlanInfo(ctypes.Structure):
    _fields_ = [
        ("variant", ctypes.c_int32), ("problem_count", ctypes.c_int32), ("total_tiles", ctypes.c_int32),
        ("grid", ctypes.c_int32), ("block", ctypes.c_int32), ("lds_bytes", ctypes.c_int32),
        ("qtype_mask", ctypes.c_int32), ("splitk_slabs", ctypes.c_int32), ("workspace_bytes", ctypes.c_int64), ("workspace", ctypes.c_void_p),
        ("signature", ctypes.c_uint64), ("tile_slots", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


# every symbol include/mxmoe_gg.h declares (tests check the .so exports exactly these)
EXPORTED_SYMBOLS = (
    "mxmoe_gg_abi_version", "mxmoe_gg_last_error", "mxmoe_gg_variant_count", "mxmoe_gg_default_variant",
    "mxmoe_gg_list_variants",
    "mxmoe_gg_variant_tile", "mxmoe_gg_variant_caps", "mxmoe_gg_resolve_variant", "mxmoe_gg_workspace_size", "mxmoe_gg_plan", "mxmoe_gg_rebind", "mxmoe_gg_forget_workspace", "mxmoe_gg_launch", "mxmoe_gg_run",
    "groupgemm_mxmoe", "groupgemm_mxmoe_fmt", "mxmoe_gg_release_shim_workspaces", "mxmoe_gg_repack_weightonly", "mxmoe_gg_debug_trace",
    "mxmoe_gg_plan_tiles",
    # device planning (fixed-capacity plans: DESIGN.md §4)
    "mxmoe_gg_dynamic_workspace_size", "mxmoe_gg_plan_dynamic", "mxmoe_gg_launch_dynamic", "mxmoe_gg_dynamic_status",
    "mxmoe_gg_dynamic_tiles", "mxmoe_moe_segments", "mxmoe_moe_segments_host",
    # include/mxmoe_moe.h (MoE-layer plumbing)
    "mxmoe_moe_route", "mxmoe_moe_quant_act", "mxmoe_moe_silu_mul_quant", "mxmoe_moe_silu_mul_quant_il", "mxmoe_moe_quant_slots", "mxmoe_moe_combine",
    "mxmoe_moe_act_quant",
    "mxmoe_moe_gate", "mxmoe_moe_gate_ex",
    # gpt-oss layers: router logit bias, biased / clamped gated activation, combine with a down bias
    "mxmoe_moe_gate_ex2", "mxmoe_moe_glu_quant", "mxmoe_moe_combine_bias",
    # the router for 257 .. 512 experts
    "mxmoe_moe_gate_wide",
    # bf16 layers: the router, the gather and the combine with the element type as an argument
    "mxmoe_moe_gate_dt", "mxmoe_moe_gather_quant", "mxmoe_moe_combine_dt",
    # the decode forward (1..16 tokens, no planner)
    "mxmoe_moe_decode_gate_up", "mxmoe_moe_decode_down",
    # the decode forward for gpt-oss layers: MXFP4 weights, gate_up biases, the clamped SwiGLU
    "mxmoe_moe_decode_gate_up_ex", "mxmoe_moe_decode_down_ex",
    # the decode forward with the integer weight-only kinds (w4a16 / w8a16, per-channel or g128, sym or asym)
    "mxmoe_moe_decode_gate_up_wo", "mxmoe_moe_decode_down_wo",
)
# added to ABI 7 without a version bump (additive): a product library without them is a stale build
GPTOSS_SYMBOLS = ("mxmoe_moe_gate_ex2", "mxmoe_moe_glu_quant", "mxmoe_moe_combine_bias")
# added the same way after them: bound where present, ``symbol`` refuses the call where a build lacks it
WIDE_GATE_SYMBOLS = ("mxmoe_moe_gate_wide",)
DT_SYMBOLS = ("mxmoe_moe_gate_dt", "mxmoe_moe_gather_quant", "mxmoe_moe_combine_dt")  # (likewise: the bf16 layers)
DECODE_SYMBOLS = ("mxmoe_moe_decode_gate_up", "mxmoe_moe_decode_down")  # (likewise: the decode forward)
DECODE_EX_SYMBOLS = ("mxmoe_moe_decode_gate_up_ex", "mxmoe_moe_decode_down_ex")  # (likewise: gpt-oss layers)
DECODE_WO_SYMBOLS = ("mxmoe_moe_decode_gate_up_wo", "mxmoe_moe_decode_down_wo")  # (likewise: weight-only experts)
DT_FP16, DT_BF16 = 0, 1  # MXMOE_DT_* (include/mxmoe_moe.h)
# MXMOE_DECODE_* (include/mxmoe_moe.h): the token limit, the kinds per linear, the gate_up layouts, the status bits
DECODE_MAX_T = 16
DECODE_FP16, DECODE_W8A8, DECODE_W4A4 = 0, 1, 2
DECODE_W4A16_MX = 3  # (the _ex and _wo entries only)
# the _wo entries only: kind = 4 + (w_bits == 8) + 2 * (gsize == 128) + 4 * asym
DECODE_W4A16, DECODE_W8A16, DECODE_W4A16_G128, DECODE_W8A16_G128 = 4, 5, 6, 7
DECODE_W4A16_ASYM, DECODE_W8A16_ASYM, DECODE_W4A16_G128_ASYM, DECODE_W8A16_G128_ASYM = 8, 9, 10, 11


def decode_wo_kind(w_bits: int, gsize: int, sym: bool) -> int:
    """MXMOE_DECODE_* of an integer weight-only type (w_bits 4 or 8, gsize -1 or 128)."""
    if w_bits not in (4, 8) or gsize not in (-1, 128):
        raise ValueError(f"no decode kind for w{w_bits}a16_g{gsize}: 4 or 8 bits, per-channel or g128")
    return DECODE_W4A16 + (w_bits == 8) + 2 * (gsize == 128) + 4 * (not sym)


DECODE_GU_PLAIN, DECODE_GU_INTERLEAVED = 0, 1
DECODE_BAD_ID, DECODE_BAD_KIND = 1, 2
GLU_SILU, GLU_SWIGLU_CLAMP = 0, 1  # MXMOE_GLU_* (include/mxmoe_moe.h)


class MoeSegC(ctypes.Structure):
    """mxmoe_moe_seg (include/mxmoe_moe.h): one expert's segment of a permuted activation buffer."""

    _fields_ = [("qtag", ctypes.c_int32), ("first_slot", ctypes.c_int32), ("rows", ctypes.c_int32),
                ("width", ctypes.c_int32), ("out_off", ctypes.c_int64), ("scale_off", ctypes.c_int64)]


class GGDynRowC(ctypes.Structure):
    """mxmoe_gg_dyn_row (include/mxmoe_gg.h): one problem's rows and byte offsets for a dynamic launch."""

    _fields_ = [("rows", ctypes.c_int32), ("reserved", ctypes.c_int32), ("a_off", ctypes.c_int64),
                ("sa_off", ctypes.c_int64), ("c_off", ctypes.c_int64)]


class GGDynExtentC(ctypes.Structure):
    """mxmoe_gg_dyn_extent: bytes behind a problem's A / scale_a / C base pointers."""

    _fields_ = [("a_bytes", ctypes.c_int64), ("sa_bytes", ctypes.c_int64), ("c_bytes", ctypes.c_int64)]


class MoeSegTableC(ctypes.Structure):
    """mxmoe_moe_seg_table (include/mxmoe_moe.h): one activation buffer's segment table for mxmoe_moe_segments."""

    _fields_ = [("qtags", ctypes.c_void_p), ("width", ctypes.c_int32), ("width_shared", ctypes.c_int32),
                ("ldc", ctypes.c_int64), ("segs", ctypes.c_void_p), ("dyn", ctypes.c_void_p)]


class MoeGluC(ctypes.Structure):
    """mxmoe_moe_glu (include/mxmoe_moe.h): the gated activation and the gate_up biases of mxmoe_moe_glu_quant."""

    _fields_ = [("act", ctypes.c_int32), ("alpha", ctypes.c_float), ("limit", ctypes.c_float),
                ("bias_routed", ctypes.c_void_p), ("bias_shared", ctypes.c_void_p)]


class MoeDecodeExpertC(ctypes.Structure):
    """mxmoe_moe_decode_expert (include/mxmoe_moe.h): one expert's two weights and their kinds for the decode forward."""

    _fields_ = [("b1", ctypes.c_void_p), ("sb1", ctypes.c_void_p), ("b2", ctypes.c_void_p), ("sb2", ctypes.c_void_p),
                ("kind1", ctypes.c_int32), ("kind2", ctypes.c_int32)]


# mxmoe_gg_dynamic_status bits (MXMOE_GG_DYN_*) and mxmoe_moe_segments' (MXMOE_MOE_SEG_COUNT_MISMATCH)
DYN_ROWS_CLAMPED, DYN_JOINT_CLAMPED, DYN_SLOTS_CUT, DYN_BAD_OFFSET = 1, 2, 4, 8
SEG_COUNT_MISMATCH = 1

_lib = None


def _declare(lib: ctypes.CDLL) -> None:
    c = ctypes
    if hasattr(lib, "mxmoe_gg_plan_dynamic"):  # (device planning; builds before it lack the symbols: A/B tools)
        idx, ext, dyn = c.POINTER(c.c_int32), c.POINTER(GGDynExtentC), c.c_void_p
        lib.mxmoe_gg_dynamic_workspace_size.restype = c.c_int
        lib.mxmoe_gg_dynamic_workspace_size.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, idx, c.c_int, c.c_int64,
                                                        c.POINTER(c.c_size_t)]
        lib.mxmoe_gg_plan_dynamic.restype = c.c_int
        lib.mxmoe_gg_plan_dynamic.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, idx, c.c_int, c.c_int64, ext,
                                              c.c_void_p, c.c_size_t, c.c_void_p, c.POINTER(GGPlanInfo)]
        lib.mxmoe_gg_launch_dynamic.restype = c.c_int
        lib.mxmoe_gg_launch_dynamic.argtypes = [c.POINTER(GGPlanInfo), dyn, c.c_void_p]
        lib.mxmoe_gg_dynamic_status.restype = c.c_int
        lib.mxmoe_gg_dynamic_status.argtypes = [c.POINTER(GGPlanInfo), c.c_void_p, c.POINTER(c.c_int32), c.c_int]
        lib.mxmoe_gg_dynamic_tiles.restype = c.c_int
        lib.mxmoe_gg_dynamic_tiles.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, idx, c.c_int, c.c_int64, ext,
                                               c.POINTER(GGDynRowC), c.c_int, c.c_void_p, c.c_void_p,
                                               c.POINTER(c.c_int), c.POINTER(c.c_int32)]
    if hasattr(lib, "mxmoe_moe_segments"):
        lib.mxmoe_moe_segments.restype = c.c_int
        lib.mxmoe_moe_segments.argtypes = [c.c_void_p, c.c_int, c.c_int64, c.c_int, c.c_int, c.POINTER(MoeSegTableC),
                                           c.c_int, c.c_void_p, c.c_void_p]
        lib.mxmoe_moe_segments_host.restype = c.c_int
        lib.mxmoe_moe_segments_host.argtypes = [c.c_void_p, c.c_int, c.c_int64, c.c_int, c.c_int, c.POINTER(MoeSegTableC),
                                                c.POINTER(c.c_int32)]
    lib.mxmoe_gg_abi_version.restype = c.c_int
    lib.mxmoe_gg_abi_version.argtypes = []
    lib.mxmoe_gg_last_error.restype = c.c_char_p
    lib.mxmoe_gg_last_error.argtypes = []
    lib.mxmoe_gg_variant_count.restype = c.c_int
    lib.mxmoe_gg_variant_count.argtypes = []
    lib.mxmoe_gg_default_variant.restype = c.c_int
    lib.mxmoe_gg_default_variant.argtypes = []
    lib.mxmoe_gg_list_variants.restype = c.c_int
    lib.mxmoe_gg_list_variants.argtypes = [c.c_char_p, c.c_size_t]
    lib.mxmoe_gg_variant_tile.restype = c.c_int
    lib.mxmoe_gg_variant_tile.argtypes = [c.c_int, c.c_int, c.c_int] + [c.POINTER(c.c_int32)] * 4
    lib.mxmoe_gg_resolve_variant.restype = c.c_int
    lib.mxmoe_gg_resolve_variant.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, c.POINTER(c.c_int)]
    lib.mxmoe_gg_workspace_size.restype = c.c_int
    lib.mxmoe_gg_workspace_size.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, c.POINTER(c.c_size_t)]
    lib.mxmoe_gg_plan.restype = c.c_int
    lib.mxmoe_gg_plan.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p,
                                  c.POINTER(GGPlanInfo)]
    lib.mxmoe_gg_rebind.restype = c.c_int
    lib.mxmoe_gg_rebind.argtypes = [c.POINTER(GGProblemC), c.c_int, c.POINTER(GGPlanInfo), c.c_void_p]
    if hasattr(lib, "mxmoe_gg_forget_workspace"):  # (ABI 6+; older builds loaded by A/B tools lack it)
        lib.mxmoe_gg_forget_workspace.restype = c.c_int
        lib.mxmoe_gg_forget_workspace.argtypes = [c.c_void_p]
    if hasattr(lib, "mxmoe_gg_variant_caps"):  # (ABI 7+)
        lib.mxmoe_gg_variant_caps.restype = c.c_int
        lib.mxmoe_gg_variant_caps.argtypes = [c.c_int, c.POINTER(c.c_uint32)]
    lib.mxmoe_gg_launch.restype = c.c_int
    lib.mxmoe_gg_launch.argtypes = [c.POINTER(GGPlanInfo), c.c_void_p]
    lib.mxmoe_gg_run.restype = c.c_int
    lib.mxmoe_gg_run.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.groupgemm_mxmoe.restype = c.c_int
    lib.groupgemm_mxmoe.argtypes = [c.c_void_p] * 10 + [c.c_void_p, c.POINTER(MxmoeDim3), c.c_void_p,
                                                         c.POINTER(MxmoeQParams), c.c_int]
    lib.groupgemm_mxmoe_fmt.restype = c.c_int
    lib.groupgemm_mxmoe_fmt.argtypes = lib.groupgemm_mxmoe.argtypes + [c.c_void_p]
    lib.mxmoe_gg_release_shim_workspaces.restype = c.c_int
    lib.mxmoe_gg_release_shim_workspaces.argtypes = []
    lib.mxmoe_gg_repack_weightonly.restype = c.c_int
    lib.mxmoe_gg_repack_weightonly.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p]
    lib.mxmoe_gg_debug_trace.restype = c.c_int
    lib.mxmoe_gg_debug_trace.argtypes = [c.c_void_p, c.c_size_t, c.c_int]
    lib.mxmoe_gg_plan_tiles.restype = c.c_int
    lib.mxmoe_gg_plan_tiles.argtypes = [c.POINTER(GGProblemC), c.c_int, c.c_int, c.c_void_p, c.c_void_p,
                                        c.POINTER(c.c_int)]
    if hasattr(lib, "mxmoe_gg_pack_f6"):  # lab library only
        lib.mxmoe_gg_pack_f6.restype = c.c_int
        lib.mxmoe_gg_pack_f6.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p]
        lib.mxmoe_gg_pack_f6_host.restype = c.c_int
        lib.mxmoe_gg_pack_f6_host.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int64, c.c_void_p, c.c_int64]
    P = c.c_void_p
    lib.mxmoe_moe_route.restype = c.c_int
    lib.mxmoe_moe_route.argtypes = [P, c.c_int64, c.c_int, c.c_int, P, P, P, P, P]
    lib.mxmoe_moe_quant_act.restype = c.c_int
    lib.mxmoe_moe_quant_act.argtypes = [P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P, P, c.c_int, P, P, P]
    lib.mxmoe_moe_silu_mul_quant.restype = c.c_int
    lib.mxmoe_moe_silu_mul_quant.argtypes = [P, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P, c.c_int, P, P, P]
    for fn in ("mxmoe_moe_quant_slots", "mxmoe_moe_silu_mul_quant_il"):
        if hasattr(lib, fn):  # (builds before round 5's fused SiLU epilogue lack them: A/B tools)
            getattr(lib, fn).restype = c.c_int
            getattr(lib, fn).argtypes = [P, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P, c.c_int, P, P, P]
    if hasattr(lib, "mxmoe_moe_act_quant"):  # (the tagged activation entry; builds before MXFP4 lack it: A/B tools)
        lib.mxmoe_moe_act_quant.restype = c.c_int
        lib.mxmoe_moe_act_quant.argtypes = [c.c_int, P, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P, P, c.c_int, c.c_uint32,
                                            P, P, P]
    if hasattr(lib, "mxmoe_moe_gate"):  # (the router; builds before it lack the symbol: A/B tools)
        lib.mxmoe_moe_gate.restype = c.c_int
        lib.mxmoe_moe_gate.argtypes = [P, P, P, c.c_int64, c.c_int, c.c_int, c.c_int, c.c_int, P, P, P, P, P]
    if hasattr(lib, "mxmoe_moe_gate_ex"):  # (sigmoid / bias / group-limited routing; builds before it: A/B tools)
        lib.mxmoe_moe_gate_ex.restype = c.c_int
        lib.mxmoe_moe_gate_ex.argtypes = [P, P, P, c.c_int64, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, P, c.c_int, c.c_int,
                                          c.c_int, c.c_float, P, P, P, P, P, P]
    lib.mxmoe_moe_combine.restype = c.c_int
    lib.mxmoe_moe_combine.argtypes = [P, P, P, P, P, c.c_int64, c.c_int, c.c_int, P, P]
    if all(hasattr(lib, fn) for fn in GPTOSS_SYMBOLS):  # (builds before the gpt-oss layers lack them: A/B tools)
        lib.mxmoe_moe_gate_ex2.restype = c.c_int
        lib.mxmoe_moe_gate_ex2.argtypes = [P, P, P, c.c_int64, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, P, c.c_int,
                                           c.c_int, c.c_int, c.c_float, P, P, P, P, P, P, P]
        lib.mxmoe_moe_glu_quant.restype = c.c_int
        lib.mxmoe_moe_glu_quant.argtypes = [c.POINTER(MoeGluC), P, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P, c.c_int,
                                            c.c_uint32, P, P, P]
        lib.mxmoe_moe_combine_bias.restype = c.c_int
        lib.mxmoe_moe_combine_bias.argtypes = [P, P, P, P, P, P, P, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P]
    if all(hasattr(lib, fn) for fn in WIDE_GATE_SYMBOLS):  # (builds before the wide router lack it: A/B tools)
        lib.mxmoe_moe_gate_wide.restype = c.c_int
        lib.mxmoe_moe_gate_wide.argtypes = [P, P, P, c.c_int64, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, P, c.c_int,
                                            c.c_int, c.c_int, c.c_float, P, P, P, P, P, P, P]
    if all(hasattr(lib, fn) for fn in DT_SYMBOLS):  # (builds before the bf16 layers lack them: A/B tools)
        lib.mxmoe_moe_gate_dt.restype = c.c_int
        lib.mxmoe_moe_gate_dt.argtypes = [c.c_int] + lib.mxmoe_moe_gate_wide.argtypes
        lib.mxmoe_moe_gather_quant.restype = c.c_int
        lib.mxmoe_moe_gather_quant.argtypes = [c.c_int, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P, P, c.c_int, c.c_uint32,
                                               P, P, P]
        lib.mxmoe_moe_combine_dt.restype = c.c_int
        lib.mxmoe_moe_combine_dt.argtypes = [c.c_int] + lib.mxmoe_moe_combine_bias.argtypes
    if all(hasattr(lib, fn) for fn in DECODE_SYMBOLS):  # (builds before the decode forward lack them: A/B tools)
        lib.mxmoe_moe_decode_gate_up.restype = c.c_int
        lib.mxmoe_moe_decode_gate_up.argtypes = [c.c_int, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P, c.c_uint32, c.c_int,
                                                 c.c_int, c.c_int, c.c_int, P, P, P, P]
        lib.mxmoe_moe_decode_down.restype = c.c_int
        lib.mxmoe_moe_decode_down.argtypes = [c.c_int64, c.c_int, c.c_int, c.c_int, P, P, c.c_uint32, c.c_int, c.c_int,
                                              c.c_int, P, P, P, P, P, P]
    if all(hasattr(lib, fn) for fn in DECODE_EX_SYMBOLS):  # (builds before the gpt-oss decode forward lack them)
        lib.mxmoe_moe_decode_gate_up_ex.restype = c.c_int
        lib.mxmoe_moe_decode_gate_up_ex.argtypes = [c.POINTER(MoeGluC), c.c_int, P, c.c_int64, c.c_int, c.c_int, c.c_int, P, P,
                                                    c.c_uint32, c.c_int, c.c_int, c.c_int, c.c_int, P, P, P, P]
        lib.mxmoe_moe_decode_down_ex.restype = c.c_int
        lib.mxmoe_moe_decode_down_ex.argtypes = [c.c_int64, c.c_int, c.c_int, c.c_int, P, P, c.c_uint32, c.c_int, c.c_int,
                                                 c.c_int, P, P, P, P, P, P]
    if all(hasattr(lib, fn) for fn in DECODE_WO_SYMBOLS):  # (builds before the weight-only decode forward lack them)
        lib.mxmoe_moe_decode_gate_up_wo.restype = c.c_int
        lib.mxmoe_moe_decode_gate_up_wo.argtypes = list(lib.mxmoe_moe_decode_gate_up_ex.argtypes)
        lib.mxmoe_moe_decode_down_wo.restype = c.c_int
        lib.mxmoe_moe_decode_down_wo.argtypes = list(lib.mxmoe_moe_decode_down_ex.argtypes)


def lib() -> ctypes.CDLL:
    """The loaded library; raises NativeLibraryError (never falls back)."""
    global _lib
    if _lib is None:
        path = Path(os.environ.get("MXMOE_GG_LIB", LIB_PATH))
        if not path.exists():
            raise NativeLibraryError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no fallback path.")
        try:
            handle = ctypes.CDLL(str(path))
        except OSError as e:  # pragma: no cover - environment dependent
            raise NativeLibraryError(f"failed to load {path}: {e}") from e
        _check_abi(handle, path)
        _check_symbols(handle, path)
        _declare(handle)
        _lib = handle
        atexit.register(_release_shim)
    return _lib


def _check_abi(handle: ctypes.CDLL, path: Path) -> None:
    """The product library must carry the ABI this binding is written for (a stale or foreign .so
    raises NativeLibraryError here, not an AttributeError or a mis-typed call later). A library
    named by MXMOE_GG_LIB (the A/B tools' older or lab builds) may be older: the symbols added
    since are bound only where present."""
    try:
        fn = handle.mxmoe_gg_abi_version
    except AttributeError as e:
        raise NativeLibraryError(f"{path} exports no mxmoe_gg_abi_version: not a libmxmoe_gg build") from e
    fn.restype, fn.argtypes = ctypes.c_int, []
    got = fn()
    if got == ABI_VERSION or ("MXMOE_GG_LIB" in os.environ and 5 <= got < ABI_VERSION):
        return
    raise NativeLibraryError(f"{path} has ABI version {got}, this binding needs {ABI_VERSION}: rebuild it with "
                             "`python -c 'import __graft_entry__ as g; g.build()'`")


def _check_symbols(handle: ctypes.CDLL, path: Path) -> None:
    """The entry points added to ABI 7 after its first release (GPTOSS_SYMBOLS) must be in the product library: one
    built before them carries the right version number and would fail with an AttributeError at the first call. A
    library named by MXMOE_GG_LIB may lack them (``symbol`` then refuses the call)."""
    missing = [fn for fn in GPTOSS_SYMBOLS if not hasattr(handle, fn)]
    if missing and "MXMOE_GG_LIB" not in os.environ:
        raise NativeLibraryError(f"{path} lacks {', '.join(missing)}: a stale build, rebuild it with "
                                 "`python -c 'import __graft_entry__ as g; g.build()'`")


def symbol(name: str):
    """An entry point of the loaded library, NativeLibraryError (not AttributeError) where the build lacks it."""
    handle = lib()
    if not hasattr(handle, name):
        raise NativeLibraryError(f"the loaded library exports no {name}: it was built before that entry point")
    return getattr(handle, name)


def _release_shim() -> None:
    """Free the reference-ABI shim's per-device buffers before the HIP runtime tears down (only if
    a GPU is present: on a CPU-only host no shim call can have allocated)."""
    try:
        import torch

        if torch.cuda.is_initialized():
            _lib.mxmoe_gg_release_shim_workspaces()
    except Exception:  # pragma: no cover - interpreter shutdown
        pass


def check(status: int) -> None:
    if status != MXMOE_GG_OK:
        msg = lib().mxmoe_gg_last_error().decode(errors="replace")
        raise GGError(status, msg)


def variant_count() -> int:
    return lib().mxmoe_gg_variant_count()


GENERAL_QCFGS = ("fp16", "w8a8_g-1_sym", "w4a4_g-1_sym")


def production_variants(qcfg: str | None = "general") -> list[int]:
    """Compiled variants that compute correct results (``abl_*`` are timing ablations) and have a tile
    body for ``qcfg`` (default "general": fp16, w8a8 and w4a4 — the general-purpose kernels; ``None``:
    every one). The small-batch ``wo3_*`` kernel has fp16, w8a8, w4a4 and weight-only bodies (not
    w4a4_g128, E4M3 or bf16), so it is in the "general" set too."""
    vs = [int(ln.split()[0]) for ln in list_variants() if not ln.split()[1].startswith("abl_")]
    if qcfg is None:
        return vs
    need = GENERAL_QCFGS if qcfg == "general" else (qcfg,)
    return [v for v in vs if all(variant_supports(v, q) for q in need)]


def plan_tiles(problems, variant: int):
    """Host tile table of a plan (mxmoe_gg_plan_tiles; no device needed): (tiles [slots, 8] int32
    with columns prob/m0/n0/cls/ks0/ks1/slab/grp in blockIdx order, rows: table row -> the caller's
    problem index)."""
    import numpy as np

    P = len(problems)
    arr = (GGProblemC * P)(*problems)
    n = ctypes.c_int(0)
    check(lib().mxmoe_gg_plan_tiles(arr, P, variant, None, None, ctypes.byref(n)))
    tiles = np.zeros((n.value, 8), dtype=np.int32)
    rows = np.full(P, -1, dtype=np.int32)
    check(lib().mxmoe_gg_plan_tiles(arr, P, variant, tiles.ctypes.data, rows.ctypes.data, ctypes.byref(n)))
    return tiles, rows


def default_variant() -> int:
    return lib().mxmoe_gg_default_variant()


def list_variants() -> list[str]:
    buf = ctypes.create_string_buffer(1 << 16)
    n = lib().mxmoe_gg_list_variants(buf, len(buf))
    if n < 0:
        check(-n)
    return [ln for ln in buf.value.decode().splitlines() if ln]


def variant_supports(variant: int, qcfg: str) -> bool:
    """Whether a compiled variant has a tile body for ``qcfg`` (weight-only strategies are listed by
    their base name, e.g. ``w4a16``)."""
    from .tile_config import variant_key

    if variant == VARIANT_AUTO:
        return True
    line = list_variants()[variant]
    return f" {variant_key(qcfg)}=TileConfig(" in line


def variant_caps(variant: int) -> int:
    """Capability bits (CAP_*) of a compiled variant (mxmoe_gg_variant_caps): e.g. whether it has the
    fused SiLU epilogue."""
    out = ctypes.c_uint32()
    check(lib().mxmoe_gg_variant_caps(variant, ctypes.byref(out)))
    return out.value


def variant_tile(variant: int, a_bits: int, w_bits: int) -> dict:
    v = [ctypes.c_int32() for _ in range(4)]
    check(lib().mxmoe_gg_variant_tile(variant, a_bits, w_bits, *[ctypes.byref(x) for x in v]))
    return {"BM": v[0].value, "BN": v[1].value, "BK_bytes": v[2].value, "threads": v[3].value}


def repack_weightonly(ref_words, N: int, K: int, w_bits: int):
    """Reference weight-only packed words (numpy uint16 [N*w_bits/16, K], host) -> the kernel's
    uint8 [N, K*w_bits/8] layout (mxmoe_gg_repack_weightonly)."""
    import numpy as np

    src = np.ascontiguousarray(ref_words, dtype=np.uint16)
    out = np.empty((N, K * w_bits // 8), dtype=np.uint8)
    check(lib().mxmoe_gg_repack_weightonly(src.ctypes.data, N, K, w_bits, out.ctypes.data))
    return out


def pack_f6_host(codes, K: int):
    """Packed int4 rows (numpy uint8 [rows, K/2], pack_wxax) -> fp6 images (uint8 [rows,
    f6_row_bytes(K)]) on the host (mxmoe_gg_pack_f6_host; lab library: MXMOE_GG_LIB)."""
    import numpy as np

    src = np.ascontiguousarray(codes, dtype=np.uint8)
    rows = src.shape[0]
    out = np.empty((rows, f6_row_bytes(K)), dtype=np.uint8)
    check(lib().mxmoe_gg_pack_f6_host(src.ctypes.data, rows, K, 0, out.ctypes.data, 0))
    return out


def pack_f6(codes, K: int, out=None, stream=None):
    """Packed int4 rows (uint8 device tensor [rows, K/2]) -> fp6 images on the device
    (mxmoe_gg_pack_f6, asynchronous on ``stream`` / torch's current stream; lab library)."""
    import torch

    if codes.dtype not in (torch.uint8, torch.int8) or codes.dim() != 2 or codes.shape[1] * 2 < K:
        raise ValueError("pack_f6: codes must be a uint8 [rows, >= K/2] tensor")
    rows = codes.shape[0]
    if out is None:
        out = torch.empty((rows, f6_row_bytes(K)), dtype=torch.uint8, device=codes.device)
    s = stream if stream is not None else torch.cuda.current_stream(codes.device)
    check(lib().mxmoe_gg_pack_f6(ctypes.c_void_p(codes.data_ptr()), rows, K, codes.stride(0) // 2,
                                 ctypes.c_void_p(out.data_ptr()), out.stride(0) // 2, ctypes.c_void_p(s.cuda_stream)))
    return out


def resolve_variant(problems, problem_count: int, variant: int = VARIANT_AUTO) -> int:
    """The concrete variant AUTO (or an index) resolves to for a ctypes array of GGProblemC (host only)."""
    out = ctypes.c_int()
    check(lib().mxmoe_gg_resolve_variant(problems, problem_count, variant, ctypes.byref(out)))
    return out.value


def workspace_size(problems, problem_count: int, variant: int) -> int:
    """Workspace bytes for a ctypes array of GGProblemC (plan table + pointers + tile table)."""
    n = ctypes.c_size_t()
    check(lib().mxmoe_gg_workspace_size(problems, problem_count, variant, ctypes.byref(n)))
    return n.value


def _joint_array(joint):
    joint = [int(j) for j in joint]
    return (ctypes.c_int32 * max(len(joint), 1))(*joint), len(joint)


def dynamic_tiles(problems, variant: int, joint, rows_total: int, dyn_rows, extents=None, slot_limit: int = 0):
    """Host run of the device tile planner (mxmoe_gg_dynamic_tiles; no device needed). ``problems``: GGProblemC at
    their capacities, ``dyn_rows``: one (rows, a_off, sa_off, c_off) per problem. Returns (tiles [tile_slots, 8]
    int32 in ``plan_tiles``' format with prob = the problem's index, the rows each problem was planned with,
    the MXMOE_GG_DYN_* status bits)."""
    import numpy as np

    P = len(problems)
    arr = (GGProblemC * max(P, 1))(*problems)
    jarr, nj = _joint_array(joint)
    rows = (GGDynRowC * max(P, 1))(*[GGDynRowC(int(r[0]), 0, int(r[1]), int(r[2]), int(r[3])) for r in dyn_rows])
    ext = None if extents is None else (GGDynExtentC * max(P, 1))(*[GGDynExtentC(*map(int, e)) for e in extents])
    n, st = ctypes.c_int(0), ctypes.c_int32(0)
    args = (arr, P, variant, jarr, nj, int(rows_total), ext, rows, int(slot_limit))
    check(lib().mxmoe_gg_dynamic_tiles(*args, None, None, ctypes.byref(n), ctypes.byref(st)))
    tiles = np.zeros((n.value, 8), dtype=np.int32)
    planned = np.zeros(max(P, 1), dtype=np.int32)
    check(lib().mxmoe_gg_dynamic_tiles(*args, tiles.ctypes.data, planned.ctypes.data, ctypes.byref(n), ctypes.byref(st)))
    return tiles, planned[:P], st.value


def segments_host(counts, T: int, topk: int, qtags, width: int, width_shared: int = 0, ldc: int = 0):
    """Host run of mxmoe_moe_segments' function (mxmoe_moe_segments_host): (list of MoeSegC, list of GGDynRowC,
    status) for the routing counts; len(qtags) == len(counts) + 1 adds the shared segment."""
    import numpy as np

    E = len(counts)
    nseg = len(qtags)
    c = np.ascontiguousarray(counts, dtype=np.int32)
    tags = np.ascontiguousarray(qtags, dtype=np.int32)
    segs = (MoeSegC * nseg)()
    dyn = (GGDynRowC * nseg)()
    tb = MoeSegTableC(tags.ctypes.data, int(width), int(width_shared), int(ldc), ctypes.addressof(segs),
                      ctypes.addressof(dyn))
    st = ctypes.c_int32(0)
    check(lib().mxmoe_moe_segments_host(c.ctypes.data, E, int(T), int(topk), int(nseg == E + 1), ctypes.byref(tb),
                                        ctypes.byref(st)))
    return list(segs), list(dyn), st.value
