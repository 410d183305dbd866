"""Dump what the host planner decides for a fixed corpus of calls, one line per case, so two builds
of the library can be compared with `diff` (CPU only: mxmoe_gg_resolve_variant,
mxmoe_gg_workspace_size, mxmoe_gg_plan_tiles, mxmoe_gg_list_variants, mxmoe_gg_last_error).

python tools/plan_dump.py > a.txt                      # the product library
MXMOE_GG_LIB=<other .so> python tools/plan_dump.py > b.txt ; diff a.txt b.txt
(the planner's MXMOE_GG_* knobs are read by the lab library only: MXMOE_GG_LIB=.../libmxmoe_gg_lab.so)

The mxmoe_gg_list_variants text comes first. Then, for every variant of the loaded library and AUTO:
the qwen2_moe layer-11 gate_up / down calls at bs 128 / 512 / 2048 / 8192 in every quant
configuration (the SiLU-capable ones again with MXMOE_GG_EPI_SILU_MUL), and the edge cases: empty
problems, M = 1, explicit strides, and one call per error return of the problem validation. A line:
  <case> variant=<resolved name> status=<code> ws=<workspace bytes> tiles=<sha256> rows=<sha256> [err=<text>]
This is an instrument for changes that claim to leave the planner alone, not a test: no hashes are
committed.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from mxmoe_amd import _native as nat  # noqa: E402
from mxmoe_amd.workload import (QShape, load_workload, mixed_qconfig_lp1, parse_qstr,  # noqa: E402
                                qwen2_layer11_workload, w4a16_w8a8_qconfig)

FMT = {"": nat.FMT_DEFAULT, "E4M3": nat.FMT_E4M3, "bf16": nat.FMT_BF16, "MXFP4": nat.FMT_MXFP4, "MXFP8": nat.FMT_MXFP8}
MX4, MX4W, MX8 = "w4a4_g32_sym_MXFP4", "w4a16_g32_sym_MXFP4", "w4a8_g32_sym_MXFP8"
W8A8 = "w8a8_g-1_sym"
BATCHES = (128, 512, 2048, 8192)

# name -> (qstr | qconfig | tuple of qstrs dealt to the problems in turn, SiLU-capable)
CONFIGS = {
    "fp16": ("fp16", True), "bf16": ("bf16", False), "w8a8": (W8A8, True), "e4m3": ("w8a8_g-1_sym_E4M3", False),
    "w4a4": ("w4a4_g-1_sym", True), "w4a4_g128": ("w4a4_g128_sym", False), "mixed_lp1": (mixed_qconfig_lp1, True),
    "w4a16": ("w4a16_g128_asym", True), "w8a16": ("w8a16_g-1_asym", True), "w2a16": ("w2a16_g128_asym", True),
    "w4a16_w8a8": (w4a16_w8a8_qconfig, True),
    "mxfp4": (MX4, False), "mxfp4w": (MX4W, True), "mxfp8": (MX8, True),
    "mxfp4+mxfp4w": ((MX4, MX4W), False), "mxfp4+mxfp8": ((MX4, MX8), False), "mxfp4w+mxfp8": ((MX4W, MX8), True),
    "mxfp4+w8a8": ((MX4, W8A8), False), "mxfp4w+w8a8": ((MX4W, W8A8), True), "mxfp8+w8a8": ((MX8, W8A8), True),
}


def _shape(M, N, K, qstr="fp16"):
    q = parse_qstr(qstr)
    return QShape(shape=[M, N, K], w_bits=q["w_bits"], a_bits=q["a_bits"], gsize=q["gsize"], sym=q["sym"],
                  fmt=q.get("fmt", ""))


def _problem(s: QShape, flags=0, lda=0, ldb=0, ldc=0, fmt=None):
    return nat.GGProblemC(A=0, B=0, scale_a=0, scale_b=0, C=0, M=s.M, N=s.N, K=s.K, a_bits=s.a_bits, w_bits=s.w_bits,
                          gsize=s.gsize, sym=int(s.sym), fmt=(FMT[s.fmt] if fmt is None else fmt) | flags,
                          lda=lda, ldb=ldb, ldc=ldc)


def _layer(bs: int, cfg):
    if callable(cfg):
        return load_workload(qwen2_layer11_workload(bs, qconfig=cfg()))["layer-11"]
    if isinstance(cfg, str):
        return load_workload(qwen2_layer11_workload(bs, qstr=None if cfg == "fp16" else cfg))["layer-11"]
    layer = load_workload(qwen2_layer11_workload(bs))["layer-11"]  # the fp16 shapes, types dealt in turn
    return {gg: [_shape(s.M, s.N, s.K, cfg[i % len(cfg)]) for i, s in enumerate(lst)] for gg, lst in layer.items()}


def layer_cases():
    for name, (cfg, silu) in CONFIGS.items():
        for bs in BATCHES:
            layer = _layer(bs, cfg)
            for gg in ("gate_up", "down"):
                yield f"{name}/bs{bs}/{gg}", [_problem(s) for s in layer[gg]]
                if silu:
                    yield f"{name}+silu/bs{bs}/{gg}", [_problem(s, nat.EPI_SILU_MUL) for s in layer[gg]]


def edge_cases():
    f16 = [_shape(m, 512, 1024) for m in (300, 0, 77)]
    yield "empty/some", [_problem(s) for s in f16]
    yield "empty/all", [_problem(_shape(0, 512, 1024)), _problem(_shape(0, 256, 512, W8A8))]
    yield "empty/mxfp4_beside_fp16", [_problem(s) for s in f16] + [_problem(_shape(0, 512, 1024, MX4))]
    yield "empty/none", []
    for q in ("fp16", W8A8, "w4a4_g-1_sym", "w4a16_g128_asym", MX4, MX4W, MX8):
        yield f"m1/{q}", [_problem(_shape(1, 512, 1024, q)), _problem(_shape(1, 2048, 512, q))]
    # explicit strides, in 16-bit words (rows of 1024 fp16 / int8 / 4-bit elements: 1024 / 512 / 256 words)
    yield "ld/fp16", [_problem(_shape(300, 512, 1024), lda=1032, ldb=1040, ldc=520)]
    yield "ld/w8a8", [_problem(_shape(300, 512, 1024, W8A8), lda=520, ldb=528, ldc=1024)]
    yield "ld/w4a16", [_problem(_shape(70, 512, 1024, "w4a16_g128_asym"), lda=1032, ldb=264, ldc=520)]
    yield "ld/mxfp8", [_problem(_shape(70, 512, 1024, MX8), lda=520, ldb=264, ldc=520)]
    yield "ld/fp16+silu", [_problem(_shape(300, 512, 1024), nat.EPI_SILU_MUL, ldc=264)]
    # one call per error return of the problem validation
    yield "err/negative", [_problem(_shape(-1, 512, 1024))]
    yield "err/qtype", [_problem(_shape(64, 512, 1024, "w3a16_g-1_sym"))]
    yield "err/qtype_e4m3", [_problem(_shape(64, 512, 1024, "w4a4_g-1_sym_E4M3"))]
    yield "err/qtype_mxfp4", [_problem(_shape(64, 512, 1024, "w4a4_g64_sym_MXFP4"))]
    yield "err/qtype_mxfp8", [_problem(_shape(64, 512, 1024, "w8a8_g32_sym_MXFP8"))]
    yield "err/fmt_unknown", [_problem(_shape(64, 512, 1024), fmt=9)]
    yield "err/fmt_flags", [_problem(_shape(64, 512, 1024), flags=0x200)]
    yield "err/k_fp16", [_problem(_shape(64, 512, 1004))]
    yield "err/k_w8a8", [_problem(_shape(64, 512, 1032, W8A8))]
    yield "err/k_w4a4", [_problem(_shape(64, 512, 1040, "w4a4_g-1_sym"))]
    yield "err/k_g128", [_problem(_shape(64, 512, 1088, "w4a4_g128_sym"))]
    yield "err/k_mxfp4", [_problem(_shape(64, 512, 1040, MX4))]
    yield "err/k_mxfp8", [_problem(_shape(64, 512, 1040, MX8))]
    yield "err/k_wo", [_problem(_shape(64, 512, 1056, "w4a16_g-1_asym"))]
    yield "err/k_mxfp4w", [_problem(_shape(64, 512, 1056, MX4W))]
    yield "err/gsize_wo", [_problem(_shape(64, 512, 1024, "w4a16_g96_asym"))]
    yield "err/n", [_problem(_shape(64, 100, 1024))]
    yield "err/n_wo", [_problem(_shape(64, 100, 1024, "w4a16_g128_asym"))]
    for q in (W8A8, "w4a4_g-1_sym", "w4a4_g128_sym"):
        yield f"err/k_int32/{q}", [_problem(_shape(64, 512, 131072 + 128, q))]
    for q in ("fp16", "w8a8_g-1_sym_E4M3", MX4, MX8, "w4a16_g128_asym"):  # (no bound: floating-point accumulation)
        yield f"ok/k_int32/{q}", [_problem(_shape(64, 512, 131072 + 128, q))]
    yield "err/k_2^20_mxfp4w", [_problem(_shape(64, 512, (1 << 20) + 64, MX4W))]
    for q in ("bf16", "w8a8_g-1_sym_E4M3", "w4a4_g128_sym", MX4):
        yield f"err/silu_type/{q}", [_problem(_shape(64, 512, 1024, q), nat.EPI_SILU_MUL)]
    for q in ("w4a16_g128_asym", MX4W):  # (weight-only: an error except on the small-batch kernel)
        yield f"silu_wo/{q}", [_problem(_shape(64, 512, 1024, q), nat.EPI_SILU_MUL)]
    yield "err/silu_n", [_problem(_shape(64, 528, 1024), nat.EPI_SILU_MUL)]
    yield "err/lda_short", [_problem(_shape(64, 512, 1024), lda=1016)]
    yield "err/ldb_odd", [_problem(_shape(64, 512, 1024), ldb=1028)]
    yield "err/ld_wo", [_problem(_shape(64, 512, 1024, "w4a16_g128_asym"), ldb=248)]
    yield "err/ld_8mib", [_problem(_shape(64, 512, 1024), lda=1 << 22)]
    yield "err/ldc_short", [_problem(_shape(64, 512, 1024), ldc=504)]
    yield "err/ldc_odd", [_problem(_shape(64, 512, 1024, "w4a16_g128_asym"), ldc=516)]
    yield "err/ldc_silu", [_problem(_shape(64, 512, 1024), nat.EPI_SILU_MUL, ldc=248)]


def dump_case(lib, case: str, probs, variant: int, names, tiles_buf, rows_buf) -> str:
    P = len(probs)
    arr = (nat.GGProblemC * max(P, 1))(*probs)
    err = lambda: lib.mxmoe_gg_last_error().decode(errors="replace")  # noqa: E731
    out = ctypes.c_int(-1)
    st = lib.mxmoe_gg_resolve_variant(arr, P, variant, ctypes.byref(out))
    if st:
        return f"{case} variant=? status={st} err={err()}"
    v = out.value
    ws = ctypes.c_size_t(0)
    st = lib.mxmoe_gg_workspace_size(arr, P, v, ctypes.byref(ws))
    if st:
        return f"{case} variant={names[v]} status={st} err={err()}"
    n = ctypes.c_int(len(tiles_buf))
    rows_buf[:] = -1
    st = lib.mxmoe_gg_plan_tiles(arr, P, v, tiles_buf.ctypes.data, rows_buf.ctypes.data, ctypes.byref(n))
    if st:
        return f"{case} variant={names[v]} status={st} err={err()}"
    if n.value > len(tiles_buf):
        raise SystemExit(f"{case}: {n.value} tile slots exceed the buffer")
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    return f"{case} variant={names[v]} status=0 ws={ws.value} tiles={sha(tiles_buf[:n.value])} rows={sha(rows_buf[:P])}"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--variants", default="", help="only variants whose name contains this text (and AUTO)")
    args = ap.parse_args()
    lib = nat.lib()
    listing = nat.list_variants()
    print("\n".join(listing))
    names = [ln.split()[1] for ln in listing]
    cases = list(layer_cases()) + list(edge_cases())
    tiles_buf = np.zeros((1 << 18, 8), dtype=np.int32)
    rows_buf = np.zeros(max(len(p) for _, p in cases) + 1, dtype=np.int32)
    for v in [nat.VARIANT_AUTO] + [i for i, nm in enumerate(names) if args.variants in nm]:
        tag = "AUTO" if v == nat.VARIANT_AUTO else names[v]
        for case, probs in cases:
            print(dump_case(lib, f"{tag}:{case}", probs, v, names, tiles_buf, rows_buf))


if __name__ == "__main__":
    main()
