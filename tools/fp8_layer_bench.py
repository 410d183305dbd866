"""FP8 layers: the qwen2_moe layer-11 shape with every expert w8a8_g-1_sym_E4M3, w8a8_g-1_sym or fp16, as
PlannedForward steps at bs 128 / 512 / 2048 / 8192 in one process, the sides alternating over rounds: per-stage and
per-step device times, the variants AUTO chose, and the two E4M3 activation passes against the INT8 passes
(moe_bench.fp8_layer_bench). One JSON line per batch size; --out also writes the list to a file
(profiles/<round>/fp8_layer/bench.json).

python tools/fp8_layer_bench.py [--rounds 4] [--iters 30] [--batches 128,512,2048,8192] [--out FILE]

--gemm: instead, the layer's gate_up and down GroupGEMM calls at every batch size with every problem block-scaled
(w8a8_g128_sym_E4M3), forced onto the small-batch kernel (wo3) and onto v2x, beside per-channel E4M3 and w8a8 under
AUTO: same process, the sides alternating over rounds; per call and side the median of the rounds' medians with
min / max (ms), TOP/s, the wo3 / v2x time ratio and the variant AUTO takes for the block-scaled call.
--scheme mxfp6: the layer with every expert w6a6_g32_sym_MXFP6 beside w8a8_g-1_sym_E4M3 and w4a4_g32_sym_MXFP4 (and fp16),
the same steps and stages, with the MXFP6 / E4M3 and MXFP6 / MXFP4 ratios of the gate_up and down calls, the two
activation passes and the step. --gemm --scheme mxfp6: the two GroupGEMM calls alone, the three types under AUTO.
--gemm --scheme mxfp6 --once: a few launches of the MXFP6 gate_up call at the first batch size and nothing else (a
counter run's workload).
--gemm --ds: the same on a DeepSeek-V3-shaped call (H = 7168, N = 2048, top-8 over 16 experts), --batches in tokens.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxmoe_amd import moe_bench  # noqa: E402


GEMM_SIDES = (  # label, qstr, variant name (None: AUTO)
    ("f8g128@wo3", "w8a8_g128_sym_E4M3", "wo3_64x256_w8_3wg"),
    ("f8g128@v2x", "w8a8_g128_sym_E4M3", "v2x_256x256_w8_b3_buf_spread_edma"),
    ("e4m3@auto", "w8a8_g-1_sym_E4M3", None),
    ("w8a8@auto", "w8a8_g-1_sym", None),
)
MX6_SIDES = (("mxfp6@auto", "w6a6_g32_sym_MXFP6", None), ("e4m3@auto", "w8a8_g-1_sym_E4M3", None),
             ("mxfp4@auto", "w4a4_g32_sym_MXFP4", None))


def gemm_bench(batches, rounds: int, iters: int, deepseek: bool, sides=GEMM_SIDES, calls=("gate_up", "down")):
    import statistics

    from mxmoe_amd import _native as nat
    from mxmoe_amd.groupgemm import GroupGemm
    from mxmoe_amd.harness import build_layer_inputs, time_launches
    from mxmoe_amd.workload import QShape, layer_problems, parse_qstr, qwen2_layer11_workload

    names = [ln.split()[1] for ln in nat.list_variants()]

    def shapes(bs, q, call):
        if not deepseek:
            return layer_problems(qwen2_layer11_workload(bs, qstr=q))[call]
        E, topk, H, N = 16, 8, 7168, 2048  # tools/decode_bench.py --scheme f8g128_ds; tokens spread evenly
        rows = [bs * topk // E + (e < bs * topk % E) for e in range(E)]
        n, k = (2 * N, H) if call == "gate_up" else (H, N)
        return [QShape(shape=[m, n, k], **parse_qstr(q)) for m in rows if m > 0]

    for bs in batches:
        for call in calls:
            inputs = {lb: build_layer_inputs(shapes(bs, q, call)) for lb, q, _ in sides}
            plans = {lb: GroupGemm(inputs[lb].problems, variant=None if v is None else names.index(v)) for lb, _, v in sides}
            ms = {lb: [] for lb in plans}
            for _ in range(rounds):
                for lb in plans:
                    ms[lb].append(time_launches(plans[lb].launch, warmup=5, iters=iters)["median_ms"])
            r = {"model": "deepseek_v3_e16" if deepseek else "qwen2_moe", "bs": bs, "call": call, "rounds": rounds, "iters": iters,
                 "auto": names[GroupGemm(inputs[sides[0][0]].problems).variant]}  # what AUTO takes for the first side's call
            for lb in plans:
                med = statistics.median(ms[lb])
                r[lb] = {"median_ms": round(med, 5), "min_ms": round(min(ms[lb]), 5), "max_ms": round(max(ms[lb]), 5),
                         "tops": round(inputs[lb].flops / (med * 1e-3) / 1e12, 1), "variant": names[plans[lb].variant]}
            if sides is GEMM_SIDES:
                r["wo3_over_v2x"] = round(r["f8g128@wo3"]["median_ms"] / r["f8g128@v2x"]["median_ms"], 4)
            else:
                r["first_over"] = {lb: round(r[sides[0][0]]["median_ms"] / r[lb]["median_ms"], 4) for lb, _, _ in sides[1:]}
            yield r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", default="128,512,2048,8192")
    ap.add_argument("--out", default="")
    ap.add_argument("--gemm", action="store_true")
    ap.add_argument("--scheme", default="fp8", choices=["fp8", "mxfp6"])
    ap.add_argument("--once", action="store_true", help="--gemm --scheme mxfp6: the MXFP6 gate_up call only, a few launches")
    ap.add_argument("--ds", action="store_true", help="--gemm: the DeepSeek-V3-shaped call")
    args = ap.parse_args()
    results = []
    batches = [int(b) for b in args.batches.split(",") if b]
    mx6 = args.scheme == "mxfp6"
    if args.gemm and mx6 and args.once:
        runs = gemm_bench(batches[:1], 1, 3, False, MX6_SIDES[:1], ("gate_up",))
    elif args.gemm:
        runs = gemm_bench(batches, args.rounds, args.iters, args.ds, MX6_SIDES if mx6 else GEMM_SIDES)
    else:
        runs = moe_bench.fp8_layer_bench(batches, args.rounds, args.iters,
                                         ("mxfp6", "e4m3", "mxfp4") if mx6 else ("e4m3", "w8a8", "fp16"))
    for r in runs:
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
