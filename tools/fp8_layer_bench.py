"""FP8 layers: the qwen2_moe layer-11 shape with every expert w8a8_g-1_sym_E4M3, w8a8_g-1_sym or fp16, as
PlannedForward steps at bs 128 / 512 / 2048 / 8192 in one process, the sides alternating over rounds: per-stage and
per-step device times, the variants AUTO chose, and the two E4M3 activation passes against the INT8 passes
(moe_bench.fp8_layer_bench). One JSON line per batch size; --out also writes the list to a file
(profiles/<round>/fp8_layer/bench.json).

python tools/fp8_layer_bench.py [--rounds 4] [--iters 30] [--batches 128,512,2048,8192] [--out FILE]

--gemm: instead, the layer's gate_up and down GroupGEMM calls at the first batch size with every problem block-scaled
(w8a8_g128_sym_E4M3) against per-channel (w8a8_g-1_sym_E4M3): same process, the sides alternating over rounds; per
call and side the median of the rounds' medians with min / max (ms), TOP/s, and the block-scaled / per-channel ratio.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxmoe_amd import moe_bench  # noqa: E402


def gemm_bench(bs: int, rounds: int, iters: int):
    import statistics

    from mxmoe_amd.groupgemm import GroupGemm
    from mxmoe_amd.harness import build_layer_inputs, time_launches
    from mxmoe_amd.workload import layer_problems, qwen2_layer11_workload

    sides = ("w8a8_g128_sym_E4M3", "w8a8_g-1_sym_E4M3")
    for call in ("gate_up", "down"):
        inputs = {q: build_layer_inputs(layer_problems(qwen2_layer11_workload(bs, qstr=q))[call]) for q in sides}
        plans = {q: GroupGemm(inputs[q].problems) for q in sides}
        ms = {q: [] for q in sides}
        for _ in range(rounds):
            for q in sides:
                ms[q].append(time_launches(plans[q].launch, warmup=5, iters=iters)["median_ms"])
        r = {"model": "qwen2_moe", "bs": bs, "call": call, "rounds": rounds, "iters": iters}
        for q in sides:
            med = statistics.median(ms[q])
            r[q] = {"median_ms": round(med, 5), "min_ms": round(min(ms[q]), 5), "max_ms": round(max(ms[q]), 5),
                    "tops": round(inputs[q].flops / (med * 1e-3) / 1e12, 1), "variant": plans[q].variant}
        r["time_ratio"] = round(r[sides[0]]["median_ms"] / r[sides[1]]["median_ms"], 4)
        yield r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", default="128,512,2048,8192")
    ap.add_argument("--out", default="")
    ap.add_argument("--gemm", action="store_true")
    args = ap.parse_args()
    results = []
    batches = [int(b) for b in args.batches.split(",") if b]
    for r in (gemm_bench(batches[0], args.rounds, args.iters) if args.gemm else
              moe_bench.fp8_layer_bench(batches, args.rounds, args.iters)):
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
