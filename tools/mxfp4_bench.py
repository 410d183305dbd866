"""MXFP4 (w4a4_g32_sym_MXFP4, v2x) against w4a4_g-1_sym (AUTO -> v3) and w8a8_g-1_sym (v2x) on the
qwen2_moe layer-11 gate_up and down calls at bs 8192 and bs 512: one process, the three sides
alternating round by round, device-event time per launch.

Per call and side: the median over the rounds of each round's median launch time, with the min / max
of the rounds' medians (the side's spread), and the ratio of the MXFP4 median to the other sides'.

python tools/mxfp4_bench.py [--rounds 5] [--iters 30] [--out profiles/r08/mxfp4/bench.json]

--set a16: the weight-only type w4a16_g32_sym_MXFP4 instead — through AUTO, forced onto the small-batch
kernel (wo3) and onto v2x, against w4a16_g-1_sym through AUTO (the same kernels, integer dequant) and
w4a4_g32_sym_MXFP4 on v2x (the same weights, 4-bit activations); ratios are to the first side.

python tools/mxfp4_bench.py --set a16 --bs 128,512,2048,8192 --out profiles/r09/mxfp4_a16/bench.json

--set a8: w4a8_g32_sym_MXFP8 (MXFP8 activations on the same weights) — through AUTO, forced onto wo3 and
onto v2x (one of the two is AUTO's choice, the other "the other kernel"), against w4a4_g32_sym_MXFP4 on
v2x, w8a8_g-1_sym and w4a4_g-1_sym through AUTO; ratios are to the first side.

python tools/mxfp4_bench.py --set a8 --bs 128,512,2048,8192 --out profiles/r11/mxfp8_a8/bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mxmoe_amd import _native as nat  # noqa: E402
from mxmoe_amd.groupgemm import GroupGemm  # noqa: E402
from mxmoe_amd.harness import build_layer_inputs, time_launches  # noqa: E402
from mxmoe_amd.workload import load_workload, qwen2_layer11_workload  # noqa: E402

# side -> (qstr, forced variant name or None for AUTO); ratios are of the first side to the others
SETS = {"a4": {"mxfp4": ("w4a4_g32_sym_MXFP4", None), "w4a4": ("w4a4_g-1_sym", None), "w8a8": ("w8a8_g-1_sym", None)},
        "a16": {"a16": ("w4a16_g32_sym_MXFP4", None), "a16_wo3": ("w4a16_g32_sym_MXFP4", "wo3_64x256_w8_3wg"),
                "a16_v2x": ("w4a16_g32_sym_MXFP4", "v2x_256x256_w8_b3_buf_spread_edma"),
                "w4a16": ("w4a16_g-1_sym", None), "mxfp4": ("w4a4_g32_sym_MXFP4", None)},
        "a8": {"a8": ("w4a8_g32_sym_MXFP8", None), "a8_wo3": ("w4a8_g32_sym_MXFP8", "wo3_64x256_w8_3wg"),
               "a8_v2x": ("w4a8_g32_sym_MXFP8", "v2x_256x256_w8_b3_buf_spread_edma"),
               "mxfp4": ("w4a4_g32_sym_MXFP4", None), "w8a8": ("w8a8_g-1_sym", None), "w4a4": ("w4a4_g-1_sym", None)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="a4", choices=sorted(SETS))
    ap.add_argument("--bs", default="8192,512")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="profiles/r08/mxfp4/bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp4_bench: no GPU (a timing needs the device)")
    names = [ln.split()[1] for ln in nat.list_variants()]
    SIDES = SETS[args.set]
    first = next(iter(SIDES))
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "calls": []}
    for bs in (int(x) for x in args.bs.split(",")):
        for gg in ("gate_up", "down"):
            sides = {}
            built = {}
            for side, (qstr, vname) in SIDES.items():
                if qstr not in built:  # sides of one qcfg share their operands
                    built[qstr] = build_layer_inputs(load_workload(qwen2_layer11_workload(bs, qstr=qstr))["layer-11"][gg])
                inp = built[qstr]
                sides[side] = (inp, GroupGemm(inp.problems, variant=None if vname is None else names.index(vname)))
            t = {s: [] for s in sides}
            for _ in range(args.rounds):  # alternate: every round times every side once
                for s, (_, g) in sides.items():
                    t[s].append(time_launches(g.launch, args.warmup, args.iters)["median_ms"])
            row = {"bs": bs, "call": gg}
            for s, (inp, g) in sides.items():
                med = statistics.median(t[s])
                row[s] = {"qcfg": SIDES[s][0], "variant": names[g.variant], "tiles": g.total_tiles, "median_ms": round(med, 4),
                          "min_ms": round(min(t[s]), 4), "max_ms": round(max(t[s]), 4),
                          "spread_pct": round(100 * (max(t[s]) - min(t[s])) / med, 2),
                          "tops": round(inp.flops / (med * 1e-3) / 1e12, 1), "rounds_ms": [round(x, 4) for x in t[s]]}
            for s in list(SIDES)[1:]:
                row[f"{first}_over_{s}"] = round(row[first]["median_ms"] / row[s]["median_ms"], 4)
            res["calls"].append(row)
            print(json.dumps({k: (v if not isinstance(v, dict) else {x: v[x] for x in ("variant", "tiles", "median_ms", "min_ms",
                                                                                   "max_ms", "tops")})
                              for k, v in row.items()}), flush=True)
            del sides, built
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
