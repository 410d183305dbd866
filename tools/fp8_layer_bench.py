"""FP8 layers: the qwen2_moe layer-11 shape with every expert w8a8_g-1_sym_E4M3, w8a8_g-1_sym or fp16, as
PlannedForward steps at bs 128 / 512 / 2048 / 8192 in one process, the sides alternating over rounds: per-stage and
per-step device times, the variants AUTO chose, and the two E4M3 activation passes against the INT8 passes
(moe_bench.fp8_layer_bench). One JSON line per batch size; --out also writes the list to a file
(profiles/<round>/fp8_layer/bench.json).

python tools/fp8_layer_bench.py [--rounds 4] [--iters 30] [--batches 128,512,2048,8192] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxmoe_amd import moe_bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", default="128,512,2048,8192")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    results = []
    for r in moe_bench.fp8_layer_bench([int(b) for b in args.batches.split(",") if b], args.rounds, args.iters):
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
