"""What the host costs a MoE layer, and what the capacity grid costs the device: qwen2_moe layer 11 (LP-1 mixed
w4a4 + w8a8) at bs 1 / 16 / 128 / 512 / 2048 and the DeepSeek-V2-Lite mixed layer at bs 128, each run as
  (a) eager MoEFFN.forward — wall time per call, one synchronise per call;
  (b) PlannedForward — device time of the host-planned step (the lower bound: XCD packing, split-K);
  (c) GraphForward replayed from a captured graph — wall and device time,
in one process with the sides alternating over rounds (moe_bench.graph_forward_bench). One JSON line per (model, bs);
--out also writes the list to a file (profiles/<round>/graph_forward/bench.json).

python tools/graph_bench.py [--rounds 4] [--iters 20] [--batches 1,16,128,512,2048] [--ds2 128] [--out FILE]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", default="1,16,128,512,2048", help="qwen2_moe batch sizes ('' = none)")
    ap.add_argument("--ds2", default="128", help="DeepSeek-V2-Lite batch sizes ('' = none)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    results = []
    for model, spec in (("qwen2_moe", args.batches), ("ds2", args.ds2)):
        batches = [int(b) for b in spec.split(",") if b]
        if not batches:
            continue
        for r in moe_bench.graph_forward_bench(batches, model, args.rounds, args.iters):
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    if not all(r["bit_identical_to_eager"] and r["status"] == 0 for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
