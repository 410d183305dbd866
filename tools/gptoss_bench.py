"""A gpt-oss-20b-shaped MoE block (E = 32, top-4, H = N = 2880 padded to 2944, MXFP4 weights, biases, clamped SwiGLU,
router logit bias) at bs 1 / 16 / 128 / 512 / 2048, with fp16 (a16) and MXFP8 (a8) activations, each run as
  (a) eager MoEBlock.forward — wall time per call, one synchronise per call;
  (b) PlannedForward — device time of the host-planned step;
  (c) GraphForward replayed from a captured graph — wall and device time;
and the biased clamped activation pass against the SiLU pass, combine_bias against combine, at the same shape, in one
process with the sides alternating over rounds (moe_bench.gptoss_bench). One JSON line per (act_bits, bs); --out also writes
the list to a file (profiles/<round>/gptoss/bench.json).

python tools/gptoss_bench.py [--rounds 4] [--iters 20] [--batches 1,16,128,512,2048] [--act-bits 16,8] [--out FILE]
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
    ap.add_argument("--batches", default="1,16,128,512,2048")
    ap.add_argument("--act-bits", default="16,8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    results = []
    batches = [int(b) for b in args.batches.split(",") if b]
    for bits in [int(b) for b in args.act_bits.split(",") if b]:
        for r in moe_bench.gptoss_bench(batches, bits, args.rounds, args.iters):
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    # (the graph replay is bit-identical to the eager call only where no host plan split K: moe_bench.gptoss_bench)
    if not all(r["planned_bit_identical_to_eager"] and r["status"] == 0 and
               (r["bit_identical_to_eager"] or max(r["host_splitk_slabs"]) > 0) for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
