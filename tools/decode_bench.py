"""The decode forward against the graph forward: qwen2_moe layer 11 (LP-1 mixed w4a4 + w8a8) at T = 1 / 4 / 16, run as
  (a) GraphForward replayed from a captured graph (route, segments, device planner, two GroupGEMMs, ...);
  (b) DecodeForward replayed from a captured graph (decode_gate_up, decode_down, combine; no planner),
in one process with the sides alternating over rounds (moe_bench.decode_forward_bench): device and wall time of both,
the two decode kernels alone, the plain-layout variant and the combine. One JSON line per T; --out also writes the
list to a file (profiles/<round>/decode/bench.json). Exits 1 when an output is not bit-identical to the eager layer.

--model gpt-oss: a synthetic gpt-oss layer instead (moe_bench.decode_forward_gptoss_bench: gptoss_layer of E = 32,
topk = 4, H = N = 2880, random codes, scale bytes in [118, 126]), DecodeForwardEx against GraphForward of the same layer,
with the two _ex kernels and the bias combine alone, the weight bytes read and the TB/s they imply. Exits 1 when an
output is not within the fp16 tolerance of the eager layer (MXFP4 sums depend on their order).

--model qwen2_moe --scheme w4a16_w8a8: layer 11 with the reference's small-batch scheme instead of LP-1
(workload.w4a16_w8a8_qconfig: w4a16_g-1_asym + w8a8 per linear, the shared expert included;
moe_bench.decode_forward_wo_bench), DecodeForwardWo against GraphForward of the same layer, with the two _wo kernels and
the combine alone, the weight bytes read and the TB/s they imply. Exits 1 when an output is not within the fp16
tolerance of the eager layer (weight-only sums depend on their order).

python tools/decode_bench.py [--model qwen2_moe|gpt-oss] [--scheme lp1|w4a16_w8a8] [--rounds 4] [--iters 30]
                             [--batches 1,4,16] [--out FILE]
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
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--out", default="")
    ap.add_argument("--model", default="qwen2_moe", choices=["qwen2_moe", "gpt-oss"])
    ap.add_argument("--scheme", default="lp1", choices=["lp1", "w4a16_w8a8"], help="qwen2_moe: the layer's qconfig")
    args = ap.parse_args()
    if args.model == "gpt-oss" and args.scheme != "lp1":
        ap.error("--scheme belongs to --model qwen2_moe")
    results = []
    wo = args.scheme == "w4a16_w8a8"
    bench = moe_bench.decode_forward_gptoss_bench if args.model == "gpt-oss" else \
        moe_bench.decode_forward_wo_bench if wo else moe_bench.decode_forward_bench
    for r in bench([int(b) for b in args.batches.split(",") if b], args.rounds, args.iters):
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    same = "close_to_eager" if args.model == "gpt-oss" or wo else "bit_identical_to_eager"
    if not all(all(r[same].values()) and not any(r["status"].values()) for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
