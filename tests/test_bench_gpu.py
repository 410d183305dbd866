"""bench.py on the GPU: a plain run (no --full) times its steps and prints the result line with nothing
that needs runs of its own; --dump-outputs writes what the timed path computed. Run once, on the
small-batch fp16 config (bs 512; its calls are large enough to be sampled): the dumped outputs of
every problem against a float32 torch matmul of the same seeded inputs at the dump's indices
(bench.dump_indices), within the fp16 tolerance of the other fp16 parity tests
(tests/_util.assert_f16_close)."""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest

import bench
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
CFG = "fp16_bs512"


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench") / "dump"
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", "3", "--warmup", "2", "--config", CFG,
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), d


def test_plain_run_reports_the_headline_only(plain_run):
    line, _ = plain_run
    assert line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "TFLOP/s" and line["higher_is_better"] is True and line["dtype"] == "fp16"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    flops = sum(s.flops for gg in ("gate_up", "down") for s in bench.layer_shapes(CFG, 1, 0)[gg])
    # both are rounded in the line (ms_per_step to 1e-4 ms of a step of some 0.1 ms)
    assert line["value"] == pytest.approx(flops / (line["ms_per_step"] * 1e-3) / 1e12, rel=5e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["extras"] == {}


def test_dumped_outputs_are_the_steps_results(plain_run):
    from mxmoe_amd.harness import build_layer_inputs

    _, d = plain_run
    assert sorted(p.name for p in d.iterdir()) == ["down.npy", "gate_up.npy"]
    shapes = bench.layer_shapes(CFG, 1, 0)
    for ci, gg in enumerate(("gate_up", "down")):
        got = np.load(d / f"{gg}.npy")
        assert got.dtype == np.float32 and got.ndim == 1
        total = sum(s.M * s.N for s in shapes[gg])
        inp = build_layer_inputs(shapes[gg], device="cuda:0", seed=42 + (gg == "down"))  # the run's seeds
        at = 0
        for pi, p in enumerate(inp.problems):
            if p.M == 0:
                continue
            ref = (p.A.float() @ p.B.float().t()).reshape(-1)
            idx = bench.dump_indices(ci, pi, p.M * p.N, total)  # None: the call is dumped whole
            if idx is not None:
                ref = ref[idx.to(ref.device)]
            assert_f16_close(got[at:at + ref.numel()], ref.cpu().numpy(), p.K)
            at += ref.numel()
        assert at == got.size and got.nbytes <= 32e6
