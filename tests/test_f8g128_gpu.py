"""GPU tests of the w8a8_g128_sym_E4M3 tile body against tests/_f8g128_ref.py's f64 GEMM: random codes within the fp16
tolerance; integer codes with power-of-two scales (every fold exact in f32: tests/test_f8g128.py) bit for bit."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd.groupgemm import FP16, W8A8, W8A8_G128_E4M3, GroupGemm, Problem
from mxmoe_amd.quantize import pack_e4m3
from tests import _f8g128_ref as ref
from tests._util import HostProblem, assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
# M: the 128-row class alone, the 256-row class, 256 plus a tail tile; N: one scale block, a partial block, a 256-column
# tile plus a guarded one crossing a block boundary; K: one group, both LDS buffers, an odd count, several trips
SHAPES = [(M, N, K) for M in (1, 17, 129, 300) for N in (128, 200, 384) for K in (128, 256, 384, 1152)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _problem(M, N, K, ops) -> Problem:
    a, sa, b, sb = ops
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(DEV)  # noqa: E731
    return Problem(A=pack_e4m3(dev(a)), B=pack_e4m3(dev(b)), C=torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV),
                   M=M, N=N, K=K, q=W8A8_G128_E4M3, scale_a=dev(sa.T), scale_b=dev(sb.T))  # scales group-major


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_groupgemm_against_f64(exact):
    ops = [ref.operands(M, N, K, exact, 100 + i) for i, (M, N, K) in enumerate(SHAPES)]
    probs = [_problem(*s, o) for s, o in zip(SHAPES, ops)]
    gg = GroupGemm(probs)  # AUTO: the exact v2x build
    assert gg.variant == nat.default_variant()
    gg.launch()
    torch.cuda.synchronize()
    for (M, N, K), o, p in zip(SHAPES, ops, probs):
        out, want = p.C.cpu().numpy(), ref.gemm(*o)
        if exact:
            assert (out.view(np.uint16) == want.astype(np.float16).view(np.uint16)).all(), (M, N, K)
        else:
            assert_f16_close(out, want, K)


def test_mixed_launch_with_fp16_and_w8a8():
    """One call of the new type, fp16 and w8a8 problems: the widest fallback build; each against its own reference."""
    shapes = [(300, 384, 384), (33, 200, 1152)]
    ops = [ref.operands(*s, False, 7 + i) for i, s in enumerate(shapes)]
    probs = [_problem(*s, o) for s, o in zip(shapes, ops)]
    hps = [HostProblem(77, 128, 192, FP16, seed=1, device=DEV), HostProblem(513, 256, 128, W8A8, seed=2, device=DEV)]
    GroupGemm([probs[0], hps[0].problem, probs[1], hps[1].problem]).launch()
    torch.cuda.synchronize()
    for s, o, p in zip(shapes, ops, probs):
        assert_f16_close(p.C.cpu().numpy(), ref.gemm(*o), s[2])
    assert_f16_close(hps[0].result(), hps[0].expected(), 192)
    assert (hps[1].result().view(np.uint16) == hps[1].expected().view(np.uint16)).all()
