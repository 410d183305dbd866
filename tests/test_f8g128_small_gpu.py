"""GPU tests of the w8a8_g128_sym_E4M3 body of the small-batch kernel (wo3): forced wo3 against tests/_f8g128_ref.py's f64
GEMM and bit for bit against the default variant's body, a strided C, and an all-block-scaled layer AUTO puts on wo3."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import W8A8_G128_E4M3, GroupGemm, Problem
from mxmoe_amd.quantize import pack_e4m3
from tests import _f8g128_ref as ref
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
# M: three row blocks skipped, a block boundary, a full tile, a second tile of one row, three tiles with a 2-row tail;
# N: one tile, a guarded tile with a partial scale block, three tiles; K: one group, both buffers, an odd count, many trips
SHAPES = [(M, N, K) for M in (1, 17, 64, 65, 130) for N in (128, 200, 384) for K in (128, 256, 384, 1152)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _wo3() -> int:
    return [ln.split()[1] for ln in nat.list_variants()].index("wo3_64x256_w8_3wg")


def _problem(M, N, K, ops, ldc=None) -> Problem:
    a, sa, b, sb = ops
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(DEV)  # noqa: E731
    C = torch.full((M + 3, ldc or N), float("nan"), dtype=torch.float16, device=DEV)
    return Problem(A=pack_e4m3(dev(a)), B=pack_e4m3(dev(b)), C=C[:M, :N], M=M, N=N, K=K, q=W8A8_G128_E4M3,
                   scale_a=dev(sa.T), scale_b=dev(sb.T), ldc=ldc or 0)  # scales group-major


def _check(out, want, K, exact, what):
    if not exact:
        return assert_f16_close(out, want, K)
    assert (out.view(np.uint16) == want.astype(np.float16).view(np.uint16)).all(), what


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_forced_wo3_against_f64(exact):
    ops = [ref.operands(M, N, K, exact, 300 + i) for i, (M, N, K) in enumerate(SHAPES)]
    probs = [_problem(*s, o) for s, o in zip(SHAPES, ops)]
    GroupGemm(probs, variant=_wo3()).launch()
    torch.cuda.synchronize()
    outs = [p.C.cpu().numpy() for p in probs]
    for s, o, out in zip(SHAPES, ops, outs):
        _check(out, ref.gemm(*o), s[2], exact, s)
    if not exact:  # any operands: the same bits as the default variant's body
        twins = [_problem(*s, o) for s, o in zip(SHAPES, ops)]
        GroupGemm(twins, variant=nat.default_variant()).launch()
        torch.cuda.synchronize()
        for s, out, t in zip(SHAPES, outs, twins):
            assert (out.view(np.uint16) == t.C.cpu().numpy().view(np.uint16)).all(), s


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_strided_c(exact):
    M, N, K = 17, 200, 384
    ops = ref.operands(M, N, K, exact, 77)
    p = _problem(M, N, K, ops, ldc=256)
    GroupGemm([p], variant=_wo3()).launch()
    torch.cuda.synchronize()
    full = p.C._base.cpu().numpy()  # [M + 3, 256]
    assert np.isnan(full[:, N:]).all() and np.isnan(full[M:]).all()
    _check(full[:M, :N].copy(), ref.gemm(*ops), K, exact, "ldc")


def test_layer_runs_wo3_and_graph_matches_eager():
    E, topk, H, N, T = 8, 2, 384, 256, 40
    g = torch.Generator().manual_seed(11)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)  # noqa: E731
    ffn = moe.MoEFFN([mk(2 * N, H) for _ in range(E)], [mk(H, N) for _ in range(E)], [(W8A8_G128_E4M3,) * 2] * E, num_routed=E)
    gf = moe.GraphForward(ffn, T, topk)
    for rep in range(2):
        h = torch.randn(T, H, generator=g).half().to(DEV)
        ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
        wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
        out, mid = ffn.forward(h, ids, wts, return_intermediates=True)
        calls = ffn.gate_up_call(mid["a1"], T, topk, out.device)[0], ffn.down_call(mid["a2"], T, topk, out.device)[0]
        assert [c.variant for c in calls] == [_wo3()] * 2
        assert torch.equal(gf.launch(h, ids, wts), out), rep
    assert gf.status() == 0
