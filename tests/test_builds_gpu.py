"""One GPU call per entry of the product's kernel-build tables (gg_api.hip: kV2Builds of the default
variant v2x, kWo2Builds of the small-batch variant wo3): the exact entries and the fallbacks, the
WO_SILU list included. The other GPU tests reach the common quant-type sets only; a set that is
planned for one build and launched on another would show here as wrong results or a wrong LDS size.

A call has one problem per quant type of the entry's mask (mxmoe_amd.harness operands), checked by
mxmoe_amd.check with that module's tolerances; the plan info must name the entry's quant-type set and
its LDS size — the one observable of the build selection at run time.

Shapes: M = 129 per problem on v2x (a 128-row class tile plus a one-row tail), M = 65 on wo3 (two
64-row tiles, the second with one live row); N = 288 (one full and one partial column tile at either
width, N % 32 == 0 for SiLU); K = 640: five stages at the 128-byte stage (wraps the three-stage
rings), 2.5 stages for int4 (the in-kernel K tail), a multiple of 128 (g128), 64 (weight-only) and
32 (MX).

WO_SILU entries: the weight-only problems of the call carry MXMOE_GG_EPI_SILU_MUL over the same
operands (B rows read as gate / up blocks of 16), so their outputs are silu(gate) * up of columns of
the plain call's outputs — compared with the oracle SiLU of those to 1 fp16 ulp, as
tests/test_silu_epi.py does; the plain call of the same set is the non-SiLU entry's own test.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd.check import check_sampled
from mxmoe_amd.groupgemm import GroupGemm
from mxmoe_amd.harness import build_layer_inputs
from mxmoe_amd.workload import QShape
from oracle import moe_ref

pytestmark = pytest.mark.gpu

N, K = 288, 640
# QType bit -> (w_bits, a_bits, gsize, sym, fmt)
QTYPES = {0: (16, 16, -1, True, ""), 1: (8, 8, -1, True, ""), 2: (4, 4, -1, True, ""), 3: (4, 16, 128, False, ""),
          4: (8, 16, -1, False, ""), 5: (4, 4, 128, True, ""), 6: (2, 16, 128, False, ""), 7: (8, 8, -1, True, "E4M3"),
          8: (16, 16, -1, True, "bf16"), 10: (4, 4, 32, True, "MXFP4"), 11: (4, 16, 32, True, "MXFP4"),
          12: (4, 8, 32, True, "MXFP8")}
WEIGHT_ONLY = (1 << 3) | (1 << 4) | (1 << 6) | (1 << 11)
MX4, MXW, MX8 = 1 << 10, 1 << 11, 1 << 12
SILU = 1 << 16  # plan-info bit: a weight-only problem carries the SiLU flag

V2X, V2X_LDS = "v2x_256x256_w8_b3_buf_spread_edma", 160 * 1024
# kV2Builds, in table order: the exact entries, then the fallbacks narrowest first
V2X_BUILDS = [1, 2, 4, 6, 7, 8, 10, 16, 32, 64, 128, 256, MX4, MXW, MX8,
              63, 127, 511, 511 | MX4, 511 | MX4 | MXW, 511 | MX4 | MXW | MX8]

WO3, LDS_3WG, LDS_2WG = "wo3_64x256_w8_3wg", 52 * 1024, 78 * 1024
# kWo2Builds, in table order: (mask, LDS) — at three workgroups per CU, then the 2-WG/CU builds, then the WO_SILU list
WO3_BUILDS = [(8, LDS_3WG), (64, LDS_3WG), (10, LDS_3WG), (1, LDS_3WG), (2, LDS_3WG), (4, LDS_3WG), (6, LDS_3WG),
              (MXW, LDS_3WG), (MX8, LDS_3WG),
              (16, LDS_2WG), (95, LDS_2WG), (95 | MXW, LDS_2WG), (95 | MXW | MX8, LDS_2WG),
              (SILU | 8, LDS_3WG), (SILU | 10, LDS_3WG), (SILU | MXW, LDS_3WG),
              (SILU | 16, LDS_2WG), (SILU | 95, LDS_2WG), (SILU | 95 | MXW, LDS_2WG), (SILU | 95 | MXW | MX8, LDS_2WG)]


@pytest.fixture(scope="module")
def variants():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return [ln.split()[1] for ln in nat.list_variants()]


def _inputs(mask: int, M: int):
    bits = [b for b in sorted(QTYPES) if mask >> b & 1]
    assert sum(1 << b for b in bits) == mask & ~SILU
    shapes = [QShape([M, N, K], *QTYPES[b]) for b in bits]
    return build_layer_inputs(shapes, seed=100 + (mask & 0xFFFF)).problems, bits


def _run(problems, variant: int, mask: int, lds: int) -> None:
    gg = GroupGemm(problems, variant=variant)
    assert gg.info.qtype_mask == mask and gg.info.lds_bytes == lds, (hex(gg.info.qtype_mask), gg.info.lds_bytes)
    gg.launch()
    torch.cuda.synchronize()


@pytest.mark.parametrize("mask", V2X_BUILDS, ids=[hex(m) for m in V2X_BUILDS])
def test_v2x_build(variants, mask):
    problems, _ = _inputs(mask, 129)
    _run(problems, variants.index(V2X), mask, V2X_LDS)
    check_sampled(problems, n=129)


@pytest.mark.parametrize("mask,lds", WO3_BUILDS, ids=[hex(m) for m, _ in WO3_BUILDS])
def test_wo3_build(variants, mask, lds):
    M = 65
    problems, bits = _inputs(mask, M)
    wo3 = variants.index(WO3)
    if not mask & SILU:
        _run(problems, wo3, mask, lds)
        check_sampled(problems, n=129)
        return
    _run(problems, wo3, mask & ~SILU, dict(WO3_BUILDS)[mask & ~SILU])  # the plain call: the oracle's input
    fused = [dataclasses.replace(p, silu=True, C=torch.full((M, N // 2), float("nan"), dtype=torch.float16, device=p.C.device))
             if WEIGHT_ONLY >> b & 1 else dataclasses.replace(p, C=torch.empty_like(p.C)) for p, b in zip(problems, bits)]
    _run(fused, wo3, mask, lds)
    check_sampled([f for f in fused if not f.silu], n=129)
    # output column j = silu(gate) * up of the plain call's columns 32 (j / 16) + j % 16 and + 16
    j = np.arange(N // 2)
    gate = 32 * (j // 16) + j % 16
    for p, f in zip(problems, fused):
        if not f.silu:
            continue
        plain = p.C[:M].cpu().numpy()
        ref = moe_ref.silu_mul(np.concatenate([plain[:, gate], plain[:, gate + 16]], axis=1))
        out = f.C.cpu().numpy()
        assert np.isfinite(out).all()
        d = np.abs(out.view(np.uint16).astype(np.int32) - ref.view(np.uint16).astype(np.int32))
        same_sign = (np.signbit(out) == np.signbit(ref)) | (out == 0) | (ref == 0)
        assert same_sign.all() and (d <= 1).all(), f"{p.q.qcfg}: {int((d > 1).sum())} outputs > 1 ulp"
