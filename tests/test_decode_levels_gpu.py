"""GPU tests of the one decode kernel template behind the three entry levels (moe.DecodeForward, DecodeForwardEx,
DecodeForwardWo; DESIGN.md §4 "Decode forward: one kernel body"):

* a layer of kinds that more than one level accepts gives the same bytes through every one of them, in both kernels
  and both gate_up layouts;
* the kinds whose results depend on the order of their f32 additions (fp16, W4A16_MX, the weight-only kinds) reproduce
  the bytes recorded in tests/golden/decode_bytes.json from the three separate loops this template replaced: step
  ascending, within a step run or dword ascending, within a run element ascending. The integer kinds need no golden
  bytes: they are checked bit for bit against the eager layer (tests/test_decode_gpu.py)."""
from __future__ import annotations

import hashlib
import json
from pathlib import Path

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W4A16_G128_ASYM, W4A16_MXFP4, W8A8, QParams
from tests._decode_util import DEV, biases, bits, f16_weights, guard, hidden, mx_codes, routing

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden" / "decode_bytes.json"
LEVELS = {"first": moe.DecodeForward, "ex": moe.DecodeForwardEx, "wo": moe.DecodeForwardWo}
MX = W4A16_MXFP4
W8A16_SYM = QParams(16, 8, -1, True)

# ---- the same bytes through every level -------------------------------------------------------------------------------

# E = 5 and the shared expert; a row of kinds per layer, every linear of the layer in turn
KIND_ROWS = {"fp16": [(FP16, FP16)] * 6,
             "w8a8": [(W8A8, W8A8)] * 6,
             "w4a4": [(W4A4, W4A4)] * 6,
             "mx": [(MX, MX)] * 6}


@pytest.fixture(scope="module")
def level_data():
    """one set of fp16 weights, three routings and hidden states, shared by every case"""
    E, H, N, Ns, topk = 5, 640, 384, 256, 2
    g = torch.Generator().manual_seed(800)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    calls = {T: (hidden(g, T, H), *routing(g, T, E, topk)) for T in (1, 7, 16)}
    return gate_up, down, calls


@pytest.mark.parametrize("fuse", [True, False], ids=["interleaved", "plain"])
@pytest.mark.parametrize("row", list(KIND_ROWS))
def test_levels_give_the_same_bytes(level_data, row, fuse):
    """E = 5 plus the shared expert, H = 640, N = 384, N_shared = 256, topk = 2, T in {1, 7, 16}: a 4-bit weight row
    ends inside its first 256-byte step (gate_up: 320 bytes end inside the second; down: 192 and 128 inside the first)
    and an fp16 row of 1280 bytes spans more than one group of four steps. Kinds 0 to 2 run through all three levels,
    W4A16_MX through _ex and _wo: act, act_shared, y and ys are byte-equal across levels."""
    gate_up, down, calls = level_data
    E, topk = 5, 2
    ffn = moe.MoEFFN(gate_up, down, KIND_ROWS[row], num_routed=E, fuse_silu=fuse)
    names = ["ex", "wo"] if row == "mx" else ["first", "ex", "wo"]
    for T, (h, ids, wts, sw) in calls.items():
        dfs = [LEVELS[n](ffn, T, topk) for n in names]
        for df in dfs:
            guard(df)
            df.launch(h, ids, wts, sw)
        torch.cuda.synchronize()
        ref = dfs[0]
        assert {df.layout for df in dfs} == {nat.DECODE_GU_INTERLEAVED if fuse else nat.DECODE_GU_PLAIN}
        for name, df in zip(names[1:], dfs[1:]):
            for what in ("act", "act_shared", "y", "ys"):
                assert torch.equal(bits(getattr(df, what)), bits(getattr(ref, what))), (T, name, what)
            assert df.status() == 0
        assert ref.status() == 0


# ---- golden bytes of the order-dependent kinds ------------------------------------------------------------------------

GOLDEN_KINDS = ("fp16", "w4a16_g32_sym_MXFP4", "w4a16_g128_asym", "w8a16_g-1_sym")
GOLDEN_KS = (384, 640, 2176)


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def golden_case(kind: str, K: int) -> dict:
    """sha256 of act, y and out of one fixed-seed call: T = 7, topk = 2, E = 4 and the shared expert, H = N = N_shared =
    K (so both linears have rows of K elements), random data. fp16 through DecodeForward; W4A16_MX (random codes, scale
    bytes 120..126) with all four biases and SwigluClamp through DecodeForwardEx; the weight-only kinds through
    DecodeForwardWo."""
    T, topk, E = 7, 2, 4
    g = torch.Generator().manual_seed(900 + GOLDEN_KINDS.index(kind) * 10 + GOLDEN_KS.index(K))
    kw = {}
    if kind == "w4a16_g32_sym_MXFP4":
        mk = lambda rows, k: moe.prepare_weight_mx(*(t.to(DEV) for t in mx_codes(g, rows, k, 120, 126)), MX)
        gate_up, down = [mk(2 * K, K) for _ in range(E + 1)], [mk(K, K) for _ in range(E + 1)]
        b1, b2 = biases(g, E, K, K, K)
        kw = dict(gate_up_bias=b1, down_bias=b2, activation=moe.SwigluClamp())
        q, cls = MX, moe.DecodeForwardEx
    else:
        gate_up, down = f16_weights(g, E, K, K, K)
        q, cls = {"fp16": (FP16, moe.DecodeForward), "w4a16_g128_asym": (W4A16_G128_ASYM, moe.DecodeForwardWo),
                  "w8a16_g-1_sym": (W8A16_SYM, moe.DecodeForwardWo)}[kind]
    ffn = moe.MoEFFN(gate_up, down, [(q, q)] * (E + 1), num_routed=E, **kw)
    df = cls(ffn, T, topk)
    guard(df)
    ids, wts, sw = routing(g, T, E, topk)
    out = df.launch(hidden(g, T, K), ids, wts, sw)
    torch.cuda.synchronize()
    assert df.status() == 0
    return {"act": _sha(df.act), "y": _sha(df.y), "out": _sha(out)}


@pytest.mark.parametrize("K", GOLDEN_KS)
@pytest.mark.parametrize("kind", GOLDEN_KINDS)
def test_golden_bytes(kind, K):
    """Weight rows of K / 2 (4-bit), K (8-bit) and 2 K (fp16) bytes in steps of 256 and groups of four steps. K = 384:
    the 4-bit row ends inside the first step, the others inside the first group; 640: the fp16 row ends in the first
    step of the second group; 2176: every row ends past one group, inside a step (4-bit: second group, 8-bit: third,
    fp16: fifth). The bytes are those of the parent of the commit that folded the loops."""
    want = json.loads(GOLDEN.read_text())["cases"][f"{kind}/K{K}"]
    assert golden_case(kind, K) == want
