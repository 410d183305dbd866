"""Shared helpers of the decode forward's tests (tests/test_decode*.py): the CPU files' calls of the six
mxmoe_moe_decode_* entries on made-up addresses and their host layer, and the GPU files' seeded layers, routings and
the stage-by-stage comparison with the eager layer.

The eager intermediates are in slot order (sorted by expert), the decode buffers in pair order: row p of ``act`` / ``y``
is row inv_slot[p] of the eager one."""
from __future__ import annotations

import ctypes

import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from tests._util import assert_f16_close

DEV = "cuda:0"
GUARD = 0x7B7B
SUFFIX = {"first": "", "ex": "_ex", "wo": "_wo"}  # the entry levels, by the suffix of their symbols

# ---- the entries, called as they are (no GPU: the refusals come before any HIP call) ---------------------------------


def err():
    return nat.lib().mxmoe_gg_last_error()


def entry_gate_up(level, glu=None, dtype=nat.DT_FP16, hidden=16, T=4, topk=2, E=4, with_shared=1, ids=16, experts=16,
                  mask=0b111, H=256, N=128, Ns=256, layout=nat.DECODE_GU_PLAIN, act=16, act_shared=16, status=None):
    """mxmoe_moe_decode_gate_up<level's suffix> on made-up addresses; the _ex and _wo entries take the mxmoe_moe_glu."""
    head = () if level == "first" else (glu,)
    return nat.symbol("mxmoe_moe_decode_gate_up" + SUFFIX[level])(*head, dtype, hidden, T, topk, E, with_shared, ids, experts,
                                                                  mask, H, N, Ns, layout, act, act_shared, status, None)


def entry_down(level, T=4, topk=2, E=4, with_shared=1, ids=16, experts=16, mask=0b111, H=256, N=128, Ns=256, act=16,
               act_shared=16, y=16, ys=16, status=None):
    return nat.symbol("mxmoe_moe_decode_down" + SUFFIX[level])(T, topk, E, with_shared, ids, experts, mask, H, N, Ns, act,
                                                               act_shared, y, ys, status, None)


def cpu_ffn(qcfg, E=2, H=256, N=128, Ns=128, **kw):
    """a small layer on the host (E experts and the shared one): what the classes' constructors are asked to refuse"""
    g = torch.Generator().manual_seed(5)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half()
    return moe.MoEFFN([mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)], [mk(H, N) for _ in range(E)] + [mk(H, Ns)], qcfg,
                      num_routed=E, **kw)


def down_raw(level, T, topk, E, shared, ids, experts, mask, H, N, Ns, act, act_shared, y, ys, status):
    """The down entry of a level alone, on the caller's own device buffers."""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    nat.check(entry_down(level, T, topk, E, shared, p(ids), p(experts), mask, H, N, Ns, p(act), p(act_shared), p(y), p(ys),
                         p(status)))


# ---- seeded data ------------------------------------------------------------------------------------------------------


def bits(t):
    return t.view(torch.int16)


def guard(df):
    bufs = [t for t in (df.act, df.act_shared, df.y, df.ys, df.out) if t is not None]
    for t in bufs:
        bits(t).fill_(GUARD)
    return bufs


def hidden(g, T, H, grid=False, dtype=torch.float16, step=8, bound=2):
    """randn, or (grid) multiples of 1 / step in [-bound, bound] (exact in bf16 too)"""
    if grid:
        return (torch.randint(-step * bound, step * bound + 1, (T, H), generator=g).float() / step).to(dtype).to(DEV)
    return torch.randn(T, H, generator=g).to(dtype).to(DEV)


def routing(g, T, E, topk):
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
    sw = torch.rand(T, generator=g).to(DEV)
    return ids, wts, sw


def f16_weights(g, E, H, N, Ns, grid=False):
    """gate_up [2N, H] and down [H, N] per expert (the shared one, if Ns, last): uniform in +-0.2 as the graph tests
    draw them, or (grid) multiples of 1/4 in [-1, 1]."""
    if grid:
        mk = lambda n, k: (torch.randint(-4, 5, (n, k), generator=g).float() / 4).half().to(DEV)
    else:
        mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)
    return [mk(2 * N, H) for _ in range(E)] + ([mk(2 * Ns, H)] if Ns else []), \
        [mk(H, N) for _ in range(E)] + ([mk(H, Ns)] if Ns else [])


def biases(g, E, H, N, Ns):
    """gate_up and down bias rows in +-0.5, the shared expert's last"""
    mk = lambda n: (torch.rand(n, generator=g) - 0.5).half().to(DEV)
    return [mk(2 * N) for _ in range(E)] + ([mk(2 * Ns)] if Ns else []), [mk(H) for _ in range(E + (1 if Ns else 0))]


def mx_codes(g, rows, K, lo, hi):
    """random e2m1 codes [rows, K/2] and e8m0 scale bytes [rows, K/32] in [lo, hi] (host)"""
    return (torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.uint8),
            torch.randint(lo, hi + 1, (rows, K // 32), generator=g, dtype=torch.uint8))


# ---- against the eager layer ------------------------------------------------------------------------------------------


def eager_act(ffn, mid):
    """The eager layer's fp16 activation rows (routed in slot order, shared): its own activation pass run with fp16
    tags on its gate_up output — for a layer whose down tags are fp16, the rows it fed to the down GroupGEMM."""
    r, tags = mid["routing"], [moe.ACT_FP16] * (ffn.E + (1 if ffn.has_shared else 0))
    if mid["h1"].shape[1] == ffn.N:  # the SiLU epilogue ran: h1 is act
        return mid["h1"], mid["h1s"]
    if ffn.biased_or_gated:
        a = moe.glu_quant(mid["h1"], mid["h1s"], r, tags, ffn.activation, ffn.b1, ffn.b1s)
    else:
        a = moe.silu_mul_quant(mid["h1"], mid["h1s"], r, tags, interleaved=ffn.gate_up_layout() != "plain")
    torch.cuda.synchronize()
    return torch.cat([a.A(e) for e in range(ffn.E)]), a.A(ffn.E) if ffn.has_shared else None


def check_stages(df, ffn, h, ids, wts, sw, stages=("act", "y", "out")):
    """One call through ``df`` against the eager layer, stage by stage (so the first wrong one is named): the stages
    "act", "y", "out" bit for bit, "close": out within the project's fp16 tolerance. Returns the eager intermediates."""
    T, topk = ids.shape
    n = T * topk
    got = df.launch(h, ids, wts, sw).clone()
    want, mid = ffn.forward(h, ids, wts, sw, return_intermediates=True)
    torch.cuda.synchronize()
    inv = mid["routing"].inv_slot.long()
    if "act" in stages:
        act, act_s = eager_act(ffn, mid)
        assert torch.equal(bits(df.act[:n]), bits(act[inv])), "gate_up (routed act)"
        if ffn.has_shared:
            assert torch.equal(bits(df.act_shared[:T]), bits(act_s)), "gate_up (shared act)"
    if "y" in stages:
        assert torch.equal(bits(df.y[:n]), bits(mid["y"][inv])), "down (routed y)"
        if ffn.has_shared:
            assert torch.equal(bits(df.ys[:T]), bits(mid["ys"])), "down (shared ys)"
    if "out" in stages:
        assert torch.equal(bits(got), bits(want)), "combine"
    if "close" in stages:
        assert_f16_close(got.float().cpu().numpy(), want.float().cpu().numpy(), ffn.H)
    return mid
