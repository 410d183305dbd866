"""gpt-oss MoE layers on the GPU: the activation pass with bias and the clamped SwiGLU (mxmoe_moe_glu_quant), the
combine with a down bias (mxmoe_moe_combine_bias), the router's logit bias (mxmoe_moe_gate_ex2) and a layer built
from a synthetic MXFP4 checkpoint, stage by stage, eager / planned / graph. Reference: tests/_gptoss_ref.py (pinned to
the public model code in tests/test_gptoss.py).

Bars. Identity and indexing checks (G1-G3, G5, G8) are byte comparisons. The activation against the libm
restatement (G4, G7) takes the SiLU pass's own bars (tests/test_moe.py): 1 fp16 ulp for the activation, 1 ulp for a
scale and one step for a code. GEMM stages: assert_f16_close against the f64 product on the dequantised weights.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd import quantize as qz
from oracle import moe_ref, oracle
from tests import _gate_modes_ref as mref
from tests import _gate_ref as gref
from tests import _gptoss_ref as ref
from tests import _mxfp4_ref as ref4
from tests import _mxfp8_ref as ref8
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 8
CLAMP = moe.SwigluClamp(1.702, 7.0)
TOKENS = [(61, 4), (33, 3)]
INT_TAGS = [0, 1, 2, 3, 0, 1, 2, 3]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _ids(T, topk, n_exp, seed):
    """distinct experts per token, skewed popularity, expert 3 left empty (tests/test_moe.py's routing)"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.rand(T, n_exp, generator=g) + torch.linspace(0, 1.5, n_exp)
    logits[:, 3] = -1.0
    return torch.topk(logits, topk, dim=1).indices.to(torch.int32)


def _tags(kind, shared):
    t = {"int": INT_TAGS, "mxfp4": [4] * E, "mxfp8": [6] * E, "mixed": [4, 6, 0, 1, 2, 3, 6, 4]}[kind]
    return t + ([{"int": 1, "mxfp4": 4, "mxfp8": 6, "mixed": 6}[kind]] if shared else [])


def _same_batches(a, b, what):
    """Every segment's stored rows and scales byte for byte (what lies between segments is padding)."""
    assert a.qtags == b.qtags
    for e, s in enumerate(a.segs):
        if not s.rows:
            continue
        x, y = a.A(e), b.A(e)
        assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), \
            f"{what}: seg {e} (tag {a.qtags[e]}) rows differ"
        if a.qtags[e] != moe.ACT_FP16:
            sx, sy = a.scale(e), b.scale(e)
            assert torch.equal(sx.contiguous().view(torch.uint8), sy.contiguous().view(torch.uint8)), f"{what}: seg {e} scales"


def _grid_values(shape, g, lim=4.0, step=16):
    """multiples of 1 / step in [-lim, lim] as fp16"""
    n = int(lim * step)
    return (torch.randint(-n, n + 1, shape, generator=g).float() / step).half()


def _segments(r, slot_rows, shared_rows):
    starts = np.concatenate([[0], np.cumsum(r.counts)])
    return [slot_rows[starts[e]:starts[e + 1]] for e in range(r.E)] + ([shared_rows] if shared_rows is not None else [])


# ------------------------------------------------------------------ G1: SILU without a bias is the old pass

@pytest.mark.parametrize("kind", ["int", "mxfp4", "mxfp8"])
@pytest.mark.parametrize("N,Ns", [(256, 512), (256, 640), (384, None)])
@pytest.mark.parametrize("T,topk", TOKENS)
def test_g1_silu_without_bias_is_the_old_pass(T, topk, N, Ns, kind):
    r = moe.route(_ids(T, topk, E, 7).to(DEV), E)
    g = torch.Generator().manual_seed(8)
    routed = ((torch.rand(T * topk, 2 * N, generator=g) * 2 - 1) * 4).half().to(DEV)
    shared = ((torch.rand(T, 2 * Ns, generator=g) * 2 - 1) * 4).half().to(DEV) if Ns else None
    tags = _tags(kind, Ns is not None)
    old = moe.silu_mul_quant(routed, shared, r, tags)
    new = moe.glu_quant(routed, shared, r, tags, "silu")
    torch.cuda.synchronize()
    _same_batches(new, old, f"N={N} Ns={Ns} {kind}")


# ------------------------------------------------------------------ G2: bias indexing, bit-exact

@pytest.mark.parametrize("kind", ["int", "mixed"])
@pytest.mark.parametrize("T,topk,N,Ns", [(61, 4, 256, 512), (33, 3, 256, 640), (61, 4, 384, None), (9, 2, 2944, None),
                                          (33, 3, 256, 256)])
def test_g2_bias_is_added_per_expert_and_half(T, topk, N, Ns, kind):
    """h1 and the bias are multiples of 2^-4 in [-4, 4], so fp16(h1 + b) is exact and the biased pass must equal the
    old pass on the pre-added input byte for byte. The bias differs per expert and between its gate and up halves;
    (256, 640) splits the shared row over 4 waves (the bias then indexed from col0), 2944 is six chunks, the last
    one partial."""
    ids = _ids(T, topk, E, 17)
    r = moe.route(ids.to(DEV), E)
    g = torch.Generator().manual_seed(18)
    routed = _grid_values((T * topk, 2 * N), g)
    shared = _grid_values((T, 2 * Ns), g) if Ns else None
    b_routed = _grid_values((E, 2 * N), g)
    b_shared = _grid_values((2 * Ns,), g) if Ns else None
    assert not torch.equal(b_routed[0], b_routed[1]) and not torch.equal(b_routed[:, :N], b_routed[:, N:])
    sorted_e = torch.sort(ids.view(-1).long(), stable=True).values
    pre = (routed.float() + b_routed[sorted_e].float()).half()
    assert torch.equal(pre.float(), routed.float() + b_routed[sorted_e].float())  # exact by construction
    pre_s = (shared.float() + b_shared.float()).half() if Ns else None
    tags = _tags(kind, Ns is not None)
    dev = lambda t: None if t is None else t.to(DEV)
    new = moe.glu_quant(dev(routed), dev(shared), r, tags, "silu", dev(b_routed), dev(b_shared))
    old = moe.silu_mul_quant(dev(pre), dev(pre_s), r, tags)
    torch.cuda.synchronize()
    _same_batches(new, old, f"N={N} Ns={Ns} {kind}")
    if Ns:  # one bias without the other
        only_r = moe.glu_quant(dev(routed), dev(shared), r, tags, "silu", dev(b_routed), None)
        half = moe.silu_mul_quant(dev(pre), dev(shared), r, tags)
        torch.cuda.synchronize()
        _same_batches(only_r, half, "routed bias only")


# ------------------------------------------------------------------ G3: the clamp

@pytest.mark.parametrize("kind", ["int", "mixed"])
@pytest.mark.parametrize("T,topk", TOKENS)
def test_g3_clamp_is_idempotent(T, topk, kind):
    """SWIGLU_CLAMP on inputs spanning [-12, 12] (with +-7 exactly) equals the same call on the pre-clamped input:
    7.0 is an fp16 value, min / max of fp16 values are exact."""
    N, Ns = 256, 640
    r = moe.route(_ids(T, topk, E, 27).to(DEV), E)
    g = torch.Generator().manual_seed(28)
    routed = ((torch.rand(T * topk, 2 * N, generator=g) * 2 - 1) * 12).half()
    shared = ((torch.rand(T, 2 * Ns, generator=g) * 2 - 1) * 12).half()
    for x in (routed, shared):
        x[:, 0::7] = 7.0
        x[:, 3::7] = -7.0
    assert routed.max() > 11 and routed.min() < -11
    tags = _tags(kind, True)
    got = moe.glu_quant(routed.to(DEV), shared.to(DEV), r, tags, CLAMP)
    pre = moe.glu_quant(torch.from_numpy(ref.clamp_inputs(routed.numpy())).to(DEV),
                        torch.from_numpy(ref.clamp_inputs(shared.numpy())).to(DEV), r, tags, CLAMP)
    torch.cuda.synchronize()
    _same_batches(got, pre, kind)
    plain = moe.glu_quant(routed.to(DEV), shared.to(DEV), r, [0] * (E + 1), CLAMP)  # and the clamp does bite
    silu = moe.glu_quant(routed.to(DEV), shared.to(DEV), r, [0] * (E + 1), "silu")
    torch.cuda.synchronize()
    assert not torch.equal(plain.out, silu.out)


# ------------------------------------------------------------------ G4: the activation against the reference

def _act_against_ref(b, want_rows, tags, what):
    """tests/test_moe.py's bars for the SiLU pass; returns (exactly equal, total) elements."""
    exact = total = 0
    for e, (x, tag) in enumerate(zip(want_rows, tags)):
        if x.shape[0] == 0:
            continue
        got = b.A(e).cpu().numpy()
        if tag == moe.ACT_FP16:
            d = np.abs(got.view(np.int16).astype(np.int32) - x.view(np.int16).astype(np.int32))
            assert d.max() <= 1, f"{what} seg {e}: act differs by {d.max()} ulp"
            exact += int((d == 0).sum())
            total += d.size
            continue
        bits = 8 if tag == moe.ACT_INT8 else 4
        W = x.shape[1]
        qg = oracle.unpack_wxax(got, bits, W).astype(np.int32)
        stored, sc = moe_ref.quant_rows(x, tag)
        qr = oracle.unpack_wxax(stored, bits, W).astype(np.int32)
        sg = b.scale(e).cpu().numpy()
        ds = np.abs(sg.view(np.int16).astype(np.int32) - sc.view(np.int16).astype(np.int32))
        assert ds.max() <= 1, f"{what} seg {e}: scales differ by {ds.max()} ulp"
        assert np.abs(qg - qr).max() <= 1, f"{what} seg {e}: codes differ by more than one step"
        exact += int((qg == qr).sum())
        total += qg.size
    return exact, total


@pytest.mark.parametrize("N,Ns", [(256, 512), (256, 640)])
@pytest.mark.parametrize("T,topk", TOKENS)
def test_g4_clamped_swiglu_against_reference(T, topk, N, Ns):
    """The share of exactly equal elements / codes is printed, for the clamped activation and for the SiLU expression
    on the same biased inputs. Measured on an MI355X, the four cases together: 283900 of 283904 (99.9986 %) for the
    clamped activation, 283901 of 283904 (99.9989 %) for the SiLU expression (DESIGN.md §4 "gpt-oss layers")."""
    ids = _ids(T, topk, E, 37)
    r = moe.route(ids.to(DEV), E)
    g = torch.Generator().manual_seed(38)
    routed = ((torch.rand(T * topk, 2 * N, generator=g) * 2 - 1) * 10).half()
    shared = ((torch.rand(T, 2 * Ns, generator=g) * 2 - 1) * 10).half()
    b_routed = ((torch.rand(E, 2 * N, generator=g) * 2 - 1) * 2).half()
    b_shared = ((torch.rand(2 * Ns, generator=g) * 2 - 1) * 2).half()
    tags = INT_TAGS + [2]
    sorted_e = torch.sort(ids.view(-1).long(), stable=True).values.numpy()
    for act, name in ((CLAMP, "clamp"), ("silu", "silu")):
        b = moe.glu_quant(routed.to(DEV), shared.to(DEV), r, tags, act, b_routed.to(DEV), b_shared.to(DEV))
        torch.cuda.synchronize()
        want_r = ref.glu(routed.numpy(), b_routed.numpy()[sorted_e], name)
        want_s = ref.glu(shared.numpy(), b_shared.numpy(), name)
        exact, total = _act_against_ref(b, _segments(r, want_r, want_s), tags, name)
        print(f"G4 {name} T={T} topk={topk} N={N} Ns={Ns}: {exact}/{total} exactly equal ({100.0 * exact / total:.3f} %)")


# ------------------------------------------------------------------ G5: combine with a down bias

@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("H", [2048, 72])
def test_g5_combine_bias_bit_exact(H, shared):
    T, topk = 77, 4
    r = moe.route(_ids(T, topk, E, 9).to(DEV), E)
    g = torch.Generator().manual_seed(10)
    y = (torch.rand(T * topk, H, generator=g) * 2 - 1).half()
    w = torch.softmax(torch.rand(T, topk, generator=g), dim=1)
    bias = (torch.rand(E, H, generator=g) * 2 - 1).half()
    sh = (torch.rand(T, H, generator=g) * 2 - 1).half() if shared else None
    sw = torch.rand(T, generator=g) if shared else None
    sb = (torch.rand(H, generator=g) * 2 - 1).half() if shared else None
    dev = lambda t: None if t is None else t.to(DEV)
    npy = lambda t: None if t is None else t.numpy()
    inv, sorted_e = r.inv_slot.cpu().numpy(), r.sorted_expert.cpu().numpy()
    out = moe.combine_bias(dev(y), r, dev(w), dev(bias), dev(sh), dev(sw), dev(sb))
    want = ref.combine_bias(y.numpy(), inv, sorted_e, w.numpy(), topk, bias.numpy(), E, npy(sh), npy(sw), npy(sb))
    assert (out.cpu().numpy().view(np.uint16) == want.view(np.uint16)).all()
    if shared:  # a routed bias without a shared one
        out = moe.combine_bias(dev(y), r, dev(w), dev(bias), dev(sh), dev(sw), None)
        want = ref.combine_bias(y.numpy(), inv, sorted_e, w.numpy(), topk, bias.numpy(), E, npy(sh), npy(sw), None)
        assert (out.cpu().numpy().view(np.uint16) == want.view(np.uint16)).all()
    # an all-zero bias: mxmoe_moe_combine's output
    zero = moe.combine_bias(dev(y), r, dev(w), torch.zeros_like(bias).to(DEV), dev(sh), dev(sw),
                            None if sb is None else torch.zeros_like(sb).to(DEV))
    none = moe.combine_bias(dev(y), r, dev(w), None, dev(sh), dev(sw), None)
    old = moe.combine(dev(y), r, dev(w), dev(sh), dev(sw))
    assert torch.equal(zero.view(torch.int16), old.view(torch.int16)) and torch.equal(none.view(torch.int16), old.view(torch.int16))
    # slots whose id is no expert's (stale slots of a graph forward) add no bias and index nothing
    stale = r.sorted_expert.clone()
    stale[::5] = E
    stale[1::7] = -1
    stale[2::11] = 1 << 30
    r2 = moe.Routing(stale, r.perm_token, r.inv_slot, r.counts, r.T, r.topk, r.E)
    out = moe.combine_bias(dev(y), r2, dev(w), dev(bias), dev(sh), dev(sw), dev(sb))
    want = ref.combine_bias(y.numpy(), inv, stale.cpu().numpy(), w.numpy(), topk, bias.numpy(), E, npy(sh), npy(sw), npy(sb))
    assert (out.cpu().numpy().view(np.uint16) == want.view(np.uint16)).all()


# ------------------------------------------------------------------ G6: the router's logit bias

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bias_that_changes_rows(x, k, seed):
    """An f32 bias scaled until at least a quarter of the rows of the f64 logits x select differently."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-64, 65, size=x.shape[1]).astype(np.float32) / 256
    plain = np.sort(gref.select(x, k), axis=1)
    scale = np.float32(1)
    while True:
        b = base * scale
        changed = (np.sort(gref.select(x + b.astype(np.float64), k), axis=1) != plain).any(axis=1).mean()
        if changed >= 0.25:
            return b, changed
        scale *= 2
        assert scale < 2 ** 20


# (the last two: 32 and 64 token rows per workgroup, the builds with 2 and 4 row blocks)
@pytest.mark.parametrize("T,H,n_exp", [(50, 256, 32), (50, 256, 128), (8192 + 17, 32, 32), (16384 + 33, 32, 64)])
def test_g6_router_logit_bias(T, H, n_exp):
    k = 4
    hidden, w, _ = gref.exact_data(T, H, n_exp, seed=5)
    bias, changed = _bias_that_changes_rows(gref.logits_f64(hidden, w), k, 6)
    h, wd, bd = (torch.from_numpy(a).to(DEV) for a in (hidden, w, bias))
    base = moe.gate(h, wd, k, renormalize=True, return_logits=True)
    none = moe.gate(h, wd, k, renormalize=True, return_logits=True, logit_bias=None)
    ids, wts, sw, logits = moe.gate(h, wd, k, renormalize=True, return_logits=True, logit_bias=bd)
    torch.cuda.synchronize()
    for a, b in zip(base, none):  # logit_bias=None: today's call
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
    x0, x1 = base[3].cpu().numpy(), logits.cpu().numpy()
    assert (_bits(x1) == _bits(x0 + bias[None, :])).all(), "logits with bias != logits + bias (one f32 add)"
    rids, rwts, _, _ = mref.gate(hidden, w, k, renormalize=True, logits=x1)  # the rule on those biased logits
    assert (ids.cpu().numpy() == rids).all(), "topk_ids"
    got_changed = (np.sort(rids, axis=1) != np.sort(base[0].cpu().numpy(), axis=1)).any(axis=1).mean()
    assert got_changed >= 0.25, f"the bias changed only {got_changed:.2f} of the rows"
    ok, worst = gref.softmax_close(wts.cpu().numpy(), rwts)
    print(f"G6 E={n_exp}: {got_changed:.2f} of the rows select differently, weights' worst relative error {worst:.3e}")
    assert ok, f"weights: worst relative error {worst:.3e}"
    assert sw is None
    # without renormalisation and with a shared gate: the shared column gets no bias
    sg = torch.from_numpy(gref.exact_data(T, H, n_exp, seed=5, shared=True)[2]).to(DEV)
    b0 = moe.gate(h, wd, k, w_shared_gate=sg, return_logits=True)
    b1 = moe.gate(h, wd, k, w_shared_gate=sg, return_logits=True, logit_bias=bd)
    torch.cuda.synchronize()
    assert torch.equal(b0[2].view(torch.int32), b1[2].view(torch.int32)), "shared_w must not see the bias"
    assert (_bits(b1[3].cpu().numpy()) == _bits(b0[3].cpu().numpy() + bias[None, :])).all()
    rids, rwts, _, _ = mref.gate(hidden, w, k, renormalize=False, logits=b1[3].cpu().numpy())
    assert (b1[0].cpu().numpy() == rids).all()
    assert gref.softmax_close(b1[1].cpu().numpy(), rwts)[0]


def test_g6_logit_bias_under_sigmoid_scoring_and_groups():
    """The sigmoid builds: scores, the group stage and the selection all see the biased logits."""
    T, H, n_exp, k = 50, 256, 128, 4
    hidden, w, _ = gref.exact_data(T, H, n_exp, seed=7)
    rng = np.random.default_rng(8)
    bias = (rng.integers(-64, 65, size=n_exp) / 16).astype(np.float32)
    e_bias = mref.bias_data(n_exp, rng)
    h, wd, bd, ebd = (torch.from_numpy(a).to(DEV) for a in (hidden, w, bias, e_bias))
    kw = dict(scoring="sigmoid", n_group=4, topk_group=2, renormalize=True, routed_scaling_factor=2.5, e_bias=ebd,
              return_logits=True, return_scores=True)
    base = moe.gate(h, wd, k, **kw)
    ids, wts, _, logits, scores = (t if t is None else t.cpu().numpy() for t in moe.gate(h, wd, k, logit_bias=bd, **kw))
    x1 = base[3].cpu().numpy() + bias[None, :]
    assert (_bits(logits) == _bits(x1)).all()
    want_s = gref.sigmoid(x1.astype(np.float64))
    assert (np.abs(scores - want_s) <= gref.SOFTMAX_RTOL * want_s + gref.SOFTMAX_ATOL).all()
    rids = mref.select(mref.selection_values(scores, e_bias), k, 4, 2, 2)  # f32, on the kernel's own scores
    assert (ids == rids).all()
    want_w = mref.sigmoid_weights(scores, rids, True, 2.5)
    assert (np.abs(wts - want_w) <= gref.SOFTMAX_RTOL * want_w + gref.SOFTMAX_ATOL).all()
    assert (np.sort(ids, axis=1) != np.sort(base[0].cpu().numpy(), axis=1)).any()


# ------------------------------------------------------------------ G7 / G8: a gpt-oss-shaped layer

LAYER = dict(E=8, N=288, H=288, T=40, topk=4, pad=384)


@pytest.fixture(scope="module")
def block():
    """(MoEBlock on a gptoss_layer of a synthetic checkpoint, two padded hidden batches)"""
    L = LAYER
    ck = ref.synthetic_checkpoint(L["E"], L["N"], L["H"], seed=41)
    layer = moe.gptoss_layer(*(ck[k].to(DEV) for k in ("gate_up_blocks", "gate_up_scales", "gate_up_bias", "down_blocks",
                                                       "down_scales", "down_bias")), act_bits=16, pad_to=128)
    assert (layer.H, layer.N) == (L["pad"], L["pad"]) and layer.scale_out_of_range == 0
    g = torch.Generator().manual_seed(42)
    w_gate = (torch.randn(L["E"], L["H"], generator=g) * L["H"] ** -0.5).half()
    logit_bias = torch.randn(L["E"], generator=g) * 0.5
    blk = moe.MoEBlock(layer, moe.pad_cols(w_gate, layer.H).to(DEV), L["topk"], renormalize=True, logit_bias=logit_bias.to(DEV))
    hiddens = [moe.pad_cols(torch.randn(L["T"], L["H"], generator=g).half(), layer.H).to(DEV) for _ in range(2)]
    return blk, hiddens


def _deq(w) -> np.ndarray:
    return ref4.dequant(w.B.cpu().numpy(), qz.unpack_mxfp4_scales(w.scale_b.cpu(), w.K).numpy())


def _check_layer_stages(layer, h, out, mid, mx8: bool):
    n_exp, topk = layer.E, mid["topk_ids"].shape[1]
    r, a1, h1, a2, y = (mid[k] for k in ("routing", "a1", "h1", "a2", "y"))
    assert mid["h1s"] is None and mid["ys"] is None

    def gemm_ref(a, e, w):
        if mx8:  # tests/test_mxfp8_a8_gpu.py: the f64 product of the GPU's own quantised activations
            return ref8.gemm(a.A(e).cpu().numpy(), qz.unpack_mxfp4_scales(a.scale(e).cpu(), w.K).numpy(), w.B.cpu().numpy(),
                             qz.unpack_mxfp4_scales(w.scale_b.cpu(), w.K).numpy())
        return a.A(e).cpu().numpy().astype(np.float64) @ _deq(w).T

    for e, s in enumerate(a1.segs):  # gate_up GEMM
        if s.rows:
            assert_f16_close(h1[s.first_slot:s.first_slot + s.rows].cpu().numpy(), gemm_ref(a1, e, layer.w1[e]), layer.H)
    # the activation stage, given the GPU's own h1: G4's bar on the fp16 activation (for MXFP8: the layer's own pass with
    # fp16 tags, whose quantisation must then be the stored one exactly)
    sorted_e = r.sorted_expert.cpu().numpy()
    want = _segments(r, ref.glu(h1.cpu().numpy(), layer.b1.cpu().numpy()[sorted_e], "clamp"), None)
    own = moe.glu_quant(h1, None, r, [moe.ACT_FP16] * n_exp, layer.activation, layer.b1, None) if mx8 else a2
    torch.cuda.synchronize()
    for e, s in enumerate(a2.segs):
        if not s.rows:
            continue
        act = own.A(e).cpu()
        d = (act.view(torch.int16).int() - torch.from_numpy(want[e]).view(torch.int16).int()).abs()
        assert d.max() <= 1, f"a2 seg {e}: {d.max()} fp16 steps"
        if mx8:
            codes, sc = qz.quant_mxfp8(act)
            assert torch.equal(a2.A(e).cpu(), codes) and torch.equal(a2.scale(e).cpu(), qz.pack_mxfp4_scales(sc))
    for e, s in enumerate(a2.segs):  # down GEMM
        if s.rows:
            assert_f16_close(y[s.first_slot:s.first_slot + s.rows].cpu().numpy(), gemm_ref(a2, e, layer.w2[e]), layer.w2[e].K)
    want_out = ref.combine_bias(y.cpu().numpy(), r.inv_slot.cpu().numpy(), sorted_e, mid["topk_weights"].cpu().numpy(), topk,
                                layer.b2.cpu().numpy(), n_exp)
    got = out.cpu().numpy()
    assert (got.view(np.uint16) == want_out.view(np.uint16)).all()
    assert (got[:, LAYER["H"]:].view(np.uint16) == 0).all(), "padded output columns must be exactly +0"
    assert np.isfinite(got.astype(np.float32)).all() and np.abs(got[:, :LAYER["H"]]).max() > 0


def test_g7_layer_stage_by_stage(block):
    blk, hiddens = block
    h = hiddens[0]
    out, mid = blk.forward(h, return_intermediates=True)
    torch.cuda.synchronize()
    # the router: the rule on the kernel's own biased logits (G6), and a1 = the gathered rows, untouched
    ids, wts, _, logits = moe.gate(h, blk.w_gate, blk.topk, renormalize=True, return_logits=True, logit_bias=blk.routing["logit_bias"])
    assert torch.equal(ids, mid["topk_ids"]) and torch.equal(wts, mid["topk_weights"])
    rids, rwts, _, _ = mref.gate(None, None, blk.topk, renormalize=True, logits=logits.cpu().numpy())
    assert (ids.cpu().numpy() == rids).all() and gref.softmax_close(wts.cpu().numpy(), rwts)[0]
    _, perm, _, _ = moe_ref.route(ids.cpu().numpy(), blk.ffn.E)
    rows = _segments(mid["routing"], h.cpu()[torch.from_numpy(perm).long()], None)
    for e, s in enumerate(mid["a1"].segs):
        if s.rows:
            assert torch.equal(mid["a1"].A(e).cpu().view(torch.int16), rows[e].view(torch.int16))
    _check_layer_stages(blk.ffn, h, out, mid, mx8=False)
    # the whole block against the float64 statement of the layer, as a figure (the stages above are the bars)
    L = LAYER
    ffn = blk.ffn
    gu = np.stack([_deq(w) for w in ffn.w1])
    want = ref.layer(h.cpu().numpy(), blk.w_gate.cpu().numpy(), blk.routing["logit_bias"].cpu().numpy(), gu,
                     ffn.b1.cpu().numpy(), np.stack([_deq(w) for w in ffn.w2]), ffn.b2.cpu().numpy(), blk.topk)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)[:, :L["H"]]
    print(f"G7: block output against the f64 layer: max abs error {err.max():.3e}, rms of the output "
          f"{np.sqrt((want[:, :L['H']] ** 2).mean()):.3e}")
    # the same layer with MXFP8 activations on the same tensors
    v8 = blk.ffn.a8_view()
    assert v8.w1[0].B.data_ptr() == blk.ffn.w1[0].B.data_ptr() and v8.activation == blk.ffn.activation
    out8, mid8 = v8.forward(h, ids, wts, return_intermediates=True)
    torch.cuda.synchronize()
    mid8.update(topk_ids=ids, topk_weights=wts)
    _check_layer_stages(v8, h, out8, mid8, mx8=True)


def _captured(gf, static_hidden):
    """GraphForward.launch captured once on a side stream, as one linear chain (tests/test_dynamic_plan_gpu.py)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gf.launch(static_hidden)  # warm-up outside the capture (module loading)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gf.launch(static_hidden)
    torch.cuda.current_stream().wait_stream(side)
    return graph


def test_g8_planned_and_graph_forward(block):
    blk, hiddens = block
    gf = moe.GraphForward(blk, LAYER["T"])
    assert gf.mode == "plain" and gf._glu is not None
    static_hidden = hiddens[0].clone()
    graph = _captured(gf, static_hidden)
    for h in hiddens:
        want, mid = blk.forward(h, return_intermediates=True)
        pf = moe.PlannedForward(blk.ffn, h, mid["topk_ids"], mid["topk_weights"])
        got_p = pf()
        static_hidden.copy_(h)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got_p.view(torch.int16), want.view(torch.int16)), "planned != eager"
        assert torch.equal(gf.out.view(torch.int16), want.view(torch.int16)), "graph replay != eager"
        assert gf.status() == 0
    assert not torch.equal(hiddens[0], hiddens[1])
