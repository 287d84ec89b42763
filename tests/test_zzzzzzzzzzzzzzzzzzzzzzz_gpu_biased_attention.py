"""Biased attention on the device (csrc/biased_attention.hip) against the rule of include/dgl_amd.h evaluated by plain
torch in fp64 on the operands rounded to the case's dtype.  The bar is measured, not fixed: with e = max |x - ref| /
max |ref| per checked tensor (out, dq, dk, dv, dbias), e_fused <= 2 e_composed + u, where e_composed is the same measure
of ``fused=False`` on the same device inputs and u the unit roundoff of the dtype (the one rounding at the store).
"""
import pytest
import torch

from tests.battn_cases import CASES, NAMES, errors, formula, inputs, outputs
from tests.guarded import POISON_FLOAT, POISON_INDEX, guarded

pytestmark = pytest.mark.gpu

U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
MODES = {"bias+mask": (True, True), "bias": (True, False), "plain": (False, False)}
ids = dict(ids=lambda x: "B%d-N%d-H%d-D%d" % x if isinstance(x, tuple) else str(x).replace("torch.", ""))
_bars = {}


def check(got, ref, bars, what, rows=None):
    for name, g, r, bar in zip(NAMES, got, ref, bars):
        if r is None:
            continue
        if rows is not None and name in ("out", "dq", "dbias"):       # (the tensors with a query axis at dim 1)
            g, r = g[:, rows], r[:, rows]
        e = errors([g], [r])[0]
        print(what, name, "e_fused %.3e bar %.3e" % (e, bar))
        assert e <= bar, (what, name, e, bar)


def bars_of(dev, c, dtype, case, mode):
    """2 e_composed + u per tensor, and the fp64 reference, of operands `c` without dropout."""
    from dgl_amd import ops

    scale = case[3] ** -0.5
    ref = outputs(lambda q, k, v, b, m: formula(q, k, v, b, m, scale), c, torch.float64, "cpu", *MODES[mode])
    comp = outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, fused=False), c, dtype, dev, *MODES[mode])
    e_comp = errors(comp, ref)
    print(case, dtype, mode, "e_composed", e_comp)
    return [None if e is None else 2 * e + U[dtype] for e in e_comp], ref


def case_bars(dev, case, dtype, mode):
    if (case, dtype, mode) not in _bars:
        _bars[(case, dtype, mode)] = bars_of(dev, inputs(case, dtype), dtype, case, mode)
    return _bars[(case, dtype, mode)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("case", CASES, **ids)
def test_fused_against_the_fp64_rule(dev, case, dtype, mode):
    from dgl_amd import ops

    bars, ref = case_bars(dev, case, dtype, mode)
    got = outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, fused=True), inputs(case, dtype), dtype, dev, *MODES[mode])
    check(got, ref, bars, (case, dtype, mode))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_rows_without_a_finite_score(dev, dtype):
    """Query 3 fully masked, query 5 with its first whole key tile masked, a -inf bias entry at (query 7, key 2, head 1).
    The composed route, which gives NaN on a dead row, is measured on the same operands with one key of row 3 opened."""
    from dgl_amd import ops

    case = CASES[2]
    c = dict(inputs(case, dtype))
    c["mask"] = c["mask"].clone()
    c["mask"][:, 3, :] = True
    c["mask"][:, 5, :32] = True
    c["mask"][:, 5, 40] = False
    c["bias"] = c["bias"].clone()
    c["bias"][:, 7, 2, 1] = float("-inf")
    legal = dict(c, mask=c["mask"].clone())
    legal["mask"][:, 3, 0] = False
    bars, _ = bars_of(dev, legal, dtype, case, "bias+mask")
    ref = outputs(lambda q, k, v, b, m: formula(q, k, v, b, m, case[3] ** -0.5), c, torch.float64, "cpu")
    got = outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, fused=True), c, dtype, dev)
    for name, g in zip(NAMES, got):
        assert bool(torch.isfinite(g).all()), name
    assert bool((got[0][:, 3] == 0).all()) and bool((got[1][:, 3] == 0).all()) and bool((got[4][:, 3] == 0).all())
    assert bool((got[4][:, 7, 2, 1] == 0).all())
    check(got, ref, bars, ("dead rows", dtype), rows=[i for i in range(case[1]) if i != 3])


@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("case", CASES[1:3], **ids)
def test_dropout_against_the_host_mask(dev, case, dtype):
    from dgl_amd import _capi, ops

    p, seed = 0.25, 1234
    B, N, H, D = case
    bars, _ = case_bars(dev, case, dtype, "bias+mask")
    c = inputs(case, dtype)
    keep = _capi.biased_attention_dropout_mask_host(seed, p, B, H, N)
    ref = outputs(lambda q, k, v, b, m: formula(q, k, v, b, m, D ** -0.5, keep, p), c, torch.float64, "cpu")
    run = lambda s: outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, attn_drop=p, seed=s, fused=True), c, dtype, dev)
    got = run(seed)
    check(got, ref, [b / (1 - p) for b in bars], (case, dtype, "dropout"))
    assert all(torch.equal(a, b) for a, b in zip(got, run(seed)))
    assert not torch.equal(got[0], run(seed + 1)[0])
    off = outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, attn_drop=p, training=False, fused=True), c, dtype, dev)
    assert torch.equal(off[0], outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, fused=True), c, dtype, dev)[0])


def test_two_runs_give_the_same_bits(dev):
    from dgl_amd import ops

    c = inputs(CASES[4], torch.bfloat16)
    runs = [outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, fused=True), c, torch.bfloat16, dev) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], **ids)
def test_guard_bands(dev, dtype):
    from dgl_amd import _capi

    case = CASES[1]
    B, N, H, D = case
    c = inputs(case, dtype)
    q, k, v, bias, cot = (c[n].to(dev, dtype) for n in ("q", "k", "v", "bias", "cot"))
    mask = c["mask"].to(dev).view(torch.uint8)
    out = guarded(dev, (B, N, H, D), dtype, poison=POISON_FLOAT)
    lse = guarded(dev, (2, B, H, N), torch.float32, poison=POISON_FLOAT)
    dbias = guarded(dev, (B, N, N, H), dtype, poison=POISON_FLOAT)
    ws = guarded(dev, _capi.biased_attention_workspace_bytes(B, N, H), torch.uint8, poison=POISON_INDEX)
    _capi.biased_attention_forward(q, k, v, bias, mask, D ** -0.5, 0.25, 5, into=(out.t, lse.t))
    got = _capi.biased_attention_backward(q, k, v, bias, mask, out.t, lse.t, cot, D ** -0.5, 0.25, 5, dbias=dbias.t, ws=ws.t)
    for g, name in ((out, "out"), (lse, "lse"), (dbias, "dbias"), (ws, "workspace")):
        g.check(name)
    plain = _capi.biased_attention_forward(q, k, v, bias, mask, D ** -0.5, 0.25, 5)
    assert torch.equal(plain[0], out.t) and torch.equal(plain[1], lse.t)
    again = _capi.biased_attention_backward(q, k, v, bias, mask, out.t, lse.t, cot, D ** -0.5, 0.25, 5)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_module_with_a_reference_state_dict(dev):
    from dgl_amd import nn

    B, N, H, D = CASES[1]
    torch.manual_seed(3)
    state = {p + ".weight": torch.randn(H * D, H * D) * (H * D) ** -0.5 for p in ("q_proj", "k_proj", "v_proj", "out_proj")}
    state.update({p + ".bias": torch.randn(H * D) * 0.1 for p in ("q_proj", "k_proj", "v_proj", "out_proj")})
    m = nn.BiasedMHA(H * D, H, attn_drop=0.1)
    m.load_state_dict(state)
    m = m.to(dev).eval()
    c = inputs(CASES[1], torch.float32)
    x = torch.randn(B, N, H * D)
    heads = lambda t: t.reshape(B, N, H, D)

    def restated(dt, device):                # the reference's forward: projections, the attention, out_proj
        xx = x.to(device=device, dtype=dt)
        st = {n: t.to(device=device, dtype=dt) for n, t in state.items()}
        l = lambda t, p: t @ st[p + ".weight"].t() + st[p + ".bias"]
        a = formula(heads(l(xx, "q_proj")), heads(l(xx, "k_proj")), heads(l(xx, "v_proj")), c["bias"].to(device=device, dtype=dt),
                    c["mask"].to(device), D ** -0.5)
        return l(a.reshape(B, N, H * D), "out_proj").double().cpu()

    ref = restated(torch.float64, "cpu")
    e_comp = errors([restated(torch.float32, dev)], [ref])[0]
    bias, mask = c["bias"].to(dev, torch.float32), c["mask"].to(dev)
    with torch.no_grad():
        fused, auto = m(x.to(dev), bias, mask, fused=True), m(x.to(dev), bias, mask)
    e = errors([fused.double().cpu()], [ref])[0]
    print("module e_fused %.3e e_composed %.3e" % (e, e_comp))
    assert e <= 2 * e_comp + U[torch.float32]
    assert errors([auto.double().cpu()], [ref])[0] <= 2 * e_comp + U[torch.float32]


def test_refusals(dev):
    from dgl_amd import _capi, ops
    from dgl_amd._lib import DGLAMDError

    z = lambda *shape, **kw: torch.zeros(shape, device=dev, **kw)
    q = z(2, 5, 3, 8)
    for match, call in (
            ("biased_attention: operand dtypes differ", lambda: ops.biased_attention(q, q.half(), q)),
            ("biased_attention: operand dtypes differ", lambda: ops.biased_attention(q, q, q, z(2, 5, 5, 3).half())),
            ("biased_attention: head width 129", lambda: ops.biased_attention(z(1, 2, 1, 129), z(1, 2, 1, 129), z(1, 2, 1, 129), fused=True)),
            ("biased_attention: head width 129", lambda: _capi.biased_attention_forward(*[z(1, 2, 1, 129)] * 3, None, None, 1.0, 0.0, 0)),
            ("biased_attention: q, k, v must share one shape", lambda: ops.biased_attention(q, q[:, :4], q)),
            (r"biased_attention: attn_bias must be \(B, N, N, H\)", lambda: ops.biased_attention(q, q, q, z(2, 5, 5))),
            (r"biased_attention: attn_bias must be \(B, N, N, H\)", lambda: ops.biased_attention(q, q, q, z(2, 5, 3, 5))),
            ("biased_attention: attn_mask must be a bool or uint8", lambda: ops.biased_attention(q, q, q, None, z(2, 5, 5, 3, dtype=torch.bool))),
            ("biased_attention: attn_mask must be a bool or uint8", lambda: ops.biased_attention(q, q, q, None, z(2, 5, 5))),
            ("biased_attention: attn_drop must lie in", lambda: ops.biased_attention(q, q, q, attn_drop=1.0)),
            ("biased_attention: the dropout probability must lie in", lambda: _capi.biased_attention_forward(q, q, q, None, None, 1.0, -0.1, 0)),
            ("biased_attention: operands lie on different devices", lambda: ops.biased_attention(q, q.cpu(), q))):
        with pytest.raises(DGLAMDError, match=match):
            call()
    assert ops.biased_attention(q, q, q).shape == q.shape                                          # a valid call afterwards
