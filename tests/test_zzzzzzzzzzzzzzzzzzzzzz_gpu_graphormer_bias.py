"""Graphormer attention bias on the device (csrc/graphormer_bias.hip) against the rule of include/dgl_amd.h evaluated by
plain torch in fp64.  Inputs lie on a lattice on which every sum is exact in fp32 in any order (X in {-1, 0, 1}, W in
{-2 .. 2}, S in multiples of 1/4, cotangents 60 k: 60 is divisible by every divisor 1 .. 5), so the bars are derived:
fp32 forward 2^-22 (|q| + |s|) (one rounding of the quotient, one of the sum, doubled for a reciprocal), 16-bit forward
that plus one ulp u |ref| of the store, fp32 gradients equal to fp64, 16-bit gather gradients within u |ref|."""
import pytest
import torch

from tests.guarded import POISON_INDEX, guarded

pytestmark = pytest.mark.gpu

MAX_DIST = 4
#        P    Lp max_len H  d  E
CASES = [(1, 1, 1, 1, 1, 1),        # degenerate sizes; one lane per pair
         (33, 3, 5, 3, 8, 7),       # table longer than the paths; masked head tail; a pair group across an LDS block
         (130, 5, 3, 8, 8, 40),     # truncation at max_len with dist > max_len; two lanes per pair
         (1000, 5, 5, 32, 8, 3),    # rows of > 256 pairs (workgroup rows, several partial tables); eight lanes per pair
         (257, 4, 4, 8, 1, 9)]      # d = 1; rows of wavefront length; P one past a workgroup of pairs
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
_inputs = {}


def inputs(case):
    """The case's CPU tensors, built once: ids int64, values fp64 on the lattice."""
    if case not in _inputs:
        P, Lp, max_len, H, d, E = case
        gen = torch.Generator().manual_seed(sum(case))
        r = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
        dist = r(-1, 8, P)
        paths = r(0, E - 1, P, Lp)
        paths[torch.arange(Lp)[None, :] >= dist[:, None]] = -1
        _inputs[case] = dict(dist=dist, paths=paths, X=r(-1, 1, E, d).double(), W=r(-2, 2, max_len * H, d).double(),
                             S=r(-8, 8, MAX_DIST + 2, H).double() / 4, cot=60.0 * r(-2, 2, P, H).double())
    return _inputs[case]


def formula(dist, paths, X, W, S, max_len, table=None):
    """(q, s) in fp64: the path term and the spatial term.  With `table`, T is given instead of X and W."""
    H = (W.shape[0] if table is None else table.shape[1]) // max_len
    lc = min(paths.shape[-1], max_len)
    ids = paths[..., :lc]
    if table is None:
        data = torch.cat([X, X.new_zeros(1, X.shape[1])])[ids]                     # (-1 picks the zero row)
        q = torch.einsum("pld,lhd->ph", data, W.reshape(max_len, H, -1)[:lc])
    else:
        rows = torch.cat([table.reshape(-1, max_len, H), table.new_zeros(1, max_len, H)])
        q = rows[ids, torch.arange(lc)].sum(1)
    q = q / dist.clamp(1, max_len)[:, None]
    s = torch.zeros_like(q) if S is None else torch.nn.functional.embedding(dist.clamp(-1, MAX_DIST) + 1, S)
    return q, s


def shapes(P):
    f = next((k for k in range(2, 40) if P % k == 0 and P > k), None)
    return [(P,)] + ([(f, P // f)] if f else [])


def leaf(t, dev, dtype):
    return t.to(device=dev, dtype=dtype).requires_grad_()


@pytest.mark.parametrize("with_spatial", [True, False], ids=["spatial", "paths-only"])
@pytest.mark.parametrize("idtype", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "P%d-Lp%d-L%d-H%d-d%d-E%d" % c)
def test_operator_against_the_fp64_formula(dev, case, idtype, with_spatial):
    from dgl_amd import ops

    P, Lp, max_len, H, d, E = case
    c = inputs(case)
    ref = {k: c[k].clone().requires_grad_() for k in ("X", "W", "S")}
    q, s = formula(c["dist"], c["paths"], ref["X"], ref["W"], ref["S"] if with_spatial else None, max_len)
    (q + s).backward(c["cot"])
    q, s = q.detach(), s.detach()
    dist, paths = c["dist"].to(dev, idtype), c["paths"].to(dev, idtype)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for shape in shapes(P):
            runs = []
            for _ in range(2):
                X, W, S = (leaf(c[k], dev, dtype) for k in ("X", "W", "S"))
                out = ops.graphormer_bias(dist.reshape(shape), paths.reshape(shape + (Lp,)), X, W, S if with_spatial else None,
                                          max_len=max_len)
                assert out.shape == shape + (H,) and out.dtype == dtype
                out.backward(c["cot"].to(dev, dtype).reshape(out.shape))
                runs.append([out.detach(), X.grad, W.grad] + ([S.grad] if with_spatial else []))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), "two calls on the same inputs differ in some bit"
            got = runs[0][0].reshape(P, H).double().cpu()
            bar = 2.0 ** -22 * (q.abs() + s.abs()) + ULP.get(dtype, 0.0) * (q + s).abs()
            err = (got - (q + s)).abs()
            print(case, idtype, dtype, shape, "forward: worst err / bar", float((err / bar.clamp_min(1e-300)).max()))
            assert bool((err <= bar).all())
            if dtype == torch.float32:                    # gradients of the whole operator: equal to fp64
                for name, g in zip(("X", "W", "S"), runs[0][1:]):
                    diff = (g.double().cpu() - ref[name].grad).abs().max()
                    print(case, "d" + name, "max |diff|", float(diff), "max |ref|", float(ref[name].grad.abs().max()))
                    assert torch.equal(g.double().cpu(), ref[name].grad), "d" + name


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "P%d-Lp%d-L%d-H%d-d%d-E%d" % c)
def test_gather_gradients_in_16_bits(dev, case, dtype):
    from dgl_amd import ops

    P, Lp, max_len, H, d, E = case
    c = inputs(case)
    T = (c["X"] @ c["W"].t()).requires_grad_()
    S = c["S"].clone().requires_grad_()
    q, s = formula(c["dist"], c["paths"], None, None, S, max_len, table=T)
    (q + s).backward(c["cot"])
    runs = []
    for _ in range(2):
        t, sw = leaf(T.detach(), dev, dtype), leaf(c["S"], dev, dtype)
        out = ops.graphormer_bias_gather(c["dist"].to(dev), c["paths"].to(dev), t, sw, max_len=max_len)
        out.backward(c["cot"].to(dev, dtype))
        runs.append((t.grad, sw.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    for name, got, want in (("dT", runs[0][0], T.grad), ("dS", runs[0][1], S.grad)):
        err = (got.double().cpu() - want).abs()
        print(case, dtype, name, "worst err / (u |ref|)", float((err / (ULP[dtype] * want.abs()).clamp_min(1e-300)).max()))
        assert bool((err <= ULP[dtype] * want.abs()).all()), name


def test_padding_idx_and_the_module(dev):
    from dgl_amd import nn, ops

    case = CASES[2]
    P, Lp, max_len, H, d, E = case
    c = inputs(case)
    dist, paths = c["dist"].to(dev), c["paths"].to(dev)
    grads = []
    for pad in (None, 0):
        X, W, S = (leaf(c[k], dev, torch.float32) for k in ("X", "W", "S"))
        out = ops.graphormer_bias(dist, paths, X, W, S, padding_idx=pad)            # (max_len from the spatial table's H)
        out.backward(c["cot"].to(dev, torch.float32))
        grads.append(S.grad)
    assert bool(grads[0][0].abs().sum() > 0) and bool((grads[1][0] == 0).all()) and torch.equal(grads[0][1:], grads[1][1:])
    # the module, loaded from torch re-statements of the two encoders
    spatial = torch.nn.Module()
    spatial.embedding_table = torch.nn.Embedding(MAX_DIST + 2, H, padding_idx=0)
    path = torch.nn.Module()
    path.embedding_table = torch.nn.Embedding(max_len * H, d)
    with torch.no_grad():
        spatial.embedding_table.weight.copy_(c["S"])
        path.embedding_table.weight.copy_(c["W"])
    m = nn.GraphormerBias(MAX_DIST, max_len, d, H)
    m.spatial_encoder.load_state_dict(spatial.state_dict())
    m.path_encoder.load_state_dict(path.state_dict())
    assert "GraphormerBias" in nn.__all__
    assert torch.equal(m.to(dev)(dist, paths, X.detach()), out.detach())


def test_refusals_and_a_guarded_call_afterwards(dev):
    from dgl_amd import _capi, ops
    from dgl_amd._lib import DGLAMDError

    case = CASES[3]
    P, Lp, max_len, H, d, E = case
    c = inputs(case)
    dist, paths = c["dist"].to(dev), c["paths"].to(dev)
    X, W, S = (c[k].to(dev, torch.float32) for k in ("X", "W", "S"))
    f = lambda n, k: torch.zeros(n, k, device=dev)
    with pytest.raises(DGLAMDError, match="graphormer_bias: 257 heads"):
        ops.graphormer_bias(dist, paths, X, f(257, d), f(MAX_DIST + 2, 257))
    with pytest.raises(DGLAMDError, match="graphormer_bias: max_len 33"):
        ops.graphormer_bias(dist, paths, X, f(33 * H, d), S)
    with pytest.raises(DGLAMDError, match="graphormer_bias: dist and paths must share one id width"):
        ops.graphormer_bias(dist.int(), paths, X, W, S)
    with pytest.raises(DGLAMDError, match="graphormer_bias: operand dtypes differ"):
        ops.graphormer_bias(dist, paths, X.half(), W, S)
    with pytest.raises(DGLAMDError, match="graphormer_bias: paths must have the shape of dist"):
        ops.graphormer_bias(dist[:-1], paths, X, W, S)
    bad = paths.clone()
    bad[0, 0] = E
    with pytest.raises(DGLAMDError, match=r"graphormer_bias: paths holds an edge id outside \[-1, %d\)" % E):
        ops.graphormer_bias(dist, bad, X.clone().requires_grad_(), W, S).sum().backward()
    # a valid call afterwards, its workspace exactly the bytes the query reports, between guard bands
    T = (X @ W.t()).requires_grad_()
    Sw = S.clone().requires_grad_()
    cot = c["cot"].to(dev, torch.float32)
    ops.graphormer_bias_gather(dist, paths, T, Sw, max_len=max_len).backward(cot)
    need = _capi.graphormer_bias_workspace_bytes(P, Lp, max_len, E, H, MAX_DIST + 2)
    ws = guarded(dev, need, torch.uint8, poison=POISON_INDEX)
    d_table, d_spatial = _capi.graphormer_bias_backward(dist, paths, cot, E, max_len, MAX_DIST + 2, ws=ws.t)
    ws.check("the workspace of graphormer_bias_backward")
    Tr =(c["X"] @ c["W"].t()).requires_grad_()
    Sr = c["S"].clone().requires_grad_()
    q, s = formula(c["dist"], c["paths"], None, None, Sr, max_len, table=Tr)
    (q + s).backward(c["cot"])
    assert torch.equal(d_table, T.grad) and torch.equal(d_spatial, Sw.grad)
    assert torch.equal(d_table.double().cpu(), Tr.grad) and torch.equal(d_spatial.double().cpu(), Sr.grad)
