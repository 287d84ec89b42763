"""The fused GAT attention operator on fp16 / bf16 operands and on head widths that are not a power of two
(csrc/gat_attention.hip, the wide kernels), through the C ABI and through the public API.

Numerical contract.  `exact` is a dense index_add evaluation in float64 on the GPU of the SAME operands (16-bit values
widened exactly).  u = 2^-8 for bf16, 2^-11 for fp16 (one round-to-nearest of the final store).
  16-bit forward    |out - exact| <= (u + 1e-5) |exact| on EVERY element (1e-5: the flat fp32 bar of tests/tolerance.py)
  16-bit gradients  max |got - exact| / max |exact| <= u + 1e-5 for each of d_ft, d_el, d_er
  fp32 new widths   against the oracle's composition of the four operators under tests/tolerance.assert_fp32_sum (rows
                    under 500 edges meet the plain 1e-5 bar, the escape is tallied); gradients against the fp64 dense
                    autograd at 1e-5 normalised
  fused vs composed on the 16-bit route: rtol 1e-3 / atol 0.5 (fp16), rtol 4e-3 / atol 2.0 (bf16) — the tolerances the
                    reference gives its own half-precision operator tests; a sanity bound, the fp64 check binds.
Every figure is printed before it is asserted.

(The file name sorts after every other test file on purpose: new GPU tests are collected last, so the position of no
existing test in the collection changes.)"""
import pytest
import torch
import torch.nn.functional as F

import oracle
from tests.graphgen import synth_csr
from tests.tolerance import assert_fp32_sum, max_rel_err

pytestmark = pytest.mark.gpu
SLOPE = 0.2
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SIXTEEN = [torch.float16, torch.bfloat16]


def _h(t):
    return None if t is None else t.detach().cpu().numpy()


def _graph(dev, n, e, seed, idtype=torch.int32, hubs=0, empty_every=0):
    g = synth_csr(n, n, e, "U", seed=seed, device=dev, idtype=idtype)
    indptr, indices = g["indptr"].long(), g["indices"].long()
    deg = indptr[1:] - indptr[:-1]
    if empty_every:                                  # rows without in-edges: move their edges to the next row
        deg = deg.clone()
        idx = torch.arange(0, n - 1, empty_every, device=dev)
        deg[idx + 1] += deg[idx]
        deg[idx] = 0
    if hubs:                                         # a few rows far longer than a chunk (512 edges)
        deg = deg.clone()
        take = torch.arange(n // 2, n // 2 + 4000, device=dev)
        moved = deg[take].sum()
        deg[take] = 0
        deg[7] += moved // 2
        deg[n - 3] += moved - moved // 2
    indptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(deg, 0)])
    return indptr.to(idtype), indices.to(idtype)


def _csr_pair(dev, indptr, indices, n):
    from dgl_amd import _capi

    deg = (indptr[1:] - indptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n, device=dev), deg).to(indptr.dtype)
    o_indptr, o_indices, _ = _capi.coo_to_csr(indices, dst, None, n, n)          # rows = src, columns = dst
    return _capi.make_csr(indptr, indices, None, n), _capi.make_csr(o_indptr, o_indices, None, n), dst


def _forward(dev, csc, n, ft, el, er):
    from dgl_amd import _capi

    h, d = ft.shape[1:]
    out = torch.full((n, h, d), float("nan"), device=dev, dtype=ft.dtype)
    mz = torch.empty(n, h, 2, device=dev)
    ws = torch.empty(max(1, _capi.gat_attention_workspace_bytes(csc, h, d)), dtype=torch.uint8, device=dev)
    _capi.gat_attention_forward(csc, ft, el, er, SLOPE, out, mz, ws)
    return out, mz, ws


def _oracle_forward(indptr, indices, dst, ft, el, er):
    e = indices.shape[0]
    h = ft.shape[1]
    s = oracle.sddmm_coo("add", _h(indices), _h(dst), None, _h(el), _h(er), "u", "v").reshape(e, h)
    s = _h(F.leaky_relu(torch.from_numpy(s), SLOPE))
    a = oracle.edge_softmax_fwd(_h(indptr), None, s)
    ref, _, _ = oracle.spmm_csr("mul", "sum", _h(indptr), _h(indices), None, _h(ft), a.reshape(e, h, 1))
    return ref, a


def _dense_fp64(ft, el, er, src, dl, n):
    ft, el, er = ft.double(), el.double(), er.double()
    s = F.leaky_relu(el[src] + er[dl], SLOPE)
    mx = torch.full((n,) + tuple(s.shape[1:]), float("-inf"), device=s.device, dtype=torch.float64).index_reduce_(0, dl, s, "amax")
    ex = torch.exp(s - mx[dl])
    a = ex / torch.zeros_like(mx).index_add_(0, dl, ex)[dl]
    return torch.zeros((n,) + tuple(ft.shape[1:]), device=s.device, dtype=torch.float64).index_add_(0, dl, a * ft[src])


def _dense_fp64_grads(ft, el, er, dout, src, dl, n):
    p = [t.double().clone().requires_grad_(True) for t in (ft, el, er)]
    h, d = ft.shape[1:]
    s = F.leaky_relu(p[1][src] + p[2][dl], SLOPE)
    mx = torch.full((n, h, 1), float("-inf"), device=ft.device, dtype=torch.float64).index_reduce_(0, dl, s.detach(), "amax")
    ex = torch.exp(s - mx[dl])
    a = ex / torch.zeros(n, h, 1, device=ft.device, dtype=torch.float64).index_add_(0, dl, ex)[dl]
    o = torch.zeros(n, h, d, device=ft.device, dtype=torch.float64).index_add_(0, dl, a * p[0][src])
    return o.detach(), torch.autograd.grad((o * dout.double()).sum(), p)


def _operands(dev, n, heads, d, dtype, seed, scale=1.0):
    torch.manual_seed(seed)
    ft = (torch.rand(n, heads, d, device=dev) + 1).to(dtype)                      # U(0, 1) + 1
    el = (scale * torch.randn(n, heads, 1, device=dev)).to(dtype)
    er = (scale * torch.randn(n, heads, 1, device=dev)).to(dtype)
    return ft, el, er


def _assert_16bit_forward(out, exact, dtype, what):
    u = U[dtype]
    err = (out.double() - exact).abs()
    worst = float((err / exact.abs().clamp(min=1e-300)).max()) / u if exact.numel() else 0.0
    print("%s: worst element %.3f u (u = %.3g) against fp64" % (what, worst, u))
    bad = err > (u + 1e-5) * exact.abs()
    assert not bool(bad.any()), "%s: %d elements past (u + 1e-5) |exact|, worst %.3f u" % (what, int(bad.sum()), worst)


@pytest.mark.parametrize("heads,d", [(8, 8), (8, 32), (8, 64), (2, 12), (1, 47)])
@pytest.mark.parametrize("dtype", SIXTEEN, ids=["fp16", "bf16"])
def test_16bit_forward_at_c3_size_is_one_rounding_off_fp64(dev, dtype, heads, d):
    n, e = 169_343, 2_501_829
    indptr, indices = _graph(dev, n, e, seed=11, empty_every=97)
    csc, _, dst = _csr_pair(dev, indptr, indices, n)
    ft, el, er = _operands(dev, n, heads, d, dtype, heads * 1000 + d)
    out, mz, _ = _forward(dev, csc, n, ft, el, er)
    assert out.dtype == dtype and mz.dtype == torch.float32
    exact = _dense_fp64(ft, el, er, indices.long(), dst.long(), n)
    _assert_16bit_forward(out, exact, dtype, "forward %s H=%d D=%d" % (dtype, heads, d))
    deg = indptr[1:] - indptr[:-1]
    assert bool((out[deg == 0] == 0).all()) and int((deg == 0).sum()) > 1000
    out2, mz2, _ = _forward(dev, csc, n, ft, el, er)
    assert torch.equal(out, out2) and torch.equal(mz, mz2)           # deterministic


@pytest.mark.parametrize("heads,d", [(1, 5), (2, 12), (8, 6), (3, 24), (1, 47), (2, 100), (16, 2)])
def test_fp32_new_head_widths_match_the_oracle_composition_at_c3_size(dev, heads, d):
    n, e = 169_343, 2_501_829
    indptr, indices = _graph(dev, n, e, seed=11, empty_every=97)
    csc, _, dst = _csr_pair(dev, indptr, indices, n)
    ft, el, er = _operands(dev, n, heads, d, torch.float32, heads * 1000 + d)
    out, mz, _ = _forward(dev, csc, n, ft, el, er)
    ref, _ = _oracle_forward(indptr, indices, dst, ft, el, er)
    exact = _dense_fp64(ft, el, er, indices.long(), dst.long(), n)
    print("forward fp32 H=%d D=%d: plain max rel err vs the oracle %.3g" % (heads, d, max_rel_err(_h(out).reshape(ref.shape), ref)))
    deg = indptr[1:] - indptr[:-1]
    assert_fp32_sum(_h(out).reshape(n, -1), ref.reshape(n, -1), _h(exact).reshape(n, -1), row_len=_h(deg))
    assert bool((out[deg == 0] == 0).all()) and int((deg == 0).sum()) > 1000
    out2, mz2, _ = _forward(dev, csc, n, ft, el, er)
    assert torch.equal(out, out2) and torch.equal(mz, mz2)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("dtype,heads,d", [(torch.bfloat16, 8, 8), (torch.float32, 2, 12)], ids=["bf16_H8_D8", "fp32_H2_D12"])
def test_hub_rows_across_many_chunks(dev, dtype, heads, d, idtype):
    n, e = 60_000, 1_500_000
    indptr, indices = _graph(dev, n, e, seed=5, idtype=idtype, hubs=1, empty_every=13)
    assert int((indptr[1:] - indptr[:-1]).max()) > 20_000            # > 40 chunks of 512 edges in one row
    csc, _, dst = _csr_pair(dev, indptr, indices, n)
    ft, el, er = _operands(dev, n, heads, d, dtype, 3, scale=3.0)
    out, _, _ = _forward(dev, csc, n, ft, el, er)
    exact = _dense_fp64(ft, el, er, indices.long(), dst.long(), n)
    if dtype == torch.float32:
        ref, _ = _oracle_forward(indptr, indices, dst, ft, el, er)
        deg = _h(indptr[1:] - indptr[:-1])
        assert_fp32_sum(_h(out).reshape(n, -1), ref.reshape(n, -1), _h(exact).reshape(n, -1), row_len=deg)
    else:
        _assert_16bit_forward(out, exact, dtype, "hub rows %s H=%d D=%d %s" % (dtype, heads, d, idtype))


@pytest.mark.parametrize("dtype,heads,d", [(torch.bfloat16, 8, 32), (torch.bfloat16, 2, 12), (torch.float16, 8, 32),
                                           (torch.float16, 2, 12), (torch.float32, 2, 12), (torch.float32, 1, 5)],
                         ids=["bf16_H8_D32", "bf16_H2_D12", "fp16_H8_D32", "fp16_H2_D12", "fp32_H2_D12", "fp32_H1_D5"])
def test_backward_against_the_fp64_gradient(dev, dtype, heads, d):
    """d_ft, d_el, d_er of the C-ABI backward on the 40 k-row / 700 k-edge hub graph (two rows of ~50 k edges) against
    torch autograd of the dense fp64 evaluation of the same operands: max |got - exact| / max |exact| <= u + 1e-5
    (u = 0 for fp32)."""
    from dgl_amd import _capi

    n, e = 40_000, 700_000
    indptr, indices = _graph(dev, n, e, seed=21, hubs=1, empty_every=29)
    csc, csr, dst = _csr_pair(dev, indptr, indices, n)
    ft, el, er = _operands(dev, n, heads, d, dtype, heads + d)
    dout = torch.randn(n, heads, d, device=dev).to(dtype)
    out, mz, ws = _forward(dev, csc, n, ft, el, er)
    d_ft, d_el, d_er = (torch.full_like(t, float("nan")) for t in (ft, el, er))
    _capi.gat_attention_backward(csc, csr, ft, el, er, out, mz, dout, SLOPE, d_ft, d_el, d_er, ws)
    first = [t.clone() for t in (d_ft, d_el, d_er)]
    _capi.gat_attention_backward(csc, csr, ft, el, er, out, mz, dout, SLOPE, d_ft, d_el, d_er, ws)
    assert all(torch.equal(a, b) for a, b in zip(first, (d_ft, d_el, d_er)))
    assert all(t.dtype == dtype for t in (d_ft, d_el, d_er))
    _, want = _dense_fp64_grads(ft, el, er, dout, indices.long(), dst.long(), n)
    u = U.get(dtype, 0.0)
    errs = {}
    for got, w, name in zip((d_ft, d_el, d_er), want, ("d_ft", "d_el", "d_er")):
        errs[name] = float((got.double() - w).abs().max()) / float(w.abs().max())
        print("backward %s H=%d D=%d %s: max abs err / max |grad| = %.3g%s" % (
            dtype, heads, d, name, errs[name], " = %.3f u" % (errs[name] / u) if u else ""))
    for name, err in errs.items():
        assert err <= u + 1e-5, "%s: max abs err / max |grad| = %.3g (bar %.3g)" % (name, err, u + 1e-5)


def test_mixed_dtypes_and_unsupported_shapes_are_refused(dev):
    from dgl_amd import _capi
    from dgl_amd._lib import DGLAMDError

    n = 64
    indptr, indices = _graph(dev, n, 512, seed=1)
    csc, _, _ = _csr_pair(dev, indptr, indices, n)
    ft, el, er = _operands(dev, n, 2, 12, torch.bfloat16, 1)
    out, mz = torch.empty(n, 2, 12, device=dev), torch.empty(n, 2, 2, device=dev)
    ws = torch.empty(max(1, _capi.gat_attention_workspace_bytes(csc, 2, 12)), dtype=torch.uint8, device=dev)
    with pytest.raises(DGLAMDError):
        _capi.gat_attention_forward(csc, ft, el, er, SLOPE, out, mz, ws)          # fp32 out for bf16 operands
    ft, el, er = _operands(dev, n, 6, 121, torch.float32, 1)
    out, mz = torch.empty(n, 6, 121, device=dev), torch.empty(n, 6, 2, device=dev)
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=dev)
    with pytest.raises(DGLAMDError):
        _capi.gat_attention_forward(csc, ft, el, er, SLOPE, out, mz, ws)


# ---- public API -----------------------------------------------------------------------------------------------
def _random_graph(dev, n=3000, e=40_000, seed=17):
    import dgl_amd as dgl

    g0 = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (e,), generator=g0), torch.randint(0, n, (e,), generator=g0)
    src, dst = torch.cat([src, torch.arange(n)]), torch.cat([dst, torch.arange(n)])     # + self loops: no empty row
    perm = torch.randperm(src.numel(), generator=g0)          # unsorted COO: the CSC carries an edge-id map
    src, dst = src[perm].to(dev), dst[perm].to(dev)
    return dgl.graph((src, dst), num_nodes=n, idtype=torch.int32, device=dev), src.long(), dst.long()


CASES = [(torch.float16, 8, 32), (torch.bfloat16, 8, 64), (torch.bfloat16, 2, 12), (torch.float16, 1, 47),
         (torch.float32, 1, 5), (torch.float32, 2, 12), (torch.float32, 1, 47)]


@pytest.mark.parametrize("dtype,heads,d", CASES, ids=["%s_H%d_D%d" % (str(t)[6:], h, d) for t, h, d in CASES])
def test_public_api_takes_the_new_operands(dev, dtype, heads, d):
    import dgl_amd as dgl

    g, src, dst = _random_graph(dev)
    n = g.num_nodes()
    ps = [t.requires_grad_(True) for t in _operands(dev, n, heads, d, dtype, heads * 100 + d)]
    up = torch.randn(n, heads, d, device=dev).to(dtype)
    assert dgl.ops.gat_attention_applies(g, *ps)
    bad = _operands(dev, n, 6, 121, dtype, 1)
    assert not dgl.ops.gat_attention_applies(g, *bad)
    res = {}
    for route, kw in (("default", {}), ("fused", dict(fused=True)), ("composed", dict(fused=False))):
        o = dgl.nn.gat_attention(g, ps[0], ps[1], ps[2], SLOPE, **kw)
        assert type(o) is torch.Tensor and o.dtype == dtype and o.shape == (n, heads, d)
        gr = torch.autograd.grad((o * up).sum(), ps)
        assert all(a.dtype == dtype and a.shape == p.shape for a, p in zip(gr, ps))
        res[route] = [o.detach()] + list(gr)
    assert all(torch.equal(a, b) for a, b in zip(res["default"], res["fused"]))       # the default route IS the fused kernel
    exact_o, exact_g = _dense_fp64_grads(ps[0].detach(), ps[1].detach(), ps[2].detach(), up, src, dst, n)
    exact = [exact_o] + list(exact_g)
    for route in ("fused", "composed"):
        for got, w, name in zip(res[route], exact, ("out", "d_ft", "d_el", "d_er")):
            print("public API %s H=%d D=%d %s %s: max abs err / max |exact| = %.3g" % (
                dtype, heads, d, route, name, float((got.double() - w).abs().max()) / float(w.abs().max())))
    if dtype == torch.float32:
        for a, b in zip(res["fused"], res["composed"]):
            torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-5)
        return
    u = U[dtype]
    _assert_16bit_forward(res["fused"][0], exact_o, dtype, "public API forward %s H=%d D=%d" % (dtype, heads, d))
    for got, w, name in zip(res["fused"][1:], exact_g, ("d_ft", "d_el", "d_er")):
        err = float((got.double() - w).abs().max()) / float(w.abs().max())
        assert err <= u + 1e-5, "%s: %.3g (bar %.3g)" % (name, err, u + 1e-5)
    rtol, atol = (1e-3, 0.5) if dtype == torch.float16 else (4e-3, 2.0)
    for a, b in zip(res["fused"], res["composed"]):
        torch.testing.assert_close(a.float(), b.float(), rtol=rtol, atol=atol)


def test_dout_of_another_dtype_is_cast(dev):
    import dgl_amd as dgl

    g, _, _ = _random_graph(dev, n=500, e=4000)
    ps = [t.requires_grad_(True) for t in _operands(dev, 500, 2, 12, torch.bfloat16, 4)]
    o = dgl.nn.gat_attention(g, *ps, SLOPE)
    gr = torch.autograd.grad((o.float() * torch.randn(500, 2, 12, device=dev)).sum(), ps)
    assert all(a.dtype == torch.bfloat16 and bool(torch.isfinite(a.float()).all()) for a in gr)


@pytest.mark.parametrize("dtype,heads,d", [(torch.bfloat16, 8, 32), (torch.float32, 2, 12), (torch.float32, 4, 16)],
                         ids=["bf16_H8_D32", "fp32_H2_D12", "fp32_H4_D16"])
def test_a_block_without_destination_nodes_returns_an_empty_tensor(dev, dtype, heads, d):
    import dgl_amd as dgl

    n_src = 50
    empty = torch.zeros(0, dtype=torch.int32, device=dev)
    blk = dgl.create_block((empty, empty), num_src_nodes=n_src, num_dst_nodes=0, device=dev)
    ft = torch.randn(n_src, heads, d, device=dev).to(dtype).requires_grad_(True)
    el = torch.randn(n_src, heads, 1, device=dev).to(dtype).requires_grad_(True)
    er = torch.randn(0, heads, 1, device=dev).to(dtype).requires_grad_(True)
    assert dgl.ops.gat_attention_applies(blk, ft, el, er)
    o = dgl.nn.gat_attention(blk, ft, el, er, SLOPE)
    assert o.shape == (0, heads, d) and o.dtype == dtype
    gr = torch.autograd.grad(o.sum(), [ft, el, er])
    assert gr[0].shape == ft.shape and bool((gr[0] == 0).all()) and bool((gr[1] == 0).all()) and gr[2].shape == er.shape
    torch.cuda.synchronize()


def test_a_block_with_destinations_fused_on_16bit(dev):
    import dgl_amd as dgl

    n_src, n_dst, e, h, d = 5000, 1200, 40_000, 4, 24
    g0 = torch.Generator().manual_seed(8)
    src, dst = torch.randint(0, n_src, (e,), generator=g0).to(dev), torch.randint(5, n_dst, (e,), generator=g0).to(dev)
    blk = dgl.create_block((src, dst), num_src_nodes=n_src, num_dst_nodes=n_dst, device=dev)
    torch.manual_seed(2)
    ft = (torch.rand(n_src, h, d, device=dev) + 1).bfloat16()
    el, er = torch.randn(n_src, h, 1, device=dev).bfloat16(), torch.randn(n_dst, h, 1, device=dev).bfloat16()
    assert dgl.ops.gat_attention_applies(blk, ft, el, er)
    o = dgl.nn.gat_attention(blk, ft, el, er, SLOPE)
    ftd, eld, erd = ft.double(), el.double(), er.double()
    s = F.leaky_relu(eld[src] + erd[dst], SLOPE)
    mx = torch.full((n_dst, h, 1), float("-inf"), device=dev, dtype=torch.float64).index_reduce_(0, dst, s, "amax")
    ex = torch.exp(s - mx[dst])
    a = ex / torch.zeros_like(mx).index_add_(0, dst, ex)[dst]
    exact = torch.zeros(n_dst, h, d, device=dev, dtype=torch.float64).index_add_(0, dst, a * ftd[src])
    _assert_16bit_forward(o, exact, torch.bfloat16, "block bf16 H4 D24")
    assert bool((o[:5] == 0).all())


def test_csc_only_graph_applies_only_without_gradients(dev):
    import dgl_amd as dgl

    g, _, _ = _random_graph(dev, n=500, e=4000)
    g = g.formats(["csc"])
    ft, el, er = _operands(dev, 500, 2, 12, torch.bfloat16, 4)
    assert dgl.ops.gat_attention_applies(g, ft, el, er)
    o = dgl.nn.gat_attention(g, ft, el, er, SLOPE)
    assert o.dtype == torch.bfloat16 and o.shape == (500, 2, 12)
    for i in range(3):
        ps = [ft.clone(), el.clone(), er.clone()]
        ps[i].requires_grad_(True)
        assert not dgl.ops.gat_attention_applies(g, *ps)
