"""Sparse x sparse on the GPU (csrc/csr_mm.hip): CSRMM, CSRSum, CSRMask, their autograd, adj_product_graph /
adj_sum_graph and sparse.spspmm over them.

Reference for values: a dense fp64 matmul / sum of the operands in torch on the CPU, 16-bit operands widened first.
Graphs follow the reference test's recipe (tests/python/common/test_sparse_ops-csr.py:15-41): random (row, column) pairs,
duplicates merged, edges shuffled so that the CSR carries an edge-id map.  One departure, for every dtype alike: a merged
entry gets one random normal value whose magnitude is kept at or above 2^-6 (instead of the sum of its duplicates'
values), so that no product falls into fp16's subnormal range, where the bound below — which has no term for it — would
not describe a correctly rounded result.

The value bar is derived, not chosen.  An entry made of t terms with S = sum |a||b| is held to
    |got - exact| <= 1.01 (t + 1) u S  [+ u16 |exact| for 16-bit storage, the one final rounding]
with u = 2^-24 for fp32 and 16-bit operands (fp32 arithmetic), 2^-53 for fp64, u16 = 2^-11 (fp16) / 2^-8 (bf16): the
standard bound of a t-term inner product summed in ANY fixed order (t multiplications, t - 1 additions).  t and S come from
the product of the 0/1 pattern matrices and of the absolute values in fp64.  Gradients are held to the same bar with the
dense gradient's own t and S."""
import functools

import pytest
import torch

import dgl_amd
from dgl_amd import _capi, sparse_kernels
from dgl_amd.autograd import csrmask, csrmm, csrsum
from dgl_amd.graph_index import GraphIndex, Relation

pytestmark = pytest.mark.gpu

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -24}
U16 = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
IDS = [torch.int32, torch.int64]
F3264 = [torch.float32, torch.float64]
FALL = [torch.float32, torch.float64, torch.float16, torch.bfloat16]


def _floor(v):
    return torch.where(v < 0, -1.0, 1.0).double() * v.abs().clamp_min(2.0 ** -6)


def rand_dense(m, n, draws, dtype, seed):
    """Dense fp64 (m, n) matrix of the recipe above; its entries are exactly representable in `dtype`."""
    g = torch.Generator().manual_seed(seed)
    d = torch.zeros(m, n, dtype=torch.float64)
    if draws == 0 or m == 0 or n == 0:
        return d
    key = torch.unique(torch.randint(0, m, (draws,), generator=g) * n + torch.randint(0, n, (draws,), generator=g))
    v = _floor(torch.randn(key.shape[0], generator=g, dtype=torch.float64)).to(dtype).double()
    d.view(-1)[key] = v
    return d


def make(d, idtype, dtype, dev, with_map=True, seed=0):
    """(GraphIndex, weights, (rows, cols) in edge-id order on the CPU) of the graph whose adjacency matrix is `d`."""
    m, n = d.shape
    r, c = d.nonzero(as_tuple=True)   # row-major
    w = d[r, c].to(dtype)
    if with_map:   # shuffled COO: its CSR carries an edge-id map
        p = torch.randperm(r.shape[0], generator=torch.Generator().manual_seed(seed + 99))
        r, c, w = r[p], c[p], w[p]
        rel = Relation(m, n, r.to(idtype).to(dev), c.to(idtype).to(dev), idtype=idtype, device=dev)
    else:          # a sorted CSR without a map: edge id == position
        indptr = torch.zeros(m + 1, dtype=torch.int64)
        indptr[1:] = torch.cumsum(torch.bincount(r, minlength=m), 0)
        rel = Relation(m, n, csr=(indptr.to(idtype).to(dev), c.to(idtype).to(dev), None), idtype=idtype, device=dev)
    return GraphIndex([m, n], [(0, 1)], [rel]), w.to(dev), (r, c)


def csr_of(gidx):
    rel = gidx.relations[0]
    indptr, indices, eids = rel.csr()
    assert eids is None, "the result must not carry an edge-id map"
    assert indptr.dtype == rel.idtype and indices.dtype == rel.idtype
    return indptr.cpu().long(), indices.cpu().long()


def check_structure(gidx, w, t):
    """indptr / indices == the non-zero pattern of t in row-major order (which is: columns ascend strictly in every
    row); returns (rows, cols)."""
    indptr, indices = csr_of(gidx)
    r_ref, c_ref = (t > 0).nonzero(as_tuple=True)
    assert indptr.shape[0] == t.shape[0] + 1 and int(indptr[0]) == 0
    assert int(indptr[-1]) == indices.shape[0] == w.shape[0] == gidx.num_edges(0)
    assert torch.equal(indptr[1:] - indptr[:-1], torch.bincount(r_ref, minlength=t.shape[0]))
    assert torch.equal(indices, c_ref)
    return r_ref, c_ref


def check_values(got, exact, t, s, dtype, what):
    err = (got.detach().double().cpu() - exact).abs()
    bound = 1.01 * (t + 1) * U[dtype] * s + U16[dtype] * exact.abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: %d entries, max t %d, max err / bound %.3f" % (what, err.numel(), int(t.max()) if t.numel() else 0, ratio))
    assert bool((err <= bound).all()), what


def mm_reference(da, db):
    pa, pb = (da != 0).double(), (db != 0).double()
    return da @ db, pa @ pb, da.abs() @ db.abs()


def check_mm(gc, w, da, db, dtype, what):
    exact, t, s = mm_reference(da, db)
    r, c = check_structure(gc, w, t)
    check_values(w, exact[r, c], t[r, c], s[r, c], dtype, what)


@functools.lru_cache(maxsize=None)
def reference_operands(dtype):
    """The reference test's sizes: 500 x 600 x 700 with 9 000 draws per operand (the sum: two 500 x 600 operands)."""
    return rand_dense(500, 600, 9000, dtype, 1), rand_dense(600, 700, 9000, dtype, 2), rand_dense(500, 600, 9000, dtype, 3)


@pytest.mark.parametrize("dtype", FALL)
@pytest.mark.parametrize("idtype", IDS)
def test_csrmm_reference_sizes(dev, idtype, dtype):
    da, db, _ = reference_operands(dtype)
    ga, wa, _ = make(da, idtype, dtype, dev)
    gb, wb, _ = make(db, idtype, dtype, dev, seed=1)
    gc, w = sparse_kernels._csrmm(ga, wa, gb, wb, 2)
    assert w.dtype == dtype and gc.number_of_ntypes() == 2 and gc.num_nodes(0) == 500 and gc.num_nodes(1) == 700
    check_mm(gc, w, da, db, dtype, "csrmm %s %s" % (idtype, dtype))


@pytest.mark.parametrize("dtype", FALL)
@pytest.mark.parametrize("idtype", IDS)
def test_csrsum_reference_sizes(dev, idtype, dtype):
    da, _, db = reference_operands(dtype)
    ga, wa, _ = make(da, idtype, dtype, dev)
    gb, wb, _ = make(db, idtype, dtype, dev, seed=1)
    gc, w = sparse_kernels._csrsum([ga, gb], [wa, wb])
    t = (da != 0).double() + (db != 0).double()
    r, c = check_structure(gc, w, t)
    check_values(w, (da + db)[r, c], t[r, c], (da.abs() + db.abs())[r, c], dtype, "csrsum %s %s" % (idtype, dtype))
    # one operand: the operand itself with sorted columns and permuted weights — a copy
    g1, w1 = sparse_kernels._csrsum([ga], [wa])
    r, c = check_structure(g1, w1, (da != 0).double())
    assert torch.equal(w1.cpu().double(), da[r, c])


def _row_class_case(dtype):
    """6 x K x P: rows of A with exactly T1, T1 + 1, T2, T2 + 1 terms, an empty row and one far above T2; P spans
    several column windows of the last class.  B rows 0 .. K-5 have 16 entries, the last four 8, 4, 2 and 1."""
    t1, t2 = _capi.csr_mm_row_classes()
    targets = [t1, t1 + 1, 0, t2, t2 + 1, t2 + t2 // 2 + 11]
    g = torch.Generator().manual_seed(7)
    k16 = max(targets) // 16 + 8
    k, p = k16 + 4, 9000
    degs = [16] * k16 + [8, 4, 2, 1]
    db = torch.zeros(k, p, dtype=torch.float64)
    for i, dg in enumerate(degs):
        cols = torch.randperm(p, generator=g)[:dg]
        db[i, cols] = _floor(torch.randn(dg, generator=g, dtype=torch.float64)).to(dtype).double()
    da = torch.zeros(len(targets), k, dtype=torch.float64)
    for i, ub in enumerate(targets):
        q, r = divmod(ub, 16)
        rows = torch.randperm(k16, generator=g)[:q].tolist() + [k16 + j for j in range(4) if r & (8 >> j)]
        da[i, rows] = _floor(torch.randn(len(rows), generator=g, dtype=torch.float64)).to(dtype).double()
    assert ((da != 0).double() @ (db != 0).double()).sum(1).long().tolist() == targets   # ub is hit exactly
    return da, db


@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_row_classes(dev, idtype, dtype):
    da, db = _row_class_case(dtype)
    ga, wa, _ = make(da, idtype, dtype, dev)
    gb, wb, _ = make(db, idtype, dtype, dev, seed=1)
    gc, w = sparse_kernels._csrmm(ga, wa, gb, wb, 2)
    check_mm(gc, w, da, db, dtype, "row classes %s %s" % (idtype, dtype))
    # the sum over the same classes: operand rows of 20 / 40 / 2 000 / 0 / 3 000 entries -> 40 / 80 / 4 000 / 0 / 6 000 terms
    ds = [torch.zeros(5, 9000, dtype=torch.float64) for _ in range(2)]
    g = torch.Generator().manual_seed(11)
    for d in ds:
        for row, n in enumerate((20, 40, 2000, 0, 3000)):
            d[row, torch.randperm(9000, generator=g)[:n]] = _floor(torch.randn(n, generator=g, dtype=torch.float64)).to(dtype).double()
    ops = [make(d, idtype, dtype, dev, seed=i) for i, d in enumerate(ds)]
    gs, ws = sparse_kernels._csrsum([o[0] for o in ops], [o[1] for o in ops])
    t = (ds[0] != 0).double() + (ds[1] != 0).double()
    r, c = check_structure(gs, ws, t)
    check_values(ws, (ds[0] + ds[1])[r, c], t[r, c], (ds[0].abs() + ds[1].abs())[r, c], dtype, "sum classes")


@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_collisions_and_permutation(dev, idtype, dtype):
    da = rand_dense(50, 40, 600, dtype, 21)
    ga, wa, _ = make(da, idtype, dtype, dev)
    # every row of B identical: all products of a row of A fall on the same five columns
    row = torch.zeros(30, dtype=torch.float64)
    row[[2, 3, 11, 17, 29]] = torch.tensor([1.5, -0.75, 2.25, 0.5, -3.0], dtype=torch.float64)
    db = row.repeat(40, 1)
    gb, wb, _ = make(db, idtype, dtype, dev, seed=1)
    gc, w = sparse_kernels._csrmm(ga, wa, gb, wb, 2)
    check_mm(gc, w, da, db, dtype, "collisions")
    # B a permutation matrix: no two products meet, every entry is one product
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(5))
    dp = torch.zeros(40, 40, dtype=torch.float64)
    dp[torch.arange(40), perm] = 1.0
    gp, wp, _ = make(dp, idtype, dtype, dev, seed=2)
    gc, w = sparse_kernels._csrmm(ga, wa, gp, wp, 2)
    check_mm(gc, w, da, dp, dtype, "permutation")
    r, c = (da @ dp != 0).nonzero(as_tuple=True)
    assert torch.equal(w.cpu().double(), (da @ dp)[r, c])   # one exact product each


@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_cancellation_keeps_the_entry(dev, idtype, dtype):
    da = torch.tensor([[1.0, 1.0], [1.0, 0.0]], dtype=torch.float64)
    db = torch.tensor([[1.0, 2.0], [-1.0, 3.0]], dtype=torch.float64)
    ga, wa, _ = make(da, idtype, dtype, dev)
    gb, wb, _ = make(db, idtype, dtype, dev, seed=1)
    gc, w = sparse_kernels._csrmm(ga, wa, gb, wb, 1)
    indptr, indices = csr_of(gc)
    assert indptr.tolist() == [0, 2, 4] and indices.tolist() == [0, 1, 0, 1]
    assert w.cpu().tolist() == [0.0, 5.0, 1.0, 2.0]     # (0, 0) = 1 - 1: present, with value 0
    gs, ws = sparse_kernels._csrsum([ga, make(-da, idtype, dtype, dev, seed=3)[0]], [wa, make(-da, idtype, dtype, dev, seed=3)[1]])
    assert csr_of(gs)[1].tolist() == [0, 1, 0] and ws.cpu().tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_edge_id_map_combinations(dev, idtype, dtype):
    da, db = rand_dense(70, 90, 900, dtype, 31), rand_dense(90, 80, 900, dtype, 32)
    results = []
    for map_a in (False, True):
        for map_b in (False, True):
            ga, wa, _ = make(da, idtype, dtype, dev, with_map=map_a)
            gb, wb, _ = make(db, idtype, dtype, dev, with_map=map_b, seed=1)
            assert (ga.relations[0].csr()[2] is not None) == map_a and (gb.relations[0].csr()[2] is not None) == map_b
            gc, w = sparse_kernels._csrmm(ga, wa, gb, wb, 2)
            check_mm(gc, w, da, db, dtype, "maps %s %s" % (map_a, map_b))
            gs, ws = sparse_kernels._csrsum([ga, ga], [wa, wa])
            assert torch.equal(ws.cpu().double(), (2 * da)[da != 0])
            results.append(w)
    # B's map only relabels edges: the terms and their order are the same.  A's map changes the position order of A's rows
    # (a shuffled COO compresses to rows in shuffled order), hence the order of additions — not compared bit for bit.
    assert torch.equal(results[0], results[1]) and torch.equal(results[2], results[3])


def _empty_rel(m, n, idtype, dev):
    e = torch.empty(0, dtype=idtype, device=dev)
    return GraphIndex([m, n], [(0, 1)], [Relation(m, n, e, e.clone(), idtype=idtype, device=dev)])


@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_zero_sizes(dev, idtype, dtype):
    da, db = rand_dense(50, 60, 300, dtype, 41), rand_dense(60, 70, 300, dtype, 42)
    ga, wa, _ = make(da, idtype, dtype, dev)
    gb, wb, _ = make(db, idtype, dtype, dev, seed=1)
    none = torch.empty(0, dtype=dtype, device=dev)
    for gx, wx, gy, wy, m, p in ((_empty_rel(50, 60, idtype, dev), none, gb, wb, 50, 70),       # nnz(A) = 0
                                 (ga, wa, _empty_rel(60, 70, idtype, dev), none, 50, 70),       # nnz(B) = 0
                                 (_empty_rel(0, 60, idtype, dev), none, gb, wb, 0, 70),         # M = 0
                                 (ga, wa, _empty_rel(60, 0, idtype, dev), none, 50, 0),         # P = 0
                                 (_empty_rel(50, 0, idtype, dev), none, _empty_rel(0, 70, idtype, dev), none, 50, 70)):  # K = 0
        gc, w = sparse_kernels._csrmm(gx, wx, gy, wy, 2)
        indptr, indices = csr_of(gc)
        assert indptr.tolist() == [0] * (m + 1) and indices.numel() == 0 and w.numel() == 0 and w.dtype == dtype
        assert gc.num_nodes(0) == m and gc.num_nodes(1) == p
    gs, ws = sparse_kernels._csrsum([_empty_rel(50, 60, idtype, dev), ga], [none, wa])
    r, c = check_structure(gs, ws, (da != 0).double())
    assert torch.equal(ws.cpu().double(), da[r, c])
    gs, ws = sparse_kernels._csrsum([_empty_rel(50, 60, idtype, dev)] * 2, [none, none])
    assert csr_of(gs)[0].tolist() == [0] * 51 and ws.numel() == 0
    # the mask with A empty, B empty, or both (the reference's A_nnz, B_nnz in {9000, 0})
    big_a, big_b = rand_dense(500, 600, 9000, dtype, 43), rand_dense(500, 600, 9000, dtype, 44)
    gA, wA, _ = make(big_a, idtype, dtype, dev)
    gB, _, (rb, cb) = make(big_b, idtype, dtype, dev, seed=1)
    e = _empty_rel(500, 600, idtype, dev)
    assert torch.equal(sparse_kernels._csrmask(gA, wA, gB).cpu().double(), big_a[rb, cb])
    out = sparse_kernels._csrmask(e, none, gB)
    assert out.shape[0] == rb.shape[0] and not bool(out.any())
    assert sparse_kernels._csrmask(gA, wA, e).numel() == 0 and sparse_kernels._csrmask(e, none, e).numel() == 0


@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_determinism_stream_and_workspace(dev, idtype, dtype):
    da, db = _row_class_case(dtype)   # every row class
    ga, wa, _ = make(da, idtype, dtype, dev)
    gb, wb, _ = make(db, idtype, dtype, dev, seed=1)
    first = sparse_kernels._csrmm(ga, wa, gb, wb, 2)
    again = sparse_kernels._csrmm(ga, wa, gb, wb, 2)
    want = csr_of(first[0]) + (first[1].cpu(),)
    for x, y in zip(want, csr_of(again[0]) + (again[1].cpu(),)):
        assert torch.equal(x, y)
    # the C ABI directly: a non-default stream, and a workspace passed by the caller
    a = _capi.make_csr(*ga.relations[0].csr(), 0 + db.shape[0])
    b = _capi.make_csr(*gb.relations[0].csr(), db.shape[1])
    ws = torch.empty(_capi.csr_mm_workspace_bytes(a, b), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = _capi.csr_mm(a, wa, b, wb)
    side.synchronize()
    with_ws = _capi.csr_mm(a, wa, b, wb, workspace=ws)
    for got in (on_side, with_ws):
        assert torch.equal(got[0].cpu().long(), want[0]) and torch.equal(got[1].cpu().long(), want[1])
        assert torch.equal(got[2].cpu(), want[2])
    s1 = _capi.csr_sum([a, a], [wa, wa])
    s2 = _capi.csr_sum([a, a], [wa, wa], workspace=torch.empty(1 << 20, dtype=torch.uint8, device=dev))
    assert all(torch.equal(x, y) for x, y in zip(s1, s2))


@pytest.mark.parametrize("dtype", FALL)
@pytest.mark.parametrize("idtype", IDS)
def test_mask_is_a_copy(dev, idtype, dtype):
    da, db = rand_dense(200, 300, 5000, dtype, 51), rand_dense(200, 300, 5000, dtype, 52)
    da[7] = 0
    da[7, 123] = 0.5                       # a row of one entry
    db[7, 123], db[7, 124] = 1.0, 1.0      # queried, and its neighbour missed
    gb, _, (rb, cb) = make(db, idtype, dtype, dev, seed=1)
    # A unsorted: a shuffled COO leaves the columns of a row in shuffled order
    ga, wa, _ = make(da, idtype, dtype, dev)
    indptr, indices, _ = ga.relations[0].csr()
    assert bool((indices[1:] < indices[:-1]).sum() > indptr.shape[0])   # descents inside rows, not only at row ends
    out = sparse_kernels._csrmask(ga, wa, gb)
    assert out.dtype == dtype and torch.equal(out.cpu().double(), da[rb, cb])
    # A sorted: the sum's own output
    gs, ws = sparse_kernels._csrsum([ga], [wa])
    assert torch.equal(sparse_kernels._csrmask(gs, ws, gb).cpu().double(), da[rb, cb])
    # B given as a CSR with a map (its COO is derived and carries edge ids): still B's edge-id order
    r_sorted, c_sorted = db.nonzero(as_tuple=True)
    p = torch.randperm(r_sorted.shape[0], generator=torch.Generator().manual_seed(3))
    indptr_b = torch.zeros(201, dtype=torch.int64)
    indptr_b[1:] = torch.cumsum(torch.bincount(r_sorted, minlength=200), 0)
    rel = Relation(200, 300, csr=(indptr_b.to(idtype).to(dev), c_sorted.to(idtype).to(dev), p.to(idtype).to(dev)),
                   idtype=idtype, device=dev)
    out = sparse_kernels._csrmask(ga, wa, GraphIndex([200, 300], [(0, 1)], [rel]))
    want = torch.empty(p.shape[0], dtype=torch.float64)
    want[p] = da[r_sorted, c_sorted]
    assert torch.equal(out.cpu().double(), want)


# ---- autograd ---------------------------------------------------------------------------------------------------------
def _mm_backward_case(dev, idtype, dtype, m, k, p, draws, num_vtypes, seed):
    da, db = rand_dense(m, k, draws, dtype, seed), rand_dense(k, p, draws, dtype, seed + 1)
    ga, wa, (ra, ca) = make(da, idtype, dtype, dev)
    gb, wb, (rb, cb) = make(db, idtype, dtype, dev, seed=1)
    wa.requires_grad_()
    wb.requires_grad_()
    gc, wc = csrmm(ga, wa, gb, wb, num_vtypes)
    assert gc.number_of_ntypes() == num_vtypes and type(wc.grad_fn).__name__ == "CSRMMBackward"
    check_mm(gc, wc, da, db, dtype, "forward")
    r, c = (((da != 0).double() @ (db != 0).double()) > 0).nonzero(as_tuple=True)
    up = _floor(torch.randn(r.shape[0], generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)).to(dtype)
    (wc * up.to(dev)).sum().backward()
    # autograd through the dense fp64 product
    xa, xb = da.clone().requires_grad_(), db.clone().requires_grad_()
    dc = torch.zeros(m, p, dtype=torch.float64)
    dc[r, c] = up.double()
    ((xa @ xb) * dc).sum().backward()
    pa, pb, pc = (da != 0).double(), (db != 0).double(), (dc != 0).double()
    check_values(wa.grad, xa.grad[ra, ca], (pc @ pb.t())[ra, ca], (dc.abs() @ db.abs().t())[ra, ca], dtype, "dA")
    check_values(wb.grad, xb.grad[rb, cb], (pa.t() @ pc)[rb, cb], (da.abs().t() @ dc.abs())[rb, cb], dtype, "dB")


@pytest.mark.parametrize("num_vtypes", [1, 2])
@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_csrmm_backward_small(dev, idtype, dtype, num_vtypes):
    _mm_backward_case(dev, idtype, dtype, 3, 4, 3, 6, num_vtypes, 61)


@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_csrmm_backward_larger(dev, idtype, dtype):
    _mm_backward_case(dev, idtype, dtype, 60, 70, 80, 600, 2, 71)


@pytest.mark.parametrize("m,n,draws", [(3, 4, 6), (60, 70, 600)])
@pytest.mark.parametrize("nelems", [1, 2])
@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_csrsum_backward(dev, idtype, dtype, nelems, m, n, draws):
    ds = [rand_dense(m, n, draws, dtype, 81 + i) for i in range(nelems)]
    ops = [make(d, idtype, dtype, dev, seed=i) for i, d in enumerate(ds)]
    ws = [o[1].requires_grad_() for o in ops]
    gc, wc = csrsum([o[0] for o in ops], ws)
    assert type(wc.grad_fn).__name__ == "CSRSumBackward"
    t = sum((d != 0).double() for d in ds)
    r, c = check_structure(gc, wc, t)
    check_values(wc, sum(ds)[r, c], t[r, c], sum(d.abs() for d in ds)[r, c], dtype, "forward")
    up = _floor(torch.randn(r.shape[0], generator=torch.Generator().manual_seed(5), dtype=torch.float64)).to(dtype)
    (wc * up.to(dev)).sum().backward()
    dc = torch.zeros(m, n, dtype=torch.float64)
    dc[r, c] = up.double()
    for w, (_, _, (rk, ck)) in zip(ws, ops):   # d(sum)/dA_k = dC at A_k's entries: one term, copied
        one = torch.ones(rk.shape[0], dtype=torch.float64)
        check_values(w.grad, dc[rk, ck], one, dc[rk, ck].abs(), dtype, "dA_k")


@pytest.mark.parametrize("m,n,draws", [(3, 4, 6), (60, 70, 600)])
@pytest.mark.parametrize("dtype", F3264)
@pytest.mark.parametrize("idtype", IDS)
def test_csrmask_backward(dev, idtype, dtype, m, n, draws):
    da, db = rand_dense(m, n, draws, dtype, 91), rand_dense(m, n, draws, dtype, 92)
    ga, wa, (ra, ca) = make(da, idtype, dtype, dev)
    gb, _, (rb, cb) = make(db, idtype, dtype, dev, seed=1)
    wa.requires_grad_()
    out = csrmask(ga, wa, gb)
    assert torch.equal(out.detach().cpu().double(), da[rb, cb])
    up = _floor(torch.randn(rb.shape[0], generator=torch.Generator().manual_seed(6), dtype=torch.float64)).to(dtype)
    (out * up.to(dev)).sum().backward()
    xa = da.clone().requires_grad_()
    (xa[rb, cb] * up.double()).sum().backward()
    assert torch.equal(wa.grad.cpu().double(), xa.grad[ra, ca])   # a copy in both directions


@pytest.mark.parametrize("idtype", IDS)
def test_gradcheck_fp64(dev, idtype):
    da, db = rand_dense(3, 4, 6, torch.float64, 101), rand_dense(4, 3, 6, torch.float64, 102)
    ga, wa, _ = make(da, idtype, torch.float64, dev)
    gb, wb, _ = make(db, idtype, torch.float64, dev, seed=1)
    wa.requires_grad_()
    wb.requires_grad_()
    assert torch.autograd.gradcheck(lambda x, y: csrmm(ga, x, gb, y, 1)[1], (wa, wb))
    assert torch.autograd.gradcheck(lambda x, y: csrsum([ga, ga], [x, y])[1], (wa, wa.detach().clone().requires_grad_()))
    assert torch.autograd.gradcheck(lambda x: csrmask(ga, x, ga), (wa,))


# ---- the user-facing transforms ----------------------------------------------------------------------------------------
def _hetero(canonical, rows, cols, num_nodes, idtype, dev, w=None):
    g = dgl_amd.heterograph({canonical: (torch.tensor(rows, dtype=idtype, device=dev), torch.tensor(cols, dtype=idtype, device=dev))},
                            num_nodes_dict=num_nodes)
    g.edata["w"] = (torch.randn(len(rows), generator=torch.Generator().manual_seed(1)) if w is None else w).to(dev)
    return g


@pytest.mark.parametrize("idtype", IDS)
def test_adj_product_graph(dev, idtype):
    n = {"A": 3, "B": 4, "C": 3}
    A = _hetero(("A", "AB", "B"), [2, 2, 0, 2, 0, 1], [2, 1, 0, 0, 2, 2], {"A": 3, "B": 4}, idtype, dev)
    B = _hetero(("B", "BA", "A"), [0, 3, 2, 1, 3, 3], [1, 2, 0, 2, 1, 0], {"A": 3, "B": 4}, idtype, dev)
    A.edata["w"].requires_grad_()
    B.edata["w"].requires_grad_()
    C = dgl_amd.adj_product_graph(A, B, "w")
    assert C.ntypes == ["A"] and C.canonical_etypes == [("A", "_E", "A")] and C.idtype == idtype
    src, dst = C.edges()
    # the docstring example of the reference (transforms/functional.py:2643-2645), which lists hash order; here row-major
    assert list(zip(src.tolist(), dst.tolist())) == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (2, 2)]
    assert type(C.edata["w"].grad_fn).__name__ == "CSRMMBackward"
    da = torch.zeros(3, 4, dtype=torch.float64)
    da[[2, 2, 0, 2, 0, 1], [2, 1, 0, 0, 2, 2]] = A.edata["w"].detach().cpu().double()
    db = torch.zeros(4, 3, dtype=torch.float64)
    db[[0, 3, 2, 1, 3, 3], [1, 2, 0, 2, 1, 0]] = B.edata["w"].detach().cpu().double()
    exact, t, s = mm_reference(da, db)
    check_values(C.edata["w"], exact[src.cpu().long(), dst.cpu().long()], t[src.cpu().long(), dst.cpu().long()],
                 s[src.cpu().long(), dst.cpu().long()], torch.float32, "adj_product_graph")
    C.edata["w"].sum().backward()
    assert A.edata["w"].grad is not None and B.edata["w"].grad is not None
    B2 = _hetero(("B", "BC", "C"), [0, 3, 2, 1, 3, 3], [1, 2, 0, 2, 1, 0], {"C": 3, "B": 4}, idtype, dev)
    C2 = dgl_amd.adj_product_graph(A, B2, "w", etype="AC")
    assert C2.ntypes == ["A", "C"] and C2.canonical_etypes == [("A", "AC", "C")]
    assert C2.num_nodes("A") == n["A"] and C2.num_nodes("C") == n["C"] and C2.num_edges() == 6
    restricted = A.formats(["coo", "csc"])
    with pytest.raises(dgl_amd.DGLAMDError, match="CSR"):
        dgl_amd.adj_product_graph(restricted, B, "w")


@pytest.mark.parametrize("idtype", IDS)
def test_adj_sum_graph(dev, idtype):
    A = _hetero(("A", "AB", "B"), [2, 2, 0, 2, 0, 1], [2, 1, 0, 0, 2, 2], {"A": 3, "B": 4}, idtype, dev)
    B = _hetero(("A", "AB", "B"), [1, 2, 0, 2, 1, 0], [0, 3, 2, 1, 3, 3], {"A": 3, "B": 4}, idtype, dev,
                w=torch.randn(6, generator=torch.Generator().manual_seed(2)))
    A.edata["w"].requires_grad_()
    B.edata["w"].requires_grad_()
    C = dgl_amd.adj_sum_graph([A, B], "w")
    assert C.canonical_etypes == A.canonical_etypes and C.ntypes == A.ntypes
    src, dst = C.edges()
    # the reference's docstring example (transforms/functional.py:2786-2788), row-major here
    assert list(zip(src.tolist(), dst.tolist())) == [(0, 0), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3)]
    da, db = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64)
    da[[2, 2, 0, 2, 0, 1], [2, 1, 0, 0, 2, 2]] = A.edata["w"].detach().cpu().double()
    db[[1, 2, 0, 2, 1, 0], [0, 3, 2, 1, 3, 3]] = B.edata["w"].detach().cpu().double()
    i, j = src.cpu().long(), dst.cpu().long()
    check_values(C.edata["w"], (da + db)[i, j], ((da != 0).double() + (db != 0).double())[i, j], (da.abs() + db.abs())[i, j],
                 torch.float32, "adj_sum_graph")
    C.edata["w"].sum().backward()
    assert torch.equal(A.edata["w"].grad.cpu(), torch.ones(6)) and torch.equal(B.edata["w"].grad.cpu(), torch.ones(6))
    one = dgl_amd.adj_sum_graph([A], "w")
    assert one.canonical_etypes == A.canonical_etypes and one.num_edges() == 6
    s1, d1 = one.edges()
    assert list(zip(s1.tolist(), d1.tolist())) == [(0, 0), (0, 2), (1, 2), (2, 0), (2, 1), (2, 2)]
    with pytest.raises(ValueError):
        dgl_amd.adj_sum_graph([], "w")


@pytest.mark.parametrize("dtype", FALL)
@pytest.mark.parametrize("idtype", IDS)
def test_spspmm_takes_the_kernels(dev, idtype, dtype):
    from dgl_amd import sparse as dglsp

    da, db = rand_dense(120, 150, 1500, dtype, 111), rand_dense(150, 130, 1500, dtype, 112)
    mats = []
    for d, seed in ((da, 0), (db, 1)):
        r, c = d.nonzero(as_tuple=True)
        p = torch.randperm(r.shape[0], generator=torch.Generator().manual_seed(seed))
        mats.append(dglsp.from_coo(r[p].to(idtype).to(dev), c[p].to(idtype).to(dev), d[r[p], c[p]].to(dtype).to(dev), tuple(d.shape)))
    A, B = mats
    if dtype in F3264:
        A.val.requires_grad_()
    C = dglsp.spspmm(A, B)
    assert C.shape == (120, 130) and C.val.dtype == dtype and not C.has_duplicate()
    row, col = C.coo()
    exact, t, s = mm_reference(da, db)
    r, c = (t > 0).nonzero(as_tuple=True)
    assert torch.equal(row.cpu().long(), r) and torch.equal(col.cpu().long(), c)   # coalesced: row-major, unique
    check_values(C.val, exact[r, c], t[r, c], s[r, c], dtype, "spspmm")
    if dtype in F3264:
        assert type(C.val.grad_fn).__name__ == "CSRMMBackward"   # the new route, not the torch composition
        C.val.sum().backward()
        assert A.val.grad is not None and A.val.grad.shape == A.val.shape
