"""Guard bands (tests/guarded.py) around EVERY tensor a kernel receives: operands, the index arrays of the CSR / COO, outputs,
arg outputs and the workspace at exactly the byte count its query reports.  After the call both bands of every tensor must
still hold their poison byte (no write outside a buffer, no workspace layout that is a unit short), and the values must meet
the rule the kernel's own test already asserts — the bands of floating operands read as NaN, so a read past an operand's end
that reaches a result fails the value check.  Nothing here provokes a fault: every byte within a band's reach of a buffer
lies inside one live allocation of the test.

Shapes are tiny and chosen so that the LAST row / edge / segment / unit is partial and widths straddle the access width:
n_dst = 37, n_src = 29, e in {0, 1, 511, 512, 513}, one hub row of 300 edges, the last row empty or not, with and without an
edge-id permutation, int32 and int64 ids; 4- / 8-byte widths {1, 3, 4, 5, 8, 17, 33, 64, 65, 100}, 2-byte widths {1, 7, 8, 9,
24}; base pointers shifted by (lhs, rhs, out) elements in {(0,0,0), (1,0,0), (0,0,1), (3,2,1)} — the all-zero tuple is
256-byte aligned and takes the vector paths.  A parametrised case walks the widths and takes the next graph of the family
for each, so the cross product is covered along its diagonals, not in full; the g-SpMM, masked g-SpMM, segment and scatter
sweeps run every width on both states of the last row (_walk).

COVERED / EXEMPT at the end list every `dgl_amd._capi` entry point with an `out` or `workspace` parameter; a test that needs
no GPU keeps the two complete.  (The file name sorts after every other test file: new GPU tests are collected last.)"""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from tests import exclude_cases as xc
from tests import subgraph_cases as sc
from tests import topk_cases as tk
from tests import traversal_cases as tc
from tests.graphgen import coo_to_csc, coo_to_csr
from tests.guarded import POISON_FLOAT, POISON_INDEX, POISON_INT_OUT, guarded
from tests.tolerance import assert_fp32_sum

gpu = pytest.mark.gpu

N_DST, N_SRC, HUB, HUB_EDGES = 37, 29, 5, 300
EDGES = (0, 1, 511, 512, 513)
WIDE = (1, 3, 4, 5, 8, 17, 33, 64, 65, 100)          # 4- and 8-byte types
NARROW = (1, 7, 8, 9, 24)                            # 2-byte types
SHIFTS = ((0, 0, 0), (1, 0, 0), (0, 0, 1), (3, 2, 1))
SHIFT_IDS = ["aligned", "lhs1", "out1", "lhs3_rhs2_out1"]
HEADS_DIM = ((1, 1), (3, 8), (4, 25), (8, 16))
OPS = ("add", "sub", "mul", "div", "copy_lhs", "copy_rhs")
NP_F = {torch.float32: np.float32, torch.float64: np.float64}
T_I = {np.int32: torch.int32, np.int64: torch.int64}
U16 = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# 16-bit g-SpMM / g-SDDMM values: the (rtol, atol) of tests/test_gpu_api.py::test_half_through_api
HALF_API_TOL = {torch.float16: (1e-3, 0.5), torch.bfloat16: (4e-3, 2.0)}


def _size(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _h(t):
    return t.detach().cpu().numpy()


class Bag:
    """The guarded tensors of one call; `check` runs every band check."""

    def __init__(self, dev, *inherit):
        self.dev, self.items = dev, [it for bag in inherit for it in bag.items]

    def _add(self, name, g):
        self.items.append((name, g))
        return g.t

    def operand(self, name, values, shift=0):
        """A floating operand (numpy array or tensor), shifted by `shift` ELEMENTS."""
        if values is None:
            return None
        t = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(values))
        return self._add(name, guarded(self.dev, t.shape, t.dtype, fill=t, poison=POISON_FLOAT, shift=shift * _size(t.dtype)))

    def index(self, name, values):
        if values is None:
            return None
        t = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(values))
        return self._add(name, guarded(self.dev, t.shape, t.dtype, fill=t, poison=POISON_INDEX))

    def out(self, name, shape, dtype, shift=0):
        return self._add(name, guarded(self.dev, shape, dtype, poison=POISON_FLOAT, shift=shift * _size(dtype)))

    def int_out(self, name, shape, dtype):
        return self._add(name, guarded(self.dev, shape, dtype, poison=POISON_INT_OUT))

    def workspace(self, nbytes, name="workspace"):
        return self._add(name, guarded(self.dev, int(nbytes), torch.uint8, poison=POISON_INDEX))

    def check(self, where):
        for name, g in self.items:
            g.check("%s of %s" % (name, where))


# ---- the graph family ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coo(e, last_nonempty, n_src=N_SRC):
    """(src, dst) in a random edge order: a hub of 300 in-edges once there are 511, the last destination with 3 edges or
    with none."""
    rng = np.random.default_rng(1000 + 2 * e + int(last_nonempty))
    src = rng.integers(0, n_src, e)
    dst = rng.integers(0, N_DST - 1, e)
    if e >= 511:
        dst[:HUB_EDGES] = HUB
    if last_nonempty and e:
        dst[-min(3, e):] = N_DST - 1
    p = rng.permutation(e)
    return src[p], dst[p]


SHAPES = [(0, False)] + [(e, last) for e in EDGES[1:] for last in (False, True)]
VARIANTS = [(e, last, perm, idt) for (e, last) in SHAPES for perm in (True, False) for idt in (np.int32, np.int64)]   # 36
BIG = [v for v in VARIANTS if v[0] >= 511]                                                                          # 24


def _variant(k, pool=VARIANTS):
    return pool[k % len(pool)]


def _walk(widths, key, pool=VARIANTS):
    """(index, width, graph variant): every width on the variant `key(index)` picks AND on the same graph with the other
    state of the last row (empty / not empty)."""
    for wi, f in enumerate(widths):
        e, last, perm, idt = _variant(key(wi), pool)
        yield wi, f, (e, last, perm, idt)
        if e:
            yield wi, f, (e, not last, perm, idt)


@functools.lru_cache(maxsize=None)
def _csc(dev, e, last_nonempty, perm, idt, square=False):
    """The in-edge CSR (rows = destinations) of one member, its index arrays guarded on the device.  Without `perm` the
    CSR carries no edge-id map (edge id = position).  `square`: 37 source nodes too (ids stay below 29), the COO kept."""
    from dgl_amd import _capi

    src, dst = _coo(e, last_nonempty)
    if not perm:                                    # edge ids in destination order: the map is the identity
        o = np.lexsort((src, dst))
        src, dst = src[o], dst[o]
    indptr, indices, eids = coo_to_csc(src, dst, N_DST, idt)
    if not perm:
        assert np.array_equal(eids, np.arange(e))
        eids = None
    bag = Bag(dev)
    t = (bag.index("indptr", indptr), bag.index("indices", indices), bag.index("eids", eids))
    g = dict(src=src.astype(idt), dst=dst.astype(idt), indptr=indptr, indices=indices, eids=eids, e=e, bag=bag, idt=idt,
             deg=np.diff(indptr), csr=_capi.make_csr(t[0], t[1], t[2], N_DST if square else N_SRC),
             tag="e=%d last_%s %s %s" % (e, "nonempty" if last_nonempty else "empty", "mapped" if perm else "identity", idt.__name__))
    assert g["deg"][-1] == (3 if last_nonempty and e >= 3 else (e if last_nonempty else 0))
    return g


def _edge_pos(g):
    """CSR position -> edge id."""
    return np.arange(g["e"]) if g["eids"] is None else g["eids"].astype(np.int64)


# ---- g-SpMM -------------------------------------------------------------------------------------------------------
def _spmm_operands(rng, g, op, f, dt, scalar_e):
    """U(0, 1) + 0.5, the operands of tests/test_gpu_fuzz.py.  `sub` takes a quarter of the edge operand, so that every
    message u - e is positive: 300 differences of equal-sized operands cancel, and a bar relative to the SUM (which the
    fp32-sum rule is) then measures the cancellation, not the kernel — the reference's own fp32 loop misses it there."""
    u = (rng.random((N_SRC, f)) + 0.5).astype(dt) if op != "copy_rhs" else None
    w = (rng.random((g["e"], 1 if scalar_e else f)) + 0.5).astype(dt) if op != "copy_lhs" else None
    if op == "sub":
        w = (w * dt(0.25)).astype(dt)
    return u, w


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("red", ["sum", "max", "min"])
@pytest.mark.parametrize("op", OPS)
def test_spmm_csr(dev, op, red, tdtype, shift):
    from dgl_amd import _capi

    dt = NP_F[tdtype]
    rng = np.random.default_rng(OPS.index(op) * 100 + len(red) + shift[0])
    key = lambda wi: wi * 7 + OPS.index(op) * 11 + ["sum", "max", "min"].index(red) * 5 + SHIFTS.index(shift) * 3 + (tdtype == torch.float64)
    for wi, f, v in _walk(WIDE, key):
        g = _csc(dev, *v)
        scalar_e = wi % 3 == 2 and op in ("add", "sub", "mul", "div") and f > 1          # a broadcast edge weight
        u, w = _spmm_operands(rng, g, op, f, dt, scalar_e)
        ref, ru, re_ = oracle.spmm_csr(op, red, g["indptr"], g["indices"], g["eids"], u, w)
        bag = Bag(dev, g["bag"])
        tu, tw = bag.operand("ufeat", u, shift[0]), bag.operand("efeat", w, shift[1])
        out = bag.out("out", ref.shape, tdtype, shift[2])
        tid = T_I[g["idt"]]
        au = bag.int_out("arg_u", ref.shape, tid) if red != "sum" and u is not None else None
        ae = bag.int_out("arg_e", ref.shape, tid) if red != "sum" and w is not None else None
        ws = bag.workspace(_capi.spmm_csr_workspace_bytes(op, red, g["csr"], tdtype, tu, tw, out))
        where = "spmm_csr %s %s F=%d %s %s" % (op, red, f, tdtype, g["tag"])
        _capi.spmm_csr(op, red, g["csr"], tu, tw, out, au, ae, ws)
        bag.check(where)
        first = [None if t is None else t.clone() for t in (out, au, ae)]
        out.fill_(9.0)
        _capi.spmm_csr(op, red, g["csr"], tu, tw, out, au, ae, ws, plan_valid=True)
        bag.check(where + " (plan_valid)")
        for a, b in zip(first, (out, au, ae)):
            assert a is None or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), where
        got = _h(out)
        if red == "sum":
            f64 = lambda a: None if a is None else a.astype(np.float64)
            exact = oracle.spmm_csr(op, red, g["indptr"], g["indices"], g["eids"], f64(u), f64(w))[0]
            if tdtype == torch.float32:
                assert_fp32_sum(got, ref, exact)
            else:
                assert_fp32_sum(got, ref, exact, rtol=1e-12, atol=1e-12)
        else:
            np.testing.assert_array_equal(got, ref, err_msg=where)
            if ru is not None:
                np.testing.assert_array_equal(_h(au), ru, err_msg=where)
            if re_ is not None:
                np.testing.assert_array_equal(_h(ae), re_, err_msg=where)


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("op,red", [("copy_lhs", "sum"), ("mul", "sum"), ("copy_rhs", "sum"), ("copy_lhs", "max"), ("copy_rhs", "min")])
def test_spmm_csr_16bit(dev, op, red, tdtype, shift):
    """The band check is the new assertion for 16-bit storage.  Sums: the tolerances of test_gpu_api.py::
    test_half_through_api against the fp32 oracle of the widened operands.  max / min of a copy: the value is one of the
    operands, exactly; the arg names a source / edge of that destination that holds it, and equals the oracle's arg
    wherever the winner is unique."""
    from dgl_amd import _capi

    rng = np.random.default_rng(7 + len(op) + shift[0])
    for wi, f, v in _walk(NARROW, lambda wi: wi * 5 + len(op) + SHIFTS.index(shift) * 9 + (tdtype == torch.bfloat16)):
        g = _csc(dev, *v)
        u, w = _spmm_operands(rng, g, op, f, np.float32, False)
        u16, w16 = (None if a is None else torch.from_numpy(a).to(tdtype) for a in (u, w))
        wide = lambda t: None if t is None else t.float().numpy()
        ref, ru, re_ = oracle.spmm_csr(op, red, g["indptr"], g["indices"], g["eids"], wide(u16), wide(w16))
        bag = Bag(dev, g["bag"])
        tu, tw = bag.operand("ufeat", u16, shift[0]), bag.operand("efeat", w16, shift[1])
        out = bag.out("out", ref.shape, tdtype, shift[2])
        tid = T_I[g["idt"]]
        au = bag.int_out("arg_u", ref.shape, tid) if red != "sum" and u is not None else None
        ae = bag.int_out("arg_e", ref.shape, tid) if red != "sum" and w is not None else None
        ws = bag.workspace(_capi.spmm_csr_workspace_bytes(op, red, g["csr"], tdtype, tu, tw, out))
        where = "spmm_csr %s %s F=%d %s %s" % (op, red, f, tdtype, g["tag"])
        _capi.spmm_csr(op, red, g["csr"], tu, tw, out, au, ae, ws)
        bag.check(where)
        got = out.float().cpu().numpy()
        if red == "sum":
            rtol, atol = HALF_API_TOL[tdtype]
            np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=where)
            continue
        rows = g["deg"] > 0
        np.testing.assert_array_equal(got[rows], ref[rows], err_msg=where)
        arg, table = (_h(au), wide(u16)) if au is not None else (_h(ae), wide(w16))
        arg, cols = arg[rows], np.broadcast_to(np.arange(f), arg.shape)[rows]
        assert ((arg >= 0) & (arg < table.shape[0])).all(), where
        np.testing.assert_array_equal(table[arg, cols], ref[rows], err_msg=where + ": the arg does not hold the winner")
        # the arg is a source / edge OF THIS ROW, and the oracle's own wherever one candidate alone holds the winning value
        # (16-bit operands tie: 300 draws meet about 1 000 values; which of the tied the kernels name is not pinned here)
        full, want_arg, ids = (_h(au), ru, g["indices"].astype(np.int64)) if au is not None else (_h(ae), re_, _edge_pos(g))
        unique = 0
        for r in np.flatnonzero(rows):
            cand = np.unique(ids[g["indptr"][r]:g["indptr"][r + 1]])
            assert np.isin(full[r], cand).all(), (where, r)
            alone = (table[cand] == ref[r]).sum(0) == 1
            np.testing.assert_array_equal(full[r][alone], want_arg[r][alone], err_msg="%s row %d" % (where, r))
            unique += int(alone.sum())
        assert unique > 0 or not rows.any(), where


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("red", ["sum", "max", "min"])
@pytest.mark.parametrize("op", ["copy_lhs", "mul", "add", "copy_rhs"])
def test_spmm_coo(dev, op, red, tdtype, shift):
    from dgl_amd import _capi

    dt = NP_F[tdtype]
    rng = np.random.default_rng(31 + len(op) + shift[1])
    for wi, f, (e, last, perm, idt) in _walk(WIDE, lambda wi: wi * 7 + len(op) * 3 + len(red) + SHIFTS.index(shift) * 5):
        src, dst = (a.astype(idt) for a in _coo(e, last))
        eids = np.random.default_rng(e).permutation(e).astype(idt) if perm else None
        u = (rng.random((N_SRC, f)) + 0.5).astype(dt) if op != "copy_rhs" else None
        w = (rng.random((e, f)) + 0.5).astype(dt) if op != "copy_lhs" else None
        ref, ru, re_ = oracle.spmm_coo(op, red, src, dst, eids, N_DST, u, w)
        bag = Bag(dev)
        coo = _capi.make_coo(bag.index("row", src), bag.index("col", dst), bag.index("eids", eids), N_SRC, N_DST)
        tu, tw = bag.operand("ufeat", u, shift[0]), bag.operand("efeat", w, shift[1])
        out = bag.out("out", ref.shape, tdtype, shift[2])
        au = bag.int_out("arg_u", ref.shape, T_I[idt]) if red != "sum" else None
        ae = bag.int_out("arg_e", ref.shape, T_I[idt]) if red != "sum" else None
        where = "spmm_coo %s %s F=%d %s e=%d %s" % (op, red, f, tdtype, e, idt.__name__)
        _capi.spmm_coo(op, red, coo, tu, tw, out, au, ae)
        bag.check(where)
        if red == "sum":
            f64 = lambda a: None if a is None else a.astype(np.float64)
            exact = oracle.spmm_coo(op, red, src, dst, eids, N_DST, f64(u), f64(w))[0]
            if tdtype == torch.float32:
                assert_fp32_sum(_h(out), ref, exact)
            else:
                assert_fp32_sum(_h(out), ref, exact, rtol=1e-12, atol=1e-12)
        else:
            np.testing.assert_array_equal(_h(out), ref, err_msg=where)
            if ru is not None:
                np.testing.assert_array_equal(_h(au), ru, err_msg=where)
            if re_ is not None:
                np.testing.assert_array_equal(_h(ae), re_, err_msg=where)


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64, torch.bfloat16], ids=str)
@pytest.mark.parametrize("op", ["copy_lhs", "mul", "copy_rhs"])
def test_spmm_csr_stacked(dev, op, tdtype, shift):
    """Three relations into the 37 destinations (29, 5 and 1 source nodes; 513, 40 and 0 edges), the pointer tables
    guarded as well.  Values: tests/test_stacked.py::test_stacked_seam_equals_sum_of_relations (fp64 sum of the relations,
    rtol = atol = 1e-5 / 1e-12 / 1.2e-2)."""
    from dgl_amd import _capi
    from dgl_amd.graph_index import stack_csc

    rng = np.random.default_rng(5)
    use_u, use_e = op != "copy_rhs", op != "copy_lhs"
    for wi, f in enumerate(WIDE if tdtype != torch.bfloat16 else NARROW):
        idt = (np.int32, np.int64)[(wi + SHIFTS.index(shift)) % 2]
        rels = []
        for ns, ne in ((N_SRC, 513), (5, 40), (1, 0)):
            src = rng.integers(0, ns, ne)
            dst = rng.integers(0, N_DST - (wi % 2), ne)              # (every second width: the last row is empty)
            if ne > HUB_EDGES:
                dst[:HUB_EDGES] = HUB
            rels.append((ns, ne) + coo_to_csc(src, dst, N_DST, idt))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        stacked = stack_csc([(t(ip), t(ix), t(ei)) for _, _, ip, ix, ei in rels], N_DST, T_I[idt])
        us = [(torch.rand((ns, f), dtype=torch.float64) + 1).to(tdtype) for ns, *_ in rels]
        es = [(torch.rand((ne, f), dtype=torch.float64) + 1).to(tdtype) for _, ne, *_ in rels]
        want = 0
        for (ns, ne, ip, ix, ei), u, e in zip(rels, us, es):
            want = want + oracle.spmm_csr(op, "sum", ip, ix, ei, u.double().numpy() if use_u else None,
                                          e.double().numpy() if use_e else None)[0]
        bag = Bag(dev)
        names = ("indptr", "indices", "eids", "rel")
        indptr, indices, eids, rel = (bag.index(n, a) for n, a in zip(names, stacked))
        csr = _capi.make_csr(indptr, indices, eids, N_SRC)
        gu = [bag.operand("ufeat[%d]" % k, u, shift[0]) for k, u in enumerate(us)] if use_u else None
        ge = [bag.operand("efeat[%d]" % k, e, shift[1]) for k, e in enumerate(es)] if use_e else None
        table = lambda ts: None if ts is None else bag.index("table", torch.tensor([x.data_ptr() for x in ts], dtype=torch.int64))
        ut, et = table(gu), table(ge)
        out = bag.out("out", want.shape, tdtype, shift[2])
        ws = bag.workspace(_capi.spmm_csr_stacked_workspace_bytes(op, csr, gu[0] if use_u else None, ge[0] if use_e else None, out))
        where = "spmm_csr_stacked %s F=%d %s %s" % (op, f, tdtype, idt.__name__)
        _capi.spmm_csr_stacked(op, csr, rel, gu, ge, out, ws, u_table=ut, e_table=et)
        bag.check(where)
        tol = {torch.float32: 1e-5, torch.float64: 1e-12, torch.bfloat16: 1.2e-2}[tdtype]
        np.testing.assert_allclose(out.double().cpu().numpy(), want, rtol=tol, atol=tol, err_msg=where)
        first = out.clone()
        out.fill_(9.0)
        _capi.spmm_csr_stacked(op, csr, rel, gu, ge, out, ws, u_table=ut, e_table=et, plan_valid=True)
        bag.check(where + " (plan_valid)")
        assert torch.equal(first.view(torch.uint8), out.view(torch.uint8)), where


# ---- the max / min backward ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("form", ["plain", "other", "other_bcast", "stores"])
def test_spmm_cmp_backward(dev, form, tdtype, shift):
    """513 rows of dz scattered into 37 targets (the last one never named).  Values: the tolerances of tests/
    test_gpu_cmp_backward.py::test_cmp_backward_equals_the_reference_composition against its fp64 composition; `stores`
    (atomic = False, every target named at most once): bit-exact, and targets nobody names keep the sentinel."""
    from dgl_amd import _capi
    from dgl_amd.autograd import _bcast_group

    gen = torch.Generator().manual_seed(3 + shift[0])
    n, rows, orows = 513, N_DST, N_SRC
    tol = {torch.float32: 1e-5, torch.float64: 1e-12, torch.bfloat16: 6e-2, torch.float16: 1e-2}[tdtype]
    shapes = [(f,) for f in (WIDE if _size(tdtype) >= 4 else NARROW)] + [(3, 8), (4, 25)]
    for wi, shape in enumerate(shapes):
        idt = (torch.int32, torch.int64)[wi % 2]
        dz = torch.randn((n,) + shape, generator=gen).to(tdtype)
        other = arg_other = None
        grp = 1
        if form == "stores":
            width = int(np.prod(shape))
            # (target 0 is left out: it is shared with the destinations without in-edges and therefore ADDED to, see
            # tests/test_gpu_cmp_backward.py::test_edge_operand_row0_is_shared_with_empty_destinations)
            arg = torch.stack([torch.randperm(2 * n - 1, generator=gen)[:n] + 1 for _ in range(width)], 1).reshape((n,) + shape)
            arg[::7] = -1                                                # nothing won
            rows = 2 * n
        else:
            arg = torch.randint(-1, N_DST - 1, (n,) + shape, generator=gen)
        if form in ("other", "other_bcast"):
            oshape = shape if form == "other" or len(shape) == 1 else (shape[0], 1)
            other = torch.randn((orows,) + oshape, generator=gen).to(tdtype)
            arg_other = torch.randint(0, orows, (n,) + shape, generator=gen).to(idt)
            grp = _bcast_group(oshape, shape)[1]
        bag = Bag(dev)
        gdz, garg = bag.operand("dz", dz, shift[0]), bag.index("arg", arg.to(idt))
        gother = bag.operand("other", other, shift[1])
        gao = bag.index("arg_other", arg_other)
        out = bag.out("out", (rows,) + shape, tdtype, shift[2])
        where = "spmm_cmp_backward %s %s %s %s" % (form, shape, tdtype, idt)
        if form != "stores":
            out.zero_()
        _capi.spmm_cmp_backward(gdz, garg, out, gother, gao, grp, atomic=form != "stores")
        bag.check(where)
        ok = arg >= 0
        g = dz.double()
        if other is not None:
            g = other.double().expand(-1, *shape).gather(0, arg_other.long()) * g
        g = torch.where(ok, g, torch.zeros_like(g))
        if form == "stores":
            want = torch.full((rows,) + shape, 9.0, dtype=tdtype)
            flat = want.view(rows, -1)
            a2, d2 = arg.view(n, -1), dz.view(n, -1)
            for k in range(flat.shape[1]):
                sel = a2[:, k] >= 0
                flat[a2[sel, k], k] = d2[sel, k]
            assert torch.equal(out.cpu().view(torch.uint8), want.view(torch.uint8)), where
        else:
            want = torch.zeros((rows,) + shape, dtype=torch.float64).scatter_add_(0, arg.clamp(min=0), g)
            torch.testing.assert_close(out.double().cpu(), want, rtol=tol, atol=tol * 4)
            assert bool((out[N_DST - 1] == 0).all()), where


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("two_step", [False, True], ids=["one_step", "defer_finish"])
def test_spmm_cmp_mask_and_masked_spmm(dev, two_step, shift):
    """The gather form of the max / min backward on the family's graphs: the winner-bit mask at exactly
    spmm_cmp_mask_bytes, the masked g-SpMM over the reverse matrix with its workspace at exactly the reported size.
    Values: tests/test_gpu_cmp_backward.py::test_mask_kernel_two_step_form_equals_the_one_step_form (fp64 scatter_add,
    rtol = atol = 1e-5)."""
    from dgl_amd import _capi

    rng = np.random.default_rng(17 + shift[0])
    for wi, f, (e, last, _, idt) in _walk(WIDE, lambda wi: wi * 7 + SHIFTS.index(shift) * 3 + 12 * two_step):
        g = _csc(dev, e, last, False, idt)
        deg, indptr, indices = g["deg"], g["indptr"].astype(np.int64), g["indices"].astype(np.int64)
        pick = (rng.random((N_DST, f)) * np.maximum(deg, 1)[:, None]).astype(np.int64)
        pos = np.minimum(indptr[:-1, None] + pick, max(e - 1, 0))
        # the winner's source; rows without edges: 0
        arg = (np.where(deg[:, None] > 0, indices[pos], 0) if e else np.zeros((N_DST, f))).astype(idt)
        dz = rng.standard_normal((N_DST, f)).astype(np.float32)
        dst_of_pos = np.repeat(np.arange(N_DST), deg)
        order = np.argsort(indices * N_DST + dst_of_pos, kind="stable")
        rip = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=N_SRC))])
        bag = Bag(dev, g["bag"])
        rev = _capi.make_csr(bag.index("rev.indptr", rip.astype(idt)), bag.index("rev.indices", dst_of_pos[order].astype(idt)),
                             bag.index("rev.eids", order.astype(idt)), N_DST)
        garg, gdz = bag.index("arg", arg), bag.operand("dz", dz, shift[0])
        mask = bag.workspace(_capi.spmm_cmp_mask_bytes(torch.float32, N_DST, e, f), "mask")
        dx = bag.out("dx", (N_SRC, f), torch.float32, shift[2])
        ws = bag.workspace(_capi.spmm_csr_masked_workspace_bytes(rev, gdz, dx))
        where = "spmm_cmp_mask + spmm_csr_masked F=%d %s two_step=%s" % (f, g["tag"], two_step)
        if two_step:
            _capi.spmm_cmp_mask(g["csr"], garg, gdz, mask, dx, mode=_capi.CMP_MASK_DEFER)
            _capi.spmm_csr_masked(rev, gdz, mask, dx, workspace=ws, accumulate=False)
            _capi.spmm_cmp_mask(g["csr"], garg, gdz, mask, dx, mode=_capi.CMP_MASK_FINISH)
        else:
            dx.zero_()
            _capi.spmm_cmp_mask(g["csr"], garg, gdz, mask, dx)
            _capi.spmm_csr_masked(rev, gdz, mask, dx, workspace=ws, accumulate=True)
        bag.check(where)
        want = torch.zeros(N_SRC, f, dtype=torch.float64).scatter_add_(0, torch.from_numpy(arg.astype(np.int64)),
                                                                        torch.from_numpy(dz).double())
        torch.testing.assert_close(dx.double().cpu(), want, rtol=1e-5, atol=1e-5)
        first = dx.clone()
        if two_step:                                # the cached plan of the masked g-SpMM: the same bits
            dx.fill_(9.0)
            _capi.spmm_cmp_mask(g["csr"], garg, gdz, mask, dx, mode=_capi.CMP_MASK_DEFER)
            _capi.spmm_csr_masked(rev, gdz, mask, dx, workspace=ws, accumulate=False, plan_valid=True)
            _capi.spmm_cmp_mask(g["csr"], garg, gdz, mask, dx, mode=_capi.CMP_MASK_FINISH)
            bag.check(where + " (plan_valid)")
            assert torch.equal(first, dx), where


# ---- g-SDDMM ------------------------------------------------------------------------------------------------------
def _sddmm_case(dev, fmt, op, lt, rt, lshape, rshape, tdtype, shift, k):
    from dgl_amd import _capi

    e, last, perm, idt = _variant(k)
    src, dst = (a.astype(idt) for a in _coo(e, last))
    if fmt == "csr" and not perm:                  # edge ids in source order: the CSR's map is the identity and is left out
        o = np.lexsort((dst, src))
        src, dst = src[o], dst[o]
    cnt = {"u": N_SRC, "e": e, "v": N_DST}
    rng = np.random.default_rng(k)
    half = _size(tdtype) == 2
    draw = lambda n, shape: torch.from_numpy(rng.random((n,) + shape) + 0.5).to(tdtype)
    lhs = draw(cnt[lt], lshape) if op != "copy_rhs" else None
    rhs = draw(cnt[rt], rshape) if op != "copy_lhs" else None
    wide = lambda t: None if t is None else (t.float().numpy() if half else t.numpy())
    bag = Bag(dev)
    if fmt == "coo":
        eids = np.random.default_rng(e + 1).permutation(e).astype(idt) if perm else None
        want = oracle.sddmm_coo(op, src, dst, eids, wide(lhs), wide(rhs), lt, rt)
        sp = _capi.make_coo(bag.index("row", src), bag.index("col", dst), bag.index("eids", eids), N_SRC, N_DST)
        fn = _capi.sddmm_coo
    else:
        indptr, indices, eids = coo_to_csr(src, dst, N_SRC, idt)
        if not perm:
            assert np.array_equal(eids, np.arange(e))
            eids = None
        want = oracle.sddmm_csr(op, indptr, indices, eids, wide(lhs), wide(rhs), lt, rt)
        sp = _capi.make_csr(bag.index("indptr", indptr), bag.index("indices", indices), bag.index("eids", eids), N_DST)
        fn = _capi.sddmm_csr
    gl, gr = bag.operand("lhs", lhs, shift[0]), bag.operand("rhs", rhs, shift[1])
    out = bag.out("out", want.shape if want.ndim > 1 else (want.shape[0], 1), tdtype, shift[2])
    where = "sddmm_%s %s %s%s %s %s %s e=%d %s" % (fmt, op, lt, rt, lshape, rshape, tdtype, e, idt.__name__)
    fn(op, sp, gl, gr, out, _capi.TARGETS[lt], _capi.TARGETS[rt])
    bag.check(where)
    got = out.cpu().reshape(want.shape)
    if half:        # tests/test_gpu_api.py::test_half_through_api
        rtol, atol = HALF_API_TOL[tdtype]
        np.testing.assert_allclose(got.float().numpy(), want, rtol=rtol, atol=atol, err_msg=where)
    elif op == "dot":   # tests/test_gpu_seam.py::test_sddmm_dot_heads
        tol = 1e-5 if tdtype == torch.float32 else 1e-12
        np.testing.assert_allclose(got.numpy(), want, rtol=tol, atol=tol / 10 if tdtype == torch.float32 else tol, err_msg=where)
    else:               # one rounding per element: bit-exact (tests/test_gpu_seam.py, tests/test_gpu_fuzz.py)
        np.testing.assert_array_equal(got.numpy(), want, err_msg=where)


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("fmt", ["coo", "csr"])
@pytest.mark.parametrize("op,lt,rt", [("add", "u", "v"), ("mul", "e", "v"), ("div", "u", "e"), ("sub", "v", "u"),
                                      ("copy_lhs", "u", "v"), ("copy_rhs", "u", "e"), ("copy_lhs", "e", "v")])
def test_sddmm_elementwise(dev, fmt, op, lt, rt, tdtype, shift):
    widths = WIDE if _size(tdtype) >= 4 else NARROW
    for wi, f in enumerate(widths):
        k = wi * 7 + len(op) + SHIFTS.index(shift) * 5 + (fmt == "csr") * 3
        _sddmm_case(dev, fmt, op, lt, rt, (f,), (f,), tdtype, shift, k)
        if op in ("add", "mul", "div", "sub") and f > 1 and wi % 2:         # broadcast: (H, 1) against (H, D), (1,) against (F,)
            _sddmm_case(dev, fmt, op, lt, rt, (f, 1), (f, 3), tdtype, shift, k + 1)
            _sddmm_case(dev, fmt, op, lt, rt, (f,), (1,), tdtype, shift, k + 2)


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("fmt", ["coo", "csr"])
def test_sddmm_dot(dev, fmt, tdtype, shift):
    """u_dot_v on the vector path (D a whole number of 16-byte pieces), the scalar path and the general path, and
    e_dot_v / u_dot_e, with and without heads."""
    shapes = list(HEADS_DIM) + [(1, 64), (2, 100), (1, 65)]
    for si, hd in enumerate(shapes):
        k = si * 5 + SHIFTS.index(shift) * 7 + (fmt == "csr")
        _sddmm_case(dev, fmt, "dot", "u", "v", hd, hd, tdtype, shift, k)
        _sddmm_case(dev, fmt, "dot", "uev"[si % 3], "evu"[si % 3], (hd[0] * hd[1],), (hd[0] * hd[1],), tdtype, shift, k + 3)


# ---- edge softmax -------------------------------------------------------------------------------------------------
def _softmax_case(dev, g, dim, tdtype, use_ws, shift, flags=()):
    """Values: tests/test_gpu_seam.py::test_edge_softmax_geometries — forward and backward against the fp64 oracle of the
    same inputs, rtol 2e-5 / 1e-11 (backward x 10); the flag forms equal the flag-free kernels bit for bit, as tests/
    test_gpu_edge_order.py asserts."""
    from dgl_amd import _capi

    dt = NP_F[tdtype]
    rng = np.random.default_rng(dim * 13 + g["e"])
    e = g["e"]
    score = (rng.standard_normal((e, dim)) * 4).astype(dt)
    grad = rng.standard_normal((e, dim)).astype(dt)
    ref = oracle.edge_softmax_fwd(g["indptr"], g["eids"], score.astype(np.float64)).astype(dt)
    ref_b = oracle.edge_softmax_bwd(g["indptr"], g["eids"], ref.astype(np.float64), ref.astype(np.float64) * grad).astype(dt)
    tol = dict(rtol=2e-5, atol=1e-7) if tdtype == torch.float32 else dict(rtol=1e-11, atol=1e-14)
    btol = dict(rtol=tol["rtol"] * 10, atol=1e-6 if tdtype == torch.float32 else 1e-13)
    bag = Bag(dev, g["bag"])
    need = int(_capi.edge_softmax_workspace_bytes(g["csr"], tdtype, dim))
    fits = dim <= (8 if tdtype == torch.float64 else 16)             # the merge-path kernels' widest shape
    assert (need == 0 if not fits else need > 0 or e < 511), (need, dim, tdtype, e)
    ws = bag.workspace(need) if use_ws and need else None
    gs = bag.operand("score", score, shift[0])
    out = bag.out("out", (e, dim), tdtype, shift[2])
    where = "edge_softmax dim=%d %s ws=%s %s %s" % (dim, tdtype, ws is not None, g["tag"], flags)
    _capi.edge_softmax_forward(g["csr"], gs, out, ws)
    bag.check(where + " forward")
    np.testing.assert_allclose(_h(out), ref, err_msg=where, **tol)
    if ws is not None:
        first = out.clone()
        out.fill_(9.0)
        _capi.edge_softmax_forward(g["csr"], gs, out, ws, plan_valid=True)
        bag.check(where + " forward (plan_valid)")
        assert torch.equal(first, out), where
    gref, gsds = bag.operand("saved out", ref, shift[0]), bag.operand("sds", (ref * grad).astype(dt), shift[1])
    back = bag.out("back", (e, dim), tdtype, shift[2])
    _capi.edge_softmax_backward(g["csr"], gref, gsds, back, ws, plan_valid=ws is not None)
    bag.check(where + " backward")
    np.testing.assert_allclose(_h(back), ref_b, err_msg=where, **btol)
    if ws is None or not flags:
        return
    pos = torch.from_numpy(_edge_pos(g))
    if "sds_is_grad" in flags:
        ggrad = bag.operand("grad", grad, shift[1])
        prod = bag.operand("out * grad", torch.from_numpy(ref) * torch.from_numpy(grad), shift[1])
        want = bag.out("back (product given)", (e, dim), tdtype, shift[2])
        _capi.edge_softmax_backward(g["csr"], gref, prod, want, ws, plan_valid=True)
        back.fill_(9.0)
        _capi.edge_softmax_backward(g["csr"], gref, ggrad, back, ws, plan_valid=True, sds_is_grad=True)
        bag.check(where + " backward sds_is_grad")
        assert torch.equal(back, want), where
    if "out_position" in flags and g["eids"] is not None:
        outp = bag.out("out (position order)", (e, dim), tdtype, shift[2])
        _capi.edge_softmax_forward(g["csr"], gs, outp, ws, plan_valid=True, out_position=True)
        bag.check(where + " forward out_position")
        assert torch.equal(outp.cpu(), out.cpu()[pos]), where
        backp = bag.out("back (position order)", (e, dim), tdtype, shift[2])
        saved = bag.operand("saved out (position order)", ref[pos.numpy()], shift[0])
        for is_grad in (False, True):
            backp.fill_(9.0)
            sds = bag.operand("sds / grad", grad if is_grad else (ref * grad).astype(dt), shift[1])
            want = bag.out("back (edge-id order)", (e, dim), tdtype, shift[2])
            _capi.edge_softmax_backward(g["csr"], gref, sds, want, ws, plan_valid=True, sds_is_grad=is_grad)
            _capi.edge_softmax_backward(g["csr"], saved, sds, backp, ws, plan_valid=True, sds_is_grad=is_grad, out_position=True)
            bag.check(where + " backward out_position is_grad=%s" % is_grad)
            assert torch.equal(backp.cpu(), want.cpu()[pos]), where


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("case", ["merge_f32", "lane_group_f32", "merge_f64", "fp64_limit", "flags_f32", "flags_f64"])
def test_edge_softmax(dev, case, shift):
    si = SHIFTS.index(shift)
    if case == "merge_f32":
        for k, dim in enumerate((1, 3, 4, 8, 16)):
            for j in range(4):
                _softmax_case(dev, _csc(dev, *_variant(k * 9 + j * 5 + si)), dim, torch.float32, True, shift)
    elif case == "lane_group_f32":
        for k, dim in enumerate((3, 17, 70)):
            for j in range(4):
                _softmax_case(dev, _csc(dev, *_variant(k * 9 + j * 7 + si + 1)), dim, torch.float32, False, shift)
    elif case == "merge_f64":
        for k, dim in enumerate((1, 3, 4, 8)):
            for j in range(3):
                _softmax_case(dev, _csc(dev, *_variant(k * 5 + j * 11 + si + 2)), dim, torch.float64, True, shift)
    elif case == "fp64_limit":                     # 8: the widest merge-path shape of fp64; 9: the lane-group kernel
        for k, dim in enumerate((8, 9)):
            for j in range(4):
                for use_ws in (True, False):
                    _softmax_case(dev, _csc(dev, *_variant(k * 3 + j * 7 + si, BIG)), dim, torch.float64, use_ws, shift)
    else:
        tdtype = torch.float32 if case == "flags_f32" else torch.float64
        for k, dim in enumerate((1, 3, 8, 16) if tdtype == torch.float32 else (1, 3, 8)):
            for j in range(2):
                v = _variant(k * 4 + j * 2 + si, [b for b in VARIANTS if b[2]])           # (graphs with an edge-id map)
                _softmax_case(dev, _csc(dev, *v), dim, tdtype, True, shift, flags=("sds_is_grad", "out_position"))


# ---- segment reduce, scatter add ----------------------------------------------------------------------------------
def _segment_sum_bound(feat64, offsets, eps):
    """tests/test_segment.py::_assert_sum_close: (1e-5 (eps / 2^-24) + 2 n eps) * sum|x|, n the longest segment."""
    mag, _ = oracle.segment_reduce("sum", np.abs(feat64), offsets)
    longest = int(np.diff(offsets).max())
    return (1e-5 * (eps / 2.0 ** -24) + 2 * longest * eps) * mag + 1e-30


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("use_ws", [False, True], ids=["scratch_inside", "workspace"])
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("red", ["sum", "max", "min"])
def test_segment_reduce_and_its_backward(dev, red, tdtype, use_ws, shift):
    """Segments = the rows of the family's graphs (a hub of 300, the last segment empty or not)."""
    from dgl_amd import _capi

    dt = NP_F[tdtype]
    rng = np.random.default_rng(len(red) + shift[0] + use_ws)
    for wi, f, (e, last, _, idt) in _walk(WIDE, lambda wi: wi * 7 + len(red) + SHIFTS.index(shift) * 3 + use_ws):
        offsets = _csc(dev, e, last, False, idt)["indptr"]
        feat = rng.standard_normal((e, f)).astype(dt)
        want, warg = oracle.segment_reduce(red, feat, offsets)
        bag = Bag(dev)
        gfeat, goff = bag.operand("feat", feat, shift[0]), bag.index("offsets", offsets)
        out = bag.out("out", (N_DST, f), tdtype, shift[2])
        arg = bag.int_out("arg", (N_DST, f), T_I[idt]) if red != "sum" else None
        ws = bag.workspace(_capi.segment_reduce_workspace_bytes(red, gfeat, goff, out)) if use_ws else None
        where = "segment_reduce %s F=%d %s e=%d %s ws=%s" % (red, f, tdtype, e, idt.__name__, use_ws)
        _capi.segment_reduce(red, gfeat, goff, out, arg, ws)
        bag.check(where)
        if use_ws:
            first = out.clone()
            out.fill_(9.0)
            _capi.segment_reduce(red, gfeat, goff, out, arg, ws, plan_valid=True)
            bag.check(where + " (plan_valid)")
            assert torch.equal(first.view(torch.uint8), out.view(torch.uint8)), where
        if red == "sum":
            exact, _ = oracle.segment_reduce("sum", feat.astype(np.float64), offsets)
            err = np.abs(_h(out).astype(np.float64) - exact)
            bound = _segment_sum_bound(feat.astype(np.float64), offsets, 2.0 ** -24 if tdtype == torch.float32 else 2.0 ** -53)
            assert (err <= bound).all(), (where, float((err / bound).max()))
            continue
        np.testing.assert_array_equal(_h(out), want, err_msg=where)
        np.testing.assert_array_equal(_h(arg), warg, err_msg=where)
        # the backward: rows no winner names keep the sentinel
        dy = (np.arange(N_DST * f, dtype=np.float64).reshape(N_DST, f) / 7 + 1).astype(dt)
        gdy = bag.operand("dy", dy, shift[1])
        back = bag.out("back", (e, f), tdtype, shift[2])
        if e:
            _capi.backward_segment_cmp(gdy, arg, back)
        bag.check(where + " backward_segment_cmp")
        np.testing.assert_array_equal(_h(back), oracle.backward_segment_cmp(dy, warg, np.full((e, f), 9.0, dtype=dt)), err_msg=where)


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float16, torch.bfloat16], ids=str)
def test_segment_reduce_and_scatter_add_16bit(dev, tdtype, shift):
    """The band check is the new assertion; values as tests/test_segment.py::test_gpu_half_precision holds them (sum:
    rtol 1e-2, atol 5e-2 against the fp32 oracle of the widened values; max: arg exact, values exact where finite; scatter
    add of small integers: exact)."""
    from dgl_amd import _capi

    rng = np.random.default_rng(3 + shift[0])
    for wi, f in enumerate(NARROW):
        e, last, _, idt = _variant(wi * 7 + SHIFTS.index(shift) * 5 + (tdtype == torch.bfloat16))
        offsets = _csc(dev, e, last, False, idt)["indptr"]
        feat = torch.from_numpy(rng.standard_normal((e, f)).astype(np.float32)).to(tdtype)
        bag = Bag(dev)
        gfeat, goff = bag.operand("feat", feat, shift[0]), bag.index("offsets", offsets)
        out = bag.out("out", (N_DST, f), tdtype, shift[2])
        arg = bag.int_out("arg", (N_DST, f), T_I[idt])
        where = "segment_reduce F=%d %s e=%d %s" % (f, tdtype, e, idt.__name__)
        _capi.segment_reduce("sum", gfeat, goff, out)
        bag.check(where + " sum")
        want, _ = oracle.segment_reduce("sum", feat.float().numpy(), offsets)
        np.testing.assert_allclose(out.float().cpu().numpy(), want, rtol=1e-2, atol=5e-2, err_msg=where)
        ws = bag.workspace(_capi.segment_reduce_workspace_bytes("max", gfeat, goff, out))
        _capi.segment_reduce("max", gfeat, goff, out, arg, ws)
        bag.check(where + " max")
        want, warg = oracle.segment_reduce("max", feat.float().numpy(), offsets)
        np.testing.assert_array_equal(_h(arg), warg, err_msg=where)
        w = torch.from_numpy(want)
        assert bool((torch.isinf(w) | (out.float().cpu() == w)).all()), where
        # scatter add: -1 / 0 / 1 into the 37 targets on top of the sentinel; a target nobody names keeps it
        idx = _coo(e, last)[1].astype(idt)
        x = torch.from_numpy(rng.integers(-1, 2, (e, f)).astype(np.float32)).to(tdtype)
        gx, gidx = bag.operand("x", x, shift[1]), bag.index("idx", idx)
        acc = bag.out("acc", (N_DST, f), tdtype, shift[2])
        _capi.scatter_add(gx, gidx, acc)
        bag.check(where + " scatter_add")
        want = torch.full((N_DST, f), 9.0).index_add_(0, torch.from_numpy(idx.astype(np.int64)), x.float())
        assert torch.equal(acc.float().cpu(), want), where


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64], ids=str)
def test_scatter_add_atomic_path(dev, tdtype, shift):
    """Integer-valued rows into the 37 targets on top of the sentinel: exact whatever the order of the atomics (tests/
    test_segment.py: "exact-by-construction scatter sums"); a target nobody names keeps the sentinel."""
    from dgl_amd import _capi

    rng = np.random.default_rng(9 + shift[0])
    for wi, f, (e, last, _, idt) in _walk(WIDE, lambda wi: wi * 7 + SHIFTS.index(shift) * 3 + (tdtype == torch.float64)):
        idx = _coo(e, last)[1].astype(idt)
        x = rng.integers(-4, 5, (e, f)).astype(NP_F[tdtype])
        bag = Bag(dev)
        gx, gidx = bag.operand("feat", x, shift[0]), bag.index("idx", idx)
        out = bag.out("out", (N_DST, f), tdtype, shift[2])
        where = "scatter_add F=%d %s e=%d %s" % (f, tdtype, e, idt.__name__)
        _capi.scatter_add(gx, gidx, out)
        bag.check(where)
        want = oracle.scatter_add(x, idx, np.full((N_DST, f), 9.0, dtype=NP_F[tdtype]))
        np.testing.assert_array_equal(_h(out), want, err_msg=where)
        if not last or e == 0:
            assert bool((out[N_DST - 1] == 9.0).all()), where


@gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
def test_scatter_add_sorted_path(dev, idtype):
    """Just above 2^20 elements with dim = 3: the sorted merge-path route (tests/test_segment.py::
    test_gpu_scatter_add_sorted_path: exact for integers, what `out` held is kept, untouched targets stay)."""
    from dgl_amd import _capi

    dim, m = 3, 3001
    n = (1 << 20) // dim + 1
    assert (n - 1) * dim <= 1 << 20 < n * dim
    gen = torch.Generator().manual_seed(dim)
    idx = torch.randint(0, m - 1, (n,), generator=gen)                 # the last target is never named
    idx[idx == 7] = 8
    idx[: n // 4] = 11
    x = torch.randint(-4, 5, (n, dim), generator=gen).float()
    bag = Bag(dev)
    gx, gidx = bag.operand("feat", x), bag.index("idx", idx.to(idtype))
    out = bag.out("out", (m, dim), torch.float32)
    _capi.scatter_add(gx, gidx, out)
    bag.check("scatter_add sorted path %s" % idtype)
    want = torch.full((m, dim), 9.0, dtype=torch.float64).index_add_(0, idx, x.double())
    assert torch.equal(out.cpu().double(), want)
    assert bool((out[7] == 9.0).all()) and bool((out[m - 1] == 9.0).all())


# ---- segment_mm / gather_mm ---------------------------------------------------------------------------------------
MM_ACC_EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -24}
MM_SEGLEN = [130, 0, 77, 1]


def _mm_close(got, want, mag, dtype, k, what):
    """tests/test_mm.py::_close: |err| <= 4 sqrt(k) eps_acc sum|a||b| + one rounding of the stored result."""
    err = np.abs(got.double().cpu().numpy() - want)
    bound = 4 * np.sqrt(max(k, 1)) * MM_ACC_EPS[dtype] * mag + 1.01 * U16[dtype] * np.abs(want) + 1e-30
    if dtype == torch.float16:
        bound = bound + 2.0 ** -24
    assert (err <= bound).all(), (what, float((err / bound).max()))


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("k,n", [(64, 48), (33, 5)])
def test_segment_mm_and_its_weight_gradient(dev, k, n, tdtype, shift):
    from dgl_amd import _capi

    gen = torch.Generator().manual_seed(k * 100 + n + shift[0])
    m, r = sum(MM_SEGLEN), len(MM_SEGLEN)
    a = (torch.rand(m, k, generator=gen) - 0.3).to(tdtype)
    b = (torch.rand(r, k, n, generator=gen) - 0.6).to(tdtype)
    dc = (torch.rand(m, n, generator=gen) - 0.6).to(tdtype)
    a64, b64, c64 = a.double().numpy(), b.double().numpy(), dc.double().numpy()
    for seglen_dev, b_trans, indexed in (("cpu", False, False), ("gpu", False, False), ("gpu", True, False), ("cpu", False, True)):
        bag = Bag(dev)
        ga, gdc = bag.operand("a", a, shift[0]), bag.operand("dc", dc, shift[1])
        gb = bag.operand("b", b.transpose(1, 2).contiguous() if b_trans else b, shift[1])
        seglen = torch.tensor(MM_SEGLEN, dtype=torch.int64)
        sl = bag.index("seglen", seglen) if seglen_dev == "gpu" else seglen
        perm = torch.randperm(m, generator=gen)
        ri = bag.index("row_index", perm) if indexed else None
        c = bag.out("c", (m, n), tdtype, shift[2])
        where = "segment_mm K=%d N=%d %s seglen on %s b_trans=%s indexed=%s" % (k, n, tdtype, seglen_dev, b_trans, indexed)
        _capi.segment_mm(ga, gb, c, sl, b_trans=b_trans, row_index=ri)
        bag.check(where)
        db = bag.out("db", (r, k, n), tdtype, shift[2])
        _capi.segment_mm_backward_b(ga, gdc, db, sl, row_index=ri)
        bag.check(where + " backward_b")
        phys = perm.numpy() if indexed else np.arange(m)                 # logical row i lives at physical row phys[i]
        off = 0
        for i, rows in enumerate(MM_SEGLEN):
            at = phys[off:off + rows]
            _mm_close(c.cpu()[at], a64[at] @ b64[i], np.abs(a64[at]) @ np.abs(b64[i]), tdtype, k, where + " rel %d" % i)
            _mm_close(db[i], a64[at].T @ c64[at], np.abs(a64[at]).T @ np.abs(c64[at]), tdtype, rows, where + " dB rel %d" % i)
            off += rows


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("k,n", [(64, 48), (33, 5)])
def test_gather_mm(dev, k, n, idtype, shift):
    """c[idx_c[i]] = a[idx_a[i]] @ b[idx_b[i]]; rows of c that idx_c never names keep the sentinel.  Values: rtol = atol =
    1e-4, the bar of tests/test_mm.py::test_api_gather_mm_matches_bmm_with_grads."""
    from dgl_amd import _capi

    gen = torch.Generator().manual_seed(k + n + shift[0])
    rows, r, na, nc = sum(MM_SEGLEN), len(MM_SEGLEN), 211, 250
    a = torch.randn(na, k, generator=gen)
    b = torch.randn(r, k, n, generator=gen)
    for use_a, use_c in ((False, False), (True, True)):
        ia = torch.randint(0, na, (rows,), generator=gen) if use_a else None
        ib = torch.randint(0, r, (rows,), generator=gen)
        ic = torch.randperm(nc - 1, generator=gen)[:rows] if use_c else None      # injective; the last row of c is never named
        bag = Bag(dev)
        a_rows = a if use_a else torch.randn(rows, k, generator=gen)
        ga, gb = bag.operand("a", a_rows, shift[0]), bag.operand("b", b, shift[1])
        gia, gib, gic = (bag.index(nm, None if t is None else t.to(idtype)) for nm, t in (("idx_a", ia), ("idx_b", ib), ("idx_c", ic)))
        c = bag.out("c", (nc if use_c else rows, n), torch.float32, shift[2])
        where = "gather_mm K=%d N=%d %s idx_a=%s idx_c=%s" % (k, n, idtype, use_a, use_c)
        _capi.gather_mm(ga, gb, c, gia, gib, gic)
        bag.check(where)
        prod = torch.bmm((a_rows[ia] if use_a else a_rows).unsqueeze(1), b[ib]).squeeze(1)
        want = torch.full(tuple(c.shape), 9.0)
        want[ic if use_c else torch.arange(rows)] = prod
        assert torch.allclose(c.cpu(), want, rtol=1e-4, atol=1e-4), where
        if use_c:
            named = torch.zeros(nc, dtype=torch.bool)
            named[ic] = True
            assert bool((c.cpu()[~named] == 9.0).all()), where


# ---- fused GAT attention ------------------------------------------------------------------------------------------
SLOPE = 0.2
GAT_SEED = 0x1234_5678_9ABC_DEF


def _gat_widest(tdtype):
    """(1, D) with the largest D the operator takes: 64 lanes of one 16-byte piece each."""
    from dgl_amd import _capi

    v = 16 // _size(tdtype)
    assert _capi.gat_attention_supported(tdtype, 1, 64 * v) and not _capi.gat_attention_supported(tdtype, 1, 64 * v + v)
    return (1, 64 * v)


@functools.lru_cache(maxsize=None)
def _gat_graph(dev, e, last_nonempty, perm, idt):
    """The in-edge CSR over 37 nodes (source ids stay below 29: eight nodes without out-edges), and the out-edge CSR of the
    same edges with its edge-id map, all index arrays guarded."""
    from dgl_amd import _capi

    g = dict(_csc(dev, e, last_nonempty, perm, idt, square=True))
    indptr, indices, eids = coo_to_csr(g["src"], g["dst"], N_DST, idt)
    bag = Bag(dev, g["bag"])
    g["out_csr"] = _capi.make_csr(bag.index("out.indptr", indptr), bag.index("out.indices", indices), bag.index("out.eids", eids), N_DST)
    g["bag"] = bag
    return g


def _gat_eval(g, ft, el, er, dout, p, heads, dt):
    """The dense index_add evaluation of tests/test_zzzz_gpu_gat_attention_train.py::_exact on the CPU in `dt`, of the SAME
    operands (16-bit values widened exactly): out, (d_ft, d_el, d_er), the post-dropout weights (E, H, 1), the keep mask,
    and the softmax weights and scores the gradients' terms are made of."""
    from dgl_amd import _capi

    e = g["e"]
    src, dst = (torch.from_numpy(g[k].astype(np.int64)) for k in ("src", "dst"))
    keep = _capi.gat_dropout_mask_host(GAT_SEED, p, torch.arange(e), heads) if p else torch.ones(e, heads, dtype=torch.uint8)
    c = (keep.double().unsqueeze(-1) / (1.0 - float(np.float32(p)))).to(dt)
    ps = [t.to(dt).clone().requires_grad_(True) for t in (ft, el, er)]
    s = F.leaky_relu(ps[1][src] + ps[2][dst], SLOPE)
    mx = torch.full((N_DST, heads, 1), float("-inf"), dtype=dt).index_reduce_(0, dst, s.detach(), "amax")
    ex = torch.exp(s - mx[dst])
    a = ex / torch.zeros(N_DST, heads, 1, dtype=dt).index_add_(0, dst, ex)[dst]
    out = torch.zeros(N_DST, heads, ft.shape[2], dtype=dt).index_add_(0, dst, (a * c) * ps[0][src])
    grads = torch.autograd.grad((out * dout.to(dt)).sum(), ps)
    return out.detach(), tuple(x.detach() for x in grads), (a * c).detach(), keep, (a.detach(), c, s.detach(), src, dst)


def _gat_exact(g, ft, el, er, dout, p, heads):
    return _gat_eval(g, ft, el, er, dout, p, heads, torch.float64)


def _gat_abs_terms(parts, ft, dout, heads):
    """The sum of the ABSOLUTE values of the terms of every d_el / d_er element, in fp64: d_el[u] / d_er[v] = the sum over
    the out- / in-edges of a (c da - sum' a c da) slope', da = dout[v] . ft[u]."""
    a, c, s, src, dst = parts
    abs_da = (dout.double().abs()[dst] * ft.double().abs()[src]).sum(-1, keepdim=True)
    mean = torch.zeros(N_DST, heads, 1, dtype=torch.float64).index_add_(0, dst, a * c * abs_da)
    term = a * (c * abs_da + mean[dst]) * torch.where(s > 0, 1.0, SLOPE)
    zero = torch.zeros(N_DST, heads, 1, dtype=torch.float64)
    return zero.clone().index_add_(0, src, term), zero.clone().index_add_(0, dst, term)


def _gat_forward_bar(got, exact, tdtype, what, subnormal=False):
    """|got - exact| <= (u + 1e-5) |exact| on every element (tests/test_zzzz_gpu_gat_attention_train.py)."""
    bar = U16[tdtype] + 1e-5
    absolute = torch.finfo(tdtype).tiny * torch.finfo(tdtype).eps / 2 if subnormal else 0.0
    err = (got.double().cpu() - exact).abs()
    bad = err > bar * exact.abs() + absolute
    assert not bool(bad.any()), "%s: %d elements past the bar %.3g" % (what, int(bad.sum()), bar)


FP32_DER_FACTOR = 5


def _gat_gradient_bar(got, g, ft, el, er, dout, p, heads, tdtype, what):
    """The rule of tests/test_zzzz_gpu_gat_attention_train.py for each of d_ft, d_el, d_er: max |got - exact| / max |exact|
    <= u + 1e-5, exact the fp64 evaluation.  It stands as it is for d_ft, for d_el and for every 16-bit gradient.

    Two places where it cannot stand alone on this 37-node family, and what holds there instead:
      fp32 d_er   d_er of a softmax cancels (a row's terms a (da - mean da) sum to zero before the leaky-relu slope), and
                  the largest |d_er| of 37 rows is small next to the terms of the 300-edge hub.  A plain fp32 evaluation of
                  the same formula (_gat_eval in fp32: torch autograd on the CPU), over 20 operand draws on each of the
                  511- / 512- / 513-edge graphs, is itself up to 2.5e-5 (H = 1, D = 256) ... 5.05e-5 (H = 2, D = 25) off
                  fp64 by this measure, and below 1e-5 on other draws: the figure scatters from draw to draw, so a
                  comparison with that evaluation on the SAME operands decides nothing (measured: kernel 2.68e-5 where it
                  gave < 1e-5, 1.62e-5 where it gave 1.07e-5).  The bar for fp32 d_er is therefore FP32_DER_FACTOR = 5
                  times the rule's, 5e-5: the worst of the fp32 evaluation's own figures.  Nothing else is widened.
      max = 0     with one edge the softmax weight is 1 and d_el = d_er = 0 exactly (with no edge, every gradient is):
                  the measure does not exist.  There every element is held to (u + 1e-5) of the largest sum of absolute
                  terms of the tensor (_gat_abs_terms), which for no edges is zero: exact zeros."""
    bar = U16[tdtype] + 1e-5
    _, exact, _, _, parts = _gat_exact(g, ft, el, er, dout, p, heads)
    for k, (x, w, name) in enumerate(zip(got, exact, ("d_ft", "d_el", "d_er"))):
        assert bool(torch.isfinite(x.float()).all()), (what, name)
        err = float((x.double().cpu() - w).abs().max())
        scale = float(w.abs().max())
        if scale == 0.0:
            terms = 0.0 if name == "d_ft" else float(_gat_abs_terms(parts, ft, dout, heads)[k - 1].max())
            assert err <= bar * terms, "%s %s: exact gradient is zero, |got| up to %.3g, terms up to %.3g" % (what, name, err, terms)
            continue
        allowed = bar * FP32_DER_FACTOR if name == "d_er" and tdtype == torch.float32 else bar
        assert err / scale <= allowed, "%s %s: %.3g of max |grad| (bar %.3g, allowed %.3g)" % (what, name, err / scale, bar, allowed)


@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("train", [False, True], ids=["plain", "dropout"])
def test_gat_attention(dev, train, tdtype, shift):
    """forward, backward (plain and with dropout 0.6) and the attention-weight kernel, every tensor guarded: ft, el, er,
    dout, out, mz, d_ft, d_el, d_er, attn and the workspace at exactly gat_attention_workspace_bytes."""
    from dgl_amd import _capi

    p = 0.6 if train else 0.0
    gen = torch.Generator().manual_seed(11 + shift[0] + train)
    # (4, 25) of HEADS_DIM is outside the operator's set (an odd D takes one lane per element: H * 32 lanes > 64) and is
    # refused by name; (2, 25) is the widest odd-D shape of that kind it accepts
    assert [hd for hd in HEADS_DIM if not _capi.gat_attention_supported(tdtype, *hd)] == [(4, 25)]
    for si, (heads, d) in enumerate([hd for hd in HEADS_DIM if hd != (4, 25)] + [(2, 25), _gat_widest(tdtype)]):
        assert _capi.gat_attention_supported(tdtype, heads, d), (tdtype, heads, d)
        for j in range(2):
            g = _gat_graph(dev, *_variant(si * 7 + j * 13 + SHIFTS.index(shift) * 3 + train + (tdtype == torch.float16)))
            e = g["e"]
            ft = (torch.rand(N_DST, heads, d, generator=gen) + 1).to(tdtype)
            el, er = (torch.randn(N_DST, heads, 1, generator=gen).to(tdtype) for _ in range(2))
            dout = torch.randn(N_DST, heads, d, generator=gen).to(tdtype)
            bag = Bag(dev, g["bag"])
            gft, gel, ger = bag.operand("ft", ft, shift[0]), bag.operand("el", el, shift[1]), bag.operand("er", er, shift[1])
            gdout = bag.operand("dout", dout, shift[0])
            out = bag.out("out", (N_DST, heads, d), tdtype, shift[2])
            mz = bag.out("mz", (N_DST, heads, 2), torch.float32, shift[2])
            ws = bag.workspace(_capi.gat_attention_workspace_bytes(g["csr"], heads, d))
            grads = [bag.out(nm, t.shape, tdtype, shift[2]) for nm, t in (("d_ft", ft), ("d_el", el), ("d_er", er))]
            attn = bag.out("attn", (e, heads, 1), tdtype, shift[2])
            where = "gat_attention %s H=%d D=%d %s p=%.1f" % (tdtype, heads, d, g["tag"], p)
            if train:
                _capi.gat_attention_train_forward(g["csr"], gft, gel, ger, SLOPE, p, GAT_SEED, out, mz, ws)
                bag.check(where + " train_forward")
                _capi.gat_attention_train_backward(g["csr"], g["out_csr"], gft, gel, ger, mz, gdout, SLOPE, p, GAT_SEED, *grads, ws)
                bag.check(where + " train_backward")
            else:
                _capi.gat_attention_forward(g["csr"], gft, gel, ger, SLOPE, out, mz, ws)
                bag.check(where + " forward")
                _capi.gat_attention_backward(g["csr"], g["out_csr"], gft, gel, ger, out, mz, gdout, SLOPE, *grads, ws)
                bag.check(where + " backward")
            _capi.gat_attention_weights(g["csr"], gel, ger, mz, SLOPE, p, GAT_SEED, attn)
            bag.check(where + " weights")
            exact, _, w_exact, keep, _ = _gat_exact(g, ft, el, er, dout, p, heads)
            _gat_forward_bar(out, exact, tdtype, where + " out")
            _gat_gradient_bar(grads, g, ft, el, er, dout, p, heads, tdtype, where)
            _gat_forward_bar(attn, w_exact, tdtype, where + " attn", subnormal=True)
            assert bool((attn.cpu()[~keep.bool().unsqueeze(-1)] == 0).all()), where
            assert bool((out[torch.from_numpy(g["deg"] == 0).to(dev)] == 0).all()), where


# ---- row gather / scatter -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shift", SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64, torch.float16], ids=str)
def test_gather_rows_and_scatter_rows(dev, tdtype, shift):
    from dgl_amd import _capi

    gen = torch.Generator().manual_seed(5 + shift[0])
    for wi, f in enumerate(WIDE if _size(tdtype) >= 4 else NARROW):
        idt = (torch.int32, torch.int64)[wi % 2]
        n = (1, 511, 512, 513)[wi % 4]
        src = torch.randn(N_DST, f, generator=gen).to(tdtype)
        idx = torch.randint(0, N_DST, (n,), generator=gen)
        bag = Bag(dev)
        gsrc, gidx = bag.operand("src", src, shift[0]), bag.index("idx", idx.to(idt))
        out = bag.out("out", (n, f), tdtype, shift[2])
        where = "gather_rows F=%d %s n=%d %s" % (f, tdtype, n, idt)
        assert _capi.gather_rows(gsrc, gidx, out=out) is out
        bag.check(where)
        assert torch.equal(out.cpu().view(torch.uint8), src[idx].view(torch.uint8)), where
        # scatter: n rows to distinct targets among 600 (the last one never named); the others keep the sentinel
        rows = torch.randn(n, f, generator=gen).to(tdtype)
        to = torch.randperm(599, generator=gen)[:n]
        grows, gto = bag.operand("rows", rows, shift[1]), bag.index("to", to.to(idt))
        dest = bag.out("dest", (600, f), tdtype, shift[2])
        _capi.scatter_rows(grows, gto, dest)
        bag.check("scatter_rows" + where[11:])
        want = torch.full((600, f), 9.0, dtype=tdtype)
        want[to] = rows
        assert torch.equal(dest.cpu().view(torch.uint8), want.view(torch.uint8)), where


# ---- units whose outputs the wrapper allocates: the workspace is the caller's ---------------------------------------
def _bits(idtype):
    return 32 if idtype == torch.int32 else 64


def _ids(a, idtype, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(idtype)
    return t if dev is None else t.to(dev)


@gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64], ids=str)
def test_csr_mm_and_csr_sum_workspaces(dev, idtype, tdtype):
    """A 40 x 50 x 45 product with an empty last row, and the sum of two 40 x 50 operands.  There is no host twin of this
    unit: with the guarded workspace the results equal, bit for bit, those of the call that takes its own scratch (tests/
    test_zzzzz_gpu_csr_mm.py::test_determinism_stream_and_workspace), whose values are held to that file's bound."""
    from dgl_amd import _capi, _lib

    def rand_dense(m, n, draws, seed):
        """The recipe of tests/test_zzzzz_gpu_csr_mm.py: random (row, column) pairs, duplicates merged, one normal value
        of magnitude >= 2^-6 per entry, exactly representable in `tdtype`."""
        gen = torch.Generator().manual_seed(seed)
        key = torch.unique(torch.randint(0, m, (draws,), generator=gen) * n + torch.randint(0, n, (draws,), generator=gen))
        v = torch.randn(key.shape[0], generator=gen, dtype=torch.float64)
        v = torch.where(v < 0, -1.0, 1.0).double() * v.abs().clamp_min(2.0 ** -6)
        d = torch.zeros(m, n, dtype=torch.float64)
        d.view(-1)[key] = v.to(tdtype).double()
        return d

    da, db, dc = rand_dense(40, 50, 300, 1), rand_dense(50, 45, 300, 2), rand_dense(40, 50, 300, 3)
    da[-1] = 0
    bag = Bag(dev)

    def csr(d, name, seed):
        """The CSR of `d` from a shuffled COO, so that it carries an edge-id map; weights in edge-id order."""
        r, c = (x.numpy() for x in d.nonzero(as_tuple=True))
        o = np.random.default_rng(seed).permutation(r.shape[0])
        r, c = r[o], c[o]
        parts = coo_to_csr(r, c, d.shape[0], {torch.int32: np.int32, torch.int64: np.int64}[idtype])
        w = bag.operand(name + ".w", d[torch.from_numpy(r), torch.from_numpy(c)].to(tdtype))
        return _capi.make_csr(*(bag.index("%s.%s" % (name, n), t) for n, t in zip(("indptr", "indices", "eids"), parts)), d.shape[1]), w

    def check_values(got, exact, t, s, what):
        """The bound of tests/test_zzzzz_gpu_csr_mm.py for fp32 / fp64: |got - exact| <= 1.01 (t + 1) u S, t terms, S = sum |a||b|."""
        u = 2.0 ** -24 if tdtype == torch.float32 else 2.0 ** -53
        err = (got.double().cpu() - exact).abs()
        assert bool((err <= 1.01 * (t + 1) * u * s).all()), what

    (a, gwa), (b, gwb), (c, gwc) = csr(da, "a", 4), csr(db, "b", 5), csr(dc, "c", 6)
    ws = bag.workspace(_capi.csr_mm_workspace_bytes(a, b))
    want = _capi.csr_mm(a, gwa, b, gwb)
    got = _capi.csr_mm(a, gwa, b, gwb, workspace=ws)
    bag.check("csr_mm %s %s" % (idtype, tdtype))
    assert int(want[0][-1]) > 0 and all(torch.equal(x, y) for x, y in zip(got, want))
    exact, t, s = da @ db, (da != 0).double() @ (db != 0).double(), da.abs() @ db.abs()
    r, cc = (t > 0).nonzero(as_tuple=True)
    assert torch.equal(got[1].cpu().long(), cc)
    check_values(got[2], exact[r, cc], t[r, cc], s[r, cc], "csr_mm")
    arr = (ctypes.POINTER(_lib.CSR) * 2)(ctypes.pointer(a), ctypes.pointer(c))
    ws2 = bag.workspace(_lib.LIB.dgla_csr_sum_workspace_bytes(arr, 2), "csr_sum workspace")
    want = _capi.csr_sum([a, c], [gwa, gwc])
    got = _capi.csr_sum([a, c], [gwa, gwc], workspace=ws2)
    bag.check("csr_sum %s %s" % (idtype, tdtype))
    assert int(want[0][-1]) > 0 and all(torch.equal(x, y) for x, y in zip(got, want))
    tot = da + dc
    r, cc = ((da != 0) | (dc != 0)).nonzero(as_tuple=True)
    assert torch.equal(got[1].cpu().long(), cc) and torch.equal(got[2].cpu().double(), tot[r, cc].to(tdtype).double())


@gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("k", [8, 64, 1000])
def test_select_topk_workspace(dev, idtype, k):
    """One call from each size class of the kernel on the "ladder" graph of tests/topk_cases.py (rows of 0 .. 5000 entries),
    both directions: device == host twin."""
    from dgl_amd import _capi

    case = [c for c in tk.cases() if c["name"] == "ladder-permuted"][0]
    host = [None if case[n] is None else torch.from_numpy(case[n]).to(idtype) for n in ("indptr", "indices", "data")]
    bag = Bag(dev)
    h_csr = _capi.host_csr(*host, case["n"])
    d_csr = _capi.make_csr(*(bag.index(n, t) for n, t in zip(("indptr", "indices", "data"), host)), case["n"])
    seeds = torch.arange(case["n"], dtype=idtype)
    gseeds = bag.index("seeds", seeds)
    ws = bag.workspace(_capi.select_topk_workspace_bytes(idtype, len(seeds)))
    for name in ("dups/f4", "specials/f2", "extremes/i8"):
        wt = tk.torch_weight(*case["weights"][name])
        gw = bag.index("weight", wt) if not wt.dtype.is_floating_point else bag.operand("weight", wt)
        for ascending in (False, True):
            want = _capi.select_topk_host(h_csr, wt, seeds, k, ascending)
            got = _capi.select_topk(d_csr, gw, gseeds, k, ascending, workspace=ws)
            bag.check("select_topk k=%d %s %s ascending=%s" % (k, idtype, name, ascending))
            total = int(want[0][-1])
            assert total > 0 and torch.equal(got[0].cpu(), want[0])
            assert torch.equal(got[1][:total].cpu(), want[1]) and torch.equal(got[2][:total].cpu(), want[2])


@gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
def test_traverse_workspace(dev, idtype):
    """The smallest case of tests/traversal_cases.py with a non-empty result ("isolated": 10 nodes, 3 edges, a shuffled
    edge-id map), all three modes, both directions: device == host twin."""
    from dgl_amd import _capi

    case = [c for c in tc.cases() if c["name"] == "isolated"][0]
    dirs = tc.directions(case)
    bag = Bag(dev)
    pairs = {}
    for rev in (False, True):
        host = [None if dirs[rev][n] is None else _ids(dirs[rev][n], idtype) for n in ("indptr", "indices", "data")]
        there = [bag.index("%s.%s" % ("in" if rev else "out", n), t) for n, t in zip(("indptr", "indices", "data"), host)]
        pairs[rev] = (_capi.host_csr(*host, case["n"]), _capi.make_csr(*there, case["n"]))
    ws = bag.workspace(_capi.traverse_workspace_bytes(idtype, case["n"]))
    for rev in (False, True):
        (h_csr, d_csr), (h_opp, d_opp) = pairs[rev], pairs[not rev]
        calls = [(mode, None, None, torch.tensor(s, dtype=idtype)) for s in case["sources"] for mode in (tc.BFS_NODES, tc.BFS_EDGES)]
        calls.append((tc.TOPO_NODES, h_opp, d_opp, None))
        for mode, ho, do, src in calls:
            want = _capi.traverse_host(mode, h_csr, ho, src)
            got = _capi.traverse(mode, d_csr, do, bag.index("sources", src), workspace=ws)
            bag.check("traverse mode %d reverse=%s %s" % (mode, rev, idtype))
            assert got[1] == want[1] and torch.equal(got[0].cpu(), want[0])
    assert len(want[1]) > 0


@gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("eid_order", [True, False], ids=["eid_order", "row_order"])
def test_induced_subgraph_workspace(dev, idtype, eid_order):
    """The smallest graph of tests/subgraph_cases.py ("bipartite-mapped": 37 rows, 90 columns), its non-empty selections,
    the workspace at exactly the bytes reported for the result's size: device == host twin."""
    from dgl_amd import _capi, _lib

    g = [x for x in sc.graphs() if x["name"] == "bipartite-mapped"][0]
    host = [_ids(g[n], idtype) for n in ("indptr", "indices", "data")]
    h_csr = _capi.host_csr(*host, g["num_cols"])
    for name, rows, cols in sc.selections(g):
        want = _capi.induced_subgraph_host(h_csr, _ids(rows, idtype), _ids(cols, idtype), eid_order)
        total = int(want[0][-1])
        if want[4] != 0 or total == 0:
            continue
        bag = Bag(dev)
        d_csr = _capi.make_csr(*(bag.index(n, t) for n, t in zip(("indptr", "indices", "data"), host)), g["num_cols"])
        col_map = bag.index("col_map", torch.full((g["num_cols"],), -1, dtype=torch.int32))
        grows, gcols = bag.index("rows", _ids(rows, idtype)), bag.index("cols", _ids(cols, idtype))
        ws = bag.workspace(_lib.LIB.dgla_induced_subgraph_workspace_bytes(_bits(idtype), len(rows), total))
        got = _capi.induced_subgraph(d_csr, grows, col_map, eid_order, col_ids=gcols, workspace=ws)
        bag.check("induced_subgraph %s %s eid_order=%s" % (name, idtype, eid_order))
        for a, b in zip(got, want[:4]):
            assert torch.equal(a.cpu(), b), (name, eid_order)
        assert bool((col_map == -1).all()), name


@gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
def test_exclude_set_frontier_exclude_and_compact_nodes_workspaces(dev, idtype):
    """The smallest cases of tests/exclude_cases.py with a non-empty result, each workspace at exactly its reported
    size: device == host twins."""
    from dgl_amd import _capi, _lib

    L = _lib.LIB
    for name, ids, rev, num_edges, flagged in xc.set_cases():
        if flagged or not len(ids):
            continue
        h_ids, h_rev = _ids(ids, idtype), None if rev is None else _ids(rev, idtype)
        want, flags = _capi.exclude_set_host(h_ids, num_edges, h_rev)
        bag = Bag(dev)
        ws = bag.workspace(L.dgla_exclude_set_workspace_bytes(_bits(idtype), len(ids), 0 if rev is None else 1))
        got = _capi.exclude_set(bag.index("ids", h_ids), num_edges, bag.index("reverse", h_rev), workspace=ws)
        bag.check("exclude_set %s %s" % (name, idtype))
        assert flags == 0 and want.numel() > 0 and torch.equal(got.cpu(), want), name
    for short in (False, True):
        base = xc.BASES[idtype][-1]
        indptr, src, eids = (_ids(a, idtype) for a in xc.frontier(base, short))
        for name, x in xc.exclusion_lists(base):
            want = _capi.frontier_exclude_host(indptr, src, eids, _ids(x, idtype))
            bag = Bag(dev)
            ws = bag.workspace(L.dgla_frontier_exclude_workspace_bytes(_bits(idtype), indptr.shape[0] - 1, src.shape[0]))
            d = [bag.index(n, t) for n, t in (("indptr", indptr), ("src", src), ("eids", eids), ("x", _ids(x, idtype)))]
            got = _capi.frontier_exclude(*d, workspace=ws)
            bag.check("frontier_exclude %s short=%s %s" % (name, short, idtype))
            total = int(got[0][-1])
            for a, b in zip((got[0], got[1][:total], got[2][:total]), want):
                assert torch.equal(a.cpu(), b), (name, short)
    for name, preserve, ends, num_nodes in xc.compact_cases():
        if not len(preserve) + len(ends):
            continue
        want = _capi.compact_nodes_host(_ids(preserve, idtype), _ids(ends, idtype), num_nodes)
        bag = Bag(dev)
        node_map = bag.index("node_map", torch.full((num_nodes,), -1, dtype=torch.int32))
        ws = bag.workspace(L.dgla_compact_nodes_workspace_bytes(_bits(idtype), len(preserve), len(ends)))
        got = _capi.compact_nodes(bag.index("preserve", _ids(preserve, idtype)), bag.index("ends", _ids(ends, idtype)), node_map,
                                  workspace=ws)
        bag.check("compact_nodes %s %s" % (name, idtype))
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]) and want[2] == 0, name
        assert bool((node_map == -1).all()), name


@gpu
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
def test_neighbor_matching_workspace(dev, idtype):
    """The smallest cases of tests/matching_cases.py, plain and relabelled, every weight form, one round per read-back
    and the default batching: device == host twin (labels and rounds)."""
    from dgl_amd import _capi, _lib
    from tests import matching_cases as mc

    for case in sorted(mc.cases(), key=lambda c: c["n"])[:2]:
        host = [None if case[n] is None else _ids(case[n], idtype) for n in ("indptr", "indices", "data")]
        h_csr = _capi.host_csr(*host, case["n"])
        bag = Bag(dev)
        d_csr = _capi.make_csr(*(bag.index(n, t) for n, t in zip(("indptr", "indices", "data"), host)), case["n"])
        ws = bag.workspace(_lib.LIB.dgla_neighbor_matching_workspace_bytes(_bits(idtype), case["n"]))
        for form in mc.FORMS:
            w = mc.weights(case, form)
            wt = None if w is None else torch.from_numpy(w)
            want, rounds, relabelled = _capi.neighbor_matching_host(h_csr, wt, 1, relabel=True)
            gw = bag.operand("weight", wt)
            for batch in (1, 0):
                label, used = _capi.neighbor_matching(d_csr, gw, 1, batch_rounds=batch, workspace=ws)
                got, _ = _capi.neighbor_matching(d_csr, gw, 1, relabel=True, batch_rounds=batch, workspace=ws)
                bag.check("neighbor_matching %s %s %s batch=%d" % (case["name"], form, idtype, batch))
                assert used == rounds and torch.equal(label.cpu(), want) and torch.equal(got.cpu(), relabelled), (case["name"], form)


# ---- coverage: no entry point with an `out` or a `workspace` goes unguarded ------------------------------------------
COVERED = {
    "spmm_csr": "test_spmm_csr, test_spmm_csr_16bit",
    "spmm_csr_workspace_bytes": "test_spmm_csr (the size the workspace is guarded at)",
    "spmm_coo": "test_spmm_coo",
    "spmm_csr_stacked": "test_spmm_csr_stacked",
    "spmm_csr_stacked_workspace_bytes": "test_spmm_csr_stacked (the size the workspace is guarded at)",
    "spmm_cmp_backward": "test_spmm_cmp_backward",
    "spmm_cmp_mask": "test_spmm_cmp_mask_and_masked_spmm",
    "spmm_csr_masked": "test_spmm_cmp_mask_and_masked_spmm",
    "spmm_csr_masked_workspace_bytes": "test_spmm_cmp_mask_and_masked_spmm (the size the workspace is guarded at)",
    "sddmm_coo": "test_sddmm_elementwise, test_sddmm_dot",
    "sddmm_csr": "test_sddmm_elementwise, test_sddmm_dot",
    "edge_softmax_forward": "test_edge_softmax",
    "edge_softmax_backward": "test_edge_softmax",
    "segment_reduce": "test_segment_reduce_and_its_backward, test_segment_reduce_and_scatter_add_16bit",
    "segment_reduce_workspace_bytes": "test_segment_reduce_and_its_backward (the size the workspace is guarded at)",
    "backward_segment_cmp": "test_segment_reduce_and_its_backward",
    "scatter_add": "test_scatter_add_atomic_path, test_scatter_add_sorted_path, test_segment_reduce_and_scatter_add_16bit",
    "segment_mm": "test_segment_mm_and_its_weight_gradient",
    "segment_mm_backward_b": "test_segment_mm_and_its_weight_gradient",
    "gather_mm": "test_gather_mm",
    "gat_attention_forward": "test_gat_attention",
    "gat_attention_backward": "test_gat_attention",
    "gat_attention_train_forward": "test_gat_attention",
    "gat_attention_train_backward": "test_gat_attention",
    "gat_attention_weights": "test_gat_attention",
    "gather_rows": "test_gather_rows_and_scatter_rows",
    "scatter_rows": "test_gather_rows_and_scatter_rows",
    # the workspace is the caller's, the outputs are the wrapper's
    "csr_mm": "test_csr_mm_and_csr_sum_workspaces",
    "csr_sum": "test_csr_mm_and_csr_sum_workspaces",
    "select_topk": "test_select_topk_workspace",
    "traverse": "test_traverse_workspace",
    "induced_subgraph": "test_induced_subgraph_workspace",
    "exclude_set": "test_exclude_set_frontier_exclude_and_compact_nodes_workspaces",
    "frontier_exclude": "test_exclude_set_frontier_exclude_and_compact_nodes_workspaces",
    "compact_nodes": "test_exclude_set_frontier_exclude_and_compact_nodes_workspaces",
    "neighbor_matching": "test_neighbor_matching_workspace",
}
# name -> the reason; only entry points that need more than one GPU, and the stream_copy* benchmark tool
EXEMPT = {}


def _public_functions():
    from dgl_amd import _capi

    return {name: fn for name, fn in vars(_capi).items()
            if inspect.isfunction(fn) and fn.__module__ == _capi.__name__ and not name.startswith("_")}


def test_every_entry_point_with_an_out_or_a_workspace_is_listed():
    fns = _public_functions()
    must = {name for name, fn in fns.items() if {"out", "workspace"} & set(inspect.signature(fn).parameters)}
    assert must, "the inspection found nothing: the module's layout changed"
    both = set(COVERED) & set(EXEMPT)
    assert not both, "listed twice: %s" % sorted(both)
    missing = must - set(COVERED) - set(EXEMPT)
    assert not missing, "entry points with an `out` or `workspace` parameter that no guard test covers: %s" % sorted(missing)
    gone = (set(COVERED) | set(EXEMPT)) - set(fns)
    assert not gone, "COVERED / EXEMPT name functions that dgl_amd._capi does not have: %s" % sorted(gone)
    for name, reason in EXEMPT.items():
        assert name.startswith("stream_copy") or "GPU" in reason, "%s: only multi-GPU entry points and stream_copy* are exempt" % name
        assert isinstance(reason, str) and reason and "\n" not in reason


def test_every_covering_test_exists():
    here = globals()
    for name, tests in COVERED.items():
        for t in tests.split(" (")[0].split(", "):
            assert callable(here.get(t)) and t.startswith("test_"), (name, t)
