"""Global uniform negative sampling (include/dgl_amd.h "Negative sampling", csrc/negative_sample_step.h) through the
HOST function — runs without a GPU.

dgla_negative_sample_host compiles the one definition of the rule that the kernels of csrc/negative_sampling.hip compile
for the device, so what is pinned here is pinned for the kernels too (tests/test_zzzzzzzzz_gpu_negative_sampling.py checks
device == host bit for bit).  The checker is an independent restatement of the rule written below from the text of the
header: draws with the numpy generator of tests/test_random_walk_host.py, the edge test by a Python set of (u, v) pairs
(no bisection), selection and duplicates by Python lists and sets.

Exact: host == model (pairs, count, padding) over six graphs, both id types, both flags both ways, T in {1, 3}, three
seeds and five (num_samples, n_slots); recorded pairs of one fixed case.  Properties; the law of the accepted pairs
(upper 1e-6 chi-square quantile); dgla_csr_has_edges_host == set membership; the C ABI's refusals; the closed-form
redundancy; the Python surface.
Reference: python/dgl/sampling/negative.py, src/array/cuda/negative_sampling.cu,
python/dgl/dataloading/negative_sampler.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_random_walk_host import SEEDS, chi2, csr_from_coo, draw, mulhi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(20, 20), (20, 69), (20, 7), (0, 0), (2000, 2000)]       # (num_samples, n_slots)
FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # (exclude_self_loops, replace)
GRAPHS = ["random20", "bipartite", "empty", "one_edge", "complete", "hub"]


# ---- the graphs ----------------------------------------------------------------------------------
def make_graph(name):
    """Out-edge CSR (as csr_from_coo) of a named graph."""
    rng = np.random.default_rng(3)
    if name == "random20":      # 300 edges on 20 nodes: duplicates are certain, self-loops added on top
        src, dst = rng.integers(0, 20, 292), rng.integers(0, 20, 292)
        loops = np.array([0, 3, 3, 7, 11, 12, 19, 19])
        return csr_from_coo(np.concatenate([src, loops]), np.concatenate([dst, loops]), 20, 20)
    if name == "bipartite":
        return csr_from_coo(rng.integers(0, 20, 250), rng.integers(0, 40, 250), 20, 40)
    if name == "empty":
        return csr_from_coo([], [], 1000, 1000)
    if name == "one_edge":
        return csr_from_coo([0], [1], 2, 2)
    if name == "complete":      # every pair, self-loops included: nothing is a negative
        u, v = np.divmod(np.arange(64), 8)
        return csr_from_coo(u, v, 8, 8)
    if name == "hub":           # one row of degree 5000 (the bisection runs 13 levels deep), the rest sparse
        src = np.concatenate([np.full(5000, 17), rng.integers(0, 6000, 3000)])
        dst = np.concatenate([rng.choice(6000, 5000, replace=False), rng.integers(0, 6000, 3000)])
        return csr_from_coo(src, dst, 6000, 6000)
    raise KeyError(name)


def edge_set(R):
    ip, ix = R["indptr"], R["indices"]
    return {(r, int(c)) for r in range(R["num_rows"]) for c in ix[ip[r]:ip[r + 1]]}


def member_of(R):
    m = np.array(R["indices"], dtype=np.int64)
    ip = R["indptr"]
    for r in range(R["num_rows"]):
        m[ip[r]:ip[r + 1]].sort()
    return m


# ---- the model of the rule -------------------------------------------------------------------------
def model_slots(R, edges, n_slots, T, excl, seed):
    """Rule 1: the pair of every slot, or None for an empty slot."""
    nr, nc = R["num_rows"], R["num_cols"]
    out = [None] * n_slots
    if nr == 0 or nc == 0 or n_slots == 0:
        return out
    i = np.arange(n_slots)
    for t in range(T):
        u = mulhi(draw(seed, i, t, 0), nr).astype(np.int64)
        v = mulhi(draw(seed, i, t, 1), nc).astype(np.int64)
        for k in range(n_slots):
            if out[k] is None:
                p = (int(u[k]), int(v[k]))
                if not (excl and p[0] == p[1]) and p not in edges:
                    out[k] = p
    return out


def model_select(slots, num_samples, replace):
    """Rules 2-4: (src, dst, count), padded with -1."""
    acc = [p for p in slots if p is not None]
    if not replace:
        seen, first = set(), []
        for p in acc:
            if p not in seen:
                seen.add(p)
                first.append(p)
        acc = first
    acc = acc[:num_samples]
    src = np.full(num_samples, -1, dtype=np.int64)
    dst = np.full(num_samples, -1, dtype=np.int64)
    if acc:
        src[:len(acc)], dst[:len(acc)] = np.array(acc).T
    return src, dst, len(acc)


# ---- the host function -----------------------------------------------------------------------------
def host_csr_of(R, idtype, member=None):
    from dgl_amd import _capi

    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(idtype)
    csr = _capi.host_csr(t_(R["indptr"]), t_(R["indices"]), None, R["num_cols"])
    return csr, t_(member_of(R) if member is None else member)


def host_neg(R, n_slots, num_samples, T, excl, replace, seed, idtype=torch.int64, lookup=None):
    from dgl_amd import _capi

    csr, member = lookup or host_csr_of(R, idtype)
    src, dst, count = _capi.negative_sample_host(csr, member, n_slots, num_samples, T, excl, replace, seed)
    assert src.dtype == idtype and dst.dtype == idtype and count.dtype == torch.int64
    assert src.shape == (num_samples,) and dst.shape == (num_samples,)
    return src.numpy().astype(np.int64), dst.numpy().astype(np.int64), int(count)


class Cases:
    """Graphs, their edge sets and the model's slots, each computed once and shared (never modified)."""

    def __init__(self):
        self.graphs, self.slots = {}, {}

    def graph(self, name):
        if name not in self.graphs:
            R = make_graph(name)
            self.graphs[name] = (R, edge_set(R))
        return self.graphs[name]

    def model(self, name, n_slots, T, excl, seed):
        key = (name, n_slots, T, excl, seed)
        if key not in self.slots:
            R, edges = self.graph(name)
            self.slots[key] = model_slots(R, edges, n_slots, T, excl, seed)
        return self.slots[key]


@pytest.fixture(scope="module")
def cases():
    return Cases()


# ---- exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", GRAPHS)
def test_host_equals_model(cases, name, idtype):
    R, edges = cases.graph(name)
    lookup = host_csr_of(R, idtype)
    counts = []
    for seed in SEEDS:
        for T in (1, 3):
            for excl, replace in FLAGS:
                for num_samples, n_slots in SHAPES:
                    ms, md, mc = model_select(cases.model(name, n_slots, T, excl, seed), num_samples, replace)
                    hs, hd, hc = host_neg(R, n_slots, num_samples, T, excl, replace, seed, idtype, lookup)
                    case = (seed, T, excl, replace, num_samples, n_slots)
                    assert hc == mc, case
                    assert np.array_equal(hs, ms) and np.array_equal(hd, md), case
                    assert (hs[hc:] == -1).all() and (hd[hc:] == -1).all() and (hs[:hc] >= 0).all()
                    counts.append(hc)
    if name == "complete":
        assert max(counts) == 0
    else:
        assert max(counts) > 0
    if name == "empty":           # every slot accepts unless it is an excluded self-loop (one chance in 1000)
        assert sorted(set(counts))[-1] >= 1990


# slot -> pair of (random20, seed 7, T = 3, exclude_self_loops), written down once from the model
RECORDED = ([(0, 7, 15), (2, 9, 16), (3, 11, 6), (66, 17, 7), (67, 14, 12), (68, 17, 7)], 61)


def test_recorded_pairs(cases):
    R, _ = cases.graph("random20")
    src, dst, count = host_neg(R, 69, 69, 3, True, True, 7)
    slots = cases.model("random20", 69, 3, True, 7)
    acc = [(i,) + p for i, p in enumerate(slots) if p is not None]
    assert [(u, v) for _, u, v in acc] == list(zip(src[:count].tolist(), dst[:count].tolist()))
    assert (acc[:3] + acc[-3:], count) == RECORDED


# ---- properties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random20", "bipartite", "hub", "one_edge"])
def test_properties(cases, name):
    R, edges = cases.graph(name)
    lookup = host_csr_of(R, torch.int64)
    for seed in SEEDS:
        for excl, replace in FLAGS:
            src, dst, count = host_neg(R, 3000, 3000, 3, excl, replace, seed, lookup=lookup)
            pairs = list(zip(src[:count].tolist(), dst[:count].tolist()))
            assert not edges & set(pairs)                                   # no returned pair is an edge
            assert all(0 <= u < R["num_rows"] and 0 <= v < R["num_cols"] for u, v in pairs)
            if excl:
                assert all(u != v for u, v in pairs)
            elif name == "one_edge":
                assert any(u == v for u, v in pairs)                         # (0, 0) and (1, 1) are negatives now
            if not replace:
                assert len(set(pairs)) == len(pairs)
            elif name != "hub":
                assert len(set(pairs)) < len(pairs)                         # 3000 draws from < 1000 cells repeat
            for k in (0, 1, 17, 500):                                        # the prefix property
                ps, pd, pc = host_neg(R, 3000, k, 3, excl, replace, seed, lookup=lookup)
                assert pc == min(k, count) and np.array_equal(ps[:pc], src[:pc]) and np.array_equal(pd[:pc], dst[:pc])
            if name == "one_edge" and excl:                                  # (0, 1) is the edge: only (1, 0) is left
                assert set(pairs) <= {(1, 0)}
                if not replace:
                    assert pairs in ([], [(1, 0)])


def test_two_nodes_return_nothing_or_the_one_pair(cases):
    R, _ = cases.graph("one_edge")
    seen = set()
    for seed in range(40):
        for n_slots in (1, 2, 5):
            src, dst, count = host_neg(R, n_slots, 5, 3, True, False, seed)
            got = list(zip(src[:count].tolist(), dst[:count].tolist()))
            assert got in ([], [(1, 0)])
            seen.add(count)
    assert seen == {0, 1}


# ---- the law -------------------------------------------------------------------------------------------
LAW_EDGES = [(0, 1), (0, 2), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (5, 0), (5, 3), (1, 4)]
CHI2_19_1E6 = 63.68      # upper 1e-6 quantile of the chi-square law at 19 degrees of freedom


@pytest.mark.parametrize("seed", SEEDS)
def test_accepted_pairs_are_uniform_over_the_negative_cells(seed):
    """R = C = 6, 10 edges, self-loops excluded: 36 - 10 - 6 = 20 negative cells.  A trial is rejected with probability
    16/36, so a slot stays empty with probability (4/9)^3 and the accepted share is 1 - (4/9)^3 = 0.912."""
    R = csr_from_coo(*zip(*LAW_EDGES), 6, 6)
    slots = 40000
    src, dst, count = host_neg(R, slots, slots, 3, True, True, seed)
    cells = [(u, v) for u in range(6) for v in range(6) if u != v and (u, v) not in LAW_EDGES]
    assert len(cells) == 20
    got = np.bincount(src[:count] * 6 + dst[:count], minlength=36)
    counts = np.array([got[u * 6 + v] for u, v in cells])
    assert counts.sum() == count                                          # nothing outside the negative cells
    share = 1 - (4 / 9) ** 3
    x = chi2(counts, np.full(20, count / 20))
    print("seed", seed, "accepted", count, "of", slots, "expected share %.4f" % share, "chi2(19) = %.2f" % x)
    assert abs(count - slots * share) < 6 * np.sqrt(slots * share * (1 - share))     # six binomial standard deviations
    assert x < CHI2_19_1E6


# ---- the edge lookup -------------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", GRAPHS)
def test_has_edges_host_is_set_membership(cases, name, idtype):
    from dgl_amd import _capi

    R, edges = cases.graph(name)
    csr, member = host_csr_of(R, idtype)
    nr, nc = R["num_rows"], R["num_cols"]
    rng = np.random.default_rng(1)
    u = np.concatenate([rng.integers(0, nr, 3000), [-1, nr, 0, 0, nr - 1, 2 ** 31 - 1, -2 ** 31, 0]])
    v = np.concatenate([rng.integers(0, nc, 3000), [0, 0, -1, nc, nc, 0, 0, 2 ** 31 - 1]])
    if edges:                                  # real edges too: a random pair of the hub graph is hardly ever one
        eu, ev = np.array(sorted(edges)[::max(1, len(edges) // 500)]).T
        u, v = np.concatenate([u, eu]), np.concatenate([v, ev])
    got = _capi.csr_has_edges_host(csr, member, torch.as_tensor(u).to(idtype), torch.as_tensor(v).to(idtype))
    assert got.dtype == torch.bool
    want = [(int(a), int(b)) in edges for a, b in zip(u, v)]
    assert got.tolist() == want
    assert any(want) == bool(edges)


# ---- C ABI -------------------------------------------------------------------------------------------------
NEW = ["dgla_negative_sample_workspace_bytes", "dgla_negative_sample", "dgla_negative_sample_host", "dgla_csr_has_edges",
       "dgla_csr_has_edges_host"]


def test_header_declares_and_library_exports_the_entry_points():
    from dgl_amd import _lib

    with open(os.path.join(ROOT, "include", "dgl_amd.h")) as fh:
        hdr = fh.read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(_lib.LIB, name), name
    # the header quotes the rule of csrc/negative_sample_step.h in full
    with open(os.path.join(ROOT, "dgl_amd", "csrc", "negative_sample_step.h")) as fh:
        step = fh.read()
    squeeze = lambda s: " ".join(re.sub(r"^\s*(//|\*)", "", line).strip() for line in s.splitlines())
    rule = step[step.index("// Setting."):step.index("#pragma once")]
    assert len(rule.splitlines()) > 25 and squeeze(rule) in squeeze(hdr)
    assert '#include "node2vec_step.h"' in step
    for name in ("rw_mix64", "rw_walk_key", "rw_step_key", "rw_draw", "rw_index", "n2v_member"):
        assert re.search(r"\b%s\s*\(" % name, step), name                  # used ...
        assert not re.search(r"\b%s\s*\([^)]*\)\s*\{" % name, step), name + " is defined again instead of included"   # ... not restated
    with open(os.path.join(ROOT, "dgl_amd", "csrc", "Makefile")) as fh:
        mk = fh.read()
    assert "negative_sampling.hip" in mk and "negative_sample_step.h" in mk


def test_bad_arguments_fail_with_a_message():
    from dgl_amd import _capi, _lib

    L, ref = _lib.LIB, ctypes.byref
    err = lambda: L.dgla_last_error().decode()
    full = _capi.host_csr(torch.tensor([0, 1, 2]), torch.tensor([1, 0]), None, 2)
    member = full._keep[1].data_ptr()
    out = torch.zeros(8, dtype=torch.int64)
    cnt = torch.zeros(1, dtype=torch.int64)
    o, c = out.data_ptr(), cnt.data_ptr()
    host, dev = L.dgla_negative_sample_host, L.dgla_negative_sample
    assert host(None, member, 4, 4, 3, 1, 0, 0, o, o, c) == -1 and "csr is null" in err()
    assert host(ref(full), None, 4, 4, 3, 1, 0, 0, o, o, c) == -1 and "member is null" in err()
    assert host(ref(full), member, 4, 4, 3, 1, 0, 0, None, o, c) == -1 and "out_src / out_dst are null" in err()
    assert host(ref(full), member, 4, 4, 3, 1, 0, 0, o, o, None) == -1 and "out_count is null" in err()
    for T in (0, -1, 65):
        assert host(ref(full), member, 4, 4, T, 1, 0, 0, o, o, c) == -1 and "num_trials must be in 1 .. 64" in err()
    assert host(ref(full), member, 4, 4, 64, 1, 0, 0, o, o, c) == 0
    assert host(ref(full), member, -1, 4, 3, 1, 0, 0, o, o, c) == -1 and "negative" in err()
    assert host(ref(full), member, 2 ** 31, 4, 3, 1, 0, 0, o, o, c) == -1 and "below 2^31" in err()
    # the device entry refuses before it touches the GPU: the same checks, then the workspace
    assert dev(None, member, 4, 4, 3, 1, 0, 0, o, o, c, None, 0, None) == -1 and "csr is null" in err()
    assert dev(ref(full), member, 4, 4, 0, 1, 0, 0, o, o, c, None, 0, None) == -1 and "num_trials" in err()
    assert dev(ref(full), member, 2 ** 31, 4, 3, 1, 0, 0, o, o, c, None, 0, None) == -1 and "below 2^31" in err()
    need = L.dgla_negative_sample_workspace_bytes(64, 4)
    assert need > 0 and L.dgla_negative_sample_workspace_bytes(64, 0) == 0
    assert L.dgla_negative_sample_workspace_bytes(64, 2 ** 31) == 0 and L.dgla_negative_sample_workspace_bytes(16, 4) == 0
    assert dev(ref(full), member, 4, 4, 3, 1, 0, 0, o, o, c, None, 0, None) == -1 and "workspace of %d bytes" % need in err()
    assert dev(ref(full), member, 4, 4, 3, 1, 0, 0, o, o, c, o, need - 1, None) == -1 and "workspace" in err()
    # the workspace follows the number of slots and nothing else: under 100 bytes per slot
    big = L.dgla_negative_sample_workspace_bytes(64, 1 << 20)
    assert big < 100 * (1 << 20) and L.dgla_negative_sample_workspace_bytes(32, 1 << 20) < big
    # the lookup
    u = torch.zeros(2, dtype=torch.int64)
    ob = torch.zeros(2, dtype=torch.uint8)
    assert L.dgla_csr_has_edges_host(None, member, u.data_ptr(), u.data_ptr(), 2, ob.data_ptr()) == -1 and "csr is null" in err()
    assert L.dgla_csr_has_edges_host(ref(full), None, u.data_ptr(), u.data_ptr(), 2, ob.data_ptr()) == -1 and "member" in err()
    assert L.dgla_csr_has_edges_host(ref(full), member, None, u.data_ptr(), 2, ob.data_ptr()) == -1 and "u / v / out" in err()
    assert L.dgla_csr_has_edges(ref(full), member, u.data_ptr(), u.data_ptr(), 2, None, None) == -1 and "u / v / out" in err()
    assert L.dgla_csr_has_edges(ref(full), member, u.data_ptr(), u.data_ptr(), -2, ob.data_ptr(), None) == -1
    with pytest.raises(_lib.DGLAMDError, match="member"):
        _capi.negative_sample_host(full, full._keep[1].int(), 4, 4)
    with pytest.raises(_lib.DGLAMDError, match="id type"):
        _capi.csr_has_edges_host(full, full._keep[1], u.int(), u.int())


# ---- Python surface ------------------------------------------------------------------------------------------
def test_redundancy_in_closed_form():
    """The reference solves a N^2 + b N + c = 0 with numpy's polynomial roots and takes the last one."""
    from numpy.polynomial import polynomial

    from dgl_amd.sampling import _negative_redundancy

    for k, e, pairs in ((10, 3, 16), (1000, 61859140, 2449029 ** 2), (1000000, 123718280, 2449029 ** 2), (50, 380, 400),
                        (7, 0, 1000000), (1, 1, 2)):
        p_m = e / pairs
        p_k = 1 - p_m
        n = polynomial.Polynomial([k ** 2, -p_k * (2 * k + 9 * p_m), p_k ** 2]).roots()[-1]
        want = (n.real if np.iscomplexobj(n) else n) / k - 1.0
        got = _negative_redundancy(k, e, pairs)
        assert got >= 0 or abs(got) < 1e-12
        assert abs(got - want) <= 1e-12 * (1.0 + abs(want)), (k, e, pairs, got, want)    # 1e-12 relative in N / k


def test_surface_without_a_gpu():
    import dgl_amd
    from dgl_amd import negative_sampler, sampling

    assert dgl_amd.global_uniform_negative_sampling is sampling.global_uniform_negative_sampling
    assert dgl_amd.DGLGraph.global_uniform_negative_sampling is sampling.global_uniform_negative_sampling
    assert negative_sampler.Uniform is negative_sampler.PerSourceUniform
    g = dgl_amd.graph(([0, 1, 2], [1, 2, 3]))
    hg = dgl_amd.heterograph({("user", "follow", "user"): ([0, 1], [1, 2]), ("user", "view", "item"): ([0, 1, 2], [0, 1, 1])})
    with pytest.raises(dgl_amd.DGLError, match="no CPU fallback"):
        sampling.global_uniform_negative_sampling(g, 3)
    with pytest.raises(dgl_amd.DGLError, match="no CPU fallback"):
        g.global_uniform_negative_sampling(3, etype=("_N", "_E", "_N"), redundancy=2.0, seed=1)
    with pytest.raises(dgl_amd.DGLError, match="does not exist"):
        sampling.global_uniform_negative_sampling(hg, 3, etype="likes")
    with pytest.raises(dgl_amd.DGLError, match="must not be negative"):
        sampling.global_uniform_negative_sampling(g, -1)
    with pytest.raises(dgl_amd.DGLError, match="no CPU fallback"):
        negative_sampler.GlobalUniform(2)(g, torch.tensor([0, 1]))
    # PerSourceUniform is plain torch: k pairs per edge, the edge's source repeated, dtype and device of the ids
    for ids in (torch.tensor([0, 2, 1]), torch.tensor([2, 2], dtype=torch.int32), torch.zeros(0, dtype=torch.int64)):
        src, dst = negative_sampler.PerSourceUniform(4)(g, ids)
        assert src.shape == dst.shape == (4 * len(ids),) and src.dtype == dst.dtype == ids.dtype
        assert src.tolist() == np.repeat(ids.numpy(), 4).tolist()          # edge i of this graph starts at node i
        assert ((dst >= 0) & (dst < 4)).all()
    out = negative_sampler.Uniform(2)(hg, {"view": torch.tensor([0, 2]), ("user", "follow", "user"): torch.tensor([1])})
    assert set(out) == {("user", "view", "item"), ("user", "follow", "user")}
    src, dst = out[("user", "view", "item")]
    assert src.tolist() == [0, 0, 2, 2] and ((dst >= 0) & (dst < 2)).all() and dst.shape == (4,)
    assert out[("user", "follow", "user")][0].tolist() == [1, 1]
    with pytest.raises(dgl_amd.DGLError, match="dict of etypes"):
        negative_sampler.Uniform(2)(hg, torch.tensor([0]))
    # has_edges_between on a CPU graph keeps its lines
    assert g.has_edges_between([0, 1, 3], [1, 0, 3]).tolist() == [True, False, False]
