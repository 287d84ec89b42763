"""select_topk without a GPU: the host twin of the rule (dgla_select_topk_host, compiled from csrc/topk_step.h) equals the
independent Python model of tests/topk_cases.py on every case, weight type and direction; every refusal by its message;
the public function on CPU graphs: the reference's docstring example and its own tests restated."""
import ctypes

import numpy as np
import pytest
import torch

from tests import topk_cases as tc

CASES = tc.cases()
IDTYPES = [torch.int32, torch.int64]


def host_csr(case, idtype):
    from dgl_amd import _capi

    t = lambda a: None if a is None else torch.from_numpy(a).to(idtype)
    return _capi.host_csr(t(case["indptr"]), t(case["indices"]), t(case["data"]), case["n"])


def test_the_table_covers_what_it_should():
    degrees = set(d for c in CASES for d in c["degrees"])
    assert {0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 5000} <= degrees
    for k in (2, 7, 8, 64, 1000, 1024):
        assert {k - 1, k, k + 1} <= degrees, k
    assert 5000 % 16 and 5000 % 64
    for c in CASES:
        assert set(k for _, k in c["calls"]) >= set(tc.KS)
        assert any(len(set(s)) < len(s) for s, _ in c["calls"]) and any(len(s) == 0 for s, _ in c["calls"])
        assert set(dt for dt, _ in c["weights"].values()) == set(tc.DTYPES)
        kinds = set(name.split("/")[0] for name in c["weights"])
        assert kinds >= {"equal", "ascending", "descending", "dups", "specials", "extremes", "collide"}
        dt, w = c["weights"]["ascending/f4"]
        q = np.arange(c["nnz"]) if c["data"] is None else c["data"]
        for r in range(c["n"]):                                      # strictly ascending ALONG THE ROW
            lo, hi = c["indptr"][r], c["indptr"][r + 1]
            assert np.all(np.diff(w[q[lo:hi]]) > 0)
        dt, w = c["weights"]["specials/f4"]
        assert np.isnan(w).any() and np.isinf(w).any() and (w[w == 0].view(np.uint32) >> 31).any() and (w == 0).sum() > 1
        dt, w = c["weights"]["specials-negative-nan/f4"]
        assert (w.view(np.uint32) == 0xFFC00001).any()
        dt, w = c["weights"]["extremes/i8"]
        assert {2 ** 63 - 1, -(2 ** 63 - 1), 0, 1, -1} <= set(int(x) for x in w)
        dt, w = c["weights"]["collide/f2"]
        assert len(set(w.tolist())) < 64                             # 64 fp32 values collide in fp16
        dt, w = c["weights"]["collide/bf16"]
        assert len(set(w.tolist())) == 1
    permuted = [c for c in CASES if c["data"] is not None]
    assert permuted and len(permuted) < len(CASES)
    for c in permuted:          # position order != edge-id order inside a row of equal weights: a position tie-break shows
        lo, hi = c["indptr"][-2], c["indptr"][-1]
        assert np.any(np.diff(c["data"][lo:hi]) < 0)
    means = sorted(c["nnz"] / c["n"] for c in CASES)
    assert means[0] <= 32 < means[-1]                                # both sides of the 16-lane / 64-lane rule
    assert any(max(c["degrees"]) <= 32 for c in CASES) and any(32 < max(c["degrees"]) <= 128 for c in CASES)


@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_host_twin_equals_the_model(case, idtype):
    from dgl_amd import _capi

    csr = host_csr(case, idtype)
    for name, (dt, w) in case["weights"].items():
        if idtype == torch.int32 and name.split("/")[0] not in ("dups", "specials", "extremes"):
            continue                                                 # (the id width does not meet the weights: a sample)
        wt = tc.torch_weight(dt, w)
        for ascending in (False, True):
            model = tc.Model(case, dt, w, ascending)
            for seeds, k in case["calls"]:
                got = _capi.select_topk_host(csr, wt, torch.tensor(seeds, dtype=idtype), k, ascending)
                want = model.select(seeds, k)
                assert all(t.dtype == idtype for t in got)
                assert [t.tolist() for t in got] == list(want), (case["name"], name, ascending, k, seeds[:4])


def _tiny():
    from dgl_amd import _capi

    indptr, indices = torch.tensor([0, 2, 3]), torch.tensor([1, 0, 1])
    return _capi.host_csr(indptr, indices, None, 2), torch.tensor([1.0, 2.0, 3.0])


def test_host_refusals_by_message():
    from dgl_amd import DGLAMDError, _capi
    from dgl_amd._lib import LIB

    csr, w = _tiny()
    seeds = lambda *a: torch.tensor(a, dtype=torch.int64)
    with pytest.raises(DGLAMDError, match=r"select_topk_host: a seed lies outside \[0, 2\)"):
        _capi.select_topk_host(csr, w, seeds(0, 2), 1)
    with pytest.raises(DGLAMDError, match=r"select_topk_host: a seed lies outside \[0, 2\)"):
        _capi.select_topk_host(csr, w, seeds(-1), -1)
    with pytest.raises(DGLAMDError, match="unsupported weight dtype"):
        _capi.select_topk_host(csr, torch.tensor([1, 2, 3], dtype=torch.int16), seeds(0), 1)
    with pytest.raises(DGLAMDError, match="one value per edge"):
        _capi.select_topk_host(csr, w[:2].contiguous(), seeds(0), 1)
    with pytest.raises(DGLAMDError, match="seeds must be a contiguous 1-D tensor of the csr's id type"):
        _capi.select_topk_host(csr, w, torch.tensor([0], dtype=torch.int32), 1)
    out = torch.empty(2, dtype=torch.int64)
    raw = lambda c, wp, dt, k: LIB.dgla_select_topk_host(c, wp, dt, seeds(0).data_ptr(), 1, k, 0, out.data_ptr(), None, None)
    last = lambda: LIB.dgla_last_error().decode()
    assert raw(None, w.data_ptr(), 0, 1) == -1 and "select_topk_host: csr is null" in last()
    assert raw(ctypes.byref(csr), None, 0, 1) == -1 and "select_topk_host: weight is null" in last()
    assert raw(ctypes.byref(csr), w.data_ptr(), 6, 1) == -1 and "select_topk_host: unsupported weight dtype 6" in last()
    assert raw(ctypes.byref(csr), w.data_ptr(), 0, -2) == -1 and "k must be -1 (all), 0 or positive, got -2" in last()
    # a row that yields more picks than the limit is refused by name, with the number and the limit
    deg = _capi.select_topk_max_picks() + 1
    hub = _capi.host_csr(torch.tensor([0, deg, deg + 3]), torch.zeros(deg + 3, dtype=torch.int64), None, 2)
    wh = torch.arange(deg + 3, dtype=torch.float32)
    for k in (-1, deg):
        with pytest.raises(DGLAMDError, match="select_topk_host: a row yields 1025 picks, which exceeds the limit of 1024"):
            _capi.select_topk_host(hub, wh, seeds(1, 0), k)
    got = _capi.select_topk_host(hub, wh, seeds(1, 0), 1024)          # the same row within the limit
    assert got[0].tolist() == [0, 3, 1027] and got[2][:4].tolist() == [deg + 2, deg + 1, deg, deg - 1]
    assert _capi.select_topk_host(hub, wh, seeds(1), -1)[2].tolist() == [deg + 2, deg + 1, deg]
    assert _capi.select_topk_workspace_bytes(torch.int64, 0) == 0 and _capi.select_topk_workspace_bytes(torch.int64, 5) > 0


def test_a_malformed_indptr_reads_nothing_outside_the_arrays():
    from dgl_amd import _capi

    indptr, indices = torch.tensor([-5, 2, 1, 99]), torch.tensor([1, 0, 1])
    csr = _capi.host_csr(indptr, indices, None, 3)
    got = _capi.select_topk_host(csr, torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0, 1, 2]), -1)
    assert got[0].tolist() == [0, 2, 2, 4] and got[2].tolist() == [1, 0, 2, 1]
    bad_map = _capi.host_csr(torch.tensor([0, 3]), indices, torch.tensor([7, 1, -2]), 3)      # ids outside the weights
    got = _capi.select_topk_host(bad_map, torch.tensor([1.0, 2.0, 3.0]), torch.tensor([0]), -1)
    assert got[2].tolist() == [1, 7, -2]                           # unsigned order among the entries that read no weight


# ---- the public function on CPU graphs ----------------------------------------------------------------
def test_the_docstring_example_of_the_reference():
    import dgl_amd as dgl

    g = dgl.graph(([0, 0, 1, 1, 2, 2], [1, 2, 0, 1, 2, 0]))
    g.edata["weight"] = torch.FloatTensor([0, 1, 0, 1, 0, 1])
    sg = dgl.sampling.select_topk(g, 1, "weight")
    u, v = sg.edges(order="eid")
    assert (u.tolist(), v.tolist()) == ([2, 1, 0], [0, 1, 2])
    assert sg.edata[dgl.EID].tolist() == [5, 3, 1]
    assert g.select_topk(1, "weight").edata[dgl.EID].tolist() == [5, 3, 1]


def _topk_graphs(reverse):
    import dgl_amd as dgl

    follow = ([1, 2, 3, 0, 2, 3, 0], [0, 0, 0, 1, 1, 1, 2])
    play = ([0, 0, 1, 3], [0, 1, 2, 2])
    liked = ([2, 2, 2, 1, 1, 0], [0, 1, 2, 0, 3, 0])
    flips = ([0, 1, 2, 3], [0, 0, 0, 0])
    flip = (lambda p: (p[1], p[0])) if reverse else (lambda p: p)
    names = (lambda s, e, d: (d, e, s)) if reverse else (lambda s, e, d: (s, e, d))
    g = dgl.heterograph({("user", "follow", "user"): flip(follow)})
    g.edata["weight"] = torch.tensor([0.5, 0.3, 0.0, -5.0, 22.0, 0.0, 1.0])
    hg = dgl.heterograph({names("user", "follow", "user"): flip(follow), names("user", "play", "game"): flip(play),
                          names("game", "liked-by", "user"): flip(liked), names("user", "flips", "coin"): flip(flips)})
    hg.edges["follow"].data["weight"] = torch.tensor([0.5, 0.3, 0.0, -5.0, 22.0, 0.0, 1.0])
    hg.edges["play"].data["weight"] = torch.tensor([0.8, 0.5, 0.4, 0.5])
    hg.edges["liked-by"].data["weight"] = torch.tensor([0.3, 0.5, 0.2, 0.5, 0.1, 0.1])
    hg.edges["flips"].data["weight"] = torch.tensor([10.0, 2.0, 13.0, -1.0])
    return g, hg


def _pairs(u, v, reverse):
    return set(zip(v.tolist(), u.tolist())) if reverse else set(zip(u.tolist(), v.tolist()))


@pytest.mark.parametrize("reverse", [False, True], ids=["in", "out"])
def test_the_reference_tests_restated(reverse):
    """_test_sample_neighbors_topk / _test_sample_neighbors_topk_outedge of the reference's test_sampling.py; the out-edge
    form is the in-edge form on the reversed graphs, so the expected pairs are written once and flipped."""
    import dgl_amd as dgl

    g, hg = _topk_graphs(reverse)
    edge_dir = "out" if reverse else "in"
    for seeds, want, count in (([0, 1], {(2, 0), (1, 0), (2, 1), (3, 1)}, 4), ([0, 2], {(2, 0), (1, 0), (0, 2)}, 3)):
        subg = dgl.sampling.select_topk(g, -1, "weight", seeds, edge_dir=edge_dir)
        assert subg.num_nodes() == g.num_nodes()
        u_ans, v_ans = subg.out_edges(seeds) if reverse else subg.in_edges(seeds)
        assert _pairs(*subg.edges(), False) == _pairs(u_ans, v_ans, False)
        subg = dgl.sampling.select_topk(g, 2, "weight", seeds, edge_dir=edge_dir)
        assert subg.num_nodes() == g.num_nodes() and subg.num_edges() == count
        u, v = subg.edges()
        assert torch.equal(g.edge_ids(u, v), subg.edata[dgl.EID])
        assert _pairs(u, v, reverse) == want
    subg = dgl.sampling.select_topk(hg, 2, "weight", {"user": [0, 1], "game": 0}, edge_dir=edge_dir)
    assert len(subg.ntypes) == 3 and len(subg.etypes) == 4
    for etype, want in (("follow", {(2, 0), (1, 0), (2, 1), (3, 1)}), ("play", {(0, 0)}),
                        ("liked-by", {(2, 0), (2, 1), (1, 0)})):
        u, v = subg[etype].edges()
        assert torch.equal(hg[etype].edge_ids(u, v), subg[etype].edata[dgl.EID])
        assert _pairs(u, v, reverse) == want, etype
    assert subg["flips"].num_edges() == 0
    # different k for different relations
    subg = dgl.sampling.select_topk(hg, {"follow": 1, "play": 2, "liked-by": 0, "flips": -1}, "weight",
                                    {"user": [0, 1], "game": 0, "coin": 0}, edge_dir=edge_dir)
    assert len(subg.ntypes) == 3 and len(subg.etypes) == 4
    assert [subg[e].num_edges() for e in ("follow", "play", "liked-by", "flips")] == [2, 1, 0, 4]


def test_rank_order_features_and_errors_of_the_public_function():
    import dgl_amd as dgl
    from dgl_amd import DGLAMDError

    g, hg = _topk_graphs(False)
    g.ndata["x"] = torch.arange(4.0)
    g.edata["tag"] = torch.arange(70, 77)
    sg = dgl.sampling.select_topk(g, 2, "weight", [1, 0, 1])
    # in-edges of 1: ids 3, 4, 5 with weights -5, 22, 0; of 0: ids 0, 1, 2 with 0.5, 0.3, 0: by seed as given, then by rank
    assert sg.edata[dgl.EID].tolist() == [4, 5, 0, 1, 4, 5]
    u, v = sg.edges(order="eid")
    assert u.tolist() == [2, 3, 1, 2, 2, 3] and v.tolist() == [1, 1, 0, 0, 1, 1]
    assert sg.edata["tag"].tolist() == [74, 75, 70, 71, 74, 75] and torch.equal(sg.edata["weight"], g.edata["weight"][sg.edata[dgl.EID]])
    assert torch.equal(sg.ndata["x"], g.ndata["x"])
    asc = dgl.sampling.select_topk(g, 1, "weight", [1, 0], ascending=True, copy_ndata=False, copy_edata=False)
    assert asc.edata[dgl.EID].tolist() == [3, 2] and "x" not in asc.ndata and "tag" not in asc.edata
    assert dgl.sampling.select_topk(g, 0, "weight").num_edges() == 0
    ints = dgl.graph(([0, 1, 2], [0, 0, 0]))
    ints.edata["w"] = torch.tensor([5, -9, 5])
    assert dgl.sampling.select_topk(ints, 2, "w", [0]).edata[dgl.EID].tolist() == [0, 2]
    # (the first edge type without the feature is quoted; "follow" has it)
    with pytest.raises(DGLAMDError, match=r'Edge weights "nope" do not exist for relation graph "\(\'\w+\', \'(play|liked-by|flips)\', \'\w+\'\)"'):
        hg.edges["follow"].data["nope"] = torch.zeros(7)
        dgl.sampling.select_topk(hg, 1, "nope", {"user": [0]})
    with pytest.raises(DGLAMDError, match="K value must be specified for each edge type"):
        dgl.sampling.select_topk(hg, {"follow": 1}, "weight", {"user": [0]})
    with pytest.raises(DGLAMDError, match="Must specify node type"):
        dgl.sampling.select_topk(hg, 1, "weight", [0])
    g.edata["wide"] = torch.zeros(7, 2)
    with pytest.raises(DGLAMDError, match="must have one element per edge"):
        dgl.sampling.select_topk(g, 1, "wide")
    with pytest.raises(ValueError):
        dgl.sampling.select_topk(g, 1, "weight", edge_dir="both")
