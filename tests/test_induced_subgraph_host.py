"""Induced subgraphs without a GPU: the host twin of csrc/subgraph.hip (dgla_induced_subgraph_host) against a numpy
model of the rule on every case of tests/subgraph_cases.py, its flags, and the Python surface on CPU graphs:
khop_in_subgraph / khop_out_subgraph against the answers the reference documents (python/dgl/subgraph.py), out_subgraph,
the DGLGraph aliases, and the ShaDow / SAINT samplers."""
import numpy as np
import pytest
import torch

from tests import subgraph_cases as sc

GRAPHS = sc.graphs()
same_graph = sc.same_graph


def model(g, rows, cols, eid_order):
    """The rule as a plain loop over the entries: ``(out_indptr, row, col, eid)``."""
    cmap = -np.ones(g["num_cols"], dtype=np.int64)
    for i, c in enumerate(cols):
        cmap[c] = i
    indptr, indices, data = g["indptr"], g["indices"], g["data"]
    out_indptr, trip = [0], []
    for i, r in enumerate(rows):
        if 0 <= r < g["num_rows"]:
            for j in range(indptr[r], indptr[r + 1]):
                u = indices[j]
                if 0 <= u < g["num_cols"] and cmap[u] >= 0:
                    trip.append((i, cmap[u], j if data is None else data[j]))
        out_indptr.append(len(trip))
    if eid_order:
        trip.sort(key=lambda t: t[2])
    t = np.array(trip, dtype=np.int64).reshape(-1, 3)
    return np.array(out_indptr, dtype=np.int64), t[:, 0], t[:, 1], t[:, 2]


def host_csr(g, idtype):
    from dgl_amd import _capi

    t = lambda a: None if a is None else torch.from_numpy(a).to(idtype)
    return _capi.host_csr(t(g["indptr"]), t(g["indices"]), t(g["data"]), g["num_cols"])


@pytest.mark.parametrize("g", GRAPHS, ids=lambda g: g["name"])
def test_host_equals_numpy_model(g):
    from dgl_amd import _capi

    kept = 0
    for idtype in (torch.int32, torch.int64):
        csr = host_csr(g, idtype)
        for name, rows, cols in sc.selections(g):
            for eid_order in (True, False):
                want = model(g, rows, cols, eid_order)
                got = _capi.induced_subgraph_host(csr, torch.from_numpy(rows).to(idtype), torch.from_numpy(cols).to(idtype),
                                                  eid_order)
                assert got[4] == 0, (g["name"], name)
                for a, b in zip(got[:4], want):
                    assert a.dtype == idtype and np.array_equal(a.numpy(), b), (g["name"], name, eid_order)
                kept += len(want[1])
    assert kept > 0


def test_all_nodes_in_order_is_the_whole_graph():
    from dgl_amd import _capi

    g = GRAPHS[1]       # with an edge-id map
    n = g["num_rows"]
    every = torch.arange(n)
    indptr, row, col, eid, flags = _capi.induced_subgraph_host(host_csr(g, torch.int64), every, every, eid_order=False)
    assert flags == 0 and np.array_equal(indptr.numpy(), g["indptr"]) and np.array_equal(col.numpy(), g["indices"])
    assert np.array_equal(eid.numpy(), g["data"])
    assert np.array_equal(row.numpy(), np.repeat(np.arange(n), np.diff(g["indptr"])))
    indptr, row, col, eid, flags = _capi.induced_subgraph_host(host_csr(g, torch.int64), every, every, eid_order=True)
    assert np.array_equal(eid.numpy(), np.arange(g["indices"].size))


def test_flags():
    from dgl_amd import _capi

    g = GRAPHS[0]
    n = g["num_rows"]
    csr = host_csr(g, torch.int64)
    t = lambda a: torch.tensor(a, dtype=torch.int64)
    assert _capi.induced_subgraph_host(csr, t([3, 5]), t([3, 5]))[4] == 0
    assert _capi.induced_subgraph_host(csr, t([3, 5, 3]), t([3, 5, 3]))[4] == _capi.SUBGRAPH_DUPLICATE
    for bad in (-1, n):     # nothing is read through such an id: the call returns, with the flag and without its rows
        indptr, row, col, eid, flags = _capi.induced_subgraph_host(csr, t([9, bad, 4]), t([9, bad, 4]), eid_order=False)
        assert flags == _capi.SUBGRAPH_OUT_OF_RANGE
        assert indptr[1] == indptr[2] and set(row.tolist()) <= {0, 2} and set(col.tolist()) <= {0, 2}
    assert _capi.induced_subgraph_host(csr, t([n, 1, 1]), t([n, 1, 1]))[4] == 3
    # a bad row id alone is reported too
    assert _capi.induced_subgraph_host(csr, t([n + 7]), t([2]))[4] == _capi.SUBGRAPH_OUT_OF_RANGE


def test_refusals():
    from dgl_amd import _capi, _lib

    csr = host_csr(GRAPHS[0], torch.int64)
    with pytest.raises(_lib.DGLAMDError, match="id type"):
        _capi.induced_subgraph_host(csr, torch.tensor([1], dtype=torch.int32), torch.tensor([1], dtype=torch.int32))
    assert _lib.LIB.dgla_induced_subgraph_workspace_bytes(16, 4, 4) == 0
    assert _lib.LIB.dgla_induced_subgraph_workspace_bytes(32, -1, 4) == 0
    small = _lib.LIB.dgla_induced_subgraph_workspace_bytes(32, 100, 0)
    assert 0 < small < _lib.LIB.dgla_induced_subgraph_workspace_bytes(32, 100, 1000) \
        < _lib.LIB.dgla_induced_subgraph_workspace_bytes(64, 100, 5000)
    # every device entry point refuses bad arguments before any launch, so this needs no GPU
    assert _lib.LIB.dgla_node_map_mark(16, None, 0, None, 0, None, None) == -1
    assert "int32 or int64" in _lib.LIB.dgla_last_error().decode()
    assert _lib.LIB.dgla_node_map_mark(32, None, 1, None, 4, None, None) == -1
    assert _lib.LIB.dgla_node_map_clear(32, None, 2 ** 31, None, 4, None) == -1
    assert "2^31" in _lib.LIB.dgla_last_error().decode()
    assert _lib.LIB.dgla_induced_subgraph_count(None, None, 0, None, None, None, 0, None) == -1
    assert "csr is null" in _lib.LIB.dgla_last_error().decode()
    assert _lib.LIB.dgla_induced_subgraph_fill(None, None, 0, None, None, 0, None, None, None, 1, None, 0, None) == -1


# ---- the Python surface on CPU graphs ---------------------------------------------------------------
def triples(sg, etype=None):
    u, v = sg.edges(etype=etype)
    frame = sg._edge_frames[sg.get_etype_id(etype)]
    return sorted(zip(frame["_ID"].tolist(), u.tolist(), v.tolist()))


def test_khop_in_subgraph_documented_answer():
    import dgl_amd as dgl

    g = dgl.graph(([1, 1, 2, 3, 4], [0, 2, 0, 4, 2]))
    g.edata["w"] = torch.arange(10).view(5, 2)
    sg, inverse = dgl.khop_in_subgraph(g, 0, k=2)
    assert sg.num_nodes() == 4 and sg.ndata["_ID"].tolist() == [0, 1, 2, 4]
    assert triples(sg) == [(0, 1, 0), (1, 1, 2), (2, 2, 0), (4, 3, 2)]
    assert sg.edata["w"].tolist() == [[0, 1], [2, 3], [4, 5], [8, 9]]
    assert inverse.tolist() == [0]
    assert dgl.khop_in_subgraph(g, 0, k=2, relabel_nodes=False).num_nodes() == 5      # (no inverse without relabelling)


def test_khop_out_subgraph_documented_answer():
    import dgl_amd as dgl

    g = dgl.graph(([0, 2, 0, 4, 2], [1, 1, 2, 3, 4]))
    sg, inverse = dgl.khop_out_subgraph(g, 0, k=2)
    assert sg.num_nodes() == 4
    assert triples(sg) == [(0, 0, 1), (1, 2, 1), (2, 0, 2), (4, 2, 3)]
    assert inverse.tolist() == [0]


def test_khop_documented_heterograph_answers():
    """The `out` example documents 2 `plays` edges; its own node set (users 0, 1, 3 and games 0, 2) spans three of the
    example's `plays` edges, (0, 0), (1, 0) and (1, 2), and node_subgraph of the reference keeps every edge between kept
    nodes.  The docstring's count is a slip; the test asserts 3 and cross-checks node_subgraph on that node set."""
    import dgl_amd as dgl

    g = dgl.heterograph({("user", "plays", "game"): ([0, 1, 1, 2], [0, 0, 2, 1]),
                         ("user", "follows", "user"): ([0, 1, 1], [1, 2, 2])})
    sg, inverse = dgl.khop_in_subgraph(g, {"game": 0}, k=2)
    assert (sg.num_nodes("game"), sg.num_nodes("user")) == (1, 2)
    assert (sg.num_edges("plays"), sg.num_edges("follows")) == (2, 1)
    assert list(inverse) == ["game"] and inverse["game"].tolist() == [0]

    g = dgl.heterograph({("user", "plays", "game"): ([0, 1, 1, 2], [0, 0, 2, 1]),
                         ("user", "follows", "user"): ([0, 1], [1, 3])})
    sg, inverse = dgl.khop_out_subgraph(g, {"user": 0}, k=2)
    assert (sg.num_nodes("game"), sg.num_nodes("user")) == (2, 3)
    assert sg._node_frames[sg.get_ntype_id("user")]["_ID"].tolist() == [0, 1, 3]
    assert sg._node_frames[sg.get_ntype_id("game")]["_ID"].tolist() == [0, 2]
    assert (sg.num_edges("plays"), sg.num_edges("follows")) == (3, 2)
    want = dgl.node_subgraph(g, {"user": [0, 1, 3], "game": [0, 2]})
    assert triples(sg, "plays") == triples(want, "plays") and triples(sg, "follows") == triples(want, "follows")
    assert inverse["user"].tolist() == [0]


def test_khop_in_on_the_reverse_graph_is_khop_out():
    import dgl_amd as dgl

    torch.manual_seed(5)
    u, v = torch.randint(0, 60, (240,)), torch.randint(0, 60, (240,))
    g, r = dgl.graph((u, v), num_nodes=60), dgl.graph((v, u), num_nodes=60)
    for k in (0, 1, 2, 3):
        a, ia = dgl.khop_out_subgraph(g, [7, 3], k)
        b, ib = dgl.khop_in_subgraph(r, [7, 3], k)
        assert torch.equal(a.ndata["_ID"], b.ndata["_ID"]) and torch.equal(ia, ib)
        assert torch.equal(a.edata["_ID"], b.edata["_ID"])
        assert torch.equal(a.edges()[0], b.edges()[1]) and torch.equal(a.edges()[1], b.edges()[0])
    with pytest.raises(dgl.DGLError, match="out of range"):
        dgl.khop_in_subgraph(g, [60], 1)


def test_blocks_are_refused():
    import dgl_amd as dgl

    blk = dgl.create_block(([0, 1], [0, 0]), num_src_nodes=2, num_dst_nodes=1)
    with pytest.raises(dgl.DGLError, match="block"):
        dgl.khop_in_subgraph(blk, 0, 1)


def test_out_subgraph_against_a_direct_construction():
    import dgl_amd as dgl

    u, v = torch.tensor([0, 1, 1, 2, 3, 3, 4]), torch.tensor([1, 2, 0, 2, 0, 4, 4])
    g = dgl.graph((u, v))
    g.edata["w"] = torch.arange(7.0)
    sg = dgl.out_subgraph(g, [1, 3])
    keep = torch.tensor([1, 2, 4, 5])
    assert sg.num_nodes() == 5 and torch.equal(sg.edata["_ID"], keep)
    assert torch.equal(sg.edges()[0], u[keep]) and torch.equal(sg.edges()[1], v[keep])
    assert torch.equal(sg.edata["w"], g.edata["w"][keep])
    rl = dgl.out_subgraph(g, [1, 3], relabel_nodes=True)
    nid = rl.ndata["_ID"]
    assert nid.tolist() == [0, 1, 2, 3, 4][:5] and torch.equal(nid[rl.edges()[0]], u[keep])
    # the mirror image of in_subgraph
    rev = dgl.in_subgraph(dgl.graph((v, u)), [1, 3])
    assert torch.equal(rev.edata["_ID"], sg.edata["_ID"]) and torch.equal(rev.edges()[1], sg.edges()[0])


def test_graph_aliases():
    import dgl_amd as dgl

    g = dgl.graph(([0, 1, 2, 3], [1, 2, 3, 0]))
    same = lambda a, b: triples(a) == triples(b) and a.num_nodes() == b.num_nodes()
    assert same(g.subgraph([0, 1, 2]), dgl.node_subgraph(g, [0, 1, 2]))
    assert same(g.edge_subgraph([0, 2]), dgl.edge_subgraph(g, [0, 2]))
    assert same(g.in_subgraph([1]), dgl.in_subgraph(g, [1]))
    assert same(g.out_subgraph([1]), dgl.out_subgraph(g, [1]))
    assert same(g.khop_in_subgraph(1, 2)[0], dgl.khop_in_subgraph(g, 1, 2)[0])
    assert same(g.khop_out_subgraph(1, 2)[0], dgl.khop_out_subgraph(g, 1, 2)[0])


def test_shadow_sampler_on_a_cpu_graph():
    import dgl_amd as dgl

    torch.manual_seed(1)
    g = dgl.rand_graph(80, 400)
    g.ndata["x"] = torch.rand(80, 3)
    g.edata["w"] = torch.rand(400)
    seeds = torch.tensor([11, 5, 42])
    input_nodes, output_nodes, subg = dgl.ShaDowKHopSampler([-1, -1]).sample(g, seeds)
    assert torch.equal(output_nodes, seeds) and torch.equal(input_nodes[:3], seeds)          # seeds first
    assert torch.equal(subg.ndata["_ID"], input_nodes)
    same_graph(subg, dgl.node_subgraph(g, subg.ndata["_ID"]))
    khop, _ = dgl.khop_in_subgraph(g, seeds, 2)
    assert torch.equal(torch.sort(input_nodes)[0], khop.ndata["_ID"])
    with pytest.raises(dgl.DGLError, match="exclude_eids"):
        dgl.ShaDowKHopSampler([-1]).sample(g, seeds, exclude_eids=torch.tensor([0]))
    with pytest.raises(dgl.DGLError, match="prefetch_node_feats"):
        dgl.ShaDowKHopSampler([-1], prefetch_node_feats=["x"])
    with pytest.raises(dgl.DGLError, match="prefetch_edge_feats"):
        dgl.ShaDowKHopSampler([-1], prefetch_edge_feats=["w"])
    with pytest.raises(dgl.DGLError, match="GPU"):
        dgl.ShaDowKHopSampler([3]).sample(g, seeds)


def test_shadow_sampler_on_a_cpu_heterograph():
    import dgl_amd as dgl

    g = dgl.heterograph({("user", "plays", "game"): ([0, 1, 1, 2], [0, 0, 2, 1]),
                         ("user", "follows", "user"): ([0, 1, 1], [1, 2, 2])})
    inp, out, subg = dgl.ShaDowKHopSampler([-1, {"plays": -1, "follows": -1}]).sample(g, {"game": [0]})
    assert out["game"].tolist() == [0] and inp["game"].tolist() == [0] and sorted(inp["user"].tolist()) == [0, 1]
    same_graph(subg, dgl.node_subgraph(g, inp))


def test_saint_sampler_on_a_cpu_graph():
    import dgl_amd as dgl

    torch.manual_seed(2)
    g = dgl.rand_graph(200, 1500)
    g.ndata["x"] = torch.rand(200, 2)
    for mode in ("node", "edge"):
        sampler = dgl.SAINTSampler(mode, 20)
        for _ in range(2):      # (the second call uses the cached probabilities)
            subg = sampler.sample(g, None)
            nid = subg.ndata["_ID"]
            assert nid.dtype == g.idtype and torch.equal(nid, torch.unique(nid))         # distinct, ascending
            assert 0 < nid.shape[0] <= (20 if mode == "node" else 40)
            same_graph(subg, dgl.node_subgraph(g, nid))
    with pytest.raises(dgl.DGLError, match="'node', 'edge' or 'walk', got cluster"):
        dgl.SAINTSampler("cluster", 20)
    hg = dgl.heterograph({("a", "r", "b"): ([0], [0])})
    with pytest.raises(dgl.DGLError, match="homogeneous"):
        dgl.SAINTSampler("node", 2).sample(hg, None)
