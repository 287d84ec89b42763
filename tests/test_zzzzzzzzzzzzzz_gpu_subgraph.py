"""Induced subgraphs on the device (csrc/subgraph.hip): device == host twin bit for bit on every case of
tests/subgraph_cases.py (both orders, both id widths, both lane-group widths, with and without a caller's workspace), the
node map left all -1 whatever happens, the refusals, and the Python surface on GPU graphs: _induced_rows against the torch
node_subgraph, khop_in_subgraph / khop_out_subgraph against the CPU copy of the graph, the ShaDow and SAINT samplers."""
import numpy as np
import pytest
import torch

from tests import subgraph_cases as sc

pytestmark = pytest.mark.gpu

GRAPHS = sc.graphs()
same_graph = sc.same_graph
_HOST = {}


def host(g, idtype):
    """The host twin's results on every selection of ``g``, both orders: computed once per (graph, id type)."""
    from dgl_amd import _capi

    key = (g["name"], idtype)
    if key not in _HOST:
        t = lambda a: None if a is None else torch.from_numpy(a).to(idtype)
        csr = _capi.host_csr(t(g["indptr"]), t(g["indices"]), t(g["data"]), g["num_cols"])
        out = {}
        for name, rows, cols in sc.selections(g):
            for eid_order in (True, False):
                got = _capi.induced_subgraph_host(csr, t(rows), t(cols), eid_order)
                assert got[4] == 0
                out[name, eid_order] = [a.numpy() for a in got[:4]]
        _HOST[key] = out
    return _HOST[key]


def device_csr(g, idtype, dev):
    from dgl_amd import _capi

    t = lambda a: None if a is None else torch.from_numpy(a).to(idtype).to(dev)
    return _capi.make_csr(t(g["indptr"]), t(g["indices"]), t(g["data"]), g["num_cols"])


@pytest.mark.parametrize("g", GRAPHS, ids=lambda g: g["name"])
def test_device_equals_host_bit_for_bit(dev, g):
    from dgl_amd import _capi, _lib

    col_map = torch.full((g["num_cols"],), -1, dtype=torch.int32, device=dev)
    for idtype in (torch.int32, torch.int64):
        csr = device_csr(g, idtype, dev)
        want = host(g, idtype)
        bits = 32 if idtype == torch.int32 else 64
        for name, rows, cols in sc.selections(g):
            r, c = (torch.from_numpy(a).to(idtype).to(dev) for a in (rows, cols))
            # a caller's workspace sized for the largest result the selection can have
            ws = torch.empty(_lib.LIB.dgla_induced_subgraph_workspace_bytes(bits, len(rows), g["indices"].size),
                             dtype=torch.uint8, device=dev)
            for eid_order in (True, False):
                for workspace in (None, ws):
                    got = _capi.induced_subgraph(csr, r, col_map, eid_order, col_ids=c, workspace=workspace)
                    for a, b in zip(got, want[name, eid_order]):
                        assert a.dtype == idtype and np.array_equal(a.cpu().numpy(), b), (g["name"], name, eid_order)
                    assert bool((col_map == -1).all()), (g["name"], name)


def test_bad_ids_are_refused_and_the_map_stays_clean(dev):
    """Duplicate and out-of-range ids raise; the count kernel skips a row id outside the graph and mark / clear skip a
    node id outside the map (csrc/subgraph_step.h subgraph_row, node_map_kernel), so nothing is read through them."""
    from dgl_amd import _capi, _lib

    g = GRAPHS[0]
    n = g["num_rows"]
    csr = device_csr(g, torch.int64, dev)
    col_map = torch.full((n,), -1, dtype=torch.int32, device=dev)
    t = lambda a: torch.tensor(a, dtype=torch.int64, device=dev)
    for ids, message in (([3, 5, 3], "duplicate node id"), ([9, n, 4], "node id out of range"),
                         ([9, -1, 4], "node id out of range")):
        with pytest.raises(_lib.DGLAMDError, match=message):
            _capi.induced_subgraph(csr, t(ids), col_map, col_ids=t(ids))
        assert bool((col_map == -1).all())
    # a workspace that is too small is refused by name, and the map is cleared all the same
    with pytest.raises(_lib.DGLAMDError, match="workspace"):
        _capi.induced_subgraph(csr, t([9, 4]), col_map, col_ids=t([9, 4]), workspace=torch.empty(8, dtype=torch.uint8, device=dev))
    assert bool((col_map == -1).all())
    with pytest.raises(_lib.DGLAMDError, match="id type"):
        _capi.induced_subgraph(csr, t([1]).int(), col_map, col_ids=t([1]).int())
    assert bool((col_map == -1).all())
    # mark and clear on their own
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.node_map_mark(t([7, 2, 11]), col_map, flags)
    assert col_map[[7, 2, 11]].tolist() == [0, 1, 2] and int(flags) == 0 and int((col_map >= 0).sum()) == 3
    _capi.node_map_clear(t([7, 2, 11]), col_map)
    assert bool((col_map == -1).all())


def graph_of(g, idtype, dev, seed):
    """The square case ``g`` as a graph (its CSR read as in-edges), with node and edge features."""
    import dgl_amd as dgl

    dst = np.repeat(np.arange(g["num_rows"]), np.diff(g["indptr"]))
    order = np.random.default_rng(seed).permutation(dst.size)          # edge ids in no particular order
    out = dgl.graph((torch.from_numpy(g["indices"][order]), torch.from_numpy(dst[order])), num_nodes=g["num_rows"],
                    idtype=idtype, device=torch.device(dev))
    gen = torch.Generator().manual_seed(seed)
    out.ndata["x"] = torch.rand(g["num_rows"], 3, generator=gen).to(dev)
    out.edata["w"] = torch.rand(dst.size, generator=gen).to(dev)
    return out


def hetero_graph(dev):
    import dgl_amd as dgl

    gen = torch.Generator().manual_seed(9)
    users, games = 300, 70
    e = lambda n_src, n_dst, m: (torch.randint(0, n_src, (m,), generator=gen), torch.randint(0, n_dst, (m,), generator=gen))
    plays = e(users, games, 1500)
    plays[1][:700] = 3                                                  # game 3 is a hub of 700 in-edges
    g = dgl.heterograph({("user", "plays", "game"): plays, ("user", "follows", "user"): e(users, users, 2000),
                         ("game", "played-by", "user"): e(games, users, 900)}, {"user": users, "game": games}, device=torch.device(dev))
    g._node_frames[g.get_ntype_id("user")]["x"] = torch.rand(users, 2, generator=gen).to(dev)
    g._edge_frames[g.get_etype_id("follows")]["w"] = torch.rand(2000, generator=gen).to(dev)
    return g


@pytest.mark.parametrize("relabel", [True, False])
def test_induced_rows_equals_torch_node_subgraph(dev, relabel):
    import dgl_amd as dgl
    from dgl_amd import transforms

    for case, idtype in ((GRAPHS[0], torch.int64), (GRAPHS[2], torch.int32)):       # short (hub of 5 000) and long rows
        g = graph_of(case, idtype, dev, 4)
        for name, sel, _ in sc.selections(case):
            if name in ("all-reversed", "tenth", "hub", "hub-neighbours", "first-17", "empty"):
                ids = torch.from_numpy(sel).to(dev)
                got = transforms._induced_rows(g, {"_N": ids}, relabel, True)
                same_graph(got, dgl.node_subgraph(g, ids, relabel_nodes=relabel))
                assert bool((g._sampling_node_map == -1).all())
    g = hetero_graph(dev)
    gen = torch.Generator().manual_seed(1)
    for k_user, k_game in ((40, 10), (300, 70), (25, 0)):
        ids = {"user": torch.randperm(300, generator=gen)[:k_user].to(dev), "game": torch.randperm(70, generator=gen)[:k_game].to(dev)}
        if k_game:
            ids["game"][0] = 3 if 3 not in ids["game"].tolist() else ids["game"][0]      # the hub is selected
        got = transforms._induced_rows(g, ids, relabel, True)
        same_graph(got, dgl.node_subgraph(g, ids, relabel_nodes=relabel))
        assert got.num_edges() > 0
    with pytest.raises(dgl.DGLError, match="duplicate node id"):
        transforms._induced_rows(g, {"user": torch.tensor([1, 2, 1], device=dev), "game": torch.tensor([0], device=dev)})
    assert all(bool((m == -1).all()) for m in g._sampling_node_maps.values())


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_khop_subgraphs_equal_the_cpu_graph(dev, k):
    import dgl_amd as dgl

    g = graph_of(GRAPHS[0], torch.int64, "cpu", 6)
    h = hetero_graph("cpu")
    for cpu, seeds in ((g, [33, 150, 4]), (h, {"game": [5, 3]}), (h, {"user": [17], "game": [60]})):
        gpu = cpu.to(dev)
        for fn in (dgl.khop_in_subgraph, dgl.khop_out_subgraph):
            want, want_inv = fn(cpu, seeds, k)
            got, got_inv = fn(gpu, seeds, k)
            assert got.device.type == "cuda"
            same_graph(got.to("cpu"), want)
            if isinstance(seeds, dict):
                assert {n: t.tolist() for n, t in got_inv.items()} == {n: t.tolist() for n, t in want_inv.items()}
            else:
                assert got_inv.tolist() == want_inv.tolist()
        same_graph(dgl.khop_in_subgraph(gpu, seeds, k, relabel_nodes=False).to("cpu"),
                   dgl.khop_in_subgraph(cpu, seeds, k, relabel_nodes=False))


def test_shadow_sampler(dev):
    import dgl_amd as dgl

    g = graph_of(GRAPHS[0], torch.int64, dev, 8)
    seeds = torch.tensor([33, 150, 4, 9], device=dev)
    reach = set(dgl.khop_in_subgraph(g, seeds, 2)[0].ndata["_ID"].tolist())
    runs = []
    for seed in (1, 1, 2):
        input_nodes, output_nodes, subg = dgl.ShaDowKHopSampler([3, 3], seed=seed).sample(g, seeds)
        assert torch.equal(output_nodes, seeds) and torch.equal(input_nodes[:4], seeds)      # seeds first
        assert torch.equal(subg.ndata["_ID"], input_nodes)
        same_graph(subg, dgl.node_subgraph(g, input_nodes))
        assert set(input_nodes.tolist()) <= reach
        runs.append(input_nodes.tolist())
    assert runs[0] == runs[1] and runs[0] != runs[2]
    input_nodes, _, subg = dgl.ShaDowKHopSampler([-1, -1]).sample(g, seeds)
    assert set(input_nodes.tolist()) == reach and len(input_nodes) == len(reach)
    # several relations, fanouts per edge type
    h = hetero_graph(dev)
    inp, out, subg = dgl.ShaDowKHopSampler([{"plays": 2, "follows": 3, "played-by": 1}, 2], seed=5).sample(h, {"game": [5, 3]})
    assert out["game"].tolist() == [5, 3] and inp["game"][:2].tolist() == [5, 3]
    same_graph(subg, dgl.node_subgraph(h, inp))


def test_saint_sampler(dev):
    import dgl_amd as dgl
    from dgl_amd import sampling

    g = graph_of(GRAPHS[2], torch.int64, dev, 3)
    for mode in ("node", "edge"):
        subg = dgl.SAINTSampler(mode, 30).sample(g, None)
        nid = subg.ndata["_ID"]
        assert torch.equal(nid, torch.unique(nid)) and 0 < nid.shape[0] <= (30 if mode == "node" else 60)
        same_graph(subg, dgl.node_subgraph(g, nid))
    torch.manual_seed(3)
    subg = dgl.SAINTSampler("walk", (8, 4)).sample(g, None)
    torch.manual_seed(3)
    roots = torch.randint(0, g.num_nodes(), (8,)).to(dev)
    traces, _ = sampling.random_walk(g, roots, length=4)
    assert torch.equal(subg.ndata["_ID"], torch.unique(traces[traces >= 0]))     # every node lies on some root's walk
    same_graph(subg, dgl.node_subgraph(g, subg.ndata["_ID"]))
