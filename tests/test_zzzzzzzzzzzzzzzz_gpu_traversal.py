"""Graph traversal on the device (csrc/traversal.hip): device == host twin, element for element, on every case of
tests/traversal_cases.py (both id types, both directions, all three modes, with and without a caller's workspace), the
refusals that need the device, the Python generators on GPU graphs against the sequential-queue model, the reference's
own checks restated (layers as sets, tree edges), and prop_nodes_topo / prop_nodes_bfs / prop_edges end to end."""
import numpy as np
import pytest
import torch

from tests import traversal_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.cases()
IDTYPES = [torch.int32, torch.int64]


def t_(a, idtype, dev=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(idtype)
    return t if dev is None else t.to(dev)


def csr_pair(csr, idtype, dev):
    """(host dgla_csr, device dgla_csr) of one CSR of the table."""
    from dgl_amd import _capi

    host = [t_(csr[k], idtype) for k in ("indptr", "indices", "data")]
    there = [None if t is None else t.to(dev) for t in host]
    return _capi.host_csr(*host, csr["n"]), _capi.make_csr(*there, csr["n"])


def same(got, want, what):
    assert got[1] == want[1], what
    assert got[0].dtype == want[0].dtype and got[0].is_cuda and torch.equal(got[0].cpu(), want[0]), what


# ---- kernels against the host twin ------------------------------------------------------------------
@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_device_equals_the_host_twin(dev, case, idtype):
    from dgl_amd import DGLAMDError, _capi

    dirs = tc.directions(case)
    pairs = {r: csr_pair(dirs[r], idtype, dev) for r in (False, True)}
    ws = torch.empty(_capi.traverse_workspace_bytes(idtype, case["n"]), dtype=torch.uint8, device=dev)
    for reverse in (False, True):
        (h_csr, d_csr), (h_opp, d_opp) = pairs[reverse], pairs[not reverse]
        for workspace in (None, ws):
            for sources in case["sources"]:
                src = torch.tensor(sources, dtype=idtype)
                for mode in (tc.BFS_NODES, tc.BFS_EDGES):
                    want = _capi.traverse_host(mode, h_csr, None, src)
                    got = _capi.traverse(mode, d_csr, None, src.to(dev), workspace=workspace)
                    same(got, want, (case["name"], reverse, mode, sources[:4], workspace is not None))
            if case["topo"] == "loop":
                with pytest.raises(DGLAMDError, match="loop detected"):
                    _capi.traverse(tc.TOPO_NODES, d_csr, d_opp, workspace=workspace)
            else:
                want = _capi.traverse_host(tc.TOPO_NODES, h_csr, h_opp)
                same(_capi.traverse(tc.TOPO_NODES, d_csr, d_opp, workspace=workspace), want,
                     (case["name"], reverse, "topo", workspace is not None))


def test_device_refusals_and_a_usable_library_afterwards(dev):
    from dgl_amd import DGLAMDError, _capi

    src, dst = tc.DOC_GRAPH
    out_csr, in_csr = tc.csr_of(6, src, dst), tc.csr_of(6, dst, src)
    (h_out, d_out), (h_in, d_in) = csr_pair(out_csr, torch.int64, dev), csr_pair(in_csr, torch.int64, dev)
    ids = lambda *a: torch.tensor(a, dtype=torch.int64, device=dev)
    with pytest.raises(DGLAMDError, match=r"traverse: a source lies outside \[0, 6\)"):
        _capi.traverse(tc.BFS_NODES, d_out, None, ids(0, 6))
    with pytest.raises(DGLAMDError, match=r"traverse: a source lies outside \[0, 6\)"):
        _capi.traverse(tc.BFS_EDGES, d_out, None, ids(-3))
    need = _capi.traverse_workspace_bytes(torch.int64, 6)
    with pytest.raises(DGLAMDError, match="traverse: workspace of %d bytes required, got %d" % (need, need - 256)):
        _capi.traverse(tc.BFS_NODES, d_out, None, ids(0), workspace=torch.empty(need - 256, dtype=torch.uint8, device=dev))
    with pytest.raises(DGLAMDError, match="the count array does not match"):
        _capi.traverse(tc.TOPO_NODES, d_out, csr_pair(tc.csr_of(5, [0], [1]), torch.int64, dev)[1])
    cyc = tc.csr_of(3, [0, 1, 2], [1, 2, 0])
    d_cyc, d_cyc_in = csr_pair(cyc, torch.int64, dev)[1], csr_pair(tc.csr_of(3, [1, 2, 0], [0, 1, 2]), torch.int64, dev)[1]
    with pytest.raises(DGLAMDError, match="loop detected in the graph: only 0 of 3"):
        _capi.traverse(tc.TOPO_NODES, d_cyc, d_cyc_in)
    got = _capi.traverse(tc.TOPO_NODES, d_out, d_in)                                 # the next call succeeds
    assert got[1] == [len(f) for f in tc.DOC_TOPO] and got[0].tolist() == [x for f in tc.DOC_TOPO for x in f]
    empty = _capi.traverse(tc.BFS_NODES, d_out, None, ids())
    assert empty[0].numel() == 0 and empty[1] == []


# ---- the Python surface on GPU graphs ---------------------------------------------------------------
def gpu_graph(case, idtype, dev):
    import dgl_amd as dgl

    return dgl.graph((t_(case["src"], idtype, dev), t_(case["dst"], idtype, dev)), num_nodes=case["n"], idtype=idtype, device=dev)


def graph_csr(g, reverse):
    rel = g._graph.relations[0]
    fmt = rel.csc() if reverse else rel.csr()
    return dict(n=rel.num_src, indptr=fmt[0].cpu().numpy(), indices=fmt[1].cpu().numpy(),
                data=None if fmt[2] is None else fmt[2].cpu().numpy())


@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
@pytest.mark.parametrize("name", ["trees64", "sparse2000", "multigraph"])
def test_generators_on_a_gpu_graph_equal_the_queue_model(dev, name, idtype):
    import dgl_amd as dgl

    case = next(c for c in CASES if c["name"] == name)
    g = gpu_graph(case, idtype, dev)
    for reverse in (False, True):
        csr = graph_csr(g, reverse)
        runs = [(dgl.bfs_nodes_generator(g, s, reverse), tc.model(tc.BFS_NODES, csr, s)) for s in case["sources"]]
        runs += [(dgl.bfs_edges_generator(g, torch.tensor(s), reverse), tc.model(tc.BFS_EDGES, csr, s)) for s in case["sources"]]
        if case["topo"] == "ok":
            runs.append((dgl.topological_nodes_generator(g, reverse), tc.model(tc.TOPO_NODES, csr)))
        else:
            with pytest.raises(dgl.DGLAMDError, match="topological_nodes_generator: loop detected"):
                dgl.topological_nodes_generator(g, reverse)
        for got, want in runs:
            assert isinstance(got, tuple) and all(f.device == g.device and f.dtype == idtype for f in got)
            assert [f.tolist() for f in got] == want


def test_layers_as_sets_equal_a_level_computation(dev):
    """The reference's own BFS / topological checks, restated: on a random 100-node graph the layers, as sets, are the
    distance classes of a numpy level computation."""
    import dgl_amd as dgl

    rng = np.random.default_rng(42)
    n = 100
    src, dst = rng.integers(0, n, 300), rng.integers(0, n, 300)
    g = dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n, device=dev)
    adj = np.zeros((n, n), dtype=bool)
    adj[src, dst] = True
    seen = np.zeros(n, dtype=bool)
    seen[0] = True
    frontier, layers = seen.copy(), [{0}]
    while True:
        frontier = adj[frontier].any(0) & ~seen
        if not frontier.any():
            break
        seen |= frontier
        layers.append(set(np.flatnonzero(frontier).tolist()))
    assert [set(f.tolist()) for f in dgl.bfs_nodes_generator(g, 0)] == layers
    # the same for a DAG: the topological layers are the classes of the longest path from a root
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    keep = lo != hi
    dag = dgl.graph((torch.from_numpy(lo[keep]), torch.from_numpy(hi[keep])), num_nodes=n, device=dev)
    depth = np.zeros(n, dtype=np.int64)
    for u, v in sorted(zip(lo[keep].tolist(), hi[keep].tolist())):                  # (u < v: sources are final when read)
        depth[v] = max(depth[v], depth[u] + 1)
    want = [set(np.flatnonzero(depth == d).tolist()) for d in range(depth.max() + 1)]
    assert [set(f.tolist()) for f in dgl.topological_nodes_generator(dag)] == want


def _tree_case():
    case = next(c for c in CASES if c["name"] == "trees64")
    roots = case["sources"][0]
    depth = np.zeros(case["n"], dtype=np.int64)
    for c, p in zip(case["src"].tolist(), case["dst"].tolist()):                     # (a parent's id is below its children's)
        depth[c] = depth[p] + 1
    size = np.ones(case["n"], dtype=np.int64)
    for c, p in sorted(zip(case["src"].tolist(), case["dst"].tolist()), reverse=True):
        size[p] += size[c]
    return case, roots, depth, size


def test_tree_edges_of_a_random_tree_match(dev):
    """Edge frontier k of a BFS down a tree is the set of edges into the nodes of depth k + 1."""
    import dgl_amd as dgl

    case, roots, depth, _ = _tree_case()
    g = gpu_graph(case, torch.int64, dev)                                            # edges child -> parent: walk them backwards
    got = dgl.bfs_edges_generator(g, roots, reverse=True)
    assert len(got) == depth.max()
    for k, f in enumerate(got):
        assert sorted(f.tolist()) == np.flatnonzero(depth[case["src"]] == k + 1).tolist()


@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
def test_prop_nodes_topo_computes_subtree_sizes(dev, idtype):
    """h = 1 + sum of the children's h, swept from the leaves to the roots, is the size of every subtree."""
    import dgl_amd as dgl
    import dgl_amd.function as fn

    case, _, _, size = _tree_case()
    want = torch.from_numpy(size).to(torch.float32).reshape(-1, 1)
    plus_one = lambda nodes: {"h": nodes.data["h"] + 1}
    g = gpu_graph(case, idtype, dev)
    g.ndata["h"] = torch.zeros(case["n"], 1, device=dev)
    dgl.prop_nodes_topo(g, fn.copy_u("h", "m"), fn.sum("m", "h"), apply_node_func=plus_one)
    assert torch.equal(g.ndata["h"].cpu(), want)
    # the same through a user-defined reduce function, over the frontiers after the leaves (h = 1 there already)
    g.ndata["h"] = torch.ones(case["n"], 1, device=dev)
    frontiers = dgl.topological_nodes_generator(g)
    g.prop_nodes(frontiers[1:], fn.copy_u("h", "m"), lambda nodes: {"h": nodes.mailbox["m"].sum(1)}, plus_one)
    assert torch.equal(g.ndata["h"].cpu(), want)


def test_prop_nodes_bfs_computes_depths(dev):
    import dgl_amd as dgl
    import dgl_amd.function as fn

    case, roots, depth, _ = _tree_case()
    g = dgl.reverse(gpu_graph(case, torch.int64, dev))                               # edges parent -> child
    g.ndata["d"] = torch.zeros(case["n"], 1, device=dev)
    dgl.prop_nodes_bfs(g, roots, fn.copy_u("d", "m"), fn.sum("m", "d"),
                       apply_node_func=lambda nodes: {"d": nodes.data["d"] + 1})
    assert torch.equal(g.ndata["d"].cpu().reshape(-1).long(), torch.from_numpy(depth) + 1)


def test_prop_edges_over_bfs_edge_frontiers(dev):
    import dgl_amd as dgl
    import dgl_amd.function as fn

    case, roots, depth, _ = _tree_case()
    g = dgl.reverse(gpu_graph(case, torch.int64, dev))
    g.ndata["d"] = torch.zeros(case["n"], 1, device=dev)
    dgl.prop_edges(g, dgl.bfs_edges_generator(g, roots), fn.copy_u("d", "m"), fn.sum("m", "d"),
                   lambda nodes: {"d": nodes.data["d"] + 1})
    assert torch.equal(g.ndata["d"].cpu().reshape(-1).long(), torch.from_numpy(depth))
