"""Shortest distances and paths (include/dgl_amd.h "Shortest distances and paths") on CPU graphs, through the host twin
dgla_shortest_dist_host: against a dense numpy level computation with the predecessor rule applied literally, and the
reference's docstring example written out.  Needs no GPU.  GRAPHS, model and in_csr also serve the GPU test."""
import functools

import numpy as np
import pytest
import torch

DOC = (4, [0, 1, 1, 2], [2, 0, 3, 3])     # python/dgl/transforms/functional.py, shortest_dist: every shortest path is unique


def _random(n):
    rng = np.random.default_rng(n)
    return n, rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)


def _loops_and_doubles():
    n, s, d = _random(65)
    loops = np.arange(0, n, 3)
    p = np.random.default_rng(7).permutation(2 * len(s) + len(loops))     # the twin of an edge gets an unrelated id
    return n, np.concatenate([s, s, loops])[p], np.concatenate([d, d, loops])[p]


GRAPHS = {
    "one_node": (1, [], []), "no_edges": (5, [], []), "doc": DOC,
    "random63": _random(63), "random64": _random(64), "random65": _random(65), "random129": _random(129),
    "loops_doubles65": _loops_and_doubles(),
    "chain70": (70, np.arange(69), np.arange(1, 70)),                      # 69 levels: L crosses the path tile's chunk
    "cycle66": (66, np.arange(66), (np.arange(66) + 1) % 66),
    "star320": (320, np.r_[np.arange(1, 301), np.zeros(19, int), 310], np.r_[np.zeros(300, int), np.arange(301, 320), 5]),
}
GRAPHS = {k: (n, np.asarray(s, np.int64), np.asarray(d, np.int64)) for k, (n, s, d) in GRAPHS.items()}


def in_csr(n, src, dst):
    """The in-edge CSR of the edge list: (indptr, indices, the edge id of every entry)."""
    order = np.argsort(dst, kind="stable")
    return np.r_[0, np.cumsum(np.bincount(dst, minlength=n))].astype(np.int64), src[order], order


def model(n, src, dst):
    """(dist, paths) of every pair; edge i is (src[i] -> dst[i])."""
    adj = np.zeros((n, n), dtype=bool)
    adj[src, dst] = True
    dist = np.full((n, n), -1, dtype=np.int64)
    for s in range(n):
        frontier, level = np.arange(n) == s, 0
        while frontier.any():
            dist[s, frontier] = level
            frontier, level = adj[frontier].any(0) & (dist[s] < 0), level + 1
    paths = np.full((n, n, dist.max()), -1, dtype=np.int64)
    for s in range(n):
        edge, node = np.full(n, -1), np.full(n, -1)
        for e in np.flatnonzero((dist[s, dst] > 0) & (dist[s, src] == dist[s, dst] - 1))[::-1]:   # the smallest id last
            edge[dst[e]], node[dst[e]] = e, src[e]
        for v in range(n):
            cur = v
            for k in range(dist[s, v] - 1, -1, -1):
                paths[s, v, k], cur = edge[cur], node[cur]
    return torch.from_numpy(dist), torch.from_numpy(paths)


@functools.lru_cache(maxsize=None)
def expected(name, edge_ids=True):
    """The model of a graph, computed once; `edge_ids` False: the ids are the positions in the in-edge CSR."""
    n, src, dst = GRAPHS[name]
    order = np.arange(len(src)) if edge_ids else in_csr(n, src, dst)[2]
    return model(n, src[order], dst[order])


def of_root(want, root):
    """What a root search returns, from the all-pairs model: L is the longest distance of that row."""
    dist, paths = want[0][root], want[1][root]
    return dist, paths[:, :max(int(dist.max()), 0)]


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_cpu_graph_equals_the_model(name, idtype):
    import dgl_amd as dgl

    n, src, dst = GRAPHS[name]
    g = dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n, idtype=idtype)
    want = expected(name)
    dist, paths = dgl.shortest_dist(g, return_paths=True)
    assert dist.dtype == paths.dtype == torch.int64 and torch.equal(dist, want[0]) and torch.equal(paths, want[1])
    assert torch.equal(dgl.shortest_dist(g), want[0])
    for root in (0, n - 1):
        dist, paths = dgl.shortest_dist(g, root=root, return_paths=True)
        assert torch.equal(dist, of_root(want, root)[0]) and torch.equal(paths, of_root(want, root)[1])
        assert torch.equal(dgl.shortest_dist(g, root), want[0][root])


def test_the_reference_docstring_example_and_refusals():
    import dgl_amd as dgl

    g = dgl.graph(([0, 1, 1, 2], [2, 0, 3, 3]))
    assert dgl.shortest_dist(g, root=0).tolist() == [0, -1, 1, 2]
    dist, paths = dgl.shortest_dist(g, root=None, return_paths=True)
    assert dist.tolist() == [[0, -1, 1, 2], [1, 0, 2, 1], [-1, -1, 0, 1], [-1, -1, -1, 0]]
    assert paths.tolist() == [[[-1, -1], [-1, -1], [0, -1], [0, 3]], [[1, -1], [-1, -1], [1, 0], [2, -1]],
                              [[-1, -1], [-1, -1], [-1, -1], [3, -1]], [[-1, -1], [-1, -1], [-1, -1], [-1, -1]]]
    empty = dgl.shortest_dist(dgl.graph(([], []), num_nodes=0), return_paths=True)
    assert empty[0].shape == (0, 0) and empty[1].shape == (0, 0, 0)
    for bad in (4, -1):
        with pytest.raises(dgl.DGLAMDError, match=r"shortest_dist: the root -?\d lies outside \[0, 4\)"):
            dgl.shortest_dist(g, root=bad)
    with pytest.raises(dgl.DGLAMDError, match="shortest_dist: takes a homogeneous graph"):
        dgl.shortest_dist(dgl.heterograph({("a", "x", "b"): ([0], [0])}))
