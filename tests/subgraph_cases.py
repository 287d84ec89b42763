"""Small CSRs plus node selections for the induced-subgraph unit (csrc/subgraph.hip): the smallest shapes at which the
row sweep can go wrong.  Shared by tests/test_induced_subgraph_host.py (host twin == numpy model) and
tests/test_zzzzzzzzzzzzzz_gpu_subgraph.py (device == host twin).

Row degrees 0, 1, 15, 16, 17, 63, 64, 65, 129 and one hub of 5 000 (a row longer than a lane group is swept in chunks of
16 / 64); one graph whose mean degree is <= 32 (groups of 16 lanes) and one above (wavefronts of 64); self-loops and
parallel edges; results below and above the size at which the eid order's sort changes kernels; the edge-id map absent or a
random permutation; a bipartite relation whose row and column node sets
differ in size.  Selections: empty, one node, all nodes in order / reversed, a random 10 %, only degree-0 nodes, the hub
alone, the hub's neighbours without the hub, and row counts that do not fill the last workgroup (256 / G rows each)."""
import numpy as np
import torch

SPECIAL = [0, 1, 15, 16, 17, 63, 64, 65, 129, 5000, 0, 0]   # degrees of rows 0 .. 11; row 9 is the hub
HUB = 9
PARTIAL = [1, 3, 4, 5, 15, 17]                              # row counts that leave the last workgroup part empty


def _csr(degrees, num_cols, rng, loops=()):
    indptr = np.zeros(len(degrees) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(degrees)
    indices = rng.integers(0, num_cols, size=int(indptr[-1]), dtype=np.int64)   # (with repeats: parallel edges)
    for r in loops:
        if degrees[r] > 0 and r < num_cols:
            indices[indptr[r]] = r                                              # a self-loop
            if degrees[r] > 2:
                indices[indptr[r + 1] - 1] = r                                  # ... twice: a parallel self-loop
    return indptr, indices


def _square(name, n, filler, seed):
    rng = np.random.default_rng(seed)
    degrees = SPECIAL + [int(d) for d in rng.integers(filler[0], filler[1] + 1, size=n - len(SPECIAL))]
    indptr, indices = _csr(degrees, n, rng, loops=(1, 4, HUB, 20))
    return dict(name=name, num_rows=n, num_cols=n, indptr=indptr, indices=indices, degrees=np.array(degrees))


def graphs():
    """The three relations, each without and with an edge-id map."""
    short = _square("short", 400, (0, 3), 1)      # mean degree ~ 15: groups of 16 lanes
    # mean degree ~ 48: wavefronts of 64; selecting every node keeps 29 000 entries, above the 16 384 keys up to which the
    # sort of the eid order runs in one workgroup
    long_ = _square("long", 600, (30, 50), 2)
    assert long_["indices"].size > 16384
    assert short["indices"].size // short["num_rows"] <= 32 < long_["indices"].size // long_["num_rows"]
    rng = np.random.default_rng(3)
    degrees = [0, 17, 65, 1, 0, 300] + [int(d) for d in rng.integers(0, 9, size=31)]
    indptr, indices = _csr(degrees, 90, rng)
    bip = dict(name="bipartite", num_rows=len(degrees), num_cols=90, indptr=indptr, indices=indices,
               degrees=np.array(degrees))
    out = []
    for g in (short, long_, bip):
        out.append(dict(g, data=None))
        perm = np.random.default_rng(7).permutation(g["indices"].size).astype(np.int64)
        out.append(dict(g, name=g["name"] + "-mapped", data=perm))
    return out


def selections(g):
    """``(name, rows, cols)`` for graph ``g``: on a square graph one list serves as both."""
    rng = np.random.default_rng(11)
    nr, nc = g["num_rows"], g["num_cols"]
    ids = lambda a: np.asarray(a, dtype=np.int64)
    if nr != nc:
        some_rows, some_cols = rng.permutation(nr)[: nr // 2], rng.permutation(nc)[: nc // 3]
        return [("empty", ids([]), ids([])),
                ("all", np.arange(nr), np.arange(nc)),
                ("all-reversed", np.arange(nr)[::-1].copy(), np.arange(nc)[::-1].copy()),
                ("some", ids(some_rows), ids(some_cols)),
                ("rows-only", ids(some_rows), ids([])),
                ("cols-only", ids([]), ids(some_cols)),
                ("long-rows", ids([5, 2, 1]), np.arange(0, nc, 2))]
    lo, hi = g["indptr"][HUB], g["indptr"][HUB + 1]
    nbrs = np.unique(g["indices"][lo:hi])
    out = [("empty", ids([])),
           ("one", ids([4])),
           ("all", np.arange(nr)),
           ("all-reversed", np.arange(nr)[::-1].copy()),
           ("tenth", ids(rng.permutation(nr)[: nr // 10])),
           ("degree-0", ids(np.nonzero(g["degrees"] == 0)[0])),
           ("hub", ids([HUB])),
           ("hub-neighbours", ids(nbrs[nbrs != HUB]))]
    special = rng.permutation(len(SPECIAL))
    for k in PARTIAL:    # the special rows first, so the long rows sit in a part-filled workgroup too
        out.append(("first-%d" % k, ids(np.concatenate([special, rng.permutation(np.arange(len(SPECIAL), nr))])[:k])))
    return [(name, sel, sel) for name, sel in out]


def same_graph(a, b):
    """Edges, ids and features of two subgraphs, exactly."""
    assert a.ntypes == b.ntypes and a.canonical_etypes == b.canonical_etypes
    for i in range(len(a.ntypes)):
        assert a._graph.num_nodes(i) == b._graph.num_nodes(i)
        assert set(a._node_frames[i].keys()) == set(b._node_frames[i].keys())
        for k, val in a._node_frames[i].items():
            assert torch.equal(val, b._node_frames[i][k]), k
    for c in a.canonical_etypes:
        for x, y in zip(a.edges(etype=c), b.edges(etype=c)):
            assert x.dtype == y.dtype and torch.equal(x, y), c
        fa, fb = a._edge_frames[a.get_etype_id(c)], b._edge_frames[b.get_etype_id(c)]
        assert set(fa.keys()) == set(fb.keys())
        for k, val in fa.items():
            assert torch.equal(val, fb[k]), (c, k)
