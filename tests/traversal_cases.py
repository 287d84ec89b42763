"""Shared by the traversal tests: the table of graphs the host and device tests run, and an independent Python model of
the SEQUENTIAL QUEUE algorithms (a FIFO of nodes, first discoverer wins for BFS, last decrement wins for the topological
order).  The model is written as a queue, not as the min / max position rule of csrc/traversal_step.h, so that it cannot
share a mistake with it."""
from collections import deque

import numpy as np

BFS_NODES, BFS_EDGES, TOPO_NODES = 0, 1, 2


# ---- the queue model --------------------------------------------------------------------------------
def _by_depth(items, depths):
    out = []
    for x, d in zip(items, depths):
        if d == len(out):
            out.append([])
        out[d].append(x)
    return out


def bfs_queue(n, indptr, indices, data, sources):
    """(node frontiers, edge frontiers) of a BFS from `sources` with a FIFO queue.  The sources form frontier 0 as
    given (duplicates kept); edge frontier k holds the tree edges into node frontier k + 1."""
    visited = np.zeros(n, dtype=bool)
    queue = deque()
    for s in sources:
        visited[s] = True
        queue.append((int(s), 0))
    nodes, ndepth, edges, edepth = [], [], [], []
    while queue:
        u, d = queue.popleft()
        nodes.append(u)
        ndepth.append(d)
        for p in range(int(indptr[u]), int(indptr[u + 1])):
            v = int(indices[p])
            if visited[v]:
                continue
            visited[v] = True
            queue.append((v, d + 1))
            edges.append(p if data is None else int(data[p]))
            edepth.append(d)
    return _by_depth(nodes, ndepth), _by_depth(edges, edepth)


def topo_queue(n, indptr, indices):
    """The node frontiers of Kahn's algorithm with a FIFO queue; raises ValueError on a loop."""
    deg = np.bincount(np.asarray(indices[: int(indptr[n])], dtype=np.int64), minlength=n)
    queue = deque((int(v), 0) for v in np.flatnonzero(deg == 0))
    nodes, depth = [], []
    while queue:
        u, d = queue.popleft()
        nodes.append(u)
        depth.append(d)
        for p in range(int(indptr[u]), int(indptr[u + 1])):
            v = int(indices[p])
            deg[v] -= 1
            if deg[v] == 0:
                queue.append((v, d + 1))
    if len(nodes) < n:
        raise ValueError("loop")
    return _by_depth(nodes, depth)


def model(mode, csr, sources=None):
    """The frontiers (a list of lists) of `mode` over csr = dict(n, indptr, indices, data)."""
    if mode == TOPO_NODES:
        return topo_queue(csr["n"], csr["indptr"], csr["indices"])
    nodes, edges = bfs_queue(csr["n"], csr["indptr"], csr["indices"], csr["data"], sources)
    return nodes if mode == BFS_NODES else edges


def flat(frontiers):
    """(ids, sections) of a list of frontiers, as the library reports them."""
    ids = [x for f in frontiers for x in f]
    return np.asarray(ids, dtype=np.int64), [len(f) for f in frontiers]


# ---- graphs -----------------------------------------------------------------------------------------
def csr_of(n, major, minor, shuffle_seed=None):
    """CSR of the entry list (major[i] -> minor[i]), edge i keeping id i.  With `shuffle_seed` the entries of a row stand
    in a random order; `data` maps positions to edge ids and is None when that map is the identity."""
    major, minor = np.asarray(major, dtype=np.int64), np.asarray(minor, dtype=np.int64)
    ids = np.arange(major.size)
    if shuffle_seed is not None:
        ids = np.random.default_rng(shuffle_seed).permutation(major.size)
    order = ids[np.argsort(major[ids], kind="stable")]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(major, minlength=n), out=indptr[1:])
    data = None if np.array_equal(order, np.arange(major.size)) else order
    return dict(n=n, indptr=indptr, indices=minor[order], data=data, nnz=int(major.size))


def directions(case):
    """{False: the out-edge CSR (forward), True: the in-edge CSR (reverse)} of a case."""
    s = case["shuffle"]
    return {False: csr_of(case["n"], case["src"], case["dst"], s),
            True: csr_of(case["n"], case["dst"], case["src"], None if s is None else s + 1)}


ROW_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65)      # the group and workgroup boundaries of the row stream


def _case(name, n, src, dst, sources, topo, shuffle=None):
    """topo: "ok" | "loop" (the topological order must raise)."""
    src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
    assert src.shape == dst.shape and (src.size == 0 or (0 <= min(src.min(), dst.min()) and max(src.max(), dst.max()) < n))
    return dict(name=name, n=n, src=src, dst=dst, sources=[list(s) for s in sources], topo=topo, shuffle=shuffle)


def random_trees(count, lo, hi, seed):
    """A batch of random trees with edges child -> parent; returns (n, src, dst, roots)."""
    rng = np.random.default_rng(seed)
    src, dst, roots, base = [], [], [], 0
    for _ in range(count):
        k = int(rng.integers(lo, hi + 1))
        roots.append(base)
        for c in range(1, k):
            src.append(base + c)
            dst.append(base + int(rng.integers(0, c)))
        base += k
    return base, np.asarray(src), np.asarray(dst), roots


def _row_length_graph(rows, targets_lo, targets_hi, seed):
    """`rows` source rows 0 .. rows - 1 with the lengths of ROW_LENGTHS cycled, targets drawn from [lo, hi)."""
    rng = np.random.default_rng(seed)
    lens = np.array([ROW_LENGTHS[i % len(ROW_LENGTHS)] for i in range(rows)])
    src = np.repeat(np.arange(rows), lens)
    return src, rng.integers(targets_lo, targets_hi, src.size)


def cases():
    out = []
    out.append(_case("empty_sources", 4, [0, 1, 2], [1, 2, 3], [[]], "ok"))
    out.append(_case("n1", 1, [], [], [[0], [0, 0]], "ok"))
    out.append(_case("isolated", 10, [2, 2, 5], [5, 7, 7], [[2], [0], [9, 2]], "ok", shuffle=1))
    n = 2000
    out.append(_case("path2000", n, np.arange(n - 1), np.arange(1, n), [[0]], "ok"))
    n = 5001
    out.append(_case("star5000", n, np.zeros(n - 1, dtype=np.int64), np.arange(1, n), [[0]], "ok"))
    out.append(_case("reverse_star5000", n, np.arange(1, n), np.zeros(n - 1, dtype=np.int64), [list(range(1, n)), [17]], "ok",
                     shuffle=2))
    a, b = np.meshgrid(np.arange(70), 70 + np.arange(70), indexing="ij")
    out.append(_case("bipartite70", 140, a.reshape(-1), b.reshape(-1), [list(range(70)), [69, 0]], "ok", shuffle=3))
    src, dst = _row_length_graph(300, 300, 2300, 4)
    out.append(_case("row_lengths", 2300, src, dst, [list(range(300)), list(range(299, -1, -1))], "ok", shuffle=4))
    src, dst = _row_length_graph(300, 0, 300, 5)
    # ... plus 1200 entries in row 0: a mean row length of 33, above 32, so the rows take whole wavefronts
    src, dst = np.concatenate([src, np.zeros(1200, dtype=np.int64)]), np.concatenate([dst, np.arange(1200) % 300])
    assert src.size // 300 > 32
    out.append(_case("row_lengths_wide", 300, src, dst, [[0, 1, 2], [299], list(range(300))], "loop", shuffle=5))
    rng = np.random.default_rng(6)
    src, dst = rng.integers(0, 12, 40), rng.integers(0, 12, 40)
    src, dst = np.concatenate([src, src[:10], [3, 3, 7]]), np.concatenate([dst, dst[:10], [3, 3, 7]])
    out.append(_case("multigraph", 12, src, dst, [[0], [3, 3, 5], [7]], "loop", shuffle=6))
    n, src, dst, roots = random_trees(64, 30, 60, 7)
    leaves = sorted(set(range(n)) - set(dst.tolist()))
    out.append(_case("trees64", n, src, dst, [roots, leaves[:5], [roots[3], roots[3]]], "ok", shuffle=7))
    rng = np.random.default_rng(8)
    src, dst = rng.integers(0, 2000, 6000), rng.integers(0, 2000, 6000)
    out.append(_case("sparse2000", 2000, src, dst, [[7], [1, 500, 1999], [5, 5, 9, 5]], "loop", shuffle=8))
    keep = src != dst
    lo, hi = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep]
    out.append(_case("lower_triangular2000", 2000, hi, lo, [[1999], [1500, 1999, 1500]], "ok", shuffle=9))
    # predecessors of a node in different levels: 4 <- {0 (level 0), 2 (level 1)}, 5 <- {0, 1 (level 0), 3 (level 1)}
    out.append(_case("layered", 7, [0, 1, 2, 0, 3, 1, 0, 4, 5, 0], [2, 3, 4, 4, 5, 5, 5, 6, 6, 6], [[0], [1, 0]], "ok", shuffle=10))
    out.append(_case("parallel_dag", 3, [0, 0, 1, 0, 0, 1], [1, 1, 2, 2, 2, 2], [[0], [1]], "ok", shuffle=11))
    out.append(_case("cycle3", 3, [0, 1, 2], [1, 2, 0], [[0], [2, 1]], "loop"))
    out.append(_case("self_loop", 2, [0, 0], [0, 1], [[0], [1]], "loop"))
    return out


# the docstring examples of python/dgl/traversal.py
DOC_GRAPH = ([0, 1, 1, 2, 2, 3], [1, 2, 3, 3, 4, 5])
DOC_BFS_NODES = [[0], [1], [2, 3], [4, 5]]
DOC_BFS_EDGES = [[0], [1, 2], [4, 5]]
DOC_TOPO = [[0], [1], [2], [3, 4], [5]]
