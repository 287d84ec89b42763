"""Cases and a numpy model for the exclusion / compaction unit (csrc/exclude.hip; the rule: include/dgl_amd.h "Edge
exclusion and compaction"): the smallest shapes at which the row sweep, the bisection and the compaction can go wrong.
Shared by tests/test_exclude_host.py (host twins == this model) and tests/test_zzzzzzzzzzzzzzz_gpu_edge_prediction.py
(device == host twins)."""
import functools

import numpy as np
import torch

NP_I = {torch.int32: np.int32, torch.int64: np.int64}
IDTYPES = (torch.int32, torch.int64)

# ---- the frontier -----------------------------------------------------------------------------------------
# the boundaries of both lane-group widths (16 and 64), a row that loops (130), rows of one entry and empty rows
ROW_LENGTHS = [0, 1, 15, 16, 17, 0, 63, 64, 65, 130, 1]
NNZ = sum(ROW_LENGTHS)      # 372
BASES = {torch.int32: [0, 2 ** 31 - 1 - NNZ], torch.int64: [0, 2 ** 31 - 1 - NNZ, 2 ** 62]}


@functools.lru_cache(maxsize=None)
def frontier(base, short_groups=False):
    """(indptr, src, eids) as int64 numpy arrays.  The mean row length is 372 / 11 = 33.8, which selects 64 lanes per
    row; ``short_groups`` appends 11 empty rows (mean 16.9), which selects 16 lanes per row."""
    rng = np.random.default_rng(181)
    lengths = ROW_LENGTHS + ([0] * len(ROW_LENGTHS) if short_groups else [])
    indptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=indptr[1:])
    eids = base + rng.permutation(NNZ).astype(np.int64)
    src = rng.integers(0, 1000, NNZ).astype(np.int64)
    return indptr, src, eids


def exclusion_lists(base):
    """(name, X) with X an ascending int64 array, for the frontier of `base`."""
    indptr, _, eids = frontier(base)
    rng = np.random.default_rng(182)
    lo, hi = base, base + NNZ - 1
    every = np.sort(eids)
    out = [("empty", np.zeros(0, dtype=np.int64)),
           ("first_of_row_1", eids[indptr[1]:indptr[1] + 1]),
           ("last_of_last_row", eids[-1:]),
           ("all", every),
           ("every_second", every[::2]),
           ("len2", every[[3, 200]]),
           ("len3", every[[0, 100, NNZ - 1]]),
           ("duplicates_and_absent", np.sort(np.concatenate([every[5:60:5], every[5:60:10], every[300:310], every[300:310],
                                                             np.full(2, hi + 1), np.full(2 if base else 0, lo - 1)])))]
    if base > 0:
        out.append(("absent_single", np.array([lo - 1], dtype=np.int64)))
        out.append(("below_and_above", np.array([lo - 7, lo - 1, hi + 1], dtype=np.int64)))
        sparse = np.unique(np.concatenate([lo - 20000 + rng.integers(0, 20000 + NNZ, 990), every[::40]]))
    else:
        out.append(("absent_single", np.array([hi + 1], dtype=np.int64)))
        out.append(("above", np.array([hi + 1, hi + 9], dtype=np.int64)))
        sparse = np.unique(np.concatenate([rng.integers(0, 50 * NNZ, 990), every[::40]]))
    out.append(("sparse_1000", sparse))       # about 1 000 ids, 10 of them present: the bisection at its depth
    return out


def model_filter(indptr, src, eids, x):
    """(out_indptr, out_src, out_eids): the entries whose edge id is not in x, rows and their order kept."""
    keep = ~np.isin(eids, x)
    kept = np.concatenate([[0], np.cumsum(keep)])
    return kept[indptr], src[keep], eids[keep]


# ---- building the set -------------------------------------------------------------------------------------
SET_EDGES = 1000


def set_cases():
    """(name, ids, reverse map or None, num_edges, flagged)."""
    E = SET_EDGES
    rng = np.random.default_rng(183)
    involution = (np.arange(E) + E // 2) % E
    ends = np.array([0, E - 1, 0, E // 2, E // 2 - 1], dtype=np.int64)
    batch = rng.integers(0, E, 300).astype(np.int64)        # (with repeats)
    out = []
    for name, ids in (("ends", ends), ("batch", batch), ("one", np.array([7], dtype=np.int64)),
                      ("none", np.zeros(0, dtype=np.int64))):
        out.append((name, ids, None, E, False))
        out.append((name + "_reverse", ids, involution, E, False))
    for name, bad in (("id_equals_num_edges", E), ("id_minus_one", -1)):
        ids = np.array([3, bad, E - 1], dtype=np.int64)
        out.append((name, ids, None, E, True))
        out.append((name + "_reverse", ids, involution, E, True))
    return out


def model_set(ids, rev, num_edges):
    """(X, flagged): an id outside [0, num_edges) stands as num_edges in its slots and is never used as an index."""
    bad = (ids < 0) | (ids >= num_edges)
    slots = [np.where(bad, num_edges, ids)]
    if rev is not None:
        slots.append(np.where(bad, num_edges, rev[np.where(bad, 0, ids)]))
    return np.sort(np.concatenate(slots)), bool(bad.any())


# ---- compaction -------------------------------------------------------------------------------------------
def model_compact(preserve, ends, num_nodes):
    """(local, nodes): preserve in the order given (first positions), then the other end points ascending."""
    _, first = np.unique(preserve, return_index=True)
    head = preserve[np.sort(first)]
    nodes = np.concatenate([head, np.setdiff1d(ends, head)]).astype(np.int64)
    where = np.full(max(1, num_nodes), -1, dtype=np.int64)
    where[nodes] = np.arange(len(nodes))
    return where[ends], nodes


def compact_cases():
    """(name, preserve, ends, num_nodes)."""
    rng = np.random.default_rng(184)
    i64 = lambda a: np.asarray(a, dtype=np.int64)
    return [("nothing", i64([]), i64([]), 10),
            ("only_preserve", i64([4, 4, 9, 0]), i64([]), 10),
            ("only_ends", i64([]), i64([5, 3, 5, 9, 0, 3]), 10),
            # an isolated node (8), a repeated id (2) and an id that is also an end point (6)
            ("preserve_mixed", i64([8, 2, 6, 2]), i64([6, 1, 7, 1, 3]), 10),
            ("many", rng.integers(0, 5000, 700).astype(np.int64), rng.integers(0, 5000, 20000).astype(np.int64), 5000),
            ("range_ends", i64([99999, 0]), i64([0, 99999, 50000]), 100000)]


# the example of the reference's compact_graphs docstring: two user-plays-game graphs over 20 users and 10 games
DOC_GRAPHS = [([1, 3], [3, 5]), ([1, 6], [6, 8])]
DOC_COUNTS = {"user": 20, "game": 10}
DOC_NID = {"user": [1, 3, 6], "game": [3, 5, 6, 8]}
DOC_EDGES = [([0, 1], [0, 1]), ([0, 2], [2, 3])]


def doc_graphs(idtype, device="cpu"):
    import dgl_amd as dgl

    out = []
    for k, (u, v) in enumerate(DOC_GRAPHS):
        g = dgl.heterograph({("user", "plays", "game"): (torch.tensor(u, dtype=idtype), torch.tensor(v, dtype=idtype))},
                            DOC_COUNTS, idtype=idtype, device=device)
        g.nodes["user"].data["h"] = torch.arange(20, dtype=torch.float32, device=device) + 100 * k
        g.edges["plays"].data["w"] = torch.tensor([1.5, 2.5], device=device) + k
        out.append(g)
    return out


def three_relation_graph(idtype, device="cpu"):
    """Three relations over two node types; node 11 of "a" and node 7 of "b" are isolated."""
    import dgl_amd as dgl

    t = lambda a: torch.tensor(a, dtype=idtype)
    return dgl.heterograph({("a", "ab", "b"): (t([9, 2, 9]), t([5, 5, 0])),
                            ("b", "ba", "a"): (t([3, 0]), t([2, 10])),
                            ("a", "aa", "a"): (t([4, 2]), t([2, 4]))}, {"a": 12, "b": 8}, idtype=idtype, device=device)


THREE_NID = {"a": [2, 4, 9, 10], "b": [0, 3, 5]}
THREE_NID_PRESERVED = {"a": [11, 9, 2, 4, 10], "b": [0, 3, 5]}       # always_preserve = {"a": [11, 9, 11]}


# ---- the block tests' graph -------------------------------------------------------------------------------
def symmetric_graph(idtype, device, num_nodes=200, half=1000, seed=185):
    """A graph with `half` random edges followed by their reverses: edge e + half is the reverse of edge e.  Returns
    ``(g, reverse_eids)``."""
    import dgl_amd as dgl

    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, num_nodes, half), rng.integers(0, num_nodes, half)
    src, dst = np.concatenate([u, v]), np.concatenate([v, u])
    g = dgl.graph((torch.from_numpy(src).to(idtype), torch.from_numpy(dst).to(idtype)), num_nodes=num_nodes, idtype=idtype,
                  device=device)
    rev = torch.from_numpy((np.arange(2 * half) + half) % (2 * half)).to(idtype).to(device)
    return g, rev
