"""What the sampler and sparse units refuse of a dgla_csr and of a workspace, pinned to a recorded table — runs without a GPU.

Every entry point of those units that takes a ``dgla_csr`` is called through ctypes with a small valid graph (a
bi-directed 4-cycle, int64 ids, host memory) carrying ONE structural defect at a time.  ``REFUSED[entry]`` lists the
defects the entry refuses; it was recorded from the library as it stood BEFORE the units moved to the shared
``check_csr`` of csrc/host_util.h, so a unit that starts to refuse more, or less, shows up here as a diff of one word.

  * a refused pair returns -1 with a message that starts with the entry's ``who`` and is no HIP error text: the
    refusal comes before any runtime call, so the device entries can be asked here as well;
  * an accepted pair is run only through a ``_host`` twin, which needs no GPU, and returns 0.  (Accepted pairs of a
    device entry are not run: they would launch.)

The second table is the workspaces: every entry with one is given ``need - 256`` bytes, and a null pointer where the
workspace is required, with ``need`` from the entry's own ``*_workspace_bytes`` query; all of them answer
``"<who>: workspace of <need> bytes required"``."""
import ctypes

import numpy as np
import pytest

from dgl_amd._lib import COO, CSR, LIB, WalkRelation

N, NNZ = 4, 8
_I = np.int64
INDPTR = np.array([0, 2, 4, 6, 8], _I)
INDICES = np.array([1, 3, 0, 2, 1, 3, 0, 2], _I)      # ascending in every row: also the `member` array
SEEDS = np.arange(N, dtype=_I)
W32 = np.ones(NNZ, np.float32)
ONES = np.ones(N, np.float64)
ZERO_PTR = np.zeros(1, _I)
OUT = [np.zeros(64, _I) for _ in range(4)]            # outputs of the host twins (at most 2 * NNZ + N entries)
I32 = np.zeros(64, np.int32)
SCRATCH = np.zeros(1 << 16, np.uint8)                 # stands in for a workspace that is too small
BFS_NODES = 0


def ptr(a):
    return a.ctypes.data


def base():
    return CSR(N, N, NNZ, 64, ptr(INDPTR), ptr(INDICES), None)


def empty():
    return CSR(0, 0, 0, 64, ptr(ZERO_PTR), None, None)


DEFECTS = {
    "null struct": lambda: None,
    "idtype_bits = 16": lambda: CSR(N, N, NNZ, 16, ptr(INDPTR), ptr(INDICES), None),
    "negative num_rows": lambda: CSR(-1, N, NNZ, 64, ptr(INDPTR), ptr(INDICES), None),
    "negative nnz": lambda: CSR(N, N, -1, 64, ptr(INDPTR), ptr(INDICES), None),
    "null indptr, num_rows > 0": lambda: CSR(N, N, NNZ, 64, None, ptr(INDICES), None),
    "null indptr, num_rows == 0": lambda: CSR(0, 0, 0, 64, None, None, None),
    "null indices, nnz > 0": lambda: CSR(N, N, NNZ, 64, ptr(INDPTR), None, None),
}
ALL = tuple(DEFECTS)
BUT_EMPTY = tuple(d for d in ALL if d != "null indptr, num_rows == 0")


def ref(c):
    return None if c is None else ctypes.byref(c)


def seeds_of(c):  # no seed for a graph without rows
    return N if c is None or c.num_rows != 0 else 0


i64 = ctypes.c_int64


def _walk(fn, c, *tail):
    rel = (WalkRelation * 1)(WalkRelation(ctypes.pointer(c) if c is not None else None, None))
    path = (ctypes.c_int32 * 2)(0, 0)
    return fn(rel, 1, path, 2, ptr(SEEDS), seeds_of(c), 0.0, None, 0, 7, ptr(OUT[0]), ptr(OUT[1]), *tail)


def _sum(fn, c, *tail):
    ops = (ctypes.POINTER(CSR) * 1)(ctypes.pointer(c) if c is not None else None)
    return fn(ops, 1, *tail)


def _subgraph_host(c):
    total, flags = i64(0), ctypes.c_int32(0)
    n = seeds_of(c)
    return LIB.dgla_induced_subgraph_host(ref(c), ptr(SEEDS), n, ptr(SEEDS), n, 0, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]),
                                          ptr(OUT[3]), ctypes.byref(total), ctypes.byref(flags))


def _other(c):  # a second operand that fits `c`
    return empty() if c is not None and c.num_rows == 0 else base()


# entry -> (who, call(csr or None)); the `_host` entries run on the CPU, the others refuse before they touch the GPU
ENTRIES = {
    "csr_sorted_columns": ("csr_sorted_columns", lambda c: LIB.dgla_csr_sorted_columns(ref(c), ptr(OUT[0]), None, 0, None)),
    "node2vec_walk": ("node2vec_walk", lambda c: LIB.dgla_node2vec_walk(
        ref(c), None, ptr(INDICES), ptr(SEEDS), seeds_of(c), 2, 1.0, 1.0, 7, ptr(OUT[0]), None, None)),
    "node2vec_walk_host": ("node2vec_walk_host", lambda c: LIB.dgla_node2vec_walk_host(
        ref(c), None, ptr(INDICES), ptr(SEEDS), seeds_of(c), 2, 1.0, 1.0, 7, ptr(OUT[0]), None, None)),
    "csr_mm_count": ("csr_mm: a", lambda c: LIB.dgla_csr_mm_count(
        ref(c), ref(_other(c)), ptr(OUT[0]), ctypes.byref(i64(0)), None, 0, None)),
    "csr_mm_fill": ("csr_mm: a", lambda c: LIB.dgla_csr_mm_fill(
        ref(c), 0, ptr(W32), ref(_other(c)), ptr(W32), ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None, 0, None)),
    "csr_sum_count": ("csr_sum: operand", lambda c: _sum(LIB.dgla_csr_sum_count, c, ptr(OUT[0]), ctypes.byref(i64(0)), None, 0,
                                                         None)),
    "csr_sum_fill": ("csr_sum: operand", lambda c: _sum(LIB.dgla_csr_sum_fill, c, 0, (ctypes.c_void_p * 1)(ptr(W32)),
                                                        ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None, 0, None)),
    "csr_mask": ("csr_mask: a", lambda c: LIB.dgla_csr_mask(ref(c), 0, ptr(W32), ctypes.byref(
        COO(seeds_of(c), seeds_of(c), seeds_of(c) // N, 64, ptr(SEEDS), ptr(SEEDS), None)), ptr(OUT[0]), None)),
    "sample_neighbors": ("sample_neighbors", lambda c: LIB.dgla_sample_neighbors(
        ref(c), ptr(SEEDS), seeds_of(c), 2, 0, 7, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None, 0, None)),
    "sample_neighbors_weighted": ("sample_neighbors_weighted", lambda c: LIB.dgla_sample_neighbors_weighted(
        ref(c), ptr(W32), 0, ptr(SEEDS), seeds_of(c), 2, 0, 7, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None, 0, None)),
    "sample_neighbors_padded": ("sample_neighbors_padded", lambda c: LIB.dgla_sample_neighbors_padded(
        ctypes.cast(ref(c), ctypes.c_void_p) if c is not None else None, None, 0, ptr(SEEDS), N, None, 2, 0, 7, None, 1,
        ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None, 0, None)),
    "traverse": ("traverse", lambda c: LIB.dgla_traverse(
        BFS_NODES, ref(c), None, ptr(SEEDS), min(1, seeds_of(c)), ptr(OUT[0]), OUT[1].ctypes.data_as(ctypes.POINTER(i64)),
        ctypes.byref(i64(0)), ctypes.byref(i64(0)), None, 0, None)),
    "traverse_host": ("traverse_host", lambda c: LIB.dgla_traverse_host(
        BFS_NODES, ref(c), None, ptr(SEEDS), min(1, seeds_of(c)), ptr(OUT[0]), OUT[1].ctypes.data_as(ctypes.POINTER(i64)),
        ctypes.byref(i64(0)), ctypes.byref(i64(0)))),
    "select_topk": ("select_topk", lambda c: LIB.dgla_select_topk(
        ref(c), ptr(W32), 0, ptr(SEEDS), seeds_of(c), 1, 0, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None, 0, None)),
    "select_topk_host": ("select_topk_host", lambda c: LIB.dgla_select_topk_host(
        ref(c), ptr(W32), 0, ptr(SEEDS), seeds_of(c), 1, 0, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]))),
    "labor_scale": ("labor_scale", lambda c: LIB.dgla_labor_scale(
        ref(c), ptr(W32), 0, ptr(SEEDS), seeds_of(c), 1, ptr(ONES), None)),
    "labor_scale_host": ("labor_scale_host", lambda c: LIB.dgla_labor_scale_host(
        ref(c), ptr(W32), 0, ptr(SEEDS), seeds_of(c), 1, ptr(ONES))),
    "labor_count": ("labor_count", lambda c: LIB.dgla_labor_count(
        ref(c), None, 0, None, ptr(SEEDS), seeds_of(c), 1, 7, ptr(OUT[0]), ptr(OUT[1]), None, 0, None)),
    "labor_fill": ("labor_fill", lambda c: LIB.dgla_labor_fill(
        ref(c), None, 0, None, ptr(SEEDS), seeds_of(c), 1, 7, NNZ, ptr(OUT[0]), ptr(OUT[1]), None, None, 0, None)),
    "labor_pick_host": ("labor_pick_host", lambda c: LIB.dgla_labor_pick_host(
        ref(c), None, 0, None, ptr(SEEDS), seeds_of(c), 1, 7, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None)),
    "negative_sample": ("negative_sample", lambda c: LIB.dgla_negative_sample(
        ref(c), ptr(INDICES), seeds_of(c), seeds_of(c), 2, 0, 1, 7, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), None, 0, None)),
    "negative_sample_host": ("negative_sample_host", lambda c: LIB.dgla_negative_sample_host(
        ref(c), ptr(INDICES), seeds_of(c), seeds_of(c), 2, 0, 1, 7, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]))),
    "csr_has_edges": ("csr_has_edges", lambda c: LIB.dgla_csr_has_edges(
        ref(c), ptr(INDICES), ptr(SEEDS), ptr(SEEDS), seeds_of(c), ptr(OUT[0]), None)),
    "csr_has_edges_host": ("csr_has_edges_host", lambda c: LIB.dgla_csr_has_edges_host(
        ref(c), ptr(INDICES), ptr(SEEDS), ptr(SEEDS), seeds_of(c), ptr(OUT[0]))),
    "induced_subgraph_count": ("induced_subgraph_count", lambda c: LIB.dgla_induced_subgraph_count(
        ref(c), ptr(SEEDS), seeds_of(c), ptr(I32), ptr(OUT[0]), None, 0, None)),
    "induced_subgraph_fill": ("induced_subgraph_fill", lambda c: LIB.dgla_induced_subgraph_fill(
        ref(c), ptr(SEEDS), seeds_of(c), ptr(I32), ptr(OUT[0]), 2 * seeds_of(c), ptr(OUT[1]), ptr(OUT[2]), ptr(OUT[3]), 1,
        None, 0, None)),
    "induced_subgraph_host": ("induced_subgraph_host", _subgraph_host),
    "neighbor_matching": ("neighbor_matching", lambda c: LIB.dgla_neighbor_matching(
        ref(c), None, 0, 7, 64, 0, ptr(OUT[0]), ctypes.byref(i64(0)), None, 0, None)),
    "neighbor_matching_host": ("neighbor_matching_host", lambda c: LIB.dgla_neighbor_matching_host(
        ref(c), None, 0, 7, 64, ptr(OUT[0]), ctypes.byref(i64(0)), None)),
    "random_walk_cdf": ("random_walk_cdf", lambda c: LIB.dgla_random_walk_cdf(ref(c), ptr(W32), 0, ptr(ONES), None, 0, None)),
    "random_walk": ("random_walk", lambda c: _walk(LIB.dgla_random_walk, c, None, 0, None)),
    "random_walk_host": ("random_walk_host", lambda c: _walk(LIB.dgla_random_walk_host, c)),
}

# entry -> the defects it refuses (recorded at the commit before the shared check)
REFUSED = {
    "csr_sorted_columns": ALL,
    "node2vec_walk": ALL,
    "node2vec_walk_host": ALL,
    "csr_mm_count": BUT_EMPTY,
    "csr_mm_fill": BUT_EMPTY,
    "csr_sum_count": BUT_EMPTY,
    "csr_sum_fill": BUT_EMPTY,
    "csr_mask": BUT_EMPTY,
    "sample_neighbors": ("null struct", "idtype_bits = 16", "null indptr, num_rows > 0", "null indptr, num_rows == 0"),
    "sample_neighbors_weighted": ("null struct", "idtype_bits = 16", "null indptr, num_rows > 0",
                                  "null indptr, num_rows == 0"),
    "sample_neighbors_padded": ("null struct", "idtype_bits = 16", "null indptr, num_rows > 0",
                                "null indptr, num_rows == 0"),
    "traverse": ALL,
    "traverse_host": ALL,
    "select_topk": ALL,
    "select_topk_host": ALL,
    "labor_scale": BUT_EMPTY,
    "labor_scale_host": BUT_EMPTY,
    "labor_count": BUT_EMPTY,
    "labor_fill": BUT_EMPTY,
    "labor_pick_host": BUT_EMPTY,
    "negative_sample": ("null struct", "idtype_bits = 16", "negative num_rows", "negative nnz", "null indptr, num_rows > 0"),
    "negative_sample_host": ("null struct", "idtype_bits = 16", "negative num_rows", "negative nnz",
                             "null indptr, num_rows > 0"),
    "csr_has_edges": ("null struct", "idtype_bits = 16", "negative num_rows", "negative nnz", "null indptr, num_rows > 0"),
    "csr_has_edges_host": ("null struct", "idtype_bits = 16", "negative num_rows", "negative nnz",
                           "null indptr, num_rows > 0"),
    "induced_subgraph_count": BUT_EMPTY,
    "induced_subgraph_fill": BUT_EMPTY,
    "induced_subgraph_host": BUT_EMPTY,
    "neighbor_matching": ALL,
    "neighbor_matching_host": ALL,
    "random_walk_cdf": tuple(d for d in ALL if d != "null indices, nnz > 0"),
    "random_walk": ALL,
    "random_walk_host": ALL,
}


def last_error():
    return LIB.dgla_last_error().decode()


def observe(entry, defect):
    """(return code, message) of `entry` given a csr with `defect`."""
    _, call = ENTRIES[entry]
    c = DEFECTS[defect]()
    rc = call(c)
    return rc, last_error() if rc else ""


def test_tables_cover_every_entry_and_defect():
    assert sorted(ENTRIES) == sorted(REFUSED) and len(ENTRIES) == 32 and len(DEFECTS) == 7
    assert all(set(r) <= set(DEFECTS) for r in REFUSED.values())
    # a device entry and its host twin refuse the same csr
    twins = [e for e in ENTRIES if e.endswith("_host") and e[:-5] in ENTRIES]
    assert len(twins) == 8 and all(REFUSED[t] == REFUSED[t[:-5]] for t in twins)


HOST = sorted(e for e in ENTRIES if e.endswith("_host"))


@pytest.mark.parametrize("entry", HOST)
def test_host_twins_run_the_undamaged_graph(entry):
    assert ENTRIES[entry][1](base()) == 0, last_error()
    assert ENTRIES[entry][1](empty()) == 0, last_error()    # no rows, an indptr of one entry


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_csr_defects_match_the_recorded_table(entry):
    who = ENTRIES[entry][0]
    for defect in DEFECTS:
        if defect in REFUSED[entry]:
            rc, msg = observe(entry, defect)
            assert rc == -1, (entry, defect)
            assert msg.startswith(who + ": ") or msg.startswith(who + " "), (entry, defect, msg)
            assert "hip" not in msg, (entry, defect, msg)       # refused before any runtime call
        elif entry.endswith("_host"):
            rc, msg = observe(entry, defect)
            assert rc == 0, (entry, defect, msg)


# ---- workspaces ---------------------------------------------------------------------------------------------------
LONG_PATH = (ctypes.c_int32 * 257)()       # 257 steps: the metapath no longer travels in the kernel arguments
CLOUD = 1 << 20                            # rows of a point cloud whose distances do not fit LDS
OFFS = np.array([0, N], _I)
X = np.zeros((N, 3), np.float32)


def _walk_ws(ws, nbytes):
    rel = (WalkRelation * 1)(WalkRelation(ctypes.pointer(base()), None))
    traces = np.zeros(N * 258, _I)
    return LIB.dgla_random_walk(rel, 1, LONG_PATH, 257, ptr(SEEDS), N, 0.0, None, 0, 7, ptr(traces), None, ws, nbytes, None)


# entry -> (who, need, call(workspace, bytes), required)
WORKSPACES = {
    "csr_sorted_columns": ("csr_sorted_columns", lambda: LIB.dgla_csr_sorted_columns_workspace_bytes(ref(base())),
                           lambda ws, b: LIB.dgla_csr_sorted_columns(ref(base()), ptr(OUT[0]), ws, b, None), True),
    "labor_count": ("labor_count", lambda: LIB.dgla_labor_workspace_bytes(64, N),
                    lambda ws, b: LIB.dgla_labor_count(ref(base()), None, 0, None, ptr(SEEDS), N, 1, 7, ptr(OUT[0]), ptr(OUT[1]),
                                                       ws, b, None), True),
    "labor_fill": ("labor_fill", lambda: LIB.dgla_labor_workspace_bytes(64, N),
                   lambda ws, b: LIB.dgla_labor_fill(ref(base()), None, 0, None, ptr(SEEDS), N, 1, 7, NNZ, ptr(OUT[0]),
                                                     ptr(OUT[1]), None, ws, b, None), True),
    "induced_subgraph_count": ("induced_subgraph_count", lambda: LIB.dgla_induced_subgraph_workspace_bytes(64, N, 0),
                               lambda ws, b: LIB.dgla_induced_subgraph_count(ref(base()), ptr(SEEDS), N, ptr(I32), ptr(OUT[0]),
                                                                             ws, b, None), True),
    "induced_subgraph_fill": ("induced_subgraph_fill", lambda: LIB.dgla_induced_subgraph_workspace_bytes(64, N, NNZ),
                              lambda ws, b: LIB.dgla_induced_subgraph_fill(ref(base()), ptr(SEEDS), N, ptr(I32), ptr(OUT[0]),
                                                                           NNZ, ptr(OUT[1]), ptr(OUT[2]), ptr(OUT[3]), 1, ws, b,
                                                                           None), True),
    "negative_sample": ("negative_sample", lambda: LIB.dgla_negative_sample_workspace_bytes(64, N),
                        lambda ws, b: LIB.dgla_negative_sample(ref(base()), ptr(INDICES), N, N, 2, 0, 1, 7, ptr(OUT[0]),
                                                               ptr(OUT[1]), ptr(OUT[2]), ws, b, None), True),
    "random_walk": ("random_walk", lambda: LIB.dgla_random_walk_workspace_bytes(1, 257), _walk_ws, True),
    "sample_neighbors_padded": ("sample_neighbors_padded", lambda: LIB.dgla_sample_neighbors_workspace_bytes(64, N),
                                lambda ws, b: LIB.dgla_sample_neighbors_padded(
                                    ctypes.cast(ctypes.pointer(base()), ctypes.c_void_p), None, 0, ptr(SEEDS), N, None, 2, 0, 7,
                                    None, 1, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), ws, b, None), True),
    "to_block_padded": ("to_block_padded", lambda: LIB.dgla_to_block_workspace_bytes(64, NNZ),
                        lambda ws, b: LIB.dgla_to_block_padded(64, ptr(SEEDS), N, None, ptr(INDICES), NNZ, N, ptr(I32),
                                                               ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), ws, b, None), True),
    "knn": ("knn", lambda: LIB.dgla_knn_workspace_bytes(1),
            lambda ws, b: LIB.dgla_knn(ptr(X), N, None, N, 0, 3, ptr(OFFS), ptr(OFFS), 1, 2, 64, ptr(OUT[0]), None, ws, b, None),
            True),
    "fps": ("fps", lambda: LIB.dgla_fps_workspace_bytes(0, 1, CLOUD),
            lambda ws, b: LIB.dgla_fps(ptr(X), 0, 1, CLOUD, 3, 1, ptr(ZERO_PTR), ptr(OUT[0]), ws, b, None), True),
    "pinsage_select_count": ("pinsage_select_count", lambda: LIB.dgla_pinsage_select_workspace_bytes(64, 2, 4, 2),
                             lambda ws, b: LIB.dgla_pinsage_select_count(64, ptr(INDICES), ptr(INDICES), 2, 4, 2,
                                                                         ctypes.byref(i64(0)), ws, b, None), True),
    "pinsage_select_fill": ("pinsage_select_fill", lambda: LIB.dgla_pinsage_select_workspace_bytes(64, 2, 4, 2),
                            lambda ws, b: LIB.dgla_pinsage_select_fill(64, 2, 4, 2, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), ws, b,
                                                                       None), True),
    "exclude_set": ("exclude_set", lambda: LIB.dgla_exclude_set_workspace_bytes(64, N, 0),
                    lambda ws, b: LIB.dgla_exclude_set(64, ptr(SEEDS), N, None, NNZ, ptr(OUT[0]), ptr(I32), ws, b, None), False),
    "frontier_exclude": ("frontier_exclude", lambda: LIB.dgla_frontier_exclude_workspace_bytes(64, N, NNZ),
                         lambda ws, b: LIB.dgla_frontier_exclude(64, ptr(INDPTR), ptr(INDICES), ptr(INDICES), N, NNZ, ptr(SEEDS),
                                                                 1, ptr(OUT[0]), ptr(OUT[1]), ptr(OUT[2]), ws, b, None), False),
    "compact_nodes": ("compact_nodes", lambda: LIB.dgla_compact_nodes_workspace_bytes(64, N, NNZ),
                      lambda ws, b: LIB.dgla_compact_nodes(64, ptr(SEEDS), N, ptr(INDICES), NNZ, ptr(I32), N, ptr(OUT[0]),
                                                           ptr(OUT[1]), ptr(OUT[2]), ptr(I32), ws, b, None), False),
    "neighbor_matching": ("neighbor_matching", lambda: LIB.dgla_neighbor_matching_workspace_bytes(64, N),
                          lambda ws, b: LIB.dgla_neighbor_matching(ref(base()), None, 0, 7, 64, 0, ptr(OUT[0]),
                                                                   ctypes.byref(i64(0)), ws, b, None), False),
    "neighbor_matching_relabel": ("neighbor_matching_relabel", lambda: LIB.dgla_neighbor_matching_workspace_bytes(64, N),
                                  lambda ws, b: LIB.dgla_neighbor_matching_relabel(ptr(SEEDS), 64, N, ptr(OUT[0]), ws, b, None),
                                  False),
    "traverse": ("traverse", lambda: LIB.dgla_traverse_workspace_bytes(64, N),
                 lambda ws, b: LIB.dgla_traverse(BFS_NODES, ref(base()), None, ptr(SEEDS), 1, ptr(OUT[0]),
                                                 OUT[1].ctypes.data_as(ctypes.POINTER(i64)), ctypes.byref(i64(0)),
                                                 ctypes.byref(i64(0)), ws, b, None), False),
    "select_topk": ("select_topk", lambda: LIB.dgla_select_topk_workspace_bytes(64, N),
                    lambda ws, b: LIB.dgla_select_topk(ref(base()), ptr(W32), 0, ptr(SEEDS), N, 1, 0, ptr(OUT[0]), ptr(OUT[1]),
                                                       ptr(OUT[2]), ws, b, None), False),
}


@pytest.mark.parametrize("entry", sorted(WORKSPACES))
def test_short_and_missing_workspaces_are_refused_in_one_wording(entry):
    who, query, call, required = WORKSPACES[entry]
    need = query()
    assert need >= 256 and need % 256 == 0
    words = "%s: workspace of %d bytes required" % (who, need)
    assert call(ptr(SCRATCH), need - 256) == -1 and words in last_error(), (entry, last_error())
    if required:
        assert call(None, 0) == -1 and words in last_error(), (entry, last_error())
        assert call(None, need) == -1 and words in last_error(), (entry, last_error())   # a size without a pointer
