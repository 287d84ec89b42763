"""Graph traversal, the rule run by the CPU (dgla_traverse_host, csrc/traversal.hip over csrc/traversal_step.h): equal,
element for element, to the independent sequential-queue model of tests/traversal_cases.py on every case, in all three
modes, both directions and both id types; every refusal by its message; the docstring examples of the reference; the
Python generators on a CPU graph; the depth-first names raise by name.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import traversal_cases as tc

CASES = tc.cases()
IDTYPES = [torch.int32, torch.int64]


def host_csr(csr, idtype):
    from dgl_amd import _capi

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(idtype)
    return _capi.host_csr(t(csr["indptr"]), t(csr["indices"]), t(csr["data"]), csr["n"])


def run_host(mode, csr, opposite=None, sources=None, idtype=torch.int64):
    from dgl_amd import _capi

    src = None if sources is None else torch.tensor(sources, dtype=idtype)
    ids, sections = _capi.traverse_host(mode, host_csr(csr, idtype), None if opposite is None else host_csr(opposite, idtype),
                                        src)
    assert ids.dtype == idtype
    return ids.numpy().astype(np.int64), sections


def check(got, frontiers, what):
    ids, sections = tc.flat(frontiers)
    assert got[1] == sections, what
    assert np.array_equal(got[0], ids), what


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_host_equals_the_queue_model(case):
    dirs = tc.directions(case)
    for reverse in (False, True):
        csr, opposite = dirs[reverse], dirs[not reverse]
        for sources in case["sources"]:
            for mode in (tc.BFS_NODES, tc.BFS_EDGES):
                want = tc.model(mode, csr, sources)
                assert all(len(f) > 0 for f in want)
                for idtype in IDTYPES:
                    check(run_host(mode, csr, None, sources, idtype), want, (case["name"], reverse, sources, mode, idtype))
        for idtype in IDTYPES:
            if case["topo"] == "loop":
                from dgl_amd import DGLAMDError

                with pytest.raises(ValueError):
                    tc.model(tc.TOPO_NODES, csr)
                with pytest.raises(DGLAMDError, match="loop detected"):
                    run_host(tc.TOPO_NODES, csr, opposite, None, idtype)
            else:
                check(run_host(tc.TOPO_NODES, csr, opposite, None, idtype), tc.model(tc.TOPO_NODES, csr),
                      (case["name"], reverse, "topo", idtype))


def test_the_table_covers_what_it_should():
    """The properties the cases were built for hold (so that a change of the table cannot quietly lose them)."""
    by = {c["name"]: c for c in CASES}
    assert len(tc.model(tc.BFS_NODES, tc.directions(by["path2000"])[False], [0])) == 2000
    star = tc.directions(by["star5000"])[False]
    assert star["data"] is None and int(np.diff(star["indptr"]).max()) == 5000 and 5000 % 64 != 0 and 5000 % 16 != 0
    assert tc.directions(by["reverse_star5000"])[True]["data"] is not None           # a non-trivial edge-id map
    lens = np.diff(tc.directions(by["row_lengths"])[False]["indptr"])[:300]
    assert set(lens.tolist()) == set(tc.ROW_LENGTHS)
    for name, wide in (("row_lengths", False), ("row_lengths_wide", True), ("bipartite70", True), ("star5000", False)):
        c = by[name]
        assert (c["src"].size // c["n"] > 32) == wide                                # both group widths are taken
    multi = by["multigraph"]
    pairs = list(zip(multi["src"].tolist(), multi["dst"].tolist()))
    assert len(set(pairs)) < len(pairs) and any(u == v for u, v in pairs)
    assert any(len(set(s)) < len(s) for c in CASES for s in c["sources"])            # duplicated sources
    assert {c["topo"] for c in CASES} == {"ok", "loop"}
    # layered: a node whose predecessors sit in different levels
    topo = tc.model(tc.TOPO_NODES, tc.directions(by["layered"])[False])
    level = {v: k for k, f in enumerate(topo) for v in f}
    preds = {level[u] for u, v in zip(by["layered"]["src"].tolist(), by["layered"]["dst"].tolist()) if v == 5}
    assert len(preds) > 1


def test_reference_docstring_examples():
    src, dst = tc.DOC_GRAPH
    out_csr, in_csr = tc.csr_of(6, src, dst), tc.csr_of(6, dst, src)
    check(run_host(tc.BFS_NODES, out_csr, None, [0]), tc.DOC_BFS_NODES, "bfs nodes")
    check(run_host(tc.BFS_EDGES, out_csr, None, [0]), tc.DOC_BFS_EDGES, "bfs edges")
    check(run_host(tc.TOPO_NODES, out_csr, in_csr), tc.DOC_TOPO, "topological")


def test_generators_on_a_cpu_graph():
    import dgl_amd as dgl

    src, dst = tc.DOC_GRAPH
    for idtype in IDTYPES:
        g = dgl.graph((torch.tensor(src), torch.tensor(dst)), num_nodes=6, idtype=idtype)
        for got, want in ((dgl.bfs_nodes_generator(g, 0), tc.DOC_BFS_NODES),
                          (dgl.bfs_edges_generator(g, torch.tensor([0])), tc.DOC_BFS_EDGES),
                          (dgl.topological_nodes_generator(g), tc.DOC_TOPO),
                          (dgl.traversal.bfs_nodes_generator(g, [5], reverse=True), [[5], [3], [1, 2], [0]]),
                          (dgl.topological_nodes_generator(g, reverse=True), [[4, 5], [3], [2], [1], [0]])):
            assert isinstance(got, tuple) and [f.tolist() for f in got] == want
            assert all(f.dtype == idtype and f.device.type == "cpu" for f in got)
        assert dgl.bfs_nodes_generator(g, []) == ()


def test_generators_follow_the_model_on_a_cpu_graph():
    import dgl_amd as dgl

    case = next(c for c in CASES if c["name"] == "trees64")
    g = dgl.graph((torch.from_numpy(case["src"]), torch.from_numpy(case["dst"])), num_nodes=case["n"])
    rel = g._graph.relations[0]
    for reverse, fmt in ((False, rel.csr()), (True, rel.csc())):
        csr = dict(n=case["n"], indptr=fmt[0].numpy(), indices=fmt[1].numpy(), data=None if fmt[2] is None else fmt[2].numpy())
        assert [f.tolist() for f in dgl.topological_nodes_generator(g, reverse)] == tc.model(tc.TOPO_NODES, csr)
        for s in case["sources"]:
            assert [f.tolist() for f in dgl.bfs_nodes_generator(g, s, reverse)] == tc.model(tc.BFS_NODES, csr, s)
            assert [f.tolist() for f in dgl.bfs_edges_generator(g, s, reverse)] == tc.model(tc.BFS_EDGES, csr, s)


def test_refusals():
    import dgl_amd as dgl
    from dgl_amd import DGLAMDError, _capi, _lib

    src, dst = tc.DOC_GRAPH
    out_csr, in_csr = tc.csr_of(6, src, dst), tc.csr_of(6, dst, src)
    with pytest.raises(DGLAMDError, match=r"a source lies outside \[0, 6\)"):
        run_host(tc.BFS_NODES, out_csr, None, [0, 6])
    with pytest.raises(DGLAMDError, match=r"a source lies outside \[0, 6\)"):
        run_host(tc.BFS_EDGES, out_csr, None, [-1])
    with pytest.raises(DGLAMDError, match="the count array does not match"):
        run_host(tc.TOPO_NODES, out_csr, tc.csr_of(5, [0], [1]))
    with pytest.raises(DGLAMDError, match="needs the opposite CSR"):
        run_host(tc.TOPO_NODES, out_csr, None)
    with pytest.raises(DGLAMDError, match="unknown mode 3"):
        run_host(3, out_csr, None, [0])
    # a NULL / invalid csr, straight at the C ABI
    n_ids, n_sec = ctypes.c_int64(0), ctypes.c_int64(0)
    ids, sections = torch.empty(8, dtype=torch.int64), (ctypes.c_int64 * 8)()
    srcs = torch.zeros(1, dtype=torch.int64)
    call = lambda csr: _lib.LIB.dgla_traverse_host(0, csr, None, srcs.data_ptr(), 1, ids.data_ptr(), sections,
                                                   ctypes.byref(n_ids), ctypes.byref(n_sec))
    assert call(None) == -1 and b"traverse_host: csr is null" in _lib.LIB.dgla_last_error()
    good = host_csr(out_csr, torch.int64)
    for change, msg in ((dict(indptr=None), b"invalid csr: indptr is null"), (dict(indices=None), b"invalid csr: indices is null"),
                        (dict(idtype_bits=16), b"idtype must be int32 or int64"), (dict(num_cols=7), b"needs a square CSR"),
                        (dict(nnz=-1), b"invalid csr: negative size")):
        bad = _lib.CSR(good.num_rows, good.num_cols, good.nnz, good.idtype_bits, good.indptr, good.indices, good.data)
        for k, v in change.items():
            setattr(bad, k, v)
        assert call(ctypes.byref(bad)) == -1 and msg in _lib.LIB.dgla_last_error(), msg
    broken = dict(out_csr, indptr=np.array([0, 1, 3, 2, 5, 6, 6]))
    with pytest.raises(DGLAMDError, match="invalid csr: indptr decreases at row 2"):
        run_host(tc.BFS_NODES, broken, None, [0])
    assert call(ctypes.byref(good)) == 0 and n_ids.value == 6                       # the library is still usable
    # the device form refuses the same before any launch (no GPU is touched)
    rc = _lib.LIB.dgla_traverse(0, None, None, None, 0, None, None, ctypes.byref(n_ids), ctypes.byref(n_sec), None, 0, None)
    assert rc == -1 and b"traverse: csr is null" in _lib.LIB.dgla_last_error()
    assert _capi.traverse_workspace_bytes(torch.int64, 0) == 0 and _capi.traverse_workspace_bytes(torch.int32, 1000) > 0
    # the Python surface
    g = dgl.graph((torch.tensor(src), torch.tensor(dst)), num_nodes=6)
    with pytest.raises(DGLAMDError, match=r"bfs_nodes_generator: a source lies outside \[0, 6\)"):
        dgl.bfs_nodes_generator(g, [9])
    loop = dgl.graph((torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])), num_nodes=3)
    with pytest.raises(DGLAMDError, match="topological_nodes_generator: loop detected"):
        dgl.topological_nodes_generator(loop)
    hetero = dgl.heterograph({("a", "x", "b"): ([0], [0]), ("b", "y", "a"): ([0], [0])})
    with pytest.raises(DGLAMDError, match="homogeneous"):
        dgl.bfs_nodes_generator(hetero, [0])
    with pytest.raises(DGLAMDError, match="homogeneous"):
        dgl.prop_nodes_topo(hetero, None, None)


def test_depth_first_names_raise_by_name():
    import dgl_amd as dgl
    from dgl_amd import DGLAMDError

    g = dgl.graph((torch.tensor([0]), torch.tensor([1])), num_nodes=2)
    with pytest.raises(DGLAMDError, match="dfs_edges_generator is absent"):
        dgl.traversal.dfs_edges_generator(g, 0)
    with pytest.raises(DGLAMDError, match="dfs_labeled_edges_generator is absent"):
        dgl.traversal.dfs_labeled_edges_generator(g, 0)
    with pytest.raises(DGLAMDError, match="prop_edges_dfs is absent"):
        dgl.propagate.prop_edges_dfs(g, 0, None, None)


def test_exports():
    import dgl_amd as dgl

    for name in ("bfs_nodes_generator", "bfs_edges_generator", "topological_nodes_generator", "prop_nodes", "prop_edges",
                 "prop_nodes_bfs", "prop_nodes_topo"):
        assert callable(getattr(dgl, name))
    assert callable(dgl.DGLGraph.prop_nodes) and callable(dgl.DGLGraph.prop_edges)
