"""Edge exclusion and compaction without a GPU: the host twins of csrc/exclude.hip (dgla_exclude_set_host,
dgla_frontier_exclude_host, dgla_compact_nodes_host) against the numpy model of tests/exclude_cases.py on every case
and both id widths, the refusals by message, and the surface that runs on CPU graphs: compact_graphs' torch path and
find_exclude_eids in every mode."""
import ctypes

import numpy as np
import pytest
import torch

from tests import exclude_cases as xc


def t_(a, idtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(idtype)


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_filter_twin_equals_the_model_and_is_idempotent(idtype):
    from dgl_amd import _capi

    for base in xc.BASES[idtype]:
        for short in (False, True):
            indptr, src, eids = xc.frontier(base, short)
            for name, x in xc.exclusion_lists(base):
                want = xc.model_filter(indptr, src, eids, x)
                got = _capi.frontier_exclude_host(t_(indptr, idtype), t_(src, idtype), t_(eids, idtype), t_(x, idtype))
                for a, b in zip(got, want):
                    assert a.dtype == idtype and np.array_equal(a.numpy(), b), (base, short, name)
                again = _capi.frontier_exclude_host(got[0], got[1].contiguous(), got[2].contiguous(), t_(x, idtype))
                for a, b in zip(again, got):
                    assert torch.equal(a, b), (base, short, name)
                if name == "all":
                    assert int(got[0][-1]) == 0
                if name == "empty":
                    assert int(got[0][-1]) == xc.NNZ


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_set_twin_equals_the_model(idtype):
    from dgl_amd import _capi

    for name, ids, rev, num_edges, flagged in xc.set_cases():
        want, want_flag = xc.model_set(ids, rev, num_edges)
        assert want_flag == flagged
        got, flags = _capi.exclude_set_host(t_(ids, idtype), num_edges, None if rev is None else t_(rev, idtype))
        assert got.dtype == idtype and np.array_equal(got.numpy(), want), name
        assert flags == (_capi.EXCLUDE_OUT_OF_RANGE if flagged else 0), name


def test_a_bad_id_is_not_read_through():
    """The reverse map handed over is SHORTER than the bad ids would need: the slot rule never indexes with them."""
    from dgl_amd import _capi

    rev = torch.tensor([1, 0], dtype=torch.int64)
    got, flags = _capi.exclude_set_host(torch.tensor([2, -1, 2 ** 40, 1], dtype=torch.int64), 2, rev)
    assert flags == _capi.EXCLUDE_OUT_OF_RANGE and got.tolist() == [0, 1, 2, 2, 2, 2, 2, 2]


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_compaction_twin_equals_the_model(idtype):
    from dgl_amd import _capi

    for name, preserve, ends, num_nodes in xc.compact_cases():
        local, nodes = xc.model_compact(preserve, ends, num_nodes)
        got = _capi.compact_nodes_host(t_(preserve, idtype), t_(ends, idtype), num_nodes)
        assert got[2] == 0, name
        assert got[0].dtype == idtype and np.array_equal(got[0].numpy(), local), name
        assert np.array_equal(got[1].numpy(), nodes), name
    local, nodes, flags = _capi.compact_nodes_host(t_([3, 10, -1], idtype), t_([3, 2], idtype), 10)
    assert flags == _capi.EXCLUDE_OUT_OF_RANGE and nodes.tolist() == [3, 2] and local.tolist() == [0, 1]


def test_refusals_by_message():
    from dgl_amd import _capi, _lib

    L = _lib.LIB
    err = lambda: L.dgla_last_error().decode()
    one = torch.zeros(4, dtype=torch.int64)
    fl = ctypes.c_int32(0)
    num = ctypes.c_int64(0)
    p = one.data_ptr()
    assert L.dgla_exclude_set_host(16, p, 1, None, 4, p, ctypes.byref(fl)) == -1 and "idtype must be int32 or int64" in err()
    assert L.dgla_exclude_set_host(64, p, -1, None, 4, p, ctypes.byref(fl)) == -1 and "negative size" in err()
    assert L.dgla_exclude_set_host(64, None, 1, None, 4, p, ctypes.byref(fl)) == -1 and "ids / out are null" in err()
    assert L.dgla_exclude_set_host(32, p, 1, None, 2 ** 31, p, ctypes.byref(fl)) == -1 and "does not fit" in err()
    assert L.dgla_exclude_set(64, p, 1, None, 4, p, None, None, 0, None) == -1 and "flags is null" in err()
    assert L.dgla_frontier_exclude_host(64, None, p, p, 1, 1, p, 1, p, p, p) == -1 and "indptr / out_indptr are null" in err()
    assert L.dgla_frontier_exclude_host(64, p, None, p, 1, 1, p, 1, p, p, p) == -1 and "src / eids" in err()
    assert L.dgla_frontier_exclude_host(64, p, p, p, 1, 1, None, 1, p, p, p) == -1 and "x is null" in err()
    assert L.dgla_frontier_exclude(8, p, p, p, 1, 1, p, 1, p, p, p, None, 0, None) == -1 and "idtype" in err()
    assert L.dgla_compact_nodes_host(64, None, 1, p, 1, 4, p, p, ctypes.byref(num), ctypes.byref(fl)) == -1 \
        and "preserve is null" in err()
    assert L.dgla_compact_nodes_host(64, p, 2 ** 30, p, 2 ** 30, 4, p, p, ctypes.byref(num), ctypes.byref(fl)) == -1 \
        and "below 2^31" in err()
    assert L.dgla_compact_nodes(64, p, 1, p, 1, None, 4, p, p, p, p, None, 0, None) == -1 and "node_map is null" in err()
    # the size queries: 0 for what the calls refuse, monotone otherwise
    assert L.dgla_exclude_set_workspace_bytes(16, 4, 0) == 0 and L.dgla_exclude_set_workspace_bytes(32, -1, 0) == 0
    assert 0 < L.dgla_exclude_set_workspace_bytes(32, 100000, 0) < L.dgla_exclude_set_workspace_bytes(32, 100000, 1) \
        < L.dgla_exclude_set_workspace_bytes(64, 100000, 1)
    assert L.dgla_frontier_exclude_workspace_bytes(16, 4, 4) == 0 and L.dgla_frontier_exclude_workspace_bytes(32, 4, -1) == 0
    assert 0 < L.dgla_frontier_exclude_workspace_bytes(32, 10, 100) < L.dgla_frontier_exclude_workspace_bytes(32, 10, 100000) \
        < L.dgla_frontier_exclude_workspace_bytes(32, 100000, 100000)
    assert L.dgla_compact_nodes_workspace_bytes(32, 2 ** 30, 2 ** 30) == 0
    assert 0 < L.dgla_compact_nodes_workspace_bytes(32, 10, 1000) < L.dgla_compact_nodes_workspace_bytes(64, 10, 100000)
    # the wrappers: a tensor of another width, a GPU entry point on CPU tensors
    with pytest.raises(_lib.DGLAMDError, match="one id type"):
        _capi.frontier_exclude_host(one, one, one, one.int())
    with pytest.raises(_lib.DGLAMDError, match="ROCm GPU"):
        _capi.frontier_exclude(one, one, one, one)
    with pytest.raises(_lib.DGLAMDError, match="ROCm GPU"):
        _capi.exclude_set(one, 10)


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_compact_graphs_on_cpu_graphs(idtype):
    import dgl_amd as dgl

    graphs = xc.doc_graphs(idtype)
    out = dgl.compact_graphs(graphs)
    for k, new in enumerate(out):
        assert new.idtype == idtype and new.ntypes == graphs[0].ntypes
        for n, want in xc.DOC_NID.items():
            assert new.nodes[n].data[dgl.NID].tolist() == want and new.num_nodes(n) == len(want)
        u, v = new.edges(etype="plays")
        assert (u.tolist(), v.tolist()) == xc.DOC_EDGES[k]
        assert torch.equal(new.nodes["user"].data["h"], graphs[k].nodes["user"].data["h"][xc.DOC_NID["user"]])
        assert torch.equal(new.edges["plays"].data["w"], graphs[k].edges["plays"].data["w"])
    bare = dgl.compact_graphs(graphs[0], copy_ndata=False, copy_edata=False)
    assert "h" not in bare.nodes["user"].data and "w" not in bare.edges["plays"].data
    assert bare.nodes["user"].data[dgl.NID].tolist() == [1, 3] and bare.nodes["game"].data[dgl.NID].tolist() == [3, 5]
    # no edges at all: zero nodes
    empty = dgl.graph((torch.empty(0, dtype=idtype), torch.empty(0, dtype=idtype)), num_nodes=9, idtype=idtype)
    assert dgl.compact_graphs(empty).num_nodes() == 0
    assert dgl.compact_graphs(empty, always_preserve=[4, 4, 1]).ndata[dgl.NID].tolist() == [4, 1]
    # three relations over two node types, with and without preserved ids
    g3 = xc.three_relation_graph(idtype)
    for keep, want in ((None, xc.THREE_NID), ({"a": torch.tensor([11, 9, 11])}, xc.THREE_NID_PRESERVED)):
        new = dgl.compact_graphs(g3, always_preserve=keep)
        for n in g3.ntypes:
            nid = new.nodes[n].data[dgl.NID]
            assert nid.tolist() == want[n]
            for c in g3.canonical_etypes:       # the edges are the input's, in its order, through NID
                u, v = new.edges(etype=c)
                u0, v0 = g3.edges(etype=c)
                assert torch.equal(new.nodes[c[0]].data[dgl.NID][u.long()], u0)
                assert torch.equal(new.nodes[c[2]].data[dgl.NID][v.long()], v0)
    # a homogeneous graph: an isolated node, a repeated id and an id that is also an end point
    g = dgl.graph((torch.tensor([6, 1, 7], dtype=idtype), torch.tensor([1, 3, 6], dtype=idtype)), num_nodes=10, idtype=idtype)
    assert dgl.compact_graphs(g, always_preserve=torch.tensor([8, 2, 6, 2])).ndata[dgl.NID].tolist() == [8, 2, 6, 1, 3, 7]


def test_compact_graphs_refusals():
    import dgl_amd as dgl

    g = dgl.graph((torch.tensor([0, 1]), torch.tensor([1, 2])), num_nodes=5)
    with pytest.raises(dgl.DGLError, match="node id out of range"):
        dgl.compact_graphs(g, always_preserve=[5])
    with pytest.raises(dgl.DGLError, match="node id out of range"):
        dgl.compact_graphs(g, always_preserve=[-1])
    with pytest.raises(dgl.DGLError, match="number of nodes"):
        dgl.compact_graphs([g, dgl.graph((torch.tensor([0]), torch.tensor([1])), num_nodes=6)])
    with pytest.raises(dgl.DGLError, match="same idtype and device"):
        dgl.compact_graphs([g, dgl.graph((torch.tensor([0]), torch.tensor([1])), num_nodes=5, idtype=torch.int32)])
    with pytest.raises(dgl.DGLError, match="same node types"):
        dgl.compact_graphs([g, xc.three_relation_graph(torch.int64)])
    with pytest.raises(dgl.DGLError, match="does not exist"):
        dgl.compact_graphs(g, always_preserve={"nope": [1]})
    blk = dgl.create_block((torch.tensor([0, 1]), torch.tensor([0, 0])), num_src_nodes=2, num_dst_nodes=1)
    with pytest.raises(dgl.DGLError, match="a block is refused"):
        dgl.compact_graphs(blk)
    assert dgl.compact_graphs([]) == []


def test_find_exclude_eids_every_mode():
    import dgl_amd as dgl
    from dgl_amd.dataloading import find_exclude_eids

    g, rev = xc.symmetric_graph(torch.int64, "cpu", num_nodes=30, half=50)
    seeds = torch.tensor([3, 77, 3, 49])
    assert find_exclude_eids(g, seeds, None) is None
    assert find_exclude_eids(g, seeds, "self") is seeds
    assert find_exclude_eids(g, seeds, "reverse_id", reverse_eids=rev).tolist() == [3, 3, 27, 49, 53, 53, 77, 99]
    given = torch.tensor([1, 2])
    assert find_exclude_eids(g, seeds, given) is given
    assert find_exclude_eids(g, seeds, lambda s: s + 1).tolist() == [4, 78, 4, 50]
    with pytest.raises(ValueError, match="unsupported mode"):
        find_exclude_eids(g, seeds, "nope")
    with pytest.raises(dgl.DGLError, match="edge id out of range"):
        find_exclude_eids(g, torch.tensor([100]), "reverse_id", reverse_eids=rev)
    with pytest.raises(dgl.DGLError, match="needs reverse_eids"):
        find_exclude_eids(g, seeds, "reverse_id")
    # a relation and its reverse: the same ids under the other type, two lists of one type concatenated
    h = dgl.heterograph({("u", "ab", "v"): (torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])),
                         ("v", "ba", "u"): (torch.tensor([1, 2, 0]), torch.tensor([0, 1, 2]))}, {"u": 3, "v": 3})
    maps = {"ab": "ba", "ba": "ab"}
    out = find_exclude_eids(h, {"ab": torch.tensor([2, 0])}, "reverse_types", reverse_etypes=maps)
    assert {k: v.tolist() for k, v in out.items()} == {("u", "ab", "v"): [2, 0], ("v", "ba", "u"): [2, 0]}
    out = find_exclude_eids(h, {"ab": torch.tensor([2]), "ba": torch.tensor([1, 2])}, "reverse_types", reverse_etypes=maps)
    assert {k: sorted(v.tolist()) for k, v in out.items()} == {("u", "ab", "v"): [1, 2, 2], ("v", "ba", "u"): [1, 2, 2]}
    out = find_exclude_eids(h, {"ab": torch.tensor([2])}, "reverse_id", reverse_eids={"ab": torch.tensor([0, 1, 2])})
    assert {k: v.tolist() for k, v in out.items()} == {("u", "ab", "v"): [2, 2]}


def test_the_edge_sampler_checks_the_wrapped_sampler():
    from dgl_amd import dataloading as dl

    class NodeOnly:
        output_device = None

        def sample(self, g, seed_nodes):
            return seed_nodes, seed_nodes, []

    with pytest.raises(TypeError, match="does not support edge or link prediction"):
        dl.as_edge_prediction_sampler(NodeOnly())
    for cls in (dl.NeighborSampler, dl.LaborSampler):
        s = dl.as_edge_prediction_sampler(cls([2]), exclude="self", prefetch_labels=["y"])
        assert isinstance(s, dl.EdgePredictionSampler) and s.output_device is None and s.sampler.output_device is None
    assert dl.as_edge_prediction_sampler(dl.ShaDowKHopSampler([2])).output_device is None
    assert dl.negative_sampler.PerSourceUniform is not None and dl.SAINTSampler is not None
