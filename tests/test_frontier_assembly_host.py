"""The graph that select_topk, sample_neighbors_biased and sample_etype_neighbors assemble from their picks, on CPU
graphs — runs without a GPU.

Every case calls the public function and, separately, the ``_capi.*_host`` entry it stands on; ``(src, dst, EID, gathered
edge feature)`` are then built here in plain torch from that call's ``(indptr, nbr, eids)`` and must equal the graph's.
The node features must be the tensors of the input graph themselves, and without ``copy_ndata`` / ``copy_edata`` the
frames hold nothing but ``EID``.  Both directions; a node listed twice, no node at all; ``k`` / ``fanout`` of 0 and -1."""
import pytest
import torch

import dgl_amd as dgl
from dgl_amd import _capi

N = 6
SRC = [0, 1, 2, 3, 4, 5, 0, 2, 4, 1, 3, 5, 0, 3]
DST = [1, 2, 3, 4, 5, 0, 2, 4, 0, 3, 5, 1, 3, 0]
NNZ = len(SRC)
ETYPE_OFFSET = [0, 6, NNZ]                      # edge ids 0..5 are type 0, 6..13 type 1
NODES = {"repeated": [2, 0, 2], "empty": [], "all": list(range(N))}
DIRS = ("in", "out")
EID = dgl.EID


def graph():
    g = dgl.graph((torch.tensor(SRC), torch.tensor(DST)), num_nodes=N)
    g.ndata["x"] = torch.arange(float(N)).reshape(N, 1) * 10
    g.edata["w"] = torch.tensor([(7 * e) % NNZ for e in range(NNZ)], dtype=torch.float32)      # all distinct
    return g


def host_view(rel, edge_dir, indices_data=None):
    indptr, indices, data = rel.csc() if edge_dir == "in" else rel.csr()
    if indices_data is not None:
        indices, data = indices_data
    return _capi.host_csr(indptr.contiguous(), indices.contiguous(), None if data is None else data.contiguous(),
                          rel.num_src if edge_dir == "in" else rel.num_dst)


def expected(seeds, rows, edge_dir, feature):
    """(src, dst, EID, feature at EID) of a CSR over `seeds`."""
    indptr, nbr, eids = rows
    counts = (indptr[1:] - indptr[:-1]).tolist()
    own = torch.tensor([s for s, c in zip(seeds.tolist(), counts) for _ in range(c)], dtype=seeds.dtype)
    n_e = sum(counts)
    assert n_e == int(indptr[-1])
    nbr, eids = nbr[:n_e], eids[:n_e]
    src, dst = (nbr, own) if edge_dir == "in" else (own, nbr)
    return src, dst, eids, feature[eids.long()]


def degrees(edge_dir, seeds):
    ends = DST if edge_dir == "in" else SRC
    return [ends.count(s) for s in seeds.tolist()]


def check(out, g, want, etid=0, copied=True):
    """`out` holds the edges `want` in relation `etid`, all nodes of `g`, and its features as asked."""
    src, dst, eids, feat = want
    row, col, _ = out._graph.relations[etid].coo()
    assert torch.equal(row, src) and torch.equal(col, dst) and row.is_contiguous() and col.is_contiguous()
    assert row.dtype == g.idtype and row.device == g.device
    frame = out._edge_frames[etid]
    assert torch.equal(frame[EID], eids) and frame[EID].dtype == g.idtype
    assert [out._graph.num_nodes(i) for i in range(len(g.ntypes))] == [g._graph.num_nodes(i) for i in range(len(g.ntypes))]
    assert out.ntypes == g.ntypes and out.canonical_etypes == g.canonical_etypes
    if copied:
        assert sorted(frame) == sorted(set(g._edge_frames[etid]) | {EID})
        for key, val in g._edge_frames[etid].items():
            if key != EID:
                assert torch.equal(frame[key], val[eids.long()])
        assert torch.equal(frame["w"], feat)
        for a, b in zip(out._node_frames, g._node_frames):
            assert sorted(a) == sorted(b) and all(a[key] is b[key] for key in b)        # the same tensors
    else:
        assert list(frame) == [EID] and all(len(f) == 0 for f in out._node_frames)


@pytest.mark.parametrize("k", [2, 0, -1])
@pytest.mark.parametrize("nodes", sorted(NODES))
@pytest.mark.parametrize("edge_dir", DIRS)
def test_select_topk(edge_dir, nodes, k):
    g = graph()
    seeds = torch.tensor(NODES[nodes], dtype=g.idtype)
    rows = _capi.select_topk_host(host_view(g._graph.relations[0], edge_dir), g.edata["w"], seeds, k)
    want = expected(seeds, rows, edge_dir, g.edata["w"])
    deg = degrees(edge_dir, seeds)
    assert want[2].shape[0] == sum(d if k < 0 else min(k, d) for d in deg)
    check(dgl.sampling.select_topk(g, k, "w", NODES[nodes], edge_dir=edge_dir), g, want)
    check(dgl.sampling.select_topk(g, k, "w", NODES[nodes], edge_dir=edge_dir, copy_ndata=False, copy_edata=False), g, want,
          copied=False)


def test_select_topk_on_two_relations_with_one_node_type_left_out():
    follow = (torch.tensor([0, 1, 2, 2, 3]), torch.tensor([1, 2, 0, 3, 0]))
    play = (torch.tensor([0, 1, 1, 3, 3, 2]), torch.tensor([0, 0, 1, 1, 0, 1]))
    hg = dgl.heterograph({("user", "follow", "user"): follow, ("user", "play", "game"): play})
    hg.nodes["user"].data["x"] = torch.arange(4.0)
    hg.nodes["game"].data["x"] = torch.arange(2.0)
    for etype, n in (("follow", 5), ("play", 6)):
        hg.edges[etype].data["w"] = torch.tensor([(3 * e) % n for e in range(n)], dtype=torch.float32)
    nodes = {"game": [1, 0, 1]}            # no "user": follow has no seed, and comes out empty
    out = dgl.sampling.select_topk(hg, 2, "w", nodes, edge_dir="in")
    for etid, (_, etype, d_t) in enumerate(hg.canonical_etypes):
        w = hg.edges[etype].data["w"]
        if d_t == "game":
            seeds = torch.tensor(nodes["game"], dtype=hg.idtype)
            rows = _capi.select_topk_host(host_view(hg._graph.relations[etid], "in"), w, seeds, 2)
            want = expected(seeds, rows, "in", w)
            assert want[2].shape[0] == 6
        else:
            none = torch.empty(0, dtype=hg.idtype)
            want = (none, none, none, w[:0])
        check(out, hg, want, etid)
    assert out.nodes["user"].data["x"] is hg.nodes["user"].data["x"] and out.nodes["game"].data["x"] is hg.nodes["game"].data["x"]


@pytest.mark.parametrize("fanout", [2, 0, -1])
@pytest.mark.parametrize("nodes", sorted(NODES))
@pytest.mark.parametrize("edge_dir", DIRS)
def test_sample_neighbors_biased(edge_dir, nodes, fanout):
    tag = torch.tensor([0, 1, 0, 1, 1, 0])
    g = (dgl.sort_csc_by_tag if edge_dir == "in" else dgl.sort_csr_by_tag)(graph(), tag)
    bias = torch.tensor([1.0, 3.0], dtype=torch.float64)
    seeds = torch.tensor(NODES[nodes], dtype=g.idtype)
    offsets = g.ndata["_TAG_OFFSET"].to(g.idtype).contiguous()
    rows = _capi.sample_neighbors_biased_host(host_view(g._graph.relations[0], edge_dir), offsets, bias, seeds, fanout, False, 11)
    want = expected(seeds, rows, edge_dir, g.edata["w"])
    if fanout == -1:
        assert want[2].shape[0] == sum(degrees(edge_dir, seeds))
    call = lambda **kw: dgl.sampling.sample_neighbors_biased(g, NODES[nodes], fanout, bias, edge_dir=edge_dir, seed=11, **kw)
    check(call(), g, want)
    check(call(copy_ndata=False, copy_edata=False), g, want, copied=False)


@pytest.mark.parametrize("fanout", [[2, 1], [0, 0], [-1, -1]], ids=str)
@pytest.mark.parametrize("nodes", sorted(NODES))
@pytest.mark.parametrize("edge_dir", DIRS)
def test_sample_etype_neighbors(edge_dir, nodes, fanout):
    g = graph()
    rel = g._graph.relations[0]
    seeds = torch.tensor(NODES[nodes], dtype=g.idtype)
    tag = (torch.arange(NNZ) >= ETYPE_OFFSET[1]).long()
    indices, data, _ = _capi.sort_csr_by_tag_host(host_view(rel, edge_dir), tag, 2)
    table = _capi.EtypeTable(ETYPE_OFFSET)
    rows = _capi.sample_etype_neighbors_host(host_view(rel, edge_dir, (indices, data)), table, table.fanouts(fanout), seeds,
                                             False, 5)
    want = expected(seeds, rows, edge_dir, g.edata["w"])
    if fanout == [-1, -1]:
        assert want[2].shape[0] == sum(degrees(edge_dir, seeds))
    call = lambda **kw: dgl.sampling.sample_etype_neighbors(g, NODES[nodes], ETYPE_OFFSET, torch.tensor(fanout),
                                                            edge_dir=edge_dir, seed=5, **kw)
    check(call(), g, want)
    check(call(copy_ndata=False, copy_edata=False), g, want, copied=False)
    check(call(_dist_training=True), g, want, copied=False)


def test_nodes_must_name_a_node_type_of_the_graph():
    hg = dgl.heterograph({("user", "play", "game"): (torch.tensor([0, 1]), torch.tensor([0, 0]))})
    hg.edges["play"].data["w"] = torch.tensor([1.0, 2.0])
    with pytest.raises(dgl.DGLError, match="Must specify node type when the graph is not homogeneous."):
        dgl.sampling.select_topk(hg, 1, "w", [0])
    with pytest.raises(dgl.DGLError, match='Node type "item" does not exist.'):
        dgl.sampling.select_topk(hg, 1, "w", {"item": [0]})
