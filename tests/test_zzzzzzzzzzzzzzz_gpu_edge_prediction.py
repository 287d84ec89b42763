"""Link-prediction batches on the device (csrc/exclude.hip): device == host twins bit for bit on every case of
tests/exclude_cases.py (both id widths, both lane-group widths, with and without a caller's workspace), the refusals,
blocks with excluded edges against the exact model of tests/neighbor_cases.py (picks, then drop, then the block rule),
the edge-wise sampler in every exclusion mode, and compact_graphs on GPU graphs against its CPU path."""

import numpy as np
import pytest
import torch

from tests import exclude_cases as xc
from tests import neighbor_cases as nc

pytestmark = pytest.mark.gpu


def t_(a, idtype, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(idtype)
    return t if dev is None else t.to(dev)


def _bits(idtype):
    return 32 if idtype == torch.int32 else 64


# ---- kernels against twins ----------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [False, True], ids=["64_lanes", "16_lanes"])
@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_filter_equals_the_host_twin(dev, idtype, short):
    from dgl_amd import _capi, _lib

    for base in xc.BASES[idtype]:
        indptr, src, eids = (t_(a, idtype) for a in xc.frontier(base, short))
        d = [a.to(dev) for a in (indptr, src, eids)]
        need = _lib.LIB.dgla_frontier_exclude_workspace_bytes(_bits(idtype), indptr.shape[0] - 1, src.shape[0])
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        for name, x in xc.exclusion_lists(base):
            want = _capi.frontier_exclude_host(indptr, src, eids, t_(x, idtype))
            for workspace in (None, ws):
                got = _capi.frontier_exclude(*d, t_(x, idtype, dev), workspace=workspace)
                total = int(got[0][-1])
                assert got[1].shape[0] == src.shape[0]          # allocated at the upper bound
                for a, b in zip((got[0], got[1][:total], got[2][:total]), want):
                    assert a.dtype == idtype and torch.equal(a.cpu(), b), (base, name, workspace is not None)
        with pytest.raises(_lib.DGLAMDError, match="frontier_exclude: workspace of %d bytes required" % need):
            _capi.frontier_exclude(*d, t_(x, idtype, dev), workspace=ws[:need - 256])


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_filter_on_empty_frontiers(dev, idtype):
    from dgl_amd import _capi

    e = torch.empty(0, dtype=idtype, device=dev)
    x = torch.tensor([1, 2], dtype=idtype, device=dev)
    got = _capi.frontier_exclude(torch.zeros(1, dtype=idtype, device=dev), e, e, x)          # no rows
    assert got[0].tolist() == [0] and got[1].numel() == 0
    got = _capi.frontier_exclude(torch.zeros(4, dtype=idtype, device=dev), e, e, x)          # rows without entries
    assert got[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_set_equals_the_host_twin(dev, idtype):
    from dgl_amd import _capi, _lib

    for name, ids, rev, num_edges, flagged in xc.set_cases():
        h_ids, h_rev = t_(ids, idtype), None if rev is None else t_(rev, idtype)
        want, want_flags = _capi.exclude_set_host(h_ids, num_edges, h_rev)
        d_ids, d_rev = h_ids.to(dev), None if rev is None else h_rev.to(dev)
        if flagged:     # the wrapper refuses by name; the raw call writes what the twin writes
            with pytest.raises(_lib.DGLAMDError, match="edge id out of range"):
                _capi.exclude_set(d_ids, num_edges, d_rev)
            out = torch.empty(want.shape[0], dtype=idtype, device=dev)
            flags = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check_call(_lib.LIB.dgla_exclude_set(_bits(idtype), d_ids.data_ptr(), d_ids.shape[0],
                                                      None if d_rev is None else d_rev.data_ptr(), num_edges, out.data_ptr(),
                                                      flags.data_ptr(), None, 0, torch.cuda.current_stream(dev).cuda_stream))
            assert int(flags.item()) == want_flags == _capi.EXCLUDE_OUT_OF_RANGE and torch.equal(out.cpu(), want), name
            continue
        need = _lib.LIB.dgla_exclude_set_workspace_bytes(_bits(idtype), len(ids), 0 if rev is None else 1)
        for workspace in (None, torch.empty(need, dtype=torch.uint8, device=dev)):
            got = _capi.exclude_set(d_ids, num_edges, d_rev, workspace=workspace)
            assert got.dtype == idtype and torch.equal(got.cpu(), want), name
        if len(ids):
            with pytest.raises(_lib.DGLAMDError, match="exclude_set: workspace of %d bytes required" % need):
                _capi.exclude_set(d_ids, num_edges, d_rev, workspace=torch.empty(8, dtype=torch.uint8, device=dev))
    # more keys than the one-workgroup sort holds, and ids near the top of the id range
    rng = np.random.default_rng(186)
    top = 2 ** 31 - 1 if idtype == torch.int32 else 2 ** 62 + 12345
    ids = t_(top - 1 - rng.integers(0, 50000, 20000), idtype)
    want, flags = _capi.exclude_set_host(ids, top)
    assert flags == 0 and torch.equal(_capi.exclude_set(ids.to(dev), top).cpu(), want)


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_a_workspace_256_bytes_short_is_refused(dev, idtype):
    """need - 256 bytes: exclude_set and compact_nodes refuse it in the one wording, before any launch."""
    from dgl_amd import _capi, _lib

    name, ids, rev, num_edges, _ = next(c for c in xc.set_cases() if len(c[1]) and not c[4])
    need = _lib.LIB.dgla_exclude_set_workspace_bytes(_bits(idtype), len(ids), 0 if rev is None else 1)
    assert need > 256
    with pytest.raises(_lib.DGLAMDError, match="exclude_set: workspace of %d bytes required, got %d" % (need, need - 256)):
        _capi.exclude_set(t_(ids, idtype, dev), num_edges, None if rev is None else t_(rev, idtype, dev),
                          workspace=torch.empty(need - 256, dtype=torch.uint8, device=dev))
    name, preserve, ends, num_nodes = next(c for c in xc.compact_cases() if len(c[1]) + len(c[2]))
    node_map = torch.full((num_nodes,), -1, dtype=torch.int32, device=dev)
    need = _lib.LIB.dgla_compact_nodes_workspace_bytes(_bits(idtype), len(preserve), len(ends))
    assert need > 256
    with pytest.raises(_lib.DGLAMDError, match="compact_nodes: workspace of %d bytes required, got %d" % (need, need - 256)):
        _capi.compact_nodes(t_(preserve, idtype, dev), t_(ends, idtype, dev), node_map,
                            workspace=torch.empty(need - 256, dtype=torch.uint8, device=dev))
    assert bool((node_map == -1).all()), name


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_compaction_equals_the_host_twin_and_cleans_the_map(dev, idtype):
    from dgl_amd import _capi, _lib

    for name, preserve, ends, num_nodes in xc.compact_cases():
        node_map = torch.full((num_nodes,), -1, dtype=torch.int32, device=dev)
        want = _capi.compact_nodes_host(t_(preserve, idtype), t_(ends, idtype), num_nodes)
        need = _lib.LIB.dgla_compact_nodes_workspace_bytes(_bits(idtype), len(preserve), len(ends))
        for workspace in (None, torch.empty(need, dtype=torch.uint8, device=dev)):
            got = _capi.compact_nodes(t_(preserve, idtype, dev), t_(ends, idtype, dev), node_map, workspace=workspace)
            assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), name
            assert bool((node_map == -1).all()), name
        with pytest.raises(_lib.DGLAMDError, match="compact_nodes: workspace of %d bytes required" % need):
            _capi.compact_nodes(t_(preserve, idtype, dev), t_(ends, idtype, dev), node_map,
                                workspace=torch.empty(8, dtype=torch.uint8, device=dev))
        assert bool((node_map == -1).all()), name
    node_map = torch.full((10,), -1, dtype=torch.int32, device=dev)
    for bad in (10, -1):
        with pytest.raises(_lib.DGLAMDError, match="node id out of range"):
            _capi.compact_nodes(t_([3, bad, 3], idtype, dev), t_([3, 2], idtype, dev), node_map)
        assert bool((node_map == -1).all())


# ---- blocks against the model -------------------------------------------------------------------------------
def _host_csc(g, etid=0):
    """The in-edge CSR of relation `etid` as the dict tests/neighbor_cases.py models."""
    rel = g._graph.relations[etid]
    indptr, indices, eids = rel.csc()
    G = {"indptr": indptr.cpu().numpy().astype(np.int64), "indices": indices.cpu().numpy().astype(np.int64),
         "num_rows": rel.num_dst, "num_cols": rel.num_src}
    G["eids"] = eids.cpu().numpy().astype(np.int64) if eids is not None else np.arange(len(G["indices"]), dtype=np.int64)
    return G


def _model_frontier(G, seeds, fanout, S, x, prob=None):
    """(src, own, eids) of one relation: the model's picks, then the entries whose edge id is in x dropped."""
    if prob is None:
        indptr, gpos = nc.model_uniform(G, seeds, fanout, False, S)
    else:
        indptr, gpos = nc.model_weighted(G, prob, seeds, fanout, False, S, True)
    src, eids = nc.gather(G, gpos, True)
    own = np.repeat(np.arange(len(seeds)), np.diff(indptr))
    keep = ~np.isin(eids, x) if x is not None else np.ones(len(eids), dtype=bool)
    return src[keep], own[keep], eids[keep]


def _model_blocks(G, seeds, fanouts, sampler_seed, x, prob=None):
    out = []
    for layer, fanout in enumerate(reversed(fanouts)):
        S = (sampler_seed * 1000003) * 64 + layer           # a fresh sampler's first call
        src, own, eids = _model_frontier(G, seeds, fanout, S, x, prob)
        local, src_nodes = nc.model_block(seeds, src)
        out.insert(0, (src_nodes, seeds, local, own, eids))
        seeds = src_nodes
    return out


def _same_blocks(blocks, model):
    import dgl_amd as dgl

    assert len(blocks) == len(model)
    for blk, (src_nodes, dst_nodes, local, own, eids) in zip(blocks, model):
        assert np.array_equal(blk.srcdata[dgl.NID].cpu().numpy(), src_nodes)
        assert np.array_equal(blk.dstdata[dgl.NID].cpu().numpy(), dst_nodes)
        assert np.array_equal(blk.edata[dgl.EID].cpu().numpy(), eids)
        u, v = blk.edges()
        assert np.array_equal(u.cpu().numpy(), local) and np.array_equal(v.cpu().numpy(), own)


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "prob"])
@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_blocks_with_excluded_edges_equal_the_model(dev, idtype, weighted):
    import dgl_amd as dgl

    g, rev = xc.symmetric_graph(idtype, dev)
    G = _host_csc(g)
    rng = np.random.default_rng(187)
    prob = None
    if weighted:
        prob = rng.integers(0, 17, g.num_edges()) / 8.0         # (about 6 % zero weights)
        g.edata["p"] = torch.from_numpy(prob).to(dev)
    seed_nodes = rng.permutation(200)[:40].astype(np.int64)
    # the in-edges of the first seeds and their reverses: every one of them would be picked somewhere
    first = np.concatenate([G["eids"][G["indptr"][r]:G["indptr"][r + 1]] for r in seed_nodes[:12]])
    x = np.concatenate([first, (first + 1000) % 2000])
    seeds = t_(seed_nodes, idtype, dev)
    for s in (0, 5):
        make = lambda: dgl.NeighborSampler([3, 2], seed=s, prob="p" if weighted else None)
        got = make().sample_blocks(g, seeds, exclude_eids=t_(x, idtype, dev))
        model = _model_blocks(G, seed_nodes, [3, 2], s, x, prob)
        assert np.array_equal(got[0].cpu().numpy(), model[0][0]) and torch.equal(got[1], seeds)
        _same_blocks(got[2], model)
        assert not np.isin(np.concatenate([m[4] for m in model]), x).any()
        assert any(len(m[4]) < len(m0[4]) for m, m0 in zip(model, _model_blocks(G, seed_nodes, [3, 2], s, None, prob)))
        # exclude_eids=None is the call without the argument, and sample() is sample_blocks()
        plain, none, via = make().sample_blocks(g, seeds), make().sample_blocks(g, seeds, exclude_eids=None), \
            make().sample(g, seeds, None)
        _same_blocks(plain[2], _model_blocks(G, seed_nodes, [3, 2], s, None, prob))
        for other in (none, via):
            assert torch.equal(other[0], plain[0])
            for a, b in zip(other[2], plain[2]):
                assert torch.equal(a.srcdata[dgl.NID], b.srcdata[dgl.NID]) and torch.equal(a.edata[dgl.EID], b.edata[dgl.EID])
                assert all(torch.equal(p, q) for p, q in zip(a.edges(), b.edges()))
    # the frontier alone, and the refusals
    fr = dgl.sampling.sample_neighbors(g, seeds, 3, seed=11, exclude_edges=t_(x, idtype, dev))
    src, own, eids = _model_frontier(G, seed_nodes, 3, 11, x)
    assert np.array_equal(fr.edata[dgl.EID].cpu().numpy(), eids)
    assert np.array_equal(fr.edges()[0].cpu().numpy(), src) and np.array_equal(fr.edges()[1].cpu().numpy(), seed_nodes[own])
    with pytest.raises(dgl.DGLError, match="edge id out of range"):
        dgl.NeighborSampler([2]).sample_blocks(g, seeds, exclude_eids=t_([2000], idtype, dev))
    with pytest.raises(dgl.DGLError, match="sample_blocks_padded: exclude_eids is not supported"):
        dgl.NeighborSampler([2]).sample_blocks_padded(g, seeds, exclude_eids=t_([1], idtype, dev))
    with pytest.raises(dgl.DGLError, match="sample_neighbors_fused: exclude_edges is not supported"):
        dgl.sampling.sample_neighbors_fused(g, seeds, 2, exclude_edges=t_([1], idtype, dev))


def _two_relation_graph(idtype, dev):
    import dgl_amd as dgl

    rng = np.random.default_rng(188)
    u, v = rng.integers(0, 60, 400), rng.integers(0, 50, 400)
    t = lambda a: torch.from_numpy(a).to(idtype)
    return dgl.heterograph({("u", "ab", "v"): (t(u), t(v)), ("v", "ba", "u"): (t(v), t(u))}, {"u": 60, "v": 50},
                           idtype=idtype, device=dev)


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_hetero_blocks_with_a_dict_of_lists_equal_the_model(dev, idtype):
    """Two relations, a list per relation.  The block's source nodes are compared in order; a relation's edges are
    compared as (source id, destination id, edge id) triples in ascending edge id, which is unique without replacement."""
    import dgl_amd as dgl

    g = _two_relation_graph(idtype, dev)
    cets = g.canonical_etypes
    Gs = [_host_csc(g, i) for i in range(len(cets))]
    rng = np.random.default_rng(189)
    seeds = {"u": rng.permutation(60)[:15].astype(np.int64), "v": rng.permutation(50)[:15].astype(np.int64)}
    x = {c: np.concatenate([Gs[i]["eids"][Gs[i]["indptr"][r]:Gs[i]["indptr"][r + 1]] for r in seeds[c[2]][:6]])
         for i, c in enumerate(cets)}
    s = 3
    got = dgl.NeighborSampler([3, 2], seed=s).sample_blocks(
        g, {n: t_(v, idtype, dev) for n, v in seeds.items()}, exclude_eids={c[1]: t_(v, idtype, dev) for c, v in x.items()})
    cur, model, hits = seeds, [], 0
    for layer, fanout in enumerate(reversed([3, 2])):
        S = (s * 1000003) * 64 + layer
        fr = {c: _model_frontier(Gs[i], cur[c[2]], fanout, S * 131 + i, x[c]) for i, c in enumerate(cets)}
        hits += sum(int(np.isin(_model_frontier(Gs[i], cur[c[2]], fanout, S * 131 + i, None)[2], x[c]).sum())
                    for i, c in enumerate(cets))
        src_nodes = {n: np.concatenate([cur[n], np.setdiff1d(np.concatenate([fr[c][0] for c in cets if c[0] == n]), cur[n])])
                     for n in g.ntypes}
        model.insert(0, (src_nodes, cur, fr))
        cur = src_nodes
    for n in g.ntypes:
        assert np.array_equal(got[0][n].cpu().numpy(), model[0][0][n])
    assert hits > 0         # (the lists do drop picks)
    for blk, (src_nodes, dst_nodes, fr) in zip(got[2], model):
        for n in g.ntypes:
            assert np.array_equal(blk.srcnodes[n].data[dgl.NID].cpu().numpy(), src_nodes[n])
            assert np.array_equal(blk.dstnodes[n].data[dgl.NID].cpu().numpy(), dst_nodes[n])
        for c in cets:
            src, own, eids = fr[c]
            u, v = (a.cpu().numpy() for a in blk.edges(etype=c))
            e = blk.edges[c].data[dgl.EID].cpu().numpy()
            o, mo = np.argsort(e, kind="stable"), np.argsort(eids, kind="stable")
            assert np.array_equal(e[o], eids[mo])
            assert np.array_equal(src_nodes[c[0]][u[o]], src[mo]) and np.array_equal(dst_nodes[c[2]][v[o]], dst_nodes[c[2]][own[mo]])
            assert not np.isin(e, x[c]).any()


# ---- the edge sampler ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "self", "reverse_id", "tensor", "callable"])
@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_edge_prediction_sampler(dev, idtype, mode):
    import dgl_amd as dgl
    from dgl_amd import dataloading as dl

    g, rev = xc.symmetric_graph(idtype, dev)
    rng = np.random.default_rng(190)
    seed_eids = t_(rng.permutation(2000)[:64], idtype, dev)
    given = t_(np.arange(0, 2000, 3), idtype, dev)
    exclude = {"tensor": given, "callable": (lambda s: torch.cat([s, s + 1]) % 2000)}.get(mode, mode)
    expected = {None: torch.empty(0, dtype=idtype, device=dev), "self": seed_eids,
                "reverse_id": torch.cat([seed_eids, rev[seed_eids.long()]]), "tensor": given,
                "callable": torch.cat([seed_eids, seed_eids + 1]) % 2000}[mode]
    neg = dgl.negative_sampler.PerSourceUniform(2)
    for sampler in (dl.NeighborSampler([3, 2], seed=2), dl.LaborSampler([3, 2], seed=2)):
        es = dl.as_edge_prediction_sampler(sampler, exclude=exclude, reverse_eids=rev if mode == "reverse_id" else None,
                                           negative_sampler=neg)
        torch.manual_seed(77)
        want_neg = neg(g, seed_eids)
        torch.manual_seed(77)
        input_nodes, pair_graph, neg_graph, blocks = es.sample(g, seed_eids)
        for blk in blocks:
            assert not torch.isin(blk.edata[dgl.EID], expected).any()
        nid = pair_graph.ndata[dgl.NID]
        assert torch.equal(blocks[-1].dstdata[dgl.NID], nid) and torch.equal(neg_graph.ndata[dgl.NID], nid)
        assert torch.equal(input_nodes, blocks[0].srcdata[dgl.NID])
        assert nid.unique().shape[0] == nid.shape[0]
        u, v = pair_graph.edges()
        u0, v0 = g.find_edges(seed_eids)
        assert torch.equal(nid[u.long()], u0) and torch.equal(nid[v.long()], v0)
        assert torch.equal(pair_graph.edata[dgl.EID], seed_eids)
        nu, nv = neg_graph.edges()
        assert torch.equal(nid[nu.long()], want_neg[0]) and torch.equal(nid[nv.long()], want_neg[1])
        # without a negative sampler: three results, the same pair graph edges
        es = dl.as_edge_prediction_sampler(type(sampler)([3, 2], seed=2), exclude=exclude,
                                           reverse_eids=rev if mode == "reverse_id" else None)
        input_nodes, pair_only, blocks = es.sample(g, seed_eids)
        assert torch.equal(pair_only.ndata[dgl.NID][pair_only.edges()[0].long()], u0)
        assert torch.equal(blocks[-1].dstdata[dgl.NID], pair_only.ndata[dgl.NID])


@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_reverse_types_on_a_relation_and_its_reverse(dev, idtype):
    import dgl_amd as dgl
    from dgl_amd import dataloading as dl

    g = _two_relation_graph(idtype, dev)        # edge e of "ba" is the reverse of edge e of "ab"
    seed_eids = {"ab": t_(np.arange(0, 400, 7), idtype, dev)}
    es = dl.as_edge_prediction_sampler(dl.NeighborSampler([4, 4], seed=1), exclude="reverse_types",
                                       reverse_etypes={"ab": "ba", "ba": "ab"})
    input_nodes, pair_graph, blocks = es.sample(g, seed_eids)
    for blk in blocks:
        for c in g.canonical_etypes:
            assert not torch.isin(blk.edges[c].data[dgl.EID], seed_eids["ab"]).any()
    plain = dl.NeighborSampler([4, 4], seed=1).sample_blocks(g, {n: pair_graph.nodes[n].data[dgl.NID] for n in g.ntypes})
    assert any(torch.isin(b.edges[c].data[dgl.EID], seed_eids["ab"]).any() for b in plain[2] for c in g.canonical_etypes)
    ab = ("u", "ab", "v")
    u, v = pair_graph.edges(etype=ab)
    u0, v0 = g.find_edges(seed_eids["ab"], etype=ab)
    assert torch.equal(pair_graph.nodes["u"].data[dgl.NID][u.long()], u0)
    assert torch.equal(pair_graph.nodes["v"].data[dgl.NID][v.long()], v0)
    assert torch.equal(pair_graph.edges[ab].data[dgl.EID], seed_eids["ab"])
    assert pair_graph.num_edges(("v", "ba", "u")) == 0
    for n in g.ntypes:
        assert torch.equal(blocks[-1].dstnodes[n].data[dgl.NID], pair_graph.nodes[n].data[dgl.NID])
        assert torch.equal(input_nodes[n], blocks[0].srcnodes[n].data[dgl.NID])


def test_a_sampler_without_the_third_argument_is_refused():
    from dgl_amd import dataloading as dl

    class NodeOnly:
        def sample(self, g, seed_nodes):
            return seed_nodes, seed_nodes, []

    with pytest.raises(TypeError, match="does not support edge or link prediction"):
        dl.as_edge_prediction_sampler(NodeOnly())


# ---- compact_graphs on GPU graphs ---------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", xc.IDTYPES, ids=str)
def test_compact_graphs_on_gpu_equals_the_cpu_path(dev, idtype):
    import dgl_amd as dgl

    def same(a, b):
        assert a.ntypes == b.ntypes and a.canonical_etypes == b.canonical_etypes and a.device.type == "cuda"
        for n in a.ntypes:
            assert a.num_nodes(n) == b.num_nodes(n)
            fa, fb = a.nodes[n].data, b.nodes[n].data
            assert set(fa.keys()) == set(fb.keys())
            for k in fa.keys():
                assert torch.equal(fa[k].cpu(), fb[k])
        for c in a.canonical_etypes:
            for p, q in zip(a.edges(etype=c), b.edges(etype=c)):
                assert torch.equal(p.cpu(), q)
            fa, fb = a.edges[c].data, b.edges[c].data
            assert set(fa.keys()) == set(fb.keys())
            for k in fa.keys():
                assert torch.equal(fa[k].cpu(), fb[k])

    for a, b in zip(dgl.compact_graphs(xc.doc_graphs(idtype, dev)), dgl.compact_graphs(xc.doc_graphs(idtype))):
        same(a, b)
        assert {n: a.nodes[n].data[dgl.NID].tolist() for n in a.ntypes} == xc.DOC_NID
    for keep in (None, {"a": [11, 9, 11]}):
        same(dgl.compact_graphs(xc.three_relation_graph(idtype, dev), always_preserve=keep),
             dgl.compact_graphs(xc.three_relation_graph(idtype), always_preserve=keep))
    g, _ = xc.symmetric_graph(idtype, dev)
    sub = dgl.graph((g.edges()[0][:50], g.edges()[1][:50]), num_nodes=200, idtype=idtype, device=dev)
    cpu = dgl.graph((g.edges()[0][:50].cpu(), g.edges()[1][:50].cpu()), num_nodes=200, idtype=idtype)
    keep = torch.tensor([199, 0, 199, 17])
    same(dgl.compact_graphs(sub, always_preserve=keep), dgl.compact_graphs(cpu, always_preserve=keep))
    empty = dgl.graph((torch.empty(0, dtype=idtype), torch.empty(0, dtype=idtype)), num_nodes=9, idtype=idtype, device=dev)
    assert dgl.compact_graphs(empty).num_nodes() == 0
    with pytest.raises(dgl.DGLError, match="node id out of range"):
        dgl.compact_graphs(sub, always_preserve=[200])
    assert bool((sub._sampling_node_map == -1).all())
