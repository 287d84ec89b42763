"""Layer-neighbour (LABOR-0) sampling on the device (csrc/labor.hip) against the host functions that compile the same
rule (csrc/labor_step.h; tests/test_labor_host.py pins those against an independent model), and the Python surface
(dgl_amd.sampling.sample_labors, DGLGraph.sample_labors, LaborSampler) as the reference's _test_sample_labors checks it
(tests/python/common/sampling/test_sampling.py:712-830).

Device == host BIT FOR BIT: indptr, neighbours, edge ids and the importances from the same c array, over the degree
ladder 0 .. 70 000 of tests/labor_cases.py, both id widths, both group widths of the kernels (the padded graph has a mean
degree under 32: 16 lanes per row; the plain one a wavefront per row) and 1 .. 20 000 seeds (the last past the
one-workgroup scan of csrc/sort.hip.h); every case runs twice and must give identical bytes."""
import numpy as np
import pytest
import torch

import dgl_amd
from dgl_amd import DGLAMDError, _capi
from dgl_amd.sampling import EID, NID, LaborSampler, NeighborSampler, sample_labors
from tests import labor_cases as lc

pytestmark = pytest.mark.gpu

NUM_SEEDS = [1, 63, 64, 65, 255, 256, 257, 1025, 20000]
REL20 = 2.0 ** -20
_CACHE = {}


def graph_on(dev, pad, idtype, use_data=True):
    """(numpy graph, host csr, device csr) of the ladder graph, built once per variant."""
    key = (pad, idtype, use_data)
    if key not in _CACHE:
        R = _CACHE.setdefault(("np", pad), lc.labor_graph(pad_rows=pad))
        h = lc.host_csr_of(R, idtype, use_data)
        d = _capi.make_csr(*lc.tensors_of(R, idtype, use_data, device=dev), R["num_cols"])
        _CACHE[key] = (R, h, d)
    return _CACHE[key]


def probs_of(R):
    key = ("prob", len(R["indices"]))
    if key not in _CACHE:
        rng = np.random.default_rng(21)
        _CACHE[key] = {torch.float32: torch.from_numpy(lc.messy_prob(len(R["indices"]), rng, np.float32)),
                       torch.float64: torch.from_numpy(lc.messy_prob(len(R["indices"]), rng, np.float64))}
    return _CACHE[key]


def same_bytes(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and bytes(a.numpy().tobytes()) == bytes(b.numpy().tobytes())


def check_device_equals_host(h, d, seeds, k, seed, dev, prob=None):
    c = None if prob is None else _capi.labor_scale_host(h, prob, seeds, k)
    want = _capi.labor_pick_host(h, seeds, k, seed, prob=prob, c=c)
    p_dev = None if prob is None else prob.to(dev)
    c_dev = None if c is None else c.to(dev)
    got = _capi.labor_sample(d, seeds.to(dev), k, seed, prob=p_dev, c=c_dev)
    again = _capi.labor_sample(d, seeds.to(dev), k, seed, prob=p_dev, c=c_dev)
    for name, g_, w_, a_ in zip(("indptr", "nbr", "eids", "importances"), got, want, again):
        assert same_bytes(g_, w_), (name, k, len(seeds))
        assert same_bytes(g_, a_), ("second run", name, k, len(seeds))
    return want


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("pad", [0, 4000])
@pytest.mark.parametrize("n", NUM_SEEDS)
def test_device_equals_host(dev, idtype, pad, n):
    R, h, d = graph_on(dev, pad, idtype)
    assert (len(R["indices"]) // R["num_rows"] <= 32) == (pad > 0)       # the two group widths
    seeds = torch.from_numpy(lc.seeds_for(R, n, np.random.default_rng(100 + n))).to(idtype)
    for k in (1, 10, -1):
        check_device_equals_host(h, d, seeds, k, 7, dev)
    probs = probs_of(R)
    for dtype in (torch.float32, torch.float64):
        want = check_device_equals_host(h, d, seeds, 5, 8, dev, prob=probs[dtype])
        assert want[3].dtype == dtype
    check_device_equals_host(h, d, seeds, -1, 8, dev, prob=probs[torch.float32])


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_without_an_edge_id_map_and_empty_inputs(dev, idtype):
    R, h, d = graph_on(dev, 0, idtype, use_data=False)
    seeds = torch.from_numpy(lc.seeds_for(R, 257, np.random.default_rng(3))).to(idtype)
    check_device_equals_host(h, d, seeds, 10, 11, dev)
    check_device_equals_host(h, d, seeds, 5, 11, dev, prob=probs_of(R)[torch.float64])
    # no seeds: indptr = [0], nothing else
    none = torch.empty(0, dtype=idtype, device=dev)
    indptr, nbr, eids, imp = _capi.labor_sample(d, none, 10, 1)
    assert indptr.tolist() == [0] and nbr.numel() == 0 and eids.numel() == 0 and imp is None
    # no edges: every row is empty and no graph memory is read (the indices pointer is NULL)
    ptr = torch.zeros(6, dtype=idtype, device=dev)
    empty = _capi.make_csr(ptr, torch.empty(0, dtype=idtype, device=dev), None, 5)
    indptr, nbr, eids, imp = _capi.labor_sample(empty, torch.arange(5, dtype=idtype, device=dev), 10, 1)
    assert indptr.tolist() == [0] * 6 and nbr.numel() == 0


@pytest.mark.parametrize("pad", [0, 4000])
def test_scale_on_the_device(dev, pad):
    R, h, d = graph_on(dev, pad, torch.int64)
    seeds_np = lc.seeds_for(R, 1025, np.random.default_rng(5))
    seeds = torch.from_numpy(seeds_np)
    for dtype, prob in probs_of(R).items():
        for k in (1, 5, 10, -1):
            want = _capi.labor_scale_host(h, prob, seeds, k).numpy()
            got = _capi.labor_scale(d, prob.to(dev), seeds.to(dev), k)
            again = _capi.labor_scale(d, prob.to(dev), seeds.to(dev), k)
            assert same_bytes(got, again)
            got = got.cpu().numpy()
            fin = np.isfinite(want) & (want > 0)
            assert np.array_equal(got[~fin], want[~fin])                 # the special rows: exactly 0 or +inf
            assert (np.abs(got[fin] - want[fin]) <= want[fin] * REL20).all()
            if k > 0:
                total = lc.saturation_sum(R, seeds_np, got, prob.numpy())
                assert (np.abs(total[fin] - k) <= k * REL20).all()


# ---- sample_labors end to end --------------------------------------------------------------------------
def random_graph(dev, n=300, e=6000, seed=0, idtype=torch.int64):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
    g = dgl_amd.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n, idtype=idtype, device=dev)
    prob = np.exp(rng.uniform(-2, 2, e)).astype(np.float32)
    prob[rng.integers(0, e, e // 10)] = 0.0
    g.edata["prob"] = torch.from_numpy(prob).to(dev)
    g.edata["feat"] = torch.arange(e, device=dev).float()
    g.ndata["h"] = torch.arange(n, device=dev).float()
    return g, src, dst, prob


def check_frontier(g, sg, src, dst):
    """Every returned edge is an edge of g under its id, and no edge is returned twice."""
    u, v = sg.edges()
    eid = sg.edata[EID].cpu().numpy()
    assert np.array_equal(u.cpu().numpy(), src[eid]) and np.array_equal(v.cpu().numpy(), dst[eid])
    assert len(np.unique(eid)) == len(eid)
    assert sg.num_nodes() == g.num_nodes()


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_sample_labors_homogeneous(dev, idtype):
    g, src, dst, prob = random_graph(dev, idtype=idtype)
    seeds = torch.tensor([0, 5, 17, 33, 299, 150], dtype=idtype)
    sg, imp = sample_labors(g, seeds, 4, random_seed=3)
    check_frontier(g, sg, src, dst)
    assert set(sg.edges()[1].cpu().tolist()) <= set(seeds.tolist())
    assert len(imp) == 1 and imp[0].numel() == 0
    assert sg.idtype == idtype and sg.edata[EID].dtype == idtype
    # the same seed: the same frontier; as a one-element tensor too; another seed: another frontier
    sg2, _ = sample_labors(g, seeds, 4, random_seed=torch.tensor([3]))
    assert torch.equal(sg.edata[EID], sg2.edata[EID])
    sg3, _ = sample_labors(g, seeds, 4, random_seed=4)
    assert not torch.equal(sg.edata[EID], sg3.edata[EID])
    # fanout = -1: every in-edge of the seeds
    sg, _ = sample_labors(g, seeds, -1)
    check_frontier(g, sg, src, dst)
    assert sorted(sg.edata[EID].cpu().tolist()) == np.nonzero(np.isin(dst, seeds.numpy()))[0].tolist()
    # with prob: every in-edge of positive weight, importances = the weights normalised to mean 1 per seed
    sg, imp = sample_labors(g, seeds, -1, prob="prob")
    check_frontier(g, sg, src, dst)
    assert sorted(sg.edata[EID].cpu().tolist()) == np.nonzero(np.isin(dst, seeds.numpy()) & (prob > 0))[0].tolist()
    assert imp[0].dtype == torch.float32 and imp[0].shape[0] == sg.num_edges()
    # weighted with a fanout: only positive weights, one importance per edge, mean 1 per seed
    sg, imp = sample_labors(g, seeds, 4, prob="prob", random_seed=3)
    check_frontier(g, sg, src, dst)
    eid = sg.edata[EID].cpu().numpy()
    assert (prob[eid] > 0).all() and imp[0].shape[0] == len(eid) and len(eid) > 0
    v = sg.edges()[1].cpu().numpy()
    for s in np.unique(v):
        assert abs(float(imp[0].cpu().numpy()[v == s].mean()) - 1.0) < 1e-5
    # edge_dir = "out"
    sg, _ = sample_labors(g, seeds, 4, edge_dir="out", random_seed=3)
    check_frontier(g, sg, src, dst)
    assert set(sg.edges()[0].cpu().tolist()) <= set(seeds.tolist())
    sg, _ = sample_labors(g, seeds, -1, edge_dir="out")
    assert sorted(sg.edata[EID].cpu().tolist()) == np.nonzero(np.isin(src, seeds.numpy()))[0].tolist()
    # the method is the function
    assert dgl_amd.DGLGraph.sample_labors is sample_labors
    sg4, _ = g.sample_labors(seeds, 4, random_seed=3)
    assert torch.equal(sg4.edata[EID], sg2.edata[EID])


def test_features_exclusion_and_output_device(dev):
    g, src, dst, prob = random_graph(dev)
    seeds = torch.tensor([0, 5, 17, 33])
    sg, _ = sample_labors(g, seeds, 5, random_seed=1)
    assert sg.ndata["h"].data_ptr() == g.ndata["h"].data_ptr()                     # the same tensor
    assert torch.equal(sg.edata["feat"], g.edata["feat"][sg.edata[EID].long()])
    assert torch.equal(sg.edata["prob"], g.edata["prob"][sg.edata[EID].long()])
    bare, _ = sample_labors(g, seeds, 5, random_seed=1, copy_ndata=False, copy_edata=False)
    assert list(bare.ndata.keys()) == [] and list(bare.edata.keys()) == [EID]
    assert torch.equal(bare.edata[EID], sg.edata[EID])
    # exclude_edges: applied after sampling, to the frontier and to the importances
    full, imp_full = sample_labors(g, seeds, 5, prob="prob", random_seed=1)
    drop = full.edata[EID][::2].clone()
    cut, imp_cut = sample_labors(g, seeds, 5, prob="prob", random_seed=1, exclude_edges=drop)
    keep = ~torch.isin(full.edata[EID], drop)
    assert torch.equal(cut.edata[EID], full.edata[EID][keep]) and torch.equal(imp_cut[0], imp_full[0][keep])
    assert not torch.isin(cut.edata[EID], drop).any()
    check_frontier(g, cut, src, dst)
    everything, _ = sample_labors(g, seeds, -1, exclude_edges=drop.tolist())
    assert not torch.isin(everything.edata[EID], drop).any()
    # output_device
    out, imp = sample_labors(g, seeds, 5, prob="prob", random_seed=1, output_device="cpu")
    assert out.device.type == "cpu" and imp[0].device.type == "cpu" and out.edata[EID].device.type == "cpu"
    assert torch.equal(out.edata[EID], full.edata[EID].cpu()) and torch.equal(imp[0], imp_full[0].cpu())


def hetero_graph(dev):
    """user -follows-> user, user -plays-> game, user -likes-> game (the same source type into one node type twice:
    every game has the same number of `plays` and `likes` edges), game -has-> tag without any seed."""
    rng = np.random.default_rng(9)
    nu, ng, nt = 200, 60, 10
    fol = (rng.integers(0, nu, 1500), rng.integers(0, nu, 1500))
    # every game: 30 distinct users per relation, over a common pool so that the two relations share many sources
    plays = (np.concatenate([rng.choice(nu, 30, replace=False) for _ in range(ng)]), np.repeat(np.arange(ng), 30))
    likes = (np.concatenate([rng.choice(nu, 30, replace=False) for _ in range(ng)]), np.repeat(np.arange(ng), 30))
    has = (rng.integers(0, ng, 100), rng.integers(0, nt, 100))
    t_ = lambda p: (torch.from_numpy(p[0]), torch.from_numpy(p[1]))
    g = dgl_amd.heterograph({("user", "follows", "user"): t_(fol), ("user", "plays", "game"): t_(plays),
                             ("user", "likes", "game"): t_(likes), ("game", "has", "tag"): t_(has)},
                            {"user": nu, "game": ng, "tag": nt}, idtype=torch.int64, device=dev)
    return g, dict(follows=fol, plays=plays, likes=likes, has=has)


def test_sample_labors_heterograph(dev):
    g, edges = hetero_graph(dev)
    nodes = {"user": torch.tensor([1, 2, 3, 50]), "game": torch.arange(20)}
    fanout = {"follows": 3, "plays": 5, "likes": -1, "has": 2}
    sg, imp = sample_labors(g, nodes, fanout, random_seed=6)
    assert len(imp) == len(g.canonical_etypes)
    assert sg.ntypes == g.ntypes and sg.canonical_etypes == g.canonical_etypes
    for c in g.canonical_etypes:
        src, dst = edges[c[1]]
        u, v = sg.edges(etype=c)
        eid = sg.edges[c].data[EID].cpu().numpy()
        assert np.array_equal(u.cpu().numpy(), src[eid]) and np.array_equal(v.cpu().numpy(), dst[eid])
        assert len(np.unique(eid)) == len(eid)
        assert sg.num_nodes(c[0]) == g.num_nodes(c[0])
    assert sg.num_edges("has") == 0                                        # no seed of type tag
    assert sorted(sg.edges["likes"].data[EID].cpu().tolist()) == np.nonzero(edges["likes"][1] < 20)[0].tolist()
    per_game = np.bincount(sg.edges(etype="plays")[1].cpu().numpy(), minlength=20)
    assert per_game.sum() > 0 and per_game.max() < 30
    # an int fanout, and a fanout of 0 for one relation
    sg, _ = sample_labors(g, nodes, 2, random_seed=6)
    assert sg.num_edges("follows") > 0 and sg.num_edges("has") == 0
    sg, _ = sample_labors(g, nodes, {"follows": 0, "plays": 1, "likes": 1, "has": 1}, random_seed=6)
    assert sg.num_edges("follows") == 0 and sg.num_edges("plays") > 0
    with pytest.raises(DGLAMDError, match="node type"):
        sample_labors(g, torch.tensor([1, 2]), 2)
    with pytest.raises(DGLAMDError, match="fanout"):
        sample_labors(g, nodes, {"follows": 1})


def test_variates_are_shared_across_relations(dev):
    """`plays` and `likes` go from users into games and every game has degree 30 in both: with ONE seed for the call a
    user kept for some game through `plays` is kept for every game that has it through `likes`, and the other way round.
    With a seed per relation (the sample_neighbors convention) the two kept user sets would be unrelated."""
    g, edges = hetero_graph(dev)
    games = torch.arange(60)
    sg, _ = sample_labors(g, {"game": games}, {"follows": 0, "plays": 6, "likes": 6, "has": 0}, random_seed=12)
    kept = {r: set(sg.edges(etype=r)[0].cpu().tolist()) for r in ("plays", "likes")}
    has = {r: set(edges[r][0].tolist()) for r in ("plays", "likes")}
    assert kept["plays"] and kept["plays"] != has["plays"]
    assert kept["plays"] & has["likes"] == kept["likes"] & has["plays"]
    assert len(kept["plays"] & kept["likes"]) > 10


# ---- LaborSampler ----------------------------------------------------------------------------------------
def sampler_graph(dev, n=5000, deg=40, seed=1):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, n * deg), np.repeat(np.arange(n), deg)       # every node has in-degree `deg`
    g = dgl_amd.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n, idtype=torch.int64, device=dev)
    g.edata["w"] = torch.from_numpy(np.exp(rng.uniform(-1, 1, n * deg)).astype(np.float32)).to(dev)
    return g, src, dst


def batch_of(n=5000, size=500):
    return torch.from_numpy(np.random.default_rng(2).choice(n, size, replace=False))


def test_labor_sampler_blocks(dev):
    g, src, dst = sampler_graph(dev)
    batch = batch_of()
    for prob in (None, "w"):
        sampler = LaborSampler([10, 5], prob=prob, seed=3)
        inputs, outputs, blocks = sampler.sample_blocks(g, batch)
        assert torch.equal(outputs.cpu(), batch) and len(blocks) == 2
        assert torch.equal(blocks[1].dstdata[NID].cpu(), batch)
        assert torch.equal(inputs, blocks[0].srcdata[NID])
        for i in range(len(blocks) - 1):                                       # the blocks chain
            nd = blocks[i].dstdata[NID]
            assert torch.equal(nd, blocks[i + 1].srcdata[NID][:nd.shape[0]])
        for b in blocks:
            assert torch.equal(b.srcdata[NID][:b.num_dst_nodes()], b.dstdata[NID])
            u, v = b.edges()
            eid = b.edata[EID].cpu().numpy()
            assert np.array_equal(b.srcdata[NID][u.long()].cpu().numpy(), src[eid])     # original edge ids
            assert np.array_equal(b.dstdata[NID][v.long()].cpu().numpy(), dst[eid])
            assert ("edge_weights" in b.edata) == (prob is not None)
            if prob is not None:
                assert b.edata["edge_weights"].shape[0] == b.num_edges()
        # two samplers with the same seed agree; a second call differs from the first
        twin = LaborSampler([10, 5], prob=prob, seed=3)
        t_in, _, t_blocks = twin.sample_blocks(g, batch)
        assert torch.equal(t_in, inputs)
        assert all(torch.equal(a.edata[EID], b.edata[EID]) for a, b in zip(blocks, t_blocks))
        n_in, _, n_blocks = sampler.sample_blocks(g, batch)
        assert not torch.equal(n_blocks[1].edata[EID], blocks[1].edata[EID])


def kept_sources(block):
    return set(block.srcdata[NID][block.edges()[0].long()].cpu().tolist())


def test_layer_dependency_shares_the_variates(dev):
    """Every node of the graph has in-degree 40 and both layers use fanout 10, so a node's keep decision is one threshold
    test of its own variate: with layer_dependency=True a source kept in the outer layer is kept in the inner layer for
    every seed there that has it, so the outer layer's kept sources that are neighbours of inner seeds are all kept."""
    g, src, dst = sampler_graph(dev)
    batch = batch_of()
    _, _, blocks = LaborSampler([10, 10], layer_dependency=True, seed=5).sample_blocks(g, batch)
    outer, inner = kept_sources(blocks[1]), kept_sources(blocks[0])
    inner_seeds = set(blocks[0].dstdata[NID].cpu().tolist())
    candidates = set(src[np.isin(dst, list(inner_seeds))].tolist())            # every neighbour of an inner seed
    assert outer and (outer & candidates) <= inner
    assert inner - outer <= candidates - set(src[np.isin(dst, batch.numpy())].tolist())   # new ones come from new seeds only
    # independent layers: the outer layer's kept sources are not all kept again
    _, _, blocks = LaborSampler([10, 10], layer_dependency=False, seed=5).sample_blocks(g, batch)
    outer, inner = kept_sources(blocks[1]), kept_sources(blocks[0])
    assert not (outer & candidates) <= inner


def test_labor_frontier_is_smaller_than_neighbor_sampling(dev):
    """5000 nodes of in-degree 40 (sources uniform), a batch of 500, fanouts [10, 10].  Input nodes of the two layers:
    LABOR 2432 (exact: dgla_labor_pick_host run with the sampler's seeds gives the same picks), NeighborSampler 4997
    on the device (4995 in a numpy simulation of independent picks without replacement; nearly every node of the
    graph).  The assertion asks for a quarter fewer, the counts say half."""
    g, src, dst = sampler_graph(dev)
    batch = batch_of()
    labor_in, _, _ = LaborSampler([10, 10], seed=0).sample_blocks(g, batch)
    neigh_in, _, _ = NeighborSampler([10, 10], seed=0).sample_blocks(g, batch.to(dev))
    print("input nodes: LABOR %d, NeighborSampler %d" % (labor_in.shape[0], neigh_in.shape[0]))
    assert labor_in.shape[0] == 2432
    assert labor_in.shape[0] < 0.75 * neigh_in.shape[0]


# ---- refusals ----------------------------------------------------------------------------------------------
def test_refusals(dev):
    g, _, _, _ = random_graph(dev)
    seeds = torch.tensor([0, 1])
    with pytest.raises(DGLAMDError, match="importance_sampling = 1 is not supported"):
        sample_labors(g, seeds, 2, importance_sampling=1)
    with pytest.raises(DGLAMDError, match="seed2_contribution = 0.5 is not supported"):
        sample_labors(g, seeds, 2, seed2_contribution=0.5)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        sample_labors(g.to("cpu"), seeds, 2)
    with pytest.raises(ValueError):
        sample_labors(g, seeds, 2, edge_dir="both")
    with pytest.raises(DGLAMDError, match="one element"):
        sample_labors(g, seeds, 2, random_seed=torch.tensor([1, 2]))
