"""PinSAGE neighbour selection on the device (csrc/pinsage.hip) against the host entry point and the numpy model of
tests/test_pinsage_host.py, and RandomWalkNeighborSampler / PinSAGESampler against the host walker followed by the host
selection.  Everything is integer work: all comparisons are equality.  Reference: SelectPinSageNeighbors
(src/graph/sampling/randomwalks/randomwalk_gpu.cu:443, randomwalk_cpu.cc:41-102) behind python/dgl/sampling/pinsage.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_pinsage_host import KINDS, NP, assert_same, host_select, make_input, model_select
from tests.test_random_walk_host import host_walk

pytestmark = pytest.mark.gpu

NUM_DST = 1003      # no multiple of 64 or 256


def _sizes():
    """1, every size-class boundary of the kernel and its neighbours, 4096 and the largest accepted S."""
    from dgl_amd import _capi

    limit = min(_capi.pinsage_max_samples(torch.int32), _capi.pinsage_max_samples(torch.int64))
    s = {1, 4096, limit}
    for b in _capi.pinsage_size_classes():
        s |= {b - 1, b, b + 1}
    return sorted(x for x in s if 1 <= x <= limit)


def _device_select(src, dst, S, k, dev):
    from dgl_amd import _capi

    d_src, d_dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    compact = _capi.select_pinsage_neighbors(d_src, d_dst, S, k)
    padded = _capi.select_pinsage_neighbors_padded(d_src, d_dst, S, k)
    assert all(t.dtype == d_src.dtype and t.device == d_src.device for t in compact + padded)
    return tuple(t.cpu().numpy() for t in compact), tuple(t.cpu().numpy() for t in padded)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("S", _sizes())
def test_device_equals_host_and_model(dev, idtype, S):
    from dgl_amd import _capi

    assert S <= _capi.pinsage_max_samples(idtype)
    for num_dst in (NUM_DST, 5) if S == _capi.pinsage_max_samples(idtype) else (NUM_DST,):
        src, dst = make_input(num_dst, S, idtype, 11 * S + num_dst)
        distinct = np.array([len(np.setdiff1d(src[j * S:(j + 1) * S], [-1])) for j in range(num_dst)])
        for k in (1, 10, S + 5):
            want, want_padded = model_select(src, dst, S, k)
            assert_same(host_select(src, dst, S, k), want, ("host", S, k))
            compact, padded = _device_select(src, dst, S, k, dev)
            assert_same(compact, want, ("device", S, k))
            kp = min(k, S)
            assert padded[0].shape == (num_dst, kp) and padded[1].shape == (num_dst, kp) and padded[2].shape == (num_dst,)
            for g, w in zip(padded, want_padded):
                assert g.dtype == w.dtype and np.array_equal(g, w), ("padded", S, k)
            # unused slots are -1 / 0 and num = min(k, distinct ids), stated without the model's padded form
            p_src, p_cnt, num = padded
            slot = np.arange(kp)[None, :]
            assert ((p_src == -1) == (slot >= num[:, None])).all() and ((p_cnt == 0) == (slot >= num[:, None])).all()
            assert np.array_equal(num, np.minimum(k, distinct))
        # the same bits on every run (k = S + 5 from the loop)
        again, again_padded = _device_select(src, dst, S, k, dev)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(compact + padded, again + again_padded))


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_every_segment_empty_and_no_segment(dev, idtype):
    src, dst = make_input(70, 9, idtype, 2, ("all_none",))
    compact, padded = _device_select(src, dst, 9, 4, dev)
    assert all(c.shape == (0,) and c.dtype == NP[idtype] for c in compact)
    assert (padded[0] == -1).all() and (padded[1] == 0).all() and (padded[2] == 0).all()
    compact, padded = _device_select(src[:0], dst[:0], 9, 4, dev)
    assert all(c.shape == (0,) for c in compact) and padded[0].shape == (0, 4) and padded[2].shape == (0,)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_error_before_launch(dev, idtype):
    from dgl_amd import _capi, _lib

    limit = _capi.pinsage_max_samples(idtype)
    S = limit + 1
    src = torch.zeros(3 * S, dtype=idtype, device=dev)
    for fn in (_capi.select_pinsage_neighbors, _capi.select_pinsage_neighbors_padded):
        with pytest.raises(_lib.DGLAMDError, match="above the largest segment"):
            fn(src, src, S, 2)
    # the C entry point itself, on device memory: -1 with the message, and the outputs keep their contents
    outs = [torch.full((3, 2), 77, dtype=idtype, device=dev), torch.full((3, 2), 77, dtype=idtype, device=dev),
            torch.full((3,), 77, dtype=idtype, device=dev), torch.full((3,), 77, dtype=idtype, device=dev)]
    bits = 32 if idtype == torch.int32 else 64
    ret = _lib.LIB.dgla_pinsage_select_padded(bits, src.data_ptr(), src.data_ptr(), 3, S, 2, *[o.data_ptr() for o in outs],
                                              torch.cuda.current_stream(dev).cuda_stream)
    assert ret == -1 and "above the largest segment" in _lib.LIB.dgla_last_error().decode()
    total = ctypes.c_int64(-5)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    ret = _lib.LIB.dgla_pinsage_select_count(bits, src.data_ptr(), src.data_ptr(), 3, S, 2, ctypes.byref(total),
                                             ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
    assert ret == -1 and total.value == -5
    torch.cuda.synchronize(dev)
    assert all(bool((o == 77).all()) for o in outs) and int(ws.sum()) == 0


# ---- the whole sampler -------------------------------------------------------------------------------
def _skewed(n_src, n_dst, e, hub, rng):
    """Skewed out-degrees (some sources without an out-edge) plus one hub source."""
    src = np.minimum(np.floor(rng.random(e) ** 3 * n_src), n_src - 1).astype(np.int64)
    src = np.concatenate([src, np.full(hub, n_src // 2, dtype=np.int64)])
    return src, rng.integers(0, n_dst, size=len(src))


def _graph(kind, idtype, dev):
    """(graph, sampler arguments after G): bipartite with two relations, homogeneous, and a cycle A -> B -> C -> A."""
    import dgl_amd

    rng = np.random.default_rng(41)
    t_ = lambda a: torch.from_numpy(a).to(device=dev, dtype=idtype)
    if kind == "homogeneous":
        s, d = _skewed(400, 400, 3000, 200, rng)
        return dgl_amd.graph((t_(s), t_(d)), num_nodes=400), dict(metapath=None)
    if kind == "bipartite":
        ni, nu = 300, 200
        s, d = _skewed(ni, nu, 2000, 150, rng)
        s2, d2 = _skewed(nu, ni, 1500, 0, rng)
        g = dgl_amd.heterograph({("item", "seen-by", "user"): (t_(s), t_(d)), ("user", "saw", "item"): (t_(s2), t_(d2))},
                                {"item": ni, "user": nu})
        return g, dict(metapath=["seen-by", "saw"])
    na, nb, nc = 250, 180, 220
    ab, bc, ca = _skewed(na, nb, 1500, 100, rng), _skewed(nb, nc, 1200, 0, rng), _skewed(nc, na, 1300, 0, rng)
    g = dgl_amd.heterograph({("A", "ab", "B"): (t_(ab[0]), t_(ab[1])), ("B", "bc", "C"): (t_(bc[0]), t_(bc[1])),
                             ("C", "ca", "A"): (t_(ca[0]), t_(ca[1]))}, {"A": na, "B": nb, "C": nc})
    return g, dict(metapath=["ab", "bc", "ca"])


def _host_sampler(sampler, seeds, seed):
    """What the sampler must return, on the host: the same table, metapath, restart tensor and seed through
    dgla_random_walk_host, the same columns, then dgla_pinsage_select_host."""
    g = sampler.G
    rels = []
    for c in g.canonical_etypes:
        rel = g._graph.relations[g.get_etype_id(c)]
        indptr, indices, data = (None if t is None else t.cpu().numpy().astype(np.int64) for t in rel.csr())
        rels.append(dict(indptr=indptr, indices=indices, data=data, cdf=None, num_rows=rel.num_src, num_cols=rel.num_dst))
    path = [g.get_etype_id(e) for e in sampler.full_metapath]
    walks = np.repeat(seeds, sampler.num_random_walks)
    traces, _ = host_walk(rels, path, walks, seed, sampler.restart_prob.cpu().numpy(), g.idtype)
    dt = NP[g.idtype]
    src = np.ascontiguousarray(traces[:, sampler.metapath_hops::sampler.metapath_hops]).reshape(-1).astype(dt)
    dst = np.repeat(traces[:, 0], sampler.num_traversals).astype(dt)
    return host_select(src, dst, sampler.num_random_walks * sampler.num_traversals, sampler.num_neighbors)


def _edges(frontier, column="weights"):
    u, v = frontier.edges()
    return u.cpu().numpy(), v.cpu().numpy(), frontier.edata[column].cpu().numpy()


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("kind", ["bipartite", "homogeneous", "cycle"])
def test_sampler_equals_host(dev, kind, idtype):
    from dgl_amd import sampling

    g, kw = _graph(kind, idtype, dev)
    walks, traversals, neighbors = 40, 3, 5
    sampler = sampling.RandomWalkNeighborSampler(g, traversals, 0.3, walks, neighbors, **kw)
    n = g.num_nodes(sampler.ntype)
    rng = np.random.default_rng(5)
    others = np.setdiff1d(np.arange(n), [n // 2, 7])
    seeds = np.concatenate([[n // 2, 7, n // 2, 7], rng.permutation(others)[:127]])   # the hub and node 7, each listed twice
    d_seeds = torch.from_numpy(seeds).to(device=dev, dtype=idtype)
    for seed in (3, 4):
        frontier = sampler(d_seeds, seed=seed)
        got = _edges(frontier)
        assert_same(got, _host_sampler(sampler, seeds, seed), (kind, seed))
        # the graph: the one node type with all of G's nodes of that type
        assert frontier.ntypes == [sampler.ntype] and frontier.num_nodes() == n and frontier.idtype == idtype
        assert frontier.edata["weights"].dtype == idtype and frontier.num_edges() == len(got[0]) > 0
        u, v, c = got
        # groups follow the seeds' order: at most `neighbors` in-edges per LISTED seed, none for other nodes
        change = np.nonzero(np.diff(v))[0] + 1
        groups = np.split(np.arange(len(v)), change)
        assert np.isin(v, seeds).all()
        assert (c >= 1).all() and ((u >= 0) & (u < n)).all()
        pos = 0                                                          # walk the listed seeds against the groups
        for gidx in groups:
            while seeds[pos] != v[gidx[0]]:                              # (a seed whose walks all died has no group)
                pos += 1
            assert len(gidx) <= neighbors and (v[gidx] == seeds[pos]).all() and c[gidx].sum() <= walks * traversals
            key = list(zip(c[gidx].tolist(), u[gidx].tolist()))
            assert key == sorted(set(key), reverse=True)                 # ranked by (count, id) descending, ids distinct
            pos += 1
    again = _edges(sampler(d_seeds, seed=4))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    # without a seed the walks follow torch's generator
    torch.manual_seed(99)
    a = _edges(sampler(d_seeds))
    torch.manual_seed(99)
    b = _edges(sampler(d_seeds))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_seeds_listed_twice(dev, idtype):
    """A node listed twice gets two groups of its own, one per listing.  The walks of the two listings are independent
    (the picks are a function of the walk's position in the call, include/dgl_amd.h "random walks"), so on a graph with
    choices the groups are two draws, each equal to the host's result for its position (test_sampler_equals_host lists
    two nodes twice).  Where the rule leaves the walks no choice — every node has one out-edge, no termination — the two
    groups are identical, which is what is asserted here."""
    import dgl_amd
    from dgl_amd import sampling

    n = 50
    ring = torch.arange(n, dtype=idtype, device=dev)
    g = dgl_amd.graph((ring, (ring * 7 + 3) % n), num_nodes=n)           # a permutation: out-degree 1 everywhere
    sampler = sampling.RandomWalkNeighborSampler(g, 4, 0.0, 6, 3)
    seeds = torch.tensor([5, 9, 5, 5, 9], dtype=idtype, device=dev)
    u, v, c = _edges(sampler(seeds, seed=1))
    assert v.tolist() == [5] * 3 + [9] * 3 + [5] * 6 + [9] * 3 and (c == 6).all()
    groups = [(u[i:i + 3].tolist(), c[i:i + 3].tolist()) for i in range(0, 15, 3)]
    assert groups[0] == groups[2] == groups[3] and groups[1] == groups[4] and groups[0] != groups[1]
    step = lambda x: (x * 7 + 3) % n
    assert groups[0][0] == sorted([step(5), step(step(5)), step(step(step(5))), step(step(step(step(5))))], reverse=True)[:3]
    assert_same((u, v, c), _host_sampler(sampler, seeds.cpu().numpy(), 1), "ring")


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_certain_termination_leaves_the_first_traversal(dev, idtype):
    from dgl_amd import sampling

    g, kw = _graph("bipartite", idtype, dev)
    seeds = torch.arange(0, 300, 3, dtype=idtype, device=dev)
    full = sampling.RandomWalkNeighborSampler(g, 4, 1.0, 25, 6, **kw)
    once = sampling.RandomWalkNeighborSampler(g, 1, 0.0, 25, 6, **kw)
    a, b = _edges(full(seeds, seed=8)), _edges(once(seeds, seed=8))
    assert_same(a, b, "termination_prob = 1")                            # only the first traversal's visits are left
    assert len(a[0]) > 0 and np.add.reduceat(a[2], np.r_[0, np.nonzero(np.diff(a[1]))[0] + 1]).max() <= 25
    assert_same(a, _host_sampler(full, seeds.cpu().numpy(), 8), "host")


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_empty_results(dev, idtype):
    import dgl_amd
    from dgl_amd import sampling

    # every seed is a dead end: all walks die at once, the result has G's nodes and no edge
    g = dgl_amd.graph((torch.tensor([0], dtype=idtype, device=dev), torch.tensor([1], dtype=idtype, device=dev)), num_nodes=6)
    sampler = sampling.RandomWalkNeighborSampler(g, 2, 0.5, 4, 3, weight_column="w")
    for seeds in ([2, 3, 4], []):
        f = sampler(torch.tensor(seeds, dtype=idtype, device=dev), seed=1)
        assert f.num_nodes() == 6 and f.num_edges() == 0 and f.edata["w"].shape == (0,) and f.edata["w"].dtype == idtype
    with pytest.raises(dgl_amd.sampling._DGLError, match="seed_nodes"):
        sampler(torch.tensor([1], dtype=torch.int16, device=dev))


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_two_bicliques_stay_apart(dev, idtype):
    """Items {0, 1} <-> users {0, 1} and items {2, 3} <-> users {2, 3}, fully connected inside a component and not at
    all across: whatever the walks draw, a selected neighbour lies in its seed's own component."""
    import dgl_amd

    item = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3], dtype=idtype, device=dev)
    user = torch.tensor([0, 1, 0, 1, 2, 3, 2, 3], dtype=idtype, device=dev)
    g = dgl_amd.heterograph({("item", "bought-by", "user"): (item, user), ("user", "bought", "item"): (user, item)})
    sampler = dgl_amd.PinSAGESampler(g, "item", "user", 3, 0.5, 50, 2)
    seeds = torch.tensor([0, 1, 2, 3, 3, 0], dtype=idtype, device=dev)
    for seed in (None, 6):
        f = sampler(seeds, seed=seed)
        u, v, c = _edges(f)
        assert f.ntypes == ["item"] and f.num_nodes() == 4
        assert len(u) == 12 and v.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 3, 3, 0, 0]      # both items of the component, every time
        assert ((u < 2) == (v < 2)).all() and (c >= 1).all() and (c <= 150).all()
        assert all(set(u[i:i + 2].tolist()) == ({0, 1} if v[i] < 2 else {2, 3}) for i in range(0, 12, 2))
