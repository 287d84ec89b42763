"""Random walks on the device (csrc/random_walk.hip) against the host walker and the numpy model of
tests/test_random_walk_host.py: random_walk_kernel == dgla_random_walk_host bit for bit (the two compile one step rule,
csrc/random_walk_step.h), the exact properties and the error bound of walk_cdf_kernel, a metapath over three relations,
and the public dgl_amd.sampling.random_walk.  Reference: src/graph/sampling/randomwalks/randomwalk_gpu.cu behind
python/dgl/sampling/randomwalks.py."""
import numpy as np
import pytest
import torch

from tests.test_random_walk_host import (check_properties, csr_from_coo, host_walk, messy_weights, model_walk, skewed_graph,
                                         usable)

pytestmark = pytest.mark.gpu

N, E, HUB = 2000, 30000, 5000
WALKS = 5003        # no multiple of 64


@pytest.fixture(scope="module")
def graphs():
    """COO in random order (edge-id map present) and row-sorted (map absent), with the hub row's every 64th position
    at weight 0 and a sprinkling of zero, negative and NaN weights; built once, never modified."""
    rng = np.random.default_rng(17)
    out = {}
    for presorted in (False, True):
        src, dst = skewed_graph(N, E, HUB, rng, presorted)
        R = csr_from_coo(src, dst, N, N)
        assert (R["data"] is None) == presorted
        deg = np.diff(R["indptr"])
        assert deg.max() >= HUB and (deg == 0).any() and (deg == 1).any()
        eid_of_pos = R["data"] if R["data"] is not None else np.arange(len(src))
        lo = R["indptr"][N // 2]
        ws = {}
        for name, dt in (("f32", np.float32), ("f64", np.float64)):
            w = messy_weights(len(src), rng, dt)
            w[eid_of_pos[lo:lo + deg[N // 2]:64]] = 0
            ws[name] = w
        out[presorted] = (R, ws)
    return out


def _seeds(rng, R):
    dead_end = int(np.nonzero(np.diff(R["indptr"]) == 0)[0][0])
    s = rng.integers(0, N, size=WALKS)
    s[:8] = [N // 2, N // 2, 3, 3, dead_end, N, -1, 2 ** 31 - 1]        # repeats, a dead end, ids outside the graph
    return s


def _device_table(R, cdf, idtype, dev):
    from dgl_amd import _capi

    t_ = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=idtype)
    return _capi.make_csr(t_(R["indptr"]), t_(R["indices"]), t_(R["data"]), R["num_cols"]), cdf


def _device_cdf(R, prob, idtype, dev):
    from dgl_amd import _capi

    csr, _ = _device_table(R, None, idtype, dev)
    return _capi.random_walk_cdf(csr, torch.from_numpy(prob).to(dev))


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("presorted", [False, True])
@pytest.mark.parametrize("weights", [None, "f32", "f64"])
def test_device_equals_host_walker(dev, graphs, idtype, presorted, weights):
    from dgl_amd import _capi

    R, ws = graphs[presorted]
    cdf = None if weights is None else _device_cdf(R, ws[weights], idtype, dev)
    Rh = dict(R, cdf=None if cdf is None else cdf.cpu().numpy())        # the device-built CDF, copied to the host
    seeds = _seeds(np.random.default_rng(3), R)
    d_seeds = torch.from_numpy(seeds).to(device=dev, dtype=idtype)
    rng = np.random.default_rng(4)
    for steps in (1, 7, 80):
        for restart in (None, 0.15, (rng.random(steps) * 0.3).astype(np.float32), rng.random(steps) * 0.3):
            kw = {}
            if restart is not None:
                if np.isscalar(restart):
                    kw["restart_prob"] = restart
                else:
                    kw["restart_steps"] = torch.from_numpy(restart).to(dev)
            seed = 1000 * steps + 5
            tr, ev = _capi.random_walk([_device_table(R, cdf, idtype, dev)], [0] * steps, d_seeds, rng_seed=seed, **kw)
            assert tr.dtype == idtype and tr.shape == (WALKS, steps + 1) and ev.shape == (WALKS, steps)
            ht, he = host_walk([Rh], [0] * steps, seeds, seed, restart, idtype)
            assert np.array_equal(tr.cpu().numpy(), ht) and np.array_equal(ev.cpu().numpy(), he), (steps, type(restart))
    # the longest walks once more through the integer properties, and without the edge-id output
    check_properties([Rh], [0] * 80, ht, he, seed, restart, [None if weights is None else ws[weights]])
    tr2, none = _capi.random_walk([_device_table(R, cdf, idtype, dev)], [0] * 80, d_seeds, rng_seed=seed,
                                  return_eids=False, **kw)
    assert none is None and torch.equal(tr2, tr)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("presorted", [False, True])
@pytest.mark.parametrize("weights", ["f32", "f64"])
def test_cdf_kernel(dev, graphs, idtype, presorted, weights):
    R, ws = graphs[presorted]
    prob = ws[weights]
    got = _device_cdf(R, prob, idtype, dev).cpu().numpy()
    again = _device_cdf(R, prob, idtype, dev).cpu().numpy()
    assert got.tobytes() == again.tobytes()                              # no atomics: the same bits
    nnz = len(got)
    ip = R["indptr"]
    eid_of_pos = R["data"] if R["data"] is not None else np.arange(nnz)
    w = usable(prob)[eid_of_pos]                                         # w' in position order
    assert (w == 0).sum() > 100 and np.isnan(prob).any() and (prob < 0).any()
    first = np.zeros(nnz, dtype=bool)
    first[ip[:-1][np.diff(ip) > 0]] = True
    prev = np.where(first, 0.0, np.concatenate([[0.0], got[:-1]]))
    assert (got >= prev).all(), "the CDF decreases inside a row"
    assert (got[w == 0] == prev[w == 0]).all(), "a zero weight moved the CDF"
    deg = np.diff(ip)
    one = ip[:-1][deg == 1]
    assert len(one) and np.array_equal(got[one], w[one])                 # (double)w exactly
    # numpy's sequential fp64 cumsum: at most deg - 1 roundings of 2^-53 relative on partial sums <= total on either
    # side -> |diff| <= deg * 2^-52 * row total
    worst = 0.0
    for r in np.nonzero(deg > 1)[0]:
        ref = np.cumsum(w[ip[r]:ip[r + 1]])
        bound = deg[r] * 2.0 ** -52 * ref[-1]
        d = np.abs(got[ip[r]:ip[r + 1]] - ref).max()
        worst = max(worst, d / bound if bound > 0 else (0.0 if d == 0 else np.inf))
    print("largest |diff| / bound =", worst)
    assert worst <= 1.0


def test_heterograph_metapath(dev):
    import dgl_amd
    from dgl_amd import sampling

    rng = np.random.default_rng(23)
    nu, ni = 300, 200
    coo = {("user", "follow", "user"): (rng.integers(0, nu, 2500), rng.integers(0, nu, 2500)),
           ("user", "view", "item"): (rng.integers(0, nu, 2000), rng.integers(0, ni, 2000)),
           ("item", "viewed-by", "user"): (rng.integers(0, ni, 1500), rng.integers(0, nu, 1500))}
    g = dgl_amd.heterograph({c: (torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev)) for c, (s, d) in coo.items()},
                            {"user": nu, "item": ni})
    wv = messy_weights(2000, rng)
    g.edges["view"].data["p"] = torch.from_numpy(wv).to(dev)
    names = ["follow", "view", "viewed-by"] * 2
    seeds = torch.arange(1000, device=dev) % nu
    restart = torch.tensor([0, 0.5, 0, 0, 0.5, 0])
    for rp in (None, restart):
        tr, ev, types = sampling.random_walk(g, seeds, metapath=names, prob="p", restart_prob=rp, return_eids=True, seed=31)
        user, item = g.get_ntype_id("user"), g.get_ntype_id("item")
        # the reference's [0, 0, 1, 0, 0, 1, 0] (user = 0, item = 1) in THIS graph's type ids: node types are numbered in
        # sorted order here as in dgl.heterograph, so item = 0 and user = 1
        assert types.tolist() == [user, user, item, user, user, item, user] and (user, item) == (1, 0)
        # the same walk by the host walker, over the graph's own CSRs and its cached, device-built CDF
        rels, probs = [], []
        for c in g.canonical_etypes:
            rel = g._graph.relations[g.get_etype_id(c)]
            indptr, indices, data = (None if t is None else t.cpu().numpy().astype(np.int64) for t in rel.csr())
            cdf = rel._walk_cdf[1].cpu().numpy() if c[1] == "view" else None
            assert c[1] == "view" or getattr(rel, "_walk_cdf", None) is None
            rels.append(dict(indptr=indptr, indices=indices, data=data, cdf=cdf, num_rows=rel.num_src, num_cols=rel.num_dst))
            probs.append(wv if c[1] == "view" else None)
        path = [g.get_etype_id(e) for e in names]
        r = None if rp is None else rp.numpy()
        ht, he = host_walk(rels, path, seeds.cpu().numpy(), 31, r)
        assert np.array_equal(tr.cpu().numpy(), ht) and np.array_equal(ev.cpu().numpy(), he)
        mt, me = model_walk(rels, path, seeds.cpu().numpy(), 31, r)
        assert np.array_equal(ht, mt) and np.array_equal(he, me)
        check_properties(rels, path, ht, he, 31, r, probs)
        # every edge id is that edge of the graph
        for t, e in enumerate(names):
            u, v = g.edges(etype=e)
            went = ev[:, t] >= 0
            assert torch.equal(u[ev[went, t]], tr[went, t]) and torch.equal(v[ev[went, t]], tr[went, t + 1])


@pytest.fixture(scope="module")
def homo(dev):
    import dgl_amd

    rng = np.random.default_rng(29)
    src, dst = skewed_graph(500, 6000, 300, rng)
    g = dgl_amd.graph((torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)), num_nodes=500)
    return g, torch.from_numpy(dst).to(dev)


def test_public_api_seeds_and_shapes(dev, homo):
    from dgl_amd import sampling

    g, _ = homo
    nodes = torch.arange(777, device=dev) % 500
    a = sampling.random_walk(g, nodes, length=6, return_eids=True, seed=5)
    b = sampling.random_walk(g, nodes, length=6, return_eids=True, seed=5)
    c = sampling.random_walk(g, nodes, length=6, return_eids=True, seed=6)
    assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    assert a[0].shape == (777, 7) and a[1].shape == (777, 6) and a[2].tolist() == [0] * 7 and a[0].dtype == g.idtype
    torch.manual_seed(123)
    d = sampling.random_walk(g, nodes, length=6)
    e = sampling.random_walk(g, nodes, length=6)
    torch.manual_seed(123)
    f = sampling.random_walk(g, nodes, length=6)
    assert len(d) == 2 and torch.equal(d[0], f[0]) and not torch.equal(d[0], e[0])
    tr, types = sampling.random_walk(g, nodes, length=0)
    assert tr.shape == (777, 1) and torch.equal(tr[:, 0], nodes) and types.tolist() == [0]
    tr, ev, types = sampling.random_walk(g, nodes[:0], length=6, return_eids=True)
    assert tr.shape == (0, 7) and ev.shape == (0, 6) and types.shape == (7,)
    tr, _ = sampling.random_walk(g, [0, 1, 2], length=3, restart_prob=0.5, seed=1)     # a list of ids, a float restart
    assert tr.shape == (3, 4)


def test_in_place_weight_write_rebuilds_the_cdf(dev, homo):
    from dgl_amd import sampling

    g, dst = homo
    even = (dst % 2 == 0).float()
    g.edata["p"] = even.clone()
    nodes = torch.arange(2000, device=dev) % 500
    tr, _ = sampling.random_walk(g, nodes, length=1, prob="p", seed=9)
    took = tr[:, 1][tr[:, 1] >= 0]
    assert took.numel() > 500 and bool((took % 2 == 0).all())
    slot = g._graph.relations[0]._walk_cdf
    sampling.random_walk(g, nodes, length=1, prob="p", seed=10)
    assert g._graph.relations[0]._walk_cdf is slot                      # unchanged weights: the cached CDF
    g.edata["p"].copy_(1 - even)                                        # in place: same tensor, new _version
    tr, _ = sampling.random_walk(g, nodes, length=1, prob="p", seed=9)
    took = tr[:, 1][tr[:, 1] >= 0]
    assert took.numel() > 500 and bool((took % 2 == 1).all())
    assert g._graph.relations[0]._walk_cdf is not slot


def test_non_default_stream(dev, homo):
    from dgl_amd import sampling

    g, dst = homo
    g.edata["q"] = (dst % 3).float()
    nodes = torch.arange(3000, device=dev) % 500
    want = sampling.random_walk(g, nodes, length=12, prob="q", restart_prob=0.05, return_eids=True, seed=77)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = sampling.random_walk(g, nodes, length=12, prob="q", restart_prob=0.05, return_eids=True, seed=77)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, got))


def test_table_and_metapath_through_the_workspace(dev, graphs):
    """More than 16 relations, or more than 256 steps, do not fit the kernel arguments: the table and the metapath are
    then read from the workspace — the same walks."""
    from dgl_amd import _capi

    R, _ = graphs[False]
    seeds = _seeds(np.random.default_rng(6), R)
    d_seeds = torch.from_numpy(seeds).to(dev)
    one = _device_table(R, None, torch.int64, dev)
    for rels, path in (([one] * 17, [(3 * t) % 17 for t in range(9)]), ([one], [0] * 300)):
        tr, ev = _capi.random_walk(rels, path, d_seeds, rng_seed=8)
        ht, he = host_walk([R] * len(rels), path, seeds, 8)
        assert np.array_equal(tr.cpu().numpy(), ht) and np.array_equal(ev.cpu().numpy(), he)
