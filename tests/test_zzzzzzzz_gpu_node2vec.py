"""node2vec walks on the device (csrc/node2vec.hip) against the host walker of tests/test_node2vec_host.py:
dgla_csr_sorted_columns == a per-row numpy sort, node2vec_walk_kernel == dgla_node2vec_walk_host bit for bit (the two
compile one step rule, csrc/node2vec_step.h) with the paths of the rule shown to be exercised, p == q == 1 == random_walk,
and the public dgl_amd.sampling.node2vec_random_walk.  Reference: python/dgl/sampling/node2vec_randomwalk.py over
src/graph/sampling/randomwalks/node2vec_randomwalk.h (CPU only)."""
import numpy as np
import pytest
import torch

from tests.test_node2vec_host import MODERATE, PQ, host_n2v, member_of, node2vec_graph, walk_seeds
from tests.test_random_walk_host import check_properties, messy_weights

pytestmark = pytest.mark.gpu

N, E, HUB = 2000, 15000, 5000       # 15 000 random edges and their reverses, cliques, a multigraph hub row of 5000
WALKS = 5003                        # no multiple of 64


@pytest.fixture(scope="module")
def graphs():
    """COO in random order (edge-id map present) and row-sorted (map absent) with messy weights; built once, never
    modified.  The membership list of the host side is numpy's per-row sort."""
    out = {}
    for presorted in (False, True):
        R, ne = node2vec_graph(presorted, N, E, HUB)
        deg = np.diff(R["indptr"])
        assert deg.max() >= HUB and (deg == 0).any() and (deg == 1).any() and 30000 < ne < 45000
        rng = np.random.default_rng(19)
        ws = {"f32": messy_weights(ne, rng, np.float32), "f64": messy_weights(ne, rng, np.float64)}
        out[presorted] = (R, ws, member_of(R))
    return out


def _seeds():
    s = walk_seeds(N, WALKS)[:WALKS]
    assert len(s) == WALKS
    return s


def _device_csr(R, idtype, dev):
    from dgl_amd import _capi

    t_ = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=idtype)
    return _capi.make_csr(t_(R["indptr"]), t_(R["indices"]), t_(R["data"]), R["num_cols"])


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("presorted", [False, True])
def test_sorted_columns(dev, graphs, idtype, presorted):
    from dgl_amd import _capi

    R, _, want = graphs[presorted]
    csr = _device_csr(R, idtype, dev)
    got = _capi.csr_sorted_columns(csr)
    again = _capi.csr_sorted_columns(csr)
    assert got.dtype == idtype and got.shape == (len(want),)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    deg = np.diff(R["indptr"])
    row = want[R["indptr"][np.argmax(deg)]:][:deg.max()]
    assert deg.max() >= HUB and (np.diff(row) == 0).any() and (deg == 0).sum() >= 10     # duplicates, empty rows


def test_sorted_columns_of_an_empty_graph(dev):
    from dgl_amd import _capi

    csr = _capi.make_csr(torch.zeros(6, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), None, 5)
    assert _capi.csr_sorted_columns(csr).shape == (0,)


def _classes(R, tr):
    """Class of every hop t >= 1 of the traces (0: back to prev, 1: x -> prev exists, 2: neither), -1 where none."""
    n = R["num_rows"]
    src = np.repeat(np.arange(n), np.diff(R["indptr"]))
    edges = np.unique(src * n + R["indices"])
    prev, x = tr[:, :-2], tr[:, 2:]
    went = x >= 0
    cls = np.where(np.isin(np.where(went, x * n + prev, -1), edges), 1, 2)
    cls[x == prev] = 0
    return np.where(went, cls, -1)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("presorted", [False, True])
@pytest.mark.parametrize("weights", [None, "f32", "f64"])
def test_device_equals_host_walker(dev, graphs, idtype, presorted, weights):
    from dgl_amd import _capi

    R, ws, member = graphs[presorted]
    csr = _device_csr(R, idtype, dev)
    cdf = None if weights is None else _capi.random_walk_cdf(csr, torch.from_numpy(ws[weights]).to(dev))
    Rh = dict(R, cdf=None if cdf is None else cdf.cpu().numpy())        # the device-built CDF, copied to the host
    d_member = _capi.csr_sorted_columns(csr)
    seeds = _seeds()
    d_seeds = torch.from_numpy(seeds).to(device=dev, dtype=idtype)
    moderate_steps, moderate_cls = 0, np.zeros(3)
    for p, q in PQ:
        for steps in (1, 7, 40):
            seed = 1000 * steps + 7
            tr, ev = _capi.node2vec_walk(csr, cdf, d_member, d_seeds, steps, p, q, rng_seed=seed)
            assert tr.dtype == idtype and tr.shape == (WALKS, steps + 1) and ev.shape == (WALKS, steps)
            ht, he, stats = host_n2v(Rh, seeds, steps, seed, p, q, idtype=idtype, stats=True, member=member)
            assert np.array_equal(tr.cpu().numpy(), ht) and np.array_equal(ev.cpu().numpy(), he), (p, q, steps)
        # the 40-step walks: the paths of the rule they took, by the host walker's counters and the traces' classes
        cls = _classes(R, ht)
        assert stats[0] == (cls >= 0).sum()
        print("(p, q) = (%g, %g): %d steps, %.3f attempts per step, %d reached the scan, classes %s"
              % (p, q, stats[0], stats[1] / stats[0], stats[2], np.bincount(cls[cls >= 0], minlength=3).tolist()))
        if (p, q) in MODERATE:
            moderate_steps += stats[0]
            moderate_cls += np.bincount(cls[cls >= 0], minlength=3)
            assert stats[1] > stats[0]                                    # some step needed a second attempt
        elif (p, q) == (1.0, 1.0):
            assert stats[1] == stats[0] and stats[2] == 0
        else:
            assert stats[2] >= 100
    assert (moderate_cls >= 0.01 * moderate_steps).all()
    check_properties([Rh], [0] * 40, ht, he, seed, None, [None if weights is None else ws[weights]])
    tr2, none = _capi.node2vec_walk(csr, cdf, d_member, d_seeds, 40, p, q, rng_seed=seed, return_eids=False)
    assert none is None and torch.equal(tr2, tr)
    # zero steps and zero seeds
    tr0, ev0 = _capi.node2vec_walk(csr, cdf, d_member, d_seeds, 0, p, q)
    assert tr0.shape == (WALKS, 1) and ev0.shape == (WALKS, 0) and torch.equal(tr0[:, 0], d_seeds)
    tr0, ev0 = _capi.node2vec_walk(csr, cdf, d_member, d_seeds[:0], 5, p, q)
    assert tr0.shape == (0, 6) and ev0.shape == (0, 5)


@pytest.fixture(scope="module")
def homo(dev, graphs):
    import dgl_amd

    R, ws, _ = graphs[False]
    order = np.argsort(R["data"])                                       # CSR positions in edge-id order
    src = np.repeat(np.arange(N), np.diff(R["indptr"]))[order]
    dst = R["indices"][order]
    g = dgl_amd.graph((torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)), num_nodes=N)
    return g, torch.from_numpy(dst).to(dev), ws["f32"]


@pytest.mark.parametrize("weighted", [False, True])
def test_p_q_one_equals_random_walk(dev, homo, weighted):
    from dgl_amd import sampling

    g, _, w = homo
    prob = None
    if weighted:
        g.edata["w"] = torch.from_numpy(w).to(dev)
        prob = "w"
    nodes = torch.from_numpy(_seeds()[8:]).to(dev)
    for s in (3, 2 ** 61 + 5):
        tr, ev = sampling.node2vec_random_walk(g, nodes, 1, 1, 12, prob=prob, return_eids=True, seed=s)
        rt, re_, _ = sampling.random_walk(g, nodes, length=12, prob=prob, return_eids=True, seed=s)
        assert torch.equal(tr, rt) and torch.equal(ev, re_)
    if weighted:
        assert g._graph.relations[0]._walk_cdf is not None              # one CDF slot for both walks


def test_public_api(dev, homo):
    from dgl_amd import sampling

    g, dst, _ = homo
    rel = g._graph.relations[0]
    nodes = torch.arange(777, device=dev) % (N - 100)
    a = sampling.node2vec_random_walk(g, nodes, 0.5, 2, 6, return_eids=True, seed=5)
    slot = rel._walk_members
    b = sampling.node2vec_random_walk(g, nodes, 0.5, 2, 6, return_eids=True, seed=5)
    c = sampling.node2vec_random_walk(g, nodes, 0.5, 2, 6, return_eids=True, seed=6)
    assert rel._walk_members is slot                                     # the membership list is built once
    assert len(a) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    assert a[0].shape == (777, 7) and a[1].shape == (777, 6) and a[0].dtype == a[1].dtype == g.idtype
    u, v = g.edges()
    went = a[1] >= 0
    assert torch.equal(u[a[1][went]], a[0][:, :-1][went]) and torch.equal(v[a[1][went]], a[0][:, 1:][went])
    only = sampling.node2vec_random_walk(g, nodes, 0.5, 2, 6, seed=5)
    assert torch.is_tensor(only) and torch.equal(only, a[0])
    torch.manual_seed(123)
    d = sampling.node2vec_random_walk(g, nodes, 2, 0.5, 6)
    e = sampling.node2vec_random_walk(g, nodes, 2, 0.5, 6)
    torch.manual_seed(123)
    f = sampling.node2vec_random_walk(g, nodes, 2, 0.5, 6)
    assert torch.equal(d, f) and not torch.equal(d, e)
    tr = sampling.node2vec_random_walk(g, nodes, 2, 0.5, 0)
    assert tr.shape == (777, 1) and torch.equal(tr[:, 0], nodes)
    tr, ev = sampling.node2vec_random_walk(g, nodes[:0], 2, 0.5, 6, return_eids=True)
    assert tr.shape == (0, 7) and ev.shape == (0, 6)
    assert sampling.node2vec_random_walk(g, [0, 1, 2], 2, 0.5, 3, seed=1).shape == (3, 4)      # a list of ids
    # an in-place write to the weights rebuilds the CDF and leaves the membership list alone
    even = (dst % 2 == 0).float()
    g.edata["p"] = even.clone()
    tr = sampling.node2vec_random_walk(g, nodes, 0.5, 2, 4, prob="p", seed=9)
    took = tr[:, 1:][tr[:, 1:] >= 0]
    assert took.numel() > 500 and bool((took % 2 == 0).all())
    cdf_slot = rel._walk_cdf
    sampling.node2vec_random_walk(g, nodes, 0.5, 2, 4, prob="p", seed=10)
    assert rel._walk_cdf is cdf_slot
    g.edata["p"].copy_(1 - even)
    tr = sampling.node2vec_random_walk(g, nodes, 0.5, 2, 4, prob="p", seed=9)
    took = tr[:, 1:][tr[:, 1:] >= 0]
    assert took.numel() > 500 and bool((took % 2 == 1).all())
    assert rel._walk_cdf is not cdf_slot and rel._walk_members is slot


def test_int32_graph_and_non_default_stream(dev, homo):
    import dgl_amd
    from dgl_amd import sampling

    g, _, _ = homo
    u, v = g.edges()
    g32 = dgl_amd.graph((u.int(), v.int()), num_nodes=N, idtype=torch.int32)
    nodes = torch.arange(3000, device=dev) % (N - 100)
    want = sampling.node2vec_random_walk(g, nodes, 4, 0.25, 12, return_eids=True, seed=77)
    got32 = sampling.node2vec_random_walk(g32, nodes.int(), 4, 0.25, 12, return_eids=True, seed=77)
    assert got32[0].dtype == torch.int32 and torch.equal(got32[0].long(), want[0]) and torch.equal(got32[1].long(), want[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = sampling.node2vec_random_walk(g, nodes, 4, 0.25, 12, return_eids=True, seed=77)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, got))
