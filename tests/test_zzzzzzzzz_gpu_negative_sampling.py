"""Negative sampling on the device (csrc/negative_sampling.hip) against the host function of
tests/test_negative_sampling_host.py: the kernels == dgla_negative_sample_host bit for bit (the two compile one rule,
csrc/negative_sample_step.h) at the block, tile, small-sort, small-scan and item-length boundaries of csrc/sort.hip.h,
dgla_csr_has_edges == host, DGLGraph.has_edges_between == the torch lines it replaces on a GPU graph, the padded and the
sliced form of dgl_amd.sampling.global_uniform_negative_sampling, a graph capture, and the one membership list per
relation.  Reference: python/dgl/sampling/negative.py over src/array/cuda/negative_sampling.cu."""
import numpy as np
import pytest
import torch

from tests.test_negative_sampling_host import FLAGS, GRAPHS, edge_set, host_csr_of, host_neg, make_graph, member_of

pytestmark = pytest.mark.gpu

SLOTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16385, 32769]
LARGE = 600000           # past kSmallInput of the sort (8192-element items) and kScanSmall of the scan


def samples_for(n_slots):
    """Three quarters of the slots: sparse graphs truncate, dense graphs pad."""
    return n_slots * 3 // 4 + 1


@pytest.fixture(scope="module")
def graphs():
    """Every graph with its host lookup (int64) — built once, never modified."""
    out = {}
    for name in GRAPHS:
        R = make_graph(name)
        out[name] = (R, host_csr_of(R, torch.int64))
    return out


@pytest.fixture(scope="module")
def host_results(graphs):
    """The host function's answers, computed once per case and shared by both id types (the host test shows that the
    id type does not change the values)."""
    memo = {}

    def get(name, n_slots, num_samples, T, excl, replace, seed):
        key = (name, n_slots, num_samples, T, excl, replace, seed)
        if key not in memo:
            R, lookup = graphs[name]
            memo[key] = host_neg(R, n_slots, num_samples, T, excl, replace, seed, lookup=lookup)
        return memo[key]

    return get


def device_lookup(R, idtype, dev):
    from dgl_amd import _capi

    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=idtype)
    csr = _capi.make_csr(t_(R["indptr"]), t_(R["indices"]), None, R["num_cols"])
    member = _capi.csr_sorted_columns(csr)
    assert np.array_equal(member.cpu().numpy().astype(np.int64), member_of(R))
    return csr, member


def check_case(csr, member, want, n_slots, num_samples, T, excl, replace, seed):
    from dgl_amd import _capi

    runs = [_capi.negative_sample(csr, member, n_slots, num_samples, T, excl, replace, seed) for _ in range(2)]
    (s1, d1, c1), (s2, d2, c2) = [tuple(t.cpu() for t in r) for r in runs]
    case = (n_slots, num_samples, T, excl, replace, seed)
    assert s1.numpy().tobytes() == s2.numpy().tobytes() and d1.numpy().tobytes() == d2.numpy().tobytes(), case
    assert int(c1) == int(c2) == want[2], case
    assert np.array_equal(s1.numpy().astype(np.int64), want[0]), case
    assert np.array_equal(d1.numpy().astype(np.int64), want[1]), case
    return int(c1)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", GRAPHS)
def test_device_equals_host(dev, graphs, host_results, name, idtype):
    R, _ = graphs[name]
    csr, member = device_lookup(R, idtype, dev)
    counts = []
    for k, n_slots in enumerate(SLOTS):
        T, seed = (1, 8) if k % 3 == 1 else (3, 7)
        for excl, replace in FLAGS:
            ns = samples_for(n_slots)
            counts.append(check_case(csr, member, host_results(name, n_slots, ns, T, excl, replace, seed), n_slots, ns, T,
                                     excl, replace, seed))
    # more samples asked for than slots drawn, and no slots at all: padding beyond the slots
    for excl, replace in FLAGS:
        check_case(csr, member, host_results(name, 257, 1000, 3, excl, replace, 42), 257, 1000, 3, excl, replace, 42)
        check_case(csr, member, host_results(name, 0, 5, 3, excl, replace, 42), 0, 5, 3, excl, replace, 42)
    assert (max(counts) == 0) == (name == "complete")


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", GRAPHS)
def test_device_equals_host_at_the_large_size(dev, graphs, host_results, name, idtype):
    """600 000 slots on every graph.  random20, bipartite and one_edge hold few distinct pairs (long runs of one pair in a
    bucket); hub hardly any duplicate; on complete every slot is empty, so the sort carries 600 000 fillers; on empty
    600 000 draws fall into 10^6 cells, so many distinct pairs and many repeats share bucket runs and a walk has to step
    over other pairs before it meets its own."""
    R, _ = graphs[name]
    csr, member = device_lookup(R, idtype, dev)
    ns = samples_for(LARGE)
    for excl, replace in FLAGS:
        got = check_case(csr, member, host_results(name, LARGE, ns, 3, excl, replace, 7), LARGE, ns, 3, excl, replace, 7)
        cells = R["num_rows"] * R["num_cols"]
        if name == "complete":
            assert got == 0
        elif name == "hub" or (name == "empty" and replace):
            assert got == ns              # sparse: more than three quarters of the slots survive
        elif name == "empty":
            assert 0.4 * cells < got <= ns                  # 1 - exp(-0.6) = 0.451 of the 10^6 cells are hit
        else:
            assert 0 < got <= (ns if replace else cells)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", GRAPHS)
def test_has_edges_equals_host(dev, graphs, name, idtype):
    from dgl_amd import _capi

    R, _ = graphs[name]
    edges = edge_set(R)
    csr, member = device_lookup(R, idtype, dev)
    h_csr, h_member = host_csr_of(R, idtype)
    nr, nc = R["num_rows"], R["num_cols"]
    rng = np.random.default_rng(4)
    u = np.concatenate([rng.integers(0, nr, 5000), [-1, nr, 0, 0, nr - 1, 2 ** 31 - 1, -2 ** 31, 0]])
    v = np.concatenate([rng.integers(0, nc, 5000), [0, 0, -1, nc, nc, 0, 0, 2 ** 31 - 1]])
    if edges:
        eu, ev = np.array(sorted(edges)[::max(1, len(edges) // 700)]).T
        u, v = np.concatenate([u, eu]), np.concatenate([v, ev])
    u, v = torch.as_tensor(u).to(idtype), torch.as_tensor(v).to(idtype)
    want = _capi.csr_has_edges_host(h_csr, h_member, u, v)
    got = _capi.csr_has_edges(csr, member, u.to(dev), v.to(dev))
    assert got.dtype == torch.bool and torch.equal(got.cpu(), want)
    assert bool(want.any()) == bool(edges)
    assert _capi.csr_has_edges(csr, member, u[:0].to(dev), v[:0].to(dev)).shape == (0,)


def torch_has_edges(g, u, v, etype=None):
    """The lines DGLGraph.has_edges_between ran before the kernel (and still runs on a CPU graph)."""
    src, dst = g.edges(etype=etype)
    n_dst = max(g._graph.relations[g.get_etype_id(etype)].num_dst, 1)
    key = torch.sort(src.long() * n_dst + dst.long())[0]
    want = u.long() * n_dst + v.long()
    if key.numel() == 0:
        return torch.zeros_like(want, dtype=torch.bool)
    at = torch.searchsorted(key, want).clamp(max=key.numel() - 1)
    return key[at] == want


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_has_edges_between_on_a_gpu_graph(dev, idtype):
    import dgl_amd

    rng = np.random.default_rng(6)
    s, d = rng.integers(0, 300, 4000), rng.integers(0, 300, 4000)
    g = dgl_amd.graph((torch.as_tensor(s), torch.as_tensor(d)), num_nodes=300, idtype=idtype, device=dev)
    u = torch.as_tensor(np.concatenate([rng.integers(0, 300, 3000), s[:500]]), device=dev)
    v = torch.as_tensor(np.concatenate([rng.integers(0, 300, 3000), d[:500]]), device=dev)
    got = g.has_edges_between(u, v)
    assert got.dtype == torch.bool and got.shape == u.shape and torch.equal(got, torch_has_edges(g, u, v))
    assert got[3000:].all() and not got.all()
    assert g.has_edges_between(int(s[0]), int(d[0])).tolist() == [True]
    assert torch.equal(g.has_edges_between(int(s[0]), v), torch_has_edges(g, torch.full_like(v, int(s[0])), v))
    hg = dgl_amd.heterograph({("user", "follow", "user"): (torch.as_tensor(s[:900] % 50), torch.as_tensor(d[:900] % 50)),
                              ("user", "view", "item"): (torch.as_tensor(s % 50), torch.as_tensor(d % 120)),
                              ("item", "sold", "user"): (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))},
                             num_nodes_dict={"user": 50, "item": 120}, idtype=idtype, device=dev)
    hu, hv = torch.as_tensor(rng.integers(0, 50, 4000), device=dev), torch.as_tensor(rng.integers(0, 120, 4000), device=dev)
    got = hg.has_edges_between(hu, hv, etype="view")
    assert torch.equal(got, torch_has_edges(hg, hu, hv, "view")) and got.any() and not got.all()
    got = hg.has_edges_between(hu, hv % 50, etype=("user", "follow", "user"))
    assert torch.equal(got, torch_has_edges(hg, hu, hv % 50, "follow")) and got.any() and not got.all()
    got = hg.has_edges_between(hv, hu, etype="sold")                         # the empty relation
    assert got.shape == hu.shape and not got.any()


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_public_function(dev, idtype):
    import dgl_amd
    from dgl_amd import negative_sampler, sampling

    rng = np.random.default_rng(9)
    s, d = rng.integers(0, 200, 3000), rng.integers(0, 200, 3000)
    g = dgl_amd.graph((torch.as_tensor(s), torch.as_tensor(d)), num_nodes=200, idtype=idtype, device=dev)
    for excl, replace in FLAGS:
        src, dst = sampling.global_uniform_negative_sampling(g, 1000, excl, replace, seed=5)
        ps, pd, count = g.global_uniform_negative_sampling(1000, excl, replace, seed=5, padded=True)
        k = int(count)
        assert src.dtype == idtype and src.device == g.device and ps.shape == pd.shape == (1000,) and count.shape == (1,)
        assert k == src.shape[0] == dst.shape[0] and torch.equal(ps[:k], src) and torch.equal(pd[:k], dst)
        assert (ps[k:] == -1).all() and (pd[k:] == -1).all() and k >= 990          # the redundancy all but fills the request
        assert not g.has_edges_between(src, dst).any()
        assert not excl or (src != dst).all()
        pairs = set(zip(src.tolist(), dst.tolist()))
        assert replace or len(pairs) == k
    # a redundancy of the caller's is honoured.  10 nodes, every edge but i -> i + 1: 10 negative cells of 100, a slot
    # finds one with probability 1 - 0.9^3 = 0.271, so 1000 slots leave about 271 pairs and the default about 20 000
    u, v = np.divmod(np.arange(100), 10)
    keep = v != (u + 1) % 10
    dense = dgl_amd.graph((torch.as_tensor(u[keep]), torch.as_tensor(v[keep])), idtype=idtype, device=dev)
    few = sampling.global_uniform_negative_sampling(dense, 1000, True, True, redundancy=0.0, seed=5)[0]
    assert 271 - 6 * 15 < few.shape[0] < 271 + 6 * 15           # (binomial standard deviation 14.1)
    assert sampling.global_uniform_negative_sampling(dense, 1000, True, True, seed=5)[0].shape[0] == 1000
    assert sampling.global_uniform_negative_sampling(dense, 1000, True, True, redundancy=9.0, seed=5)[0].shape[0] == 1000
    src, dst = sampling.global_uniform_negative_sampling(dense, 1000, seed=5)
    assert sorted(zip(src.tolist(), dst.tolist())) == [(i, (i + 1) % 10) for i in range(10)]      # all ten, once each
    a =sampling.global_uniform_negative_sampling(g, 500, seed=11)
    b = sampling.global_uniform_negative_sampling(g, 500, seed=11)
    c = sampling.global_uniform_negative_sampling(g, 500, seed=12)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    torch.manual_seed(3)
    a = sampling.global_uniform_negative_sampling(g, 500)
    torch.manual_seed(3)
    b = sampling.global_uniform_negative_sampling(g, 500)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert [t.shape[0] for t in sampling.global_uniform_negative_sampling(g, 0)] == [0, 0]
    # a relation in which every pair is an edge, and the bipartite relation of a heterograph (self-loops mean nothing)
    u, v = np.divmod(np.arange(36), 6)
    full = dgl_amd.graph((torch.as_tensor(u), torch.as_tensor(v)), idtype=idtype, device=dev)
    src, dst, count = sampling.global_uniform_negative_sampling(full, 10, padded=True)
    assert int(count) == 0 and (src == -1).all() and src.shape == (10,)
    assert sampling.global_uniform_negative_sampling(full, 10)[0].shape == (0,)
    hg = dgl_amd.heterograph({("user", "follow", "user"): (torch.as_tensor(s[:400] % 30), torch.as_tensor(d[:400] % 30)),
                              ("user", "view", "item"): (torch.as_tensor(s[:600] % 30), torch.as_tensor(d[:600] % 80))},
                             num_nodes_dict={"user": 30, "item": 80}, idtype=idtype, device=dev)
    src, dst = sampling.global_uniform_negative_sampling(hg, 2000, True, True, etype="view", seed=2)
    assert src.shape[0] > 1900 and src.max() < 30 and 30 <= dst.max() < 80 and (src == dst).any()
    assert not hg.has_edges_between(src, dst, etype="view").any()
    # the sampler classes: a tensor in, pairs out; a dict in, a dict keyed by canonical edge types out
    eids = torch.arange(50, device=dev, dtype=idtype)
    src, dst = negative_sampler.GlobalUniform(3, seed=4)(g, eids)
    assert 140 < src.shape[0] <= 150 and not g.has_edges_between(src, dst).any() and (src != dst).all()
    out = negative_sampler.GlobalUniform(2, replace=True, seed=4)(hg, {"view": eids[:20], "follow": eids[:10]})
    assert set(out) == {("user", "view", "item"), ("user", "follow", "user")}
    assert 35 < out[("user", "view", "item")][0].shape[0] <= 40 and 0 < out[("user", "follow", "user")][0].shape[0] <= 20
    src, dst = negative_sampler.PerSourceUniform(3)(g, eids)
    assert src.tolist() == np.repeat(s[:50], 3).tolist() and dst.shape == (150,) and dst.dtype == idtype and dst.device == eids.device


def test_sampling_inside_a_graph_capture(dev):
    import dgl_amd
    from dgl_amd import sampling

    rng = np.random.default_rng(10)
    g = dgl_amd.graph((torch.as_tensor(rng.integers(0, 500, 6000)), torch.as_tensor(rng.integers(0, 500, 6000))),
                      num_nodes=500, device=dev)
    step = lambda: sampling.global_uniform_negative_sampling(g, 5000, seed=21, padded=True)
    eager = [t.clone() for t in step()]          # warm-up: builds the CSR and the membership list
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(a, b)
    assert 4900 < int(eager[2]) <= 5000


def test_one_membership_list_per_relation(dev, monkeypatch):
    import dgl_amd
    from dgl_amd import _capi, sampling

    built = []
    real = _capi.csr_sorted_columns
    monkeypatch.setattr(_capi, "csr_sorted_columns", lambda csr: built.append(csr.nnz) or real(csr))
    rng = np.random.default_rng(12)
    s, d = rng.integers(0, 100, 900), rng.integers(0, 100, 900)
    g = dgl_amd.graph((torch.as_tensor(s), torch.as_tensor(d)), num_nodes=100, device=dev)
    sampling.global_uniform_negative_sampling(g, 100, seed=1)
    g.has_edges_between(torch.as_tensor(s), torch.as_tensor(d))
    sampling.node2vec_random_walk(g, torch.arange(10), 0.5, 2.0, 4, seed=1)
    g.global_uniform_negative_sampling(100, replace=True, seed=2)
    g.has_edges_between([0, 1], [1, 2])
    assert built == [900]
    assert g._graph.relations[0]._walk_members[1].shape == (900,)
