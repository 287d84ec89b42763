"""Neighbour matching on the device (csrc/matching.hip): device == host bit for bit (labels and rounds) on every case of
tests/matching_cases.py, under every batching of rounds between read-backs, with and without a caller's workspace, the
relabelled form too; then the Python surface as the reference's test_edge_coarsening checks it
(tests/python/pytorch/geometry/test_geometry.py)."""
import numpy as np
import pytest
import torch

from tests import matching_cases as mc

pytestmark = pytest.mark.gpu

CASES = mc.cases()
_HOST = {}


def host(case, form, seed, idtype):
    """The host twin's (label, rounds, relabelled), computed once per (case, form, seed, id type)."""
    from dgl_amd import _capi

    key = (case["name"], form, seed, idtype)
    if key not in _HOST:
        w = mc.weights(case, form)
        t = lambda a: None if a is None else torch.from_numpy(a).to(idtype)
        csr = _capi.host_csr(t(case["indptr"]), t(case["indices"]), t(case["data"]), case["n"])
        lab, rounds, rel = _capi.neighbor_matching_host(csr, None if w is None else torch.from_numpy(w), seed, relabel=True)
        _HOST[key] = (lab.numpy(), rounds, rel.numpy())
    return _HOST[key]


def device_csr(case, idtype, dev):
    from dgl_amd import _capi

    t = lambda a: None if a is None else torch.from_numpy(a).to(idtype).to(dev)
    return _capi.make_csr(t(case["indptr"]), t(case["indices"]), t(case["data"]), case["n"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("form", mc.FORMS)
def test_device_equals_host_bit_for_bit(dev, case, form):
    from dgl_amd import _capi

    w = mc.weights(case, form)
    wd = None if w is None else torch.from_numpy(w).to(dev)
    for idtype in (torch.int32, torch.int64):
        csr = device_csr(case, idtype, dev)
        for seed in mc.SEEDS[:2]:
            want, rounds, relabelled = host(case, form, seed, idtype)
            label, used = _capi.neighbor_matching(csr, wd, seed)
            assert label.dtype == idtype and np.array_equal(label.cpu().numpy(), want), (case["name"], form, seed)
            assert used == rounds
            got, used = _capi.neighbor_matching(csr, wd, seed, relabel=True)
            assert np.array_equal(got.cpu().numpy(), relabelled) and used == rounds


@pytest.mark.parametrize("batch", [1, 4, 64])
def test_batching_and_workspace_change_nothing(dev, batch):
    from dgl_amd import _capi, _lib

    for case in CASES:
        for form, idtype in (("none", torch.int32), ("special", torch.int64)):
            w = mc.weights(case, form)
            wd = None if w is None else torch.from_numpy(w).to(dev)
            csr = device_csr(case, idtype, dev)
            want, rounds, relabelled = host(case, form, 1, idtype)
            need = _lib.LIB.dgla_neighbor_matching_workspace_bytes(csr.idtype_bits, case["n"])
            for ws in (None, torch.empty(need, dtype=torch.uint8, device=dev)):
                label, used = _capi.neighbor_matching(csr, wd, 1, batch_rounds=batch, workspace=ws)
                assert np.array_equal(label.cpu().numpy(), want) and used == rounds, (case["name"], form, batch)
                got, _ = _capi.neighbor_matching(csr, wd, 1, relabel=True, batch_rounds=batch, workspace=ws)
                assert np.array_equal(got.cpu().numpy(), relabelled)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
def test_short_workspace_is_refused(dev, idtype):
    """need - 256 bytes: the matching and the relabelling both refuse it, in the one wording, before any launch."""
    from dgl_amd import DGLAMDError, _capi, _lib

    case = min(CASES, key=lambda c: c["n"])
    csr = device_csr(case, idtype, dev)
    n = case["n"]
    need = _lib.LIB.dgla_neighbor_matching_workspace_bytes(csr.idtype_bits, n)
    assert need > 256
    short = torch.empty(need - 256, dtype=torch.uint8, device=dev)
    with pytest.raises(DGLAMDError, match="neighbor_matching: workspace of %d bytes required, got %d" % (need, need - 256)):
        _capi.neighbor_matching(csr, None, 1, workspace=short)
    label = torch.arange(n, dtype=idtype, device=dev)
    out = torch.full_like(label, -7)
    with pytest.raises(DGLAMDError, match="neighbor_matching_relabel: workspace of %d bytes required, got %d"
                                          % (need, need - 256)):
        _lib.check_call(_lib.LIB.dgla_neighbor_matching_relabel(label.data_ptr(), csr.idtype_bits, n, out.data_ptr(),
                                                                short.data_ptr(), need - 256,
                                                                torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert bool((out == -7).all())


def test_round_cap_on_the_device(dev):
    from dgl_amd import DGLAMDError, _capi

    cyc = mc.csr_of(3, [0, 1, 2], [1, 2, 0])
    csr = device_csr(cyc, torch.int64, dev)
    for batch in (3, 8, 64):
        with pytest.raises(DGLAMDError, match=r"neighbor_matching: .*max_rounds = 8.*not bi-directed"):
            _capi.neighbor_matching(csr, None, 3, max_rounds=8, batch_rounds=batch)
    # a graph that needs exactly its rounds passes at that cap and fails below it, as on the host
    grid = next(c for c in CASES if c["name"] == "grid16x16")
    want, rounds, _ = host(grid, "none", 0, torch.int64)
    gcsr = device_csr(grid, torch.int64, dev)
    label, used = _capi.neighbor_matching(gcsr, None, 0, max_rounds=rounds)
    assert used == rounds and np.array_equal(label.cpu().numpy(), want)
    with pytest.raises(DGLAMDError, match="not bi-directed"):
        _capi.neighbor_matching(gcsr, None, 0, max_rounds=rounds - 1)


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("weight", [False, True])
@pytest.mark.parametrize("relabel", [False, True])
def test_edge_coarsening_surface(dev, idtype, weight, relabel):
    """The checks of the reference's test_edge_coarsening on ``dgl_amd.geometry.neighbor_matching``."""
    import dgl_amd
    from dgl_amd.geometry import neighbor_matching

    n = 600
    pairs = np.array(mc.random_pairs(n, 4 * n, 7))
    g = dgl_amd.graph((torch.from_numpy(pairs[:, 0]), torch.from_numpy(pairs[:, 1])), num_nodes=n, idtype=idtype)
    g = dgl_amd.add_self_loop(dgl_amd.to_bidirected(g)).to(dev)          # given with its self-loops
    ew = torch.rand(g.num_edges(), device=dev) if weight else None
    res = neighbor_matching(g, ew, relabel_idx=relabel, seed=5)
    assert res.shape == (n,) and res.dtype == idtype and res.device.type == "cuda"
    assert int(res.min()) >= 0
    ids, counts = torch.unique(res, return_counts=True)
    assert n // 2 <= ids.numel() <= n
    if relabel:
        assert torch.equal(ids.cpu(), torch.arange(ids.numel(), dtype=idtype))
    assert int(counts.max()) <= 2
    order = torch.argsort(res, stable=True)
    srt = res[order]
    twin = srt[1:] == srt[:-1]
    u, v = order[:-1][twin].to(idtype), order[1:][twin].to(idtype)
    assert bool(g.has_edges_between(u, v).all()) and bool((u != v).all())
    assert torch.equal(res, neighbor_matching(g, ew, relabel_idx=relabel, seed=5))


def test_weights_on_the_wrong_device_raise(dev):
    import dgl_amd
    from dgl_amd import DGLError
    from dgl_amd.geometry import neighbor_matching

    g = dgl_amd.graph((torch.tensor([0, 1, 1, 2]), torch.tensor([1, 0, 2, 1]))).to(dev)
    with pytest.raises(DGLError, match="e_weights is on cpu"):
        neighbor_matching(g, torch.ones(4))
    with pytest.raises(DGLError, match="one value per edge"):
        neighbor_matching(g, torch.ones(5, device=dev))
    with pytest.raises(DGLError, match="float16 / bfloat16"):
        neighbor_matching(g, torch.ones(4, device=dev, dtype=torch.float16))
    assert neighbor_matching(g, seed=None).shape == (3,)


def test_large_graph_ends_under_the_default_cap(dev):
    """20 000 nodes at mean degree 8 (more than one wavefront of workgroups; the 16-lane group)."""
    from dgl_amd import _capi

    n = 20000
    pairs = np.array(mc.random_pairs(n, 4 * n, 11))
    src, dst = mc.both_ways(pairs)
    case = mc.csr_of(n, src, dst)
    case["name"] = "random20000"
    csr = device_csr(case, torch.int32, dev)
    label, used = _capi.neighbor_matching(csr, None, 2)
    want, rounds, _ = host(case, "none", 2, torch.int32)
    print("rounds used at 20 000 nodes:", used)
    assert used == rounds < _capi.MATCHING_MAX_ROUNDS
    assert np.array_equal(label.cpu().numpy(), want)
    mc.check_properties(case, want)
