"""Top-k neighbour selection on the device (csrc/topk.hip): device == host twin, element for element, on every case of
tests/topk_cases.py (both id types, both directions, every weight type, with and without a caller's workspace; the table
crosses all three size classes of the kernel), the refusals that need the device followed by a successful call, the
Python function on GPU graphs against the same call on the CPU copy, and a captured call replayed with other weights."""
import numpy as np
import pytest
import torch

from tests import topk_cases as tc

pytestmark = pytest.mark.gpu

CASES = tc.cases()
IDTYPES = [torch.int32, torch.int64]


def csr_pair(case, idtype, dev):
    """(host dgla_csr, device dgla_csr) of one graph of the table."""
    from dgl_amd import _capi

    host = [None if case[k] is None else torch.from_numpy(case[k]).to(idtype) for k in ("indptr", "indices", "data")]
    there = [None if t is None else t.to(dev) for t in host]
    return _capi.host_csr(*host, case["n"]), _capi.make_csr(*there, case["n"])


def same(got, want, what):
    total = int(want[0][-1])
    assert all(t.is_cuda and t.dtype == want[0].dtype for t in got), what
    assert torch.equal(got[0].cpu(), want[0]), what
    assert torch.equal(got[1][:total].cpu(), want[1]) and torch.equal(got[2][:total].cpu(), want[2]), what


@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_device_equals_the_host_twin(dev, case, idtype):
    from dgl_amd import _capi

    h_csr, d_csr = csr_pair(case, idtype, dev)
    calls = [(torch.tensor(seeds, dtype=idtype), k) for seeds, k in case["calls"]]
    ws = torch.empty(_capi.select_topk_workspace_bytes(idtype, max(len(s) for s, _ in calls)), dtype=torch.uint8, device=dev)
    for name, (dt, w) in case["weights"].items():
        if idtype == torch.int32 and name.split("/")[0] not in ("dups", "specials", "extremes"):
            continue                                                 # (the id width does not meet the weights: a sample)
        wt = tc.torch_weight(dt, w)
        wd = wt.to(dev)
        for ascending in (False, True):
            for seeds, k in calls:
                want = _capi.select_topk_host(h_csr, wt, seeds, k, ascending)
                for workspace in (None, ws):
                    got = _capi.select_topk(d_csr, wd, seeds.to(dev), k, ascending, workspace=workspace)
                    same(got, want, (case["name"], name, ascending, k, workspace is not None))


def test_device_refusals_and_a_usable_library_afterwards(dev):
    from dgl_amd import DGLAMDError, _capi

    deg = _capi.select_topk_max_picks() + 1
    host = [torch.tensor([0, deg, deg + 3]), torch.zeros(deg + 3, dtype=torch.int64), None]
    h_hub = _capi.host_csr(*host, 2)
    d_hub = _capi.make_csr(host[0].to(dev), host[1].to(dev), None, 2)
    wh = torch.arange(deg + 3, dtype=torch.float32)
    wd = wh.to(dev)
    ids = lambda *a: torch.tensor(a, dtype=torch.int64, device=dev)
    for k in (-1, deg):
        with pytest.raises(DGLAMDError, match="select_topk: a row yields 1025 picks, which exceeds the limit of 1024"):
            _capi.select_topk(d_hub, wd, ids(1, 0), k)
    with pytest.raises(DGLAMDError, match=r"select_topk: a seed lies outside \[0, 2\)"):
        _capi.select_topk(d_hub, wd, ids(1, 2), -1)
    with pytest.raises(DGLAMDError, match=r"select_topk: a seed lies outside \[0, 2\)"):
        _capi.select_topk(d_hub, wd, ids(-1), 5000)
    need = _capi.select_topk_workspace_bytes(torch.int64, 2)
    with pytest.raises(DGLAMDError, match="select_topk: workspace of %d bytes required, got %d" % (need, need - 256)):
        _capi.select_topk(d_hub, wd, ids(1, 0), 2, workspace=torch.empty(need - 256, dtype=torch.uint8, device=dev))
    with pytest.raises(DGLAMDError, match="unsupported weight dtype"):
        _capi.select_topk(d_hub, wd.to(torch.int16), ids(0), 1)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        _capi.select_topk(d_hub, wh, ids(0), 1)
    # the next calls succeed: the same hub within the limit, and the one-call form, where a seed outside the graph is an
    # empty row that touches no memory
    for seeds, k in (((1, 0), 1024), ((1,), -1), ((0, 0), 3)):
        want = _capi.select_topk_host(h_hub, wh, torch.tensor(seeds), k)
        same(_capi.select_topk(d_hub, wd, ids(*seeds), k), want, (seeds, k))
    got = _capi.select_topk(d_hub, wd, ids(1, 7, -4, 1), 2)
    assert got[0].tolist() == [0, 2, 2, 2, 4] and got[2][:4].tolist() == [deg + 2, deg + 1, deg + 2, deg + 1]


def _cpu_graphs():
    import dgl_amd as dgl

    rng = np.random.default_rng(5)
    n, e = 300, 9000
    src, dst = torch.from_numpy(rng.integers(0, n, e)), torch.from_numpy(rng.integers(0, n, e))
    g = dgl.graph((src, dst), num_nodes=n)
    g.edata["w"] = torch.from_numpy(rng.integers(0, 50, e).astype(np.float32))       # many ties
    g.edata["tag"] = torch.arange(e)
    g.ndata["x"] = torch.arange(n, dtype=torch.float32)
    pairs = lambda a, b, m: (torch.from_numpy(rng.integers(0, a, m)), torch.from_numpy(rng.integers(0, b, m)))
    hg = dgl.heterograph({("user", "follow", "user"): pairs(60, 60, 900), ("user", "play", "game"): pairs(60, 20, 700),
                          ("game", "liked-by", "user"): pairs(20, 60, 500)},
                         num_nodes_dict={"user": 60, "game": 20})
    for etype, m in (("follow", 900), ("play", 700), ("liked-by", 500)):
        hg.edges[etype].data["w"] = torch.from_numpy(rng.standard_normal(m))
    return g, hg


def _same_graph(a, b):
    import dgl_amd as dgl

    assert a.ntypes == b.ntypes and a.canonical_etypes == b.canonical_etypes
    for c in a.canonical_etypes:
        assert a.num_edges(c) == b.num_edges(c), c
        for x, y in zip(a.edges(etype=c, order="eid"), b.edges(etype=c, order="eid")):
            assert x.is_cuda and torch.equal(x.cpu(), y), c
        assert torch.equal(a.edges[c].data[dgl.EID].cpu(), b.edges[c].data[dgl.EID]), c


def test_the_python_function_on_gpu_graphs_equals_the_cpu_copy(dev):
    import dgl_amd as dgl

    g, hg = _cpu_graphs()
    dg, dhg = g.to(dev), hg.to(dev)
    for k, nodes, edge_dir, ascending in ((3, None, "in", False), (40, [5, 5, 299, 0], "out", True), (-1, [7, 8], "in", False),
                                          (2000, None, "out", False)):
        want = dgl.sampling.select_topk(g, k, "w", nodes, edge_dir=edge_dir, ascending=ascending)
        got = dgl.sampling.select_topk(dg, k, "w", nodes, edge_dir=edge_dir, ascending=ascending)
        _same_graph(got, want)
        assert torch.equal(got.edata["tag"].cpu(), want.edata["tag"]) and torch.equal(got.ndata["x"].cpu(), g.ndata["x"])
    for k, nodes, edge_dir in ((2, {"user": [0, 1, 59], "game": [3]}, "in"), ({"follow": 1, "play": -1, "liked-by": 0}, None, "out"),
                               (5, {"game": torch.arange(20)}, "in")):
        _same_graph(dgl.sampling.select_topk(dhg, k, "w", nodes, edge_dir=edge_dir),
                    dgl.sampling.select_topk(hg, k, "w", nodes, edge_dir=edge_dir))
    back = dgl.sampling.select_topk(dg, 1, "w", output_device=torch.device("cpu"))
    assert back.device.type == "cpu" and back.num_edges() == int((g.in_degrees() > 0).sum())


def test_a_captured_call_replays_with_other_weights(dev):
    """0 < k <= 1024 with a workspace: no read-back and no allocation by the library, so the call can be captured."""
    from dgl_amd import _capi
    from dgl_amd.capture import CapturedStep

    case = next(c for c in CASES if c["name"] == "short-permuted")
    h_csr, d_csr = csr_pair(case, torch.int64, dev)
    seeds = torch.arange(case["n"])
    d_seeds = seeds.to(dev)
    ws = torch.empty(_capi.select_topk_workspace_bytes(torch.int64, case["n"]), dtype=torch.uint8, device=dev)
    w0 = tc.torch_weight(*case["weights"]["dups/f4"])
    w1 = tc.torch_weight(*case["weights"]["specials/f4"])
    step = CapturedStep(lambda weight: _capi.select_topk(d_csr, weight, d_seeds, 7, workspace=ws), {"weight": w0.to(dev)})
    same(step(weight=w1.to(dev)), _capi.select_topk_host(h_csr, w1, seeds, 7), "replay")
