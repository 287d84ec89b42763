"""Tag sort and biased sampling on the device (csrc/biased.hip): device == host twin, element for element, on every case
of tests/biased_cases.py (both id types; the table crosses every unit class of the sort, both counter homes and all three
pick kernels), with and without a caller's workspace and with every output and the workspace between guard bands; the
refusals that need the device followed by successful calls; the Python functions on a GPU graph against the same calls on
its CPU copy; and a captured call replayed with another bias."""
import numpy as np
import pytest
import torch

from tests import biased_cases as bc
from tests.guarded import POISON_INDEX, POISON_INT_OUT, guarded

pytestmark = pytest.mark.gpu

CASES = bc.cases()
IDTYPES = [torch.int32, torch.int64]


def csr_pair(case, idtype, dev, indices=None, data=None):
    """(host dgla_csr, device dgla_csr) of one graph of the table, or of its sorted form."""
    from dgl_amd import _capi

    host = [None if case[k] is None else torch.from_numpy(case[k]).to(idtype) for k in ("indptr", "indices", "data")]
    if indices is not None:
        host[1], host[2] = indices, data
    there = [None if t is None else t.to(dev) for t in host]
    return _capi.host_csr(*host, case["n"]), _capi.make_csr(*there, case["n"])


def outputs(dev, idtype, *shapes):
    return [guarded(dev, s, idtype, poison=POISON_INT_OUT) for s in shapes]


@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_device_equals_the_host_twin(dev, case, idtype):
    from dgl_amd import _capi

    h_csr, d_csr = csr_pair(case, idtype, dev)
    tag = torch.from_numpy(case["tag"])
    want = _capi.sort_csr_by_tag_host(h_csr, tag, case["T"])
    outs = outputs(dev, idtype, case["nnz"], case["nnz"], (case["n"], case["T"] + 1))
    got = _capi.sort_csr_by_tag(d_csr, tag.to(dev), case["T"], into=[o.t for o in outs])
    for o, g, w in zip(outs, got, want):
        o.check("sort " + case["name"])
        assert torch.equal(g.cpu(), w), case["name"]

    h_csr, d_csr = csr_pair(case, idtype, dev, want[0], want[1])
    offsets = want[2].to(dev)
    for seeds, fanout, replace, kind, bdt, rng_seed in case["calls"]:
        bias = torch.from_numpy(bc.bias_of(kind, case["T"], bdt))
        seeds = torch.tensor(seeds, dtype=idtype)
        ref = _capi.sample_neighbors_biased_host(h_csr, want[2], bias, seeds, fanout, replace, rng_seed)
        total, n = int(ref[0][-1]), len(seeds)
        cap = n * fanout if fanout >= 0 else total
        ws = guarded(dev, _capi.sample_neighbors_biased_workspace_bytes(idtype, n), torch.uint8, poison=POISON_INDEX)
        for workspace in (None, ws.t):
            outs = outputs(dev, idtype, n + 1, cap, cap)
            res = _capi.sample_neighbors_biased(d_csr, offsets, bias.to(dev), seeds.to(dev), fanout, replace, rng_seed,
                                                ws=workspace, into=[o.t for o in outs])
            what = (case["name"], fanout, replace, kind, workspace is not None)
            for o in outs + [ws]:
                o.check(str(what))
            assert torch.equal(res[0].cpu(), ref[0]), what
            assert torch.equal(res[1][:total].cpu(), ref[1]) and torch.equal(res[2][:total].cpu(), ref[2]), what


def test_device_refusals_and_a_usable_library_afterwards(dev):
    from dgl_amd import DGLAMDError, _capi

    host = [torch.tensor([0, 2, 3]), torch.tensor([1, 0, 1]), None]
    h_csr, d_csr = _capi.host_csr(*host, 2), _capi.make_csr(host[0].to(dev), host[1].to(dev), None, 2)
    tag = torch.tensor([1, 0, 1])
    ids = lambda *a: torch.tensor(a, dtype=torch.int64, device=dev)
    with pytest.raises(DGLAMDError, match=r"sort_csr_by_tag: a tag lies outside \[0, 2\)"):
        _capi.sort_csr_by_tag(d_csr, ids(0, 2, 1), 2)
    with pytest.raises(DGLAMDError, match="sort_csr_by_tag: unsupported tag dtype torch.int16"):
        _capi.sort_csr_by_tag(d_csr, tag.to(dev).to(torch.int16), 2)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        _capi.sort_csr_by_tag(d_csr, tag, 2)
    want = _capi.sort_csr_by_tag_host(h_csr, tag, 2)
    got = _capi.sort_csr_by_tag(d_csr, tag.to(dev), 2)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)) and want[2].tolist() == [[0, 1, 2], [0, 0, 1]]
    h_srt = _capi.host_csr(host[0], want[0], want[1], 2)
    d_srt = _capi.make_csr(host[0].to(dev), got[0], got[1], 2)
    bias, who = torch.tensor([1.0, 3.0]), "sample_neighbors_biased: "
    with pytest.raises(DGLAMDError, match=who + r"a seed lies outside \[0, 2\)"):
        _capi.sample_neighbors_biased(d_srt, got[2], bias.to(dev), ids(1, 2), -1)
    need = _capi.sample_neighbors_biased_workspace_bytes(torch.int64, 2)
    with pytest.raises(DGLAMDError, match=who + "workspace of %d bytes required, got %d" % (need, need - 256)):
        _capi.sample_neighbors_biased(d_srt, got[2], bias.to(dev), ids(1, 0), 1, ws=torch.empty(need - 256, dtype=torch.uint8, device=dev))
    with pytest.raises(DGLAMDError, match=who + "unsupported bias dtype torch.float16"):
        _capi.sample_neighbors_biased(d_srt, got[2], bias.to(dev).half(), ids(0), 1)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        _capi.sample_neighbors_biased(d_srt, got[2], bias, ids(0), 1)
    # the next calls succeed; without a read-back a seed outside the graph is an empty row that touches no memory
    for seeds, fanout in (((1, 0), -1), ((0, 0, 1), 2)):
        ref = _capi.sample_neighbors_biased_host(h_srt, want[2], bias, torch.tensor(seeds), fanout, False, 5)
        res = _capi.sample_neighbors_biased(d_srt, got[2], bias.to(dev), ids(*seeds), fanout, False, 5)
        assert all(torch.equal(a[:len(b)].cpu(), b) for a, b in zip(res, ref)), (seeds, fanout)
    assert _capi.sample_neighbors_biased(d_srt, got[2], bias.to(dev), ids(1, 7, -4, 0), 1)[0].tolist() == [0, 1, 1, 1, 2]


def test_the_python_functions_on_a_gpu_graph_equal_the_cpu_copy(dev):
    import dgl_amd as dgl

    rng = np.random.default_rng(6)
    n, e = 300, 9000
    g = dgl.graph((torch.from_numpy(rng.integers(0, n, e)), torch.from_numpy(rng.integers(0, n, e))), num_nodes=n)
    g.edata["mark"], g.ndata["x"] = torch.arange(e), torch.arange(n, dtype=torch.float32)
    bg = dgl.heterograph({("user", "play", "game"): (torch.from_numpy(rng.integers(0, 60, 700)), torch.from_numpy(rng.integers(0, 20, 700)))},
                         num_nodes_dict={"user": 60, "game": 20})
    node_tag, edge_tag = torch.from_numpy(rng.integers(0, 5, n)), torch.from_numpy(rng.integers(0, 70, e)).int()
    bias5, bias70 = torch.tensor([1.0, 0.0, 2.0, 0.5, 4.0]), torch.linspace(0.0, 3.0, 70, dtype=torch.float64)
    for graph, sort, fmt, tag, kind, bias, edge_dir in (
            (g, dgl.sort_csc_by_tag, "csc", node_tag, "node", bias5, "in"), (g, dgl.sort_csr_by_tag, "csr", edge_tag, "edge", bias70, "out"),
            (bg, dgl.sort_csr_by_tag, "csr", torch.from_numpy(rng.integers(0, 3, 20)), "node", bias5[:3], "out")):
        want, got = sort(graph, tag, tag_type=kind), sort(graph.to(dev), tag.to(dev), tag_type=kind)
        for a, b in zip(getattr(got._graph.relations[0], fmt)(), getattr(want._graph.relations[0], fmt)()):
            assert a.is_cuda and torch.equal(a.cpu(), b), (fmt, kind)
        a, b = ([f["_TAG_OFFSET"] for f in x._node_frames if "_TAG_OFFSET" in f] for x in (got, want))
        assert len(a) == len(b) == 1 and torch.equal(a[0].cpu(), b[0]) and not any("_TAG_OFFSET" in f for f in graph._node_frames)
        for fanout, nodes, replace in ((3, [5, 5, 19, 0], False), (40, list(range(20)), True), (-1, [7, 8], False)):
            a = dgl.sampling.sample_neighbors_biased(got, nodes, fanout, bias, edge_dir=edge_dir, replace=replace, seed=11)
            b = dgl.sampling.sample_neighbors_biased(want, nodes, fanout, bias, edge_dir=edge_dir, replace=replace, seed=11)
            assert a.num_edges() == b.num_edges() > 0 and torch.equal(a.edata[dgl.EID].cpu(), b.edata[dgl.EID])
            for x, y in zip(a.edges(order="eid"), b.edges(order="eid")):
                assert x.is_cuda and torch.equal(x.cpu(), y)
            if graph is g:
                assert torch.equal(a.edata["mark"].cpu(), b.edata[dgl.EID]) and torch.equal(a.ndata["x"].cpu(), g.ndata["x"])


def test_a_captured_call_replays_with_another_bias(dev):
    """fanout >= 0 with a workspace: no read-back and no allocation by the library, so the call can be captured; three
    replays per bias against the host twin."""
    from dgl_amd import _capi
    from dgl_amd.capture import CapturedStep

    case = next(c for c in CASES if c["name"].startswith("short-T17"))
    h_csr, _ = csr_pair(case, torch.int64, dev)
    srt = _capi.sort_csr_by_tag_host(h_csr, torch.from_numpy(case["tag"]), case["T"])
    h_csr, d_csr = csr_pair(case, torch.int64, dev, srt[0], srt[1])
    seeds = torch.arange(case["n"])
    d_seeds, offsets = seeds.to(dev), srt[2].to(dev)
    ws = torch.empty(_capi.sample_neighbors_biased_workspace_bytes(torch.int64, case["n"]), dtype=torch.uint8, device=dev)
    b0, b1 = (torch.from_numpy(bc.bias_of(kind, case["T"], "f8")) for kind in ("uniform", "zero-tag"))
    step = CapturedStep(lambda bias: _capi.sample_neighbors_biased(d_csr, offsets, bias, d_seeds, 7, False, 9, ws=ws), {"bias": b0.to(dev)})
    for bias in (b1, b0, b1):
        ref = _capi.sample_neighbors_biased_host(h_csr, srt[2], bias, seeds, 7, False, 9)
        for _ in range(3):
            res = step(bias=bias.to(dev))
            assert all(torch.equal(a[:len(b)].cpu(), b) for a, b in zip(res, ref))
