"""Per-edge-type neighbour sampling on the device (csrc/etype.hip): device == host twin, element for element, on every
case of tests/etype_cases.py (both id types, both group widths, one and several chunks of types, every prob type), with
and without a caller's workspace and with every output and the workspace between guard bands; an unsorted row under
etype_sorted=True; the Python function on a GPU graph against its CPU copy; and a captured call replayed with other
fan-outs."""
import numpy as np
import pytest
import torch

from tests import etype_cases as ec
from tests.guarded import POISON_INDEX, POISON_INT_OUT, guarded

pytestmark = pytest.mark.gpu

CASES = ec.cases()


def csr_pair(case, idtype, dev):
    from dgl_amd import _capi

    host = [None if case[k] is None else torch.from_numpy(case[k]).to(idtype) for k in ("indptr", "indices", "data")]
    return _capi.host_csr(*host, case["n"]), _capi.make_csr(*[None if t is None else t.to(dev) for t in host], case["n"])


def on(dev, prob):
    return None if prob is None else [None if p is None else p.to(dev) for p in prob]


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_device_equals_the_host_twin(dev, case, idtype):
    from dgl_amd import _capi

    h_csr, d_csr = csr_pair(case, idtype, dev)
    h_tab, d_tab = _capi.EtypeTable(case["off"]), _capi.EtypeTable(case["off"], dev)
    for seeds, fanout, replace, kind, rng_seed in case["calls"]:
        prob = ec.prob_of(case, kind)
        seeds = torch.tensor(seeds, dtype=idtype)
        ref = _capi.sample_etype_neighbors_host(h_csr, h_tab, h_tab.fanouts(fanout), seeds, replace, rng_seed, prob=prob)
        total, n = int(ref[0][-1]), len(seeds)
        ws = guarded(dev, _capi.sample_etype_neighbors_workspace_bytes(idtype, n), torch.uint8, poison=POISON_INDEX)
        d_prob = d_tab.probs(on(dev, prob))
        for workspace in (None, ws.t):
            outs = [guarded(dev, s, idtype, poison=POISON_INT_OUT) for s in (n + 1, total, total)]
            res = _capi.sample_etype_neighbors(d_csr, d_tab, d_tab.fanouts(fanout), seeds.to(dev), replace, rng_seed, prob=d_prob,
                                               ws=workspace, into=[o.t for o in outs])
            what = (case["name"], replace, kind, workspace is not None)
            for o in outs + [ws]:
                o.check(str(what))
            assert all(torch.equal(a.cpu(), b) for a, b in zip(res, ref)), what
        sized = _capi.sample_etype_neighbors(d_csr, d_tab, d_tab.fanouts(fanout), seeds.to(dev), replace, rng_seed, prob=d_prob)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(sized, ref)), (case["name"], "sizes first")


def test_an_unsorted_row_stays_inside_its_row_and_a_correct_call_follows(dev):
    """etype_sorted=True is a promise that is not tested: on a row whose types are out of order the picks are unspecified,
    but the guard bands stay intact, every pick is an entry of its seed's row, and the next call is right."""
    from dgl_amd import _capi

    case = next(c for c in CASES if c["name"].startswith("T17"))
    rng = np.random.default_rng(4)
    data = torch.from_numpy(rng.permutation(case["nnz"]))                   # no row is ordered by type any more
    indptr, indices = (torch.from_numpy(case[k]) for k in ("indptr", "indices"))
    d_csr = _capi.make_csr(indptr.to(dev), indices.to(dev), data.to(dev), case["n"])
    d_tab = _capi.EtypeTable(case["off"], dev)
    seeds = torch.arange(case["n"])
    for replace, kind in ((False, None), (True, "f8"), (False, "f4")):
        fan = d_tab.fanouts([3] * case["T"])
        cap = 3 * case["T"] * case["n"]
        ws = guarded(dev, _capi.sample_etype_neighbors_workspace_bytes(torch.int64, case["n"]), torch.uint8, poison=POISON_INDEX)
        outs = [guarded(dev, s, torch.int64, poison=POISON_INT_OUT) for s in (case["n"] + 1, cap, cap)]
        res = _capi.sample_etype_neighbors(d_csr, d_tab, fan, seeds.to(dev), replace, 8, prob=on(dev, ec.prob_of(case, kind)), ws=ws.t,
                                           into=[o.t for o in outs])
        for o in outs + [ws]:
            o.check("unsorted row")
        ptr, eids = res[0].cpu(), res[2].cpu()
        assert 0 <= int(ptr[-1]) <= cap
        for u in range(case["n"]):
            assert set(eids[ptr[u]:ptr[u + 1]].tolist()) <= set(data[indptr[u]:indptr[u + 1]].tolist())
    h_csr, d_csr = csr_pair(case, torch.int64, dev)
    seeds, fanout, replace, kind, rng_seed = case["calls"][2]
    h_tab, seeds = _capi.EtypeTable(case["off"]), torch.tensor(seeds)
    ref = _capi.sample_etype_neighbors_host(h_csr, h_tab, h_tab.fanouts(fanout), seeds, replace, rng_seed, prob=ec.prob_of(case, kind))
    res = _capi.sample_etype_neighbors(d_csr, d_tab, d_tab.fanouts(fanout), seeds.to(dev), replace, rng_seed,
                                       prob=on(dev, ec.prob_of(case, kind)))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(res, ref))


def test_the_python_function_on_a_gpu_graph_equals_the_cpu_copy(dev):
    import dgl_amd as dgl

    rng = np.random.default_rng(7)
    n, e, T = 300, 9000, 20
    off = [0] + sorted(rng.integers(0, e, T - 1).tolist()) + [e]
    g = dgl.graph((torch.from_numpy(rng.integers(0, n, e)), torch.from_numpy(rng.integers(0, n, e))), num_nodes=n)
    g.edata["mark"], g.ndata["x"] = torch.arange(e), torch.arange(n, dtype=torch.float32)
    g.edata["p"] = torch.from_numpy(rng.choice(np.array([0.0, 0.5, 2.0]), e))
    fanout = torch.tensor([(0, 1, 3, 40, -1)[t % 5] for t in range(T)])
    got = g.to(dev)
    for edge_dir in ("in", "out"):
        srt = dgl.sort_csc_by_tag if edge_dir == "in" else dgl.sort_csr_by_tag
        tag = torch.from_numpy(np.searchsorted(off, np.arange(e), side="right") - 1)
        pairs = [(g, got, False), (srt(g, tag, tag_type="edge"), srt(got, tag.to(dev), tag_type="edge"), True)]
        for want_g, got_g, etype_sorted in pairs:
            for replace, prob in ((False, None), (True, ["p" if t % 2 else None for t in range(T)])):
                kw = dict(edge_dir=edge_dir, prob=prob, replace=replace, etype_sorted=etype_sorted, seed=13)
                a = dgl.sampling.sample_etype_neighbors(got_g, [5, 5, 19, 0, 299], off, fanout, **kw)
                b = dgl.sampling.sample_etype_neighbors(want_g, [5, 5, 19, 0, 299], off, fanout, **kw)
                assert a.num_edges() == b.num_edges() > 0 and torch.equal(a.edata[dgl.EID].cpu(), b.edata[dgl.EID])
                for x, y in zip(a.edges(order="eid"), b.edges(order="eid")):
                    assert x.is_cuda and torch.equal(x.cpu(), y)
                assert torch.equal(a.edata["mark"].cpu(), b.edata[dgl.EID]) and torch.equal(a.ndata["x"].cpu(), g.ndata["x"])


def test_a_captured_call_replays_with_other_fanouts(dev):
    """Every fan-out >= 0, a workspace and a capacity: no read-back and no allocation by the library, so the call can be
    captured; three replays per fan-out tensor against the host twin."""
    from dgl_amd import _capi
    from dgl_amd.capture import CapturedStep

    case = next(c for c in CASES if c["name"].startswith("T17"))
    h_csr, d_csr = csr_pair(case, torch.int64, dev)
    h_tab, d_tab = _capi.EtypeTable(case["off"]), _capi.EtypeTable(case["off"], dev)
    seeds, T = torch.arange(case["n"]), case["T"]
    d_seeds = seeds.to(dev)
    prob = ec.prob_of(case, "f4")
    d_prob = d_tab.probs(on(dev, prob))
    ws = torch.empty(_capi.sample_etype_neighbors_workspace_bytes(torch.int64, case["n"]), dtype=torch.uint8, device=dev)
    f0, f1 = torch.tensor([(t * 5) % 7 for t in range(T)]), torch.tensor([(t * 3 + 1) % 7 for t in range(T)])
    cap = case["n"] * 6 * T
    step = CapturedStep(lambda fan: _capi.sample_etype_neighbors(d_csr, d_tab, fan, d_seeds, False, 9, prob=d_prob, ws=ws, capacity=cap),
                        {"fan": f0.to(dev)})
    for fan in (f1, f0, f1):
        ref = _capi.sample_etype_neighbors_host(h_csr, h_tab, fan, seeds, False, 9, prob=prob)
        for _ in range(3):
            res = step(fan=fan.to(dev))
            assert all(torch.equal(a[:len(b)].cpu(), b) for a, b in zip(res, ref))
