"""Per-edge-type neighbour sampling without a GPU: the host twin of the rule (compiled from csrc/etype_step.h) against the
independent model of tests/etype_cases.py on every case, the law of the picks against the binomial bound, the Python
function on a shuffled graph, and the refusals by their messages."""
from collections import Counter

import numpy as np
import pytest
import torch

from tests import etype_cases as ec

CASES = ec.cases()


def host_call(case, seeds, fanout, replace, kind, rng_seed, idtype=torch.int64):
    from dgl_amd import _capi

    csr = _capi.host_csr(*[None if case[k] is None else torch.from_numpy(case[k]).to(idtype) for k in ("indptr", "indices", "data")],
                         case["n"])
    table = _capi.EtypeTable(case["off"])
    return _capi.sample_etype_neighbors_host(csr, table, table.fanouts(fanout), torch.tensor(seeds, dtype=idtype), replace, rng_seed,
                                             prob=ec.prob_of(case, kind))


def split(case, indptr, eids, fanout, want):
    """The picked edge ids per (seed slot, type), cut by the model's counts; the totals must agree."""
    got, at = [], 0
    for i, per in enumerate(want):
        assert int(indptr[i]) == at, (case["name"], i)
        got.append([])
        for ids, pos, cnt in per:
            got[-1].append(eids[at:at + cnt])
            at += cnt
    assert int(indptr[-1]) == at == len(eids), case["name"]
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_the_host_twin_against_the_model(case):
    where = {e: q for q, e in enumerate(range(case["nnz"]) if case["data"] is None else case["data"].tolist())}
    for k, (seeds, fanout, replace, kind, rng_seed) in enumerate(case["calls"]):
        prob = ec.prob_of(case, kind)
        want = ec.model(case, seeds, fanout, replace, prob)
        indptr, nbr, eids = (x.tolist() for x in host_call(case, seeds, fanout, replace, kind, rng_seed))
        assert nbr == [int(case["indices"][where[e]]) for e in eids]
        got = split(case, indptr, eids, fanout, want)
        first = {}
        for i, (u, per) in enumerate(zip(seeds, want)):
            assert got[i] == got[first.setdefault(u, i)], "a repeated seed repeats its picks"
            for t, (ids, pos, cnt) in enumerate(per):
                picks, what = got[i][t], (case["name"], k, u, t)
                assert set(picks) <= set(pos), what                      # in the type's range, never a zero or NaN weight
                if not replace:
                    assert len(set(picks)) == len(picks), what
                if fanout[t] < 0 or (not replace and cnt == len(pos)):
                    assert picks == pos, what                            # the full range, in position order
        if k in (0, 5):          # another fan-out for type 0 leaves the picks of every other type as they were
            other = [7 if fanout[0] != 7 else 3] + fanout[1:]
            res = host_call(case, seeds, other, replace, kind, rng_seed)
            again = split(case, res[0].tolist(), res[2].tolist(), other, ec.model(case, seeds, other, replace, prob))
            assert all(a[1:] == b[1:] for a, b in zip(again, got)), case["name"]


@pytest.mark.parametrize("replace, weights", [(False, None), (True, (1.0, 2.0, 3.0, 4.0, 0.0))], ids=["uniform", "weighted-replace"])
def test_the_law_of_the_picks_on_one_row(replace, weights):
    """One row with ranges of 5 and 9 entries, f = 2, R = 4000 rng seeds.  Without replacement an entry of a range of n
    is picked by a call with probability f / n, so its count over R calls is Binomial(R, f / n); with replacement and
    weights w a call makes f independent draws with p = w / sum(w), so the count is Binomial(R f, p).  Every count must lie
    within 5 standard deviations, 5 sqrt(N p (1 - p)), of its mean N p: derived, not measured."""
    from dgl_amd import _capi

    R, f = 4000, 2
    csr = _capi.host_csr(torch.tensor([0, 14]), torch.zeros(14, dtype=torch.int64), None, 1)
    table = _capi.EtypeTable([0, 5, 14])
    prob = None if weights is None else table.probs([torch.tensor(weights, dtype=torch.float64), None])
    fan, seeds = table.fanouts([f, f]), torch.tensor([0])
    seen = Counter()
    for s in range(R):
        seen.update(_capi.sample_etype_neighbors_host(csr, table, fan, seeds, replace, s, prob=prob)[2].tolist())
    for e in range(14):
        n = 5 if e < 5 else 9
        if replace:
            N, p = R * f, (weights[e] / sum(weights) if e < 5 else 1.0 / 9)
        else:
            N, p = R, f / n
        print("edge %d: %d picks, expected %.1f +- %.1f" % (e, seen[e], N * p, 5 * (N * p * (1 - p)) ** 0.5))
        assert abs(seen[e] - N * p) <= 5 * (N * p * (1 - p)) ** 0.5, e


def test_the_python_function_sorts_a_shuffled_graph_once():
    import dgl_amd as dgl

    rng = np.random.default_rng(3)
    n, e, off = 40, 900, [0, 100, 100, 450, 900]
    src, dst = torch.from_numpy(rng.integers(0, n, e)), torch.from_numpy(rng.integers(0, n, e))
    g = dgl.graph((src, dst), num_nodes=n)
    g.edata["mark"], g.ndata["x"] = torch.arange(e) * 2, torch.arange(n, dtype=torch.float32)
    g.edata["p"] = torch.from_numpy(rng.choice(np.array([0.0, 1.0, 2.0], dtype=np.float32), e))
    nodes, fanout = [3, 3, 17, 0, 39], torch.tensor([2, 5, -1, 3])
    etype = np.searchsorted(off, np.arange(e), side="right") - 1
    for edge_dir, own, prob in (("in", dst, None), ("out", src, ["p", None, None, g.edata["p"][450:]])):
        sg = g.sample_etype_neighbors({"_N": nodes}, off, fanout, edge_dir=edge_dir, prob=prob, seed=5)
        picked = sg.edata[dgl.EID].tolist()
        usable = [i for i in range(e) if prob is None or prob[etype[i]] is None or float(g.edata["p"][i]) > 0]
        want = Counter()
        for u in nodes:
            for t, f in enumerate(fanout.tolist()):
                have = sum(1 for i in usable if int(own[i]) == u and etype[i] == t)
                want[(u, t)] += have if f < 0 else min(f, have)
        assert Counter((int(own[i]), etype[i]) for i in picked) == want
        assert all(i in usable for i in picked)
        assert torch.equal(sg.edata["mark"], sg.edata[dgl.EID] * 2) and torch.equal(sg.ndata["x"], g.ndata["x"])
        assert sg.num_nodes() == n and len(getattr(g._graph.relations[0], "_etype_sorted")[0][1]) == 5
        again = dgl.sampling.sample_etype_neighbors(g, nodes, off, fanout, edge_dir=edge_dir, prob=prob, seed=5)
        assert again.edata[dgl.EID].tolist() == picked
    with pytest.raises(dgl.DGLAMDError, match="exclude_edges is not supported for sample_etype_neighbors"):
        g.sample_etype_neighbors(nodes, off, fanout, exclude_edges=[0])
    with pytest.raises(dgl.DGLAMDError, match="The fanout should be a tensor"):
        g.sample_etype_neighbors(nodes, off, [1, 1, 1, 1])


def test_refusals_by_name():
    from dgl_amd import DGLAMDError, _capi

    csr = _capi.host_csr(torch.tensor([0, 2, 3]), torch.tensor([1, 0, 1]), None, 2)
    who, seeds = "sample_etype_neighbors_host: ", torch.tensor([0, 1])
    table = _capi.EtypeTable([0, 2, 3], who=who[:-2])
    for bad in ([0, 2, 1], [1, 2, 3], [0]):
        with pytest.raises(DGLAMDError, match="etype_offset must be non-decreasing and start at 0"):
            _capi.EtypeTable(bad)
    with pytest.raises(DGLAMDError, match="num_etypes 1025 exceeds the limit of 1024 edge types"):
        _capi.EtypeTable([0] * 1026)
    with pytest.raises(DGLAMDError, match=who + r"fanout must hold one integer per edge type \(2\)"):
        _capi.sample_etype_neighbors_host(csr, table, torch.tensor([1, 1, 1]), seeds)
    with pytest.raises(DGLAMDError, match=who + r"prob must list one tensor or None per edge type \(2\)"):
        _capi.sample_etype_neighbors_host(csr, table, table.fanouts([1, 1]), seeds, prob=[None])
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(DGLAMDError, match=who + "unsupported prob dtype " + str(dt)):
            _capi.sample_etype_neighbors_host(csr, table, table.fanouts([1, 1]), seeds, prob=[torch.ones(2, dtype=dt), None])
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        _capi.sample_etype_neighbors(csr, table, table.fanouts([1, 1]), seeds)
    assert _capi.sample_etype_neighbors_host(csr, table, table.fanouts([-1, -1]), seeds)[2].tolist() == [0, 1, 2]
