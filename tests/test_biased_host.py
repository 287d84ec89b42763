"""Tag sort and biased sampling without a GPU: the host twins of the rules (compiled from csrc/biased_step.h) against the
independent model of tests/biased_cases.py on every case, the properties of the picks, the law of the picks against the
exact one, every refusal by its message, and the reference's two docstring examples through the public functions."""
import itertools
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import biased_cases as bc

CASES = bc.cases()
IDTYPES = [torch.int32, torch.int64]
_SORTED = {}


def host_csr(case, idtype, indices=None, data=None):
    from dgl_amd import _capi

    t = lambda a: None if a is None else torch.from_numpy(a).to(idtype)
    return _capi.host_csr(t(case["indptr"]), t(case["indices"]) if indices is None else indices,
                          t(case["data"]) if data is None else data, case["n"])


def host_sorted(case, idtype):
    """(indices, data, tag_pos) of the host sort, computed once per (case, id type) and left unchanged."""
    from dgl_amd import _capi

    key = (case["name"], idtype)
    if key not in _SORTED:
        _SORTED[key] = _capi.sort_csr_by_tag_host(host_csr(case, idtype), torch.from_numpy(case["tag"]), case["T"])
    return _SORTED[key]


@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_host_sort_equals_the_model(case, idtype):
    indices, data, tag_pos = host_sorted(case, idtype)
    want = bc.sort_model(case)
    assert indices.tolist() == want[0] and data.tolist() == want[1] and tag_pos.tolist() == want[2]
    assert indices.dtype == data.dtype == tag_pos.dtype == idtype


@pytest.mark.parametrize("idtype", IDTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_host_sampler_properties(case, idtype):
    from dgl_amd import _capi

    indices, data, tag_pos = host_sorted(case, idtype)
    csr = host_csr(case, idtype, indices, data)
    pos_of = np.empty(case["nnz"], dtype=np.int64)
    pos_of[data.numpy()] = np.arange(case["nnz"])
    offs, indptr = tag_pos.tolist(), case["indptr"]
    for seeds, fanout, replace, kind, bdt, rng_seed in case["calls"]:
        bias = bc.bias_of(kind, case["T"], bdt)
        args = (csr, tag_pos, torch.from_numpy(bias), torch.tensor(seeds, dtype=idtype), fanout, replace)
        out_indptr, nbr, eids = _capi.sample_neighbors_biased_host(*args, rng_seed)
        what = (seeds[:4], fanout, replace, kind)
        assert np.diff(out_indptr.numpy()).tolist() == [bc.picks_model(offs[s], bias, fanout, replace) for s in seeds], what
        pos = pos_of[eids.numpy()]
        assert torch.equal(nbr, indices[torch.from_numpy(pos)]), what
        ok = bc.positive(bias)
        for i, s in enumerate(seeds):
            rel = pos[out_indptr[i]: out_indptr[i + 1]] - indptr[s]
            tags = np.searchsorted(np.asarray(offs[s]), rel, side="right") - 1
            assert np.all((rel >= 0) & (rel < indptr[s + 1] - indptr[s])) and all(ok[t] for t in tags), (what, s)
            if not replace:
                assert len(set(rel.tolist())) == len(rel), (what, s)
            if fanout < 0:
                assert rel.tolist() == [q for t in range(case["T"]) if ok[t] for q in range(offs[s][t], offs[s][t + 1])], (what, s)
        again = _capi.sample_neighbors_biased_host(*args, rng_seed)
        other = _capi.sample_neighbors_biased_host(*args, rng_seed + 1)
        assert all(torch.equal(a, b) for a, b in zip(again, (out_indptr, nbr, eids))), what
        if 0 < fanout <= 17 and kind == "uniform" and len(seeds) > 50:
            assert torch.equal(other[0], out_indptr) and not torch.equal(other[2], eids), what


def _exact_law(sizes, bias, fanout, replace):
    """{sorted tuple of positions: probability} of the picks of one row by successive sampling, enumerated."""
    weight = [Fraction(b).limit_denominator(1000) for n, b in zip(sizes, bias) for _ in range(n)]
    law = Counter()
    for seq in (itertools.product if replace else itertools.permutations)(range(len(weight)), **(
            {"repeat": fanout} if replace else {"r": fanout})):
        p, left = Fraction(1), sum(weight)
        for q in seq:
            p *= weight[q] / left
            if not replace:
                left -= weight[q]
        law[tuple(sorted(seq))] += p
    return law


@pytest.mark.parametrize("fanout,replace,bound", [(2, False, 54.63530553003881), (1, True, 35.888186879672865)])
def test_the_law_of_the_picks(fanout, replace, bound):
    """Tag sizes (2, 3, 1), bias (1, 2, 0.5), rng seeds 0 .. 19999: Pearson's statistic of the observed sets against the
    exact law stays below the chi-square quantile at 1 - 1e-6 (14 and 5 degrees of freedom).  The generator is counter-
    based, so the statistic is a fixed number: 10.58 without and 2.93 with replacement."""
    from dgl_amd import _capi

    sizes, bias, draws = (2, 3, 1), (1.0, 2.0, 0.5), 20000
    csr = _capi.host_csr(torch.tensor([0, 6]), torch.arange(6), None, 6)
    offsets, b, seeds = torch.tensor([[0, 2, 5, 6]]), torch.tensor(bias, dtype=torch.float64), torch.tensor([0])
    seen = Counter(tuple(sorted(_capi.sample_neighbors_biased_host(csr, offsets, b, seeds, fanout, replace, s)[2].tolist()))
                   for s in range(draws))
    law = _exact_law(sizes, bias, fanout, replace)
    assert sum(law.values()) == 1 and set(seen) <= set(law)
    stat = sum((seen[k] - draws * float(p)) ** 2 / (draws * float(p)) for k, p in law.items())
    print("pearson", fanout, replace, stat)
    assert stat < bound


def test_refusals_by_message():
    from dgl_amd import DGLAMDError, _capi

    csr = _capi.host_csr(torch.tensor([0, 2, 3]), torch.tensor([1, 0, 1]), None, 2)
    tag = torch.tensor([0, 1, 1])
    with pytest.raises(DGLAMDError, match="sort_csr_by_tag_host: unsupported tag dtype torch.int16"):
        _capi.sort_csr_by_tag_host(csr, tag.to(torch.int16), 2)
    for bad in ([0, 2, 1], [0, -1, 1]):
        with pytest.raises(DGLAMDError, match=r"sort_csr_by_tag_host: a tag lies outside \[0, 2\)"):
            _capi.sort_csr_by_tag_host(csr, torch.tensor(bad), 2)
    with pytest.raises(DGLAMDError, match="sort_csr_by_tag_host: num_tags must be positive, got 0"):
        _capi.sort_csr_by_tag_host(csr, tag, 0)
    off, bias, seeds = torch.tensor([[0, 1, 2], [0, 0, 1]]), torch.tensor([1.0, 1.0]), torch.tensor([0, 1])
    who = "sample_neighbors_biased_host: "
    with pytest.raises(DGLAMDError, match=who + "unsupported bias dtype torch.float16"):
        _capi.sample_neighbors_biased_host(csr, off, bias.half(), seeds, 1)
    with pytest.raises(DGLAMDError, match=who + r"a seed lies outside \[0, 2\)"):
        _capi.sample_neighbors_biased_host(csr, off, bias, torch.tensor([0, 2]), 1)
    with pytest.raises(DGLAMDError, match=who + r"fanout must be -1 \(all\), 0 or positive, got -2"):
        _capi.sample_neighbors_biased_host(csr, off, bias, seeds, -2)
    with pytest.raises(DGLAMDError, match=who + "tag_offset must be a contiguous"):
        _capi.sample_neighbors_biased_host(csr, off[:1], bias, seeds, 1)
    with pytest.raises(DGLAMDError, match=who + "num_tags 1025 exceeds the limit of 1024 tags"):
        _capi.sample_neighbors_biased_host(csr, torch.zeros((2, 1026), dtype=torch.int64), torch.ones(1025), seeds, 1)
    assert _capi.sample_neighbors_biased_host(csr, off, bias, seeds, -1)[2].tolist() == [0, 1, 2]


def test_the_reference_docstring_examples():
    import dgl_amd as dgl

    g = dgl.graph(([0, 0, 0, 0, 0, 1, 1, 1], [0, 1, 2, 3, 4, 0, 1, 2]))
    g.ndata["x"] = torch.arange(5.0)
    want = [[0, 2, 4, 5], [0, 1, 3, 3], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    for tag, kind in ((torch.IntTensor([1, 1, 0, 2, 0]), "node"), (torch.tensor([1, 1, 0, 2, 0, 1, 1, 0]), "edge")):
        s = dgl.sort_csr_by_tag(g, tag, tag_type=kind)
        assert s._graph.relations[0].csr()[1].tolist() == [2, 4, 0, 1, 3, 2, 0, 1]
        assert s.srcdata["_TAG_OFFSET"].tolist() == want and s.ndata["x"] is g.ndata["x"] and "_TAG_OFFSET" not in g.ndata
        assert all(torch.equal(a, b) for a, b in zip(s.edges(order="eid"), g.edges(order="eid")))
    c = dgl.sort_csc_by_tag(g, torch.tensor([1, 0, 0, 0, 0]), tag_offset_name="off")
    assert c._graph.relations[0].csc()[1].tolist() == [1, 0, 1, 0, 1, 0, 0, 0] and c.dstdata["off"].tolist()[0] == [0, 1, 2]
    g = dgl.graph(([0, 0, 1, 1, 2, 2], [1, 2, 0, 1, 2, 0]))
    s = dgl.transforms.sort_csr_by_tag(g, torch.IntTensor([0, 0, 1]))
    assert s.ndata["_TAG_OFFSET"].tolist() == [[0, 1, 2], [0, 2, 2], [0, 1, 2]]
    sg = dgl.sampling.sample_neighbors_biased(s, [0, 2], 3, torch.tensor([1.0, 0.001]), edge_dir="out")
    assert [t.tolist() for t in sg.edges(order="eid")] == [[0, 0, 2, 2], [1, 2, 0, 2]] and sg.num_nodes() == 3
    assert sorted(sg.edata[dgl.EID].tolist()) == [0, 1, 4, 5]
    one = dgl.sampling.sample_neighbors_biased(s, [0, 2], 1, [1.0, 0.0], edge_dir="out", seed=3)
    assert one.edata[dgl.EID].tolist() == [0, 5]
    with pytest.raises(dgl.DGLError, match="no tag offsets"):
        dgl.sampling.sample_neighbors_biased(s, [0], 1, [1.0, 1.0], tag_offset_name="absent")
