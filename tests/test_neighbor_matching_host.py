"""Neighbour matching, the rule run by the CPU (dgla_neighbor_matching_host, csrc/matching.hip over csrc/matching_step.h):
equal to the independent numpy model of tests/matching_cases.py on every case, form and seed, with the consequences the
header states, the statistics of the tie-break, the weighted preference, the round cap and every refusal.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import matching_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mc.cases()
IDTYPES = [torch.int32, torch.int64]
NAMES = ("dgla_neighbor_matching_workspace_bytes", "dgla_neighbor_matching", "dgla_neighbor_matching_relabel",
         "dgla_neighbor_matching_host")


def host_csr(case, idtype):
    from dgl_amd import _capi

    t = lambda a: None if a is None else torch.from_numpy(a).to(idtype)
    return _capi.host_csr(t(case["indptr"]), t(case["indices"]), t(case["data"]), case["n"])


def run_host(case, weight=None, seed=0, idtype=torch.int64, **kw):
    from dgl_amd import _capi

    w = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight))
    out = _capi.neighbor_matching_host(host_csr(case, idtype), w, seed, **kw)
    return tuple(o.numpy() if torch.is_tensor(o) else o for o in out)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("form", mc.FORMS)
def test_host_equals_model_with_its_properties(case, form):
    w = mc.weights(case, form)
    for seed in mc.SEEDS:
        want, rounds = mc.model(case["indptr"], case["indices"], case["data"], w, seed)
        mc.check_properties(case, want)
        for idtype in IDTYPES:
            label, used, relabelled = run_host(case, w, seed, idtype, relabel=True)
            assert label.dtype == (np.int32 if idtype == torch.int32 else np.int64)
            assert np.array_equal(label, want) and used == rounds, (case["name"], form, seed)
            assert np.array_equal(relabelled, np.unique(want, return_inverse=True)[1])
        again = run_host(case, w, seed)
        assert np.array_equal(again[0], want) and again[1] == rounds          # the same seed, the same result


def test_seeds_change_the_matching():
    grid = next(c for c in CASES if c["name"] == "grid16x16")
    labels = {run_host(grid, None, s)[0].tobytes() for s in range(8)}
    assert len(labels) == 8


def test_unweighted_ties_break_evenly():
    """Path 0 - 1 - 2: node 1 pairs with node 0 in a share within 5 sigma of one half over 2 000 seeds,
    |f - 0.5| <= 5 sqrt(0.25 / 2000) = 0.056."""
    path = CASES[0]
    assert path["name"] == "path3"
    hits = 0
    for s in range(2000):
        label = run_host(path, None, s)[0]
        assert label[1] in (0, 1) and (label[1] == 0) != (label[2] == 1)   # 1 pairs with exactly one end
        hits += int(label[1] == 0)
    f = hits / 2000
    print("share of seeds in which node 1 pairs with node 0:", f)
    assert abs(f - 0.5) <= 5 * (0.25 / 2000) ** 0.5


def test_star_hub_takes_the_heaviest_leaf():
    """With distinct weights the hub of the star pairs in round 0 with the heaviest leaf of the OTHER colour: a BLUE hub
    proposes to its heaviest RED leaf, whose only proposer it is; a RED hub picks the heaviest of the BLUE leaves, which
    all propose to it.  (A leaf of the hub's own colour cannot pair with it under the rule, however heavy.)"""
    star = next(c for c in CASES if c["name"] == "star300")
    rows = np.repeat(np.arange(star["n"]), np.diff(star["indptr"]))
    eid = star["data"]
    leaf = np.where(rows == 0, star["indices"], rows)                       # the leaf of every entry, both directions
    for dtype in (np.float32, np.float64):
        for seed in range(6):
            per_leaf = np.random.default_rng(seed).permutation(star["n"]).astype(dtype)   # distinct weights
            w = np.empty(star["nnz"], dtype=dtype)
            w[eid] = per_leaf[leaf]
            label = run_host(star, w, seed)[0]
            blue = mc.colours(seed, star["n"], 0)
            other = np.flatnonzero(blue != blue[0])
            assert other.size and other.min() >= 1
            heaviest = int(other[np.argmax(per_leaf[other])])
            assert label[0] == 0 and label[heaviest] == 0
            assert (np.delete(label, [0, heaviest]) == np.delete(np.arange(star["n"]), [0, heaviest])).all()


def test_heavier_proposal_is_never_passed_over():
    """Path with strictly decreasing weights: against the model's trace, a RED node never matches an edge while a heavier
    free edge was proposed to it in the same round."""
    n = 257
    case = mc._case("decreasing", n, mc.path_pairs(n), plain=True)
    rows = np.repeat(np.arange(n), np.diff(case["indptr"]))
    w = (n - np.minimum(rows, case["indices"])).astype(np.float64)          # edge (i, i + 1) weighs n - i
    weight_of = lambda u, v: n - min(u, v)
    seen = 0
    for seed in range(12):
        trace = []
        want, rounds = mc.model(case["indptr"], case["indices"], None, w, seed, trace=trace)
        label, used = run_host(case, w, seed)
        assert np.array_equal(label, want) and used == rounds == len(trace)
        for step in trace:
            for u, v in step["picks"].items():
                assert not step["blue"][u] and step["blue"][v] and step["prop"][v] == u
                for x in (u - 1, u + 1):
                    if 0 <= x < n and x != v and step["active"][x] and step["blue"][x] and step["prop"][x] == u:
                        seen += 1
                        assert weight_of(u, x) < weight_of(u, v)
    assert seen > 0            # the situation did occur


def test_directed_cycle_stops_at_the_cap():
    from dgl_amd import DGLAMDError

    cyc = mc.csr_of(3, [0, 1, 2], [1, 2, 0])
    with pytest.raises(DGLAMDError, match=r"neighbor_matching_host: .*max_rounds = 8.*not bi-directed"):
        run_host(cyc, None, 3, max_rounds=8)
    with pytest.raises(RuntimeError):
        mc.model(cyc["indptr"], cyc["indices"], None, None, 3, max_rounds=8)


def test_refusals():
    from dgl_amd import DGLAMDError, _capi, _lib
    LIB = _lib.LIB

    def refused(rc, *parts):
        assert rc == -1
        msg = LIB.dgla_last_error().decode()
        for p in parts:
            assert p in msg, msg

    case = CASES[0]
    csr = host_csr(case, torch.int64)
    w = torch.ones(case["nnz"])
    label, rounds = torch.empty(3, dtype=torch.int64), ctypes.c_int64()
    base = (("csr", ctypes.byref(csr)), ("w", None), ("wd", 0), ("seed", 1), ("cap", 256), ("label", label.data_ptr()),
            ("rounds", ctypes.byref(rounds)), ("relabel", None))
    host = lambda **kw: LIB.dgla_neighbor_matching_host(*[kw.get(n, d) for n, d in base])
    assert host() == 0 and rounds.value >= 1
    refused(host(csr=None), "neighbor_matching_host: csr is null")
    refused(host(label=None), "neighbor_matching_host: label is null")
    refused(host(rounds=None), "neighbor_matching_host: rounds is null")
    refused(host(cap=0), "neighbor_matching_host: max_rounds must be at least 1, got 0")
    refused(host(w=w.data_ptr(), wd=2), "neighbor_matching_host", "float16 / bfloat16")
    refused(host(w=w.data_ptr(), wd=3), "neighbor_matching_host", "float16 / bfloat16")
    refused(host(w=w.data_ptr(), wd=9), "neighbor_matching_host: unknown weight dtype 9")
    for field, msg in (("idtype_bits", "idtype must be int32 or int64"), ("indptr", "invalid csr: indptr is null"),
                       ("indices", "invalid csr: indices is null")):
        broken = host_csr(case, torch.int64)
        setattr(broken, field, 16 if field == "idtype_bits" else None)
        refused(host(csr=ctypes.byref(broken)), "neighbor_matching_host: " + msg)
    # the device entry points refuse the same things, and a workspace that is too small, before any launch
    need = LIB.dgla_neighbor_matching_workspace_bytes(64, 3)
    assert need > 0 and need % 256 == 0 and LIB.dgla_neighbor_matching_workspace_bytes(16, 3) == 0
    small = torch.empty(8, dtype=torch.uint8)
    dev = lambda **kw: LIB.dgla_neighbor_matching(*[kw.get(n, d) for n, d in base[:5] + (
        ("batch", 0), ("label", label.data_ptr()), ("rounds", ctypes.byref(rounds)), ("ws", small.data_ptr()),
        ("ws_bytes", 8), ("stream", None))])
    refused(dev(), "neighbor_matching: workspace of %d bytes required" % need)
    refused(dev(csr=None), "neighbor_matching: csr is null")
    refused(dev(cap=-1), "neighbor_matching: max_rounds must be at least 1")
    refused(dev(w=w.data_ptr(), wd=3), "neighbor_matching: float16 / bfloat16")
    refused(dev(label=None), "neighbor_matching: label is null")
    rel = lambda **kw: LIB.dgla_neighbor_matching_relabel(*[kw.get(n, d) for n, d in (
        ("label", label.data_ptr()), ("bits", 64), ("n", 3), ("out", label.data_ptr()), ("ws", small.data_ptr()),
        ("ws_bytes", 8), ("stream", None))])
    refused(rel(), "neighbor_matching_relabel: workspace of %d bytes required" % need)
    refused(rel(bits=8), "neighbor_matching_relabel: idtype must be int32 or int64")
    refused(rel(out=None), "neighbor_matching_relabel: label / out are null")
    # the wrappers
    with pytest.raises(DGLAMDError, match="one value per edge"):
        _capi.neighbor_matching_host(csr, torch.ones(case["nnz"] + 1))
    with pytest.raises(DGLAMDError, match="float16 / bfloat16"):
        _capi.neighbor_matching_host(csr, torch.ones(case["nnz"], dtype=torch.bfloat16))


def test_python_surface_refuses():
    import dgl_amd
    from dgl_amd import DGLError
    from dgl_amd.geometry import neighbor_matching

    assert "neighbor_matching" in dgl_amd.geometry.__all__
    g = dgl_amd.graph((torch.tensor([0, 1, 1, 2]), torch.tensor([1, 0, 2, 1])))
    with pytest.raises(DGLError, match="one value per edge"):
        neighbor_matching(g, torch.ones(3))
    with pytest.raises(DGLError, match="no CPU fallback"):                 # a CPU graph reaches no kernel
        neighbor_matching(g)
    h = dgl_amd.heterograph({("a", "x", "b"): (torch.tensor([0]), torch.tensor([0]))})
    with pytest.raises(DGLError, match="must be homogeneous"):
        neighbor_matching(h)


def test_header_declares_and_library_exports():
    from dgl_amd import _lib

    text = open(os.path.join(ROOT, "include", "dgl_amd.h")).read()
    assert "#define DGLA_ABI_VERSION 2\n" in text
    assert "Graph matching" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(_lib.LIB, name), name
