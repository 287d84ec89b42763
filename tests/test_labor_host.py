"""Layer-neighbour (LABOR-0) sampling (include/dgl_amd.h "Layer-neighbour sampling", csrc/labor_step.h) through the HOST
functions: runs without a GPU.

dgla_labor_scale_host and dgla_labor_pick_host compile the one definition of the rule that the kernels of csrc/labor.hip
compile for the device, so what is pinned here is pinned for the kernels too (tests/test_zzzzzzzzzz_gpu_labor.py checks
device == host bit for bit).  The checker is the numpy model of tests/labor_cases.py, written from the text of the rule.

Exact: host == model (indptr, neighbours, edge ids) over the degree ladder 0 .. 70 000 with a multigraph row, with and
without an edge-id map, both id types, seeds listed twice, k in {0, 1, 5, 10, -1} and 0 / 1 / 64 / 65 seeds.
Consequences of the rule; the law over 4096 fixed seeds (5 standard errors per edge and per row); the scale against an
exact solve; the importances; the C ABI's refusals and the pinned workspace sizes.
Reference: python/dgl/sampling/labor.py, src/array/labor_pick.h, src/array/cuda/labor_sampling.cu."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import labor_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FANOUTS = [0, 1, 5, 10, -1]
NUM_SEEDS = [0, 1, 64, 65]
REL20, REL40 = 2.0 ** -20, 2.0 ** -40


@pytest.fixture(scope="module")
def graph():
    return lc.labor_graph()


@pytest.fixture(scope="module")
def probs(graph):
    rng = np.random.default_rng(21)
    nnz = len(graph["indices"])
    return {np.float32: lc.messy_prob(nnz, rng, np.float32), np.float64: lc.messy_prob(nnz, rng, np.float64)}


def seeds_of(graph, n):
    return lc.seeds_for(graph, n, np.random.default_rng(100 + n))


def same_picks(got, want):
    indptr, nbr, eid, _ = got
    assert np.array_equal(indptr.numpy(), want[0])
    assert np.array_equal(nbr.numpy(), want[1])
    assert np.array_equal(eid.numpy(), want[2])


# ---- host == model -----------------------------------------------------------------------------------
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("use_data", [True, False])
@pytest.mark.parametrize("n", NUM_SEEDS)
def test_uniform_picks_equal_the_model(graph, idtype, use_data, n):
    seeds = seeds_of(graph, n)
    for k in FANOUTS:
        got = lc.host_pick(graph, seeds, k, 7, idtype=idtype, use_data=use_data)
        assert got[0].dtype == idtype and got[1].dtype == idtype and got[2].dtype == idtype and got[3] is None
        same_picks(got, lc.model_pick(graph, seeds, k, 7, use_data=use_data))


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("use_data", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weighted_picks_and_importances_equal_the_model(graph, probs, idtype, use_data, dtype):
    prob = probs[dtype]
    tol = REL20 if dtype == np.float32 else REL40
    for n in NUM_SEEDS:
        seeds = seeds_of(graph, n)
        for k in FANOUTS:
            c = lc.host_scale(graph, seeds, k, prob, idtype=idtype, use_data=use_data)
            got = lc.host_pick(graph, seeds, k, 8, prob=prob, c=c, idtype=idtype, use_data=use_data)
            want = lc.model_pick(graph, seeds, k, 8, prob=prob, c=c, use_data=use_data)
            same_picks(got, want)
            imp = got[3].numpy()
            assert imp.dtype == dtype
            np.testing.assert_allclose(imp.astype(np.float64), want[3], rtol=tol, atol=0)
            # per seed the importances sum to the kept count
            ptr = want[0]
            for i in range(len(seeds)):
                cnt = ptr[i + 1] - ptr[i]
                if cnt:
                    assert abs(imp[ptr[i]:ptr[i + 1]].astype(np.float64).sum() - cnt) <= cnt * (REL20 if dtype == np.float32 else REL40)
            # zero, negative and NaN weights are never kept
            assert (lc.usable(prob[want[2]]) > 0).all()


def test_fanout_all_keeps_every_edge_and_every_positive_weight(graph, probs):
    seeds = seeds_of(graph, 65)
    indptr, nbr, eid, _ = lc.host_pick(graph, seeds, -1, 3)
    deg = np.array([np.subtract(*lc.row_of(graph, int(s))[::-1]) for s in seeds])
    assert np.array_equal(np.diff(indptr.numpy()), deg)
    prob = probs[np.float32]
    indptr, nbr, eid, imp = lc.host_pick(graph, seeds, -1, 3, prob=prob)
    pos = np.array([(lc.usable(prob[lc.edge_ids(graph, *lc.row_of(graph, int(s)), True)]) > 0).sum() for s in seeds])
    assert np.array_equal(np.diff(indptr.numpy()), pos)
    # p = 1 everywhere: a = w', the importances are the weights normalised to mean 1 per seed
    ptr = indptr.numpy()
    w = lc.usable(prob[eid.numpy()])
    for i in range(len(seeds)):
        if ptr[i + 1] > ptr[i]:
            ww = w[ptr[i]:ptr[i + 1]]
            np.testing.assert_allclose(imp.numpy()[ptr[i]:ptr[i + 1]], ww * (len(ww) / ww.sum()), rtol=REL20)


# ---- consequences of the rule --------------------------------------------------------------------------
def rows_as_sets(seeds, picks):
    ptr, eid = picks[0].numpy(), picks[2].numpy()
    return {int(s): set(eid[ptr[i]:ptr[i + 1]].tolist()) for i, s in enumerate(seeds)}


def test_a_shared_neighbour_kept_by_the_longer_row_is_kept_by_the_shorter():
    # rows of degree 40, 25 and 12 over the same 40 neighbours (the shorter rows are prefixes)
    nb = np.random.default_rng(1).permutation(100)[:40]
    R = dict(indptr=np.array([0, 40, 65, 77]), indices=np.concatenate([nb, nb[:25], nb[:12]]).astype(np.int64), data=None,
             num_rows=3, num_cols=100)
    hits = 0
    for seed in range(40):
        ptr, nbr, _, _ = lc.host_pick(R, np.array([0, 1, 2]), 10, seed, use_data=False)
        rows = [set(nbr.numpy()[ptr[i]:ptr[i + 1]].tolist()) for i in range(3)]
        assert (rows[0] & set(nb[:25].tolist())) <= rows[1]
        assert (rows[1] & set(nb[:12].tolist())) <= rows[2]
        hits += len(rows[0] & set(nb[:25].tolist()))
    assert hits > 0


def test_picks_grow_with_the_fanout(graph):
    seeds = seeds_of(graph, 64)
    prev = None
    for k in [0, 1, 5, 10, 11, 64, 100000]:
        rows = rows_as_sets(seeds, lc.host_pick(graph, seeds, k, 42))
        if prev is not None:
            assert all(prev[s] <= rows[s] for s in rows)
        prev = rows
    assert prev == rows_as_sets(seeds, lc.host_pick(graph, seeds, -1, 42))


def test_duplicate_neighbours_are_kept_or_dropped_together(graph):
    row = len(lc.DEGREES)           # the multigraph row
    lo, hi = lc.row_of(graph, row)
    t = graph["indices"][lo:hi]
    mixed = 0
    for seed in range(30):
        ptr, nbr, eid, _ = lc.host_pick(graph, np.array([row]), 10, seed, use_data=False)
        kept = np.zeros(hi - lo, dtype=bool)
        kept[eid.numpy() - lo] = True
        for v in np.unique(t):
            assert len(set(kept[t == v].tolist())) == 1
        mixed += int(kept.any() and not kept.all())
    assert mixed > 0


def test_the_order_of_the_seeds_permutes_the_rows_only(graph, probs):
    seeds = np.arange(len(lc.DEGREES) + 1)
    perm = np.random.default_rng(2).permutation(len(seeds))
    for prob in (None, probs[np.float64]):
        a = rows_as_sets(seeds, lc.host_pick(graph, seeds, 10, 9, prob=prob))
        b = rows_as_sets(seeds[perm], lc.host_pick(graph, seeds[perm], 10, 9, prob=prob))
        assert a == b
    # a seed listed twice gets the same row twice
    ptr, nbr, eid, _ = lc.host_pick(graph, np.array([17, 3, 17]), 5, 9)
    e = eid.numpy()
    assert np.array_equal(e[ptr[0]:ptr[1]], e[ptr[2]:ptr[3]]) and ptr[1] - ptr[0] > 0


# ---- the law -------------------------------------------------------------------------------------------
LAW_SEEDS = 4096


def keep_frequencies(R, k, prob=None, c=None):
    seeds = np.arange(R["num_rows"])
    nnz = len(R["indices"])
    hits = np.zeros(nnz)
    for seed in range(LAW_SEEDS):
        _, _, eid, _ = lc.host_pick(R, seeds, k, 1000 + seed, prob=prob, c=c, use_data=False)
        hits[eid.numpy()] += 1
    return hits / LAW_SEEDS


def check_law(R, freq, target):
    se = np.sqrt(target * (1 - target) / LAW_SEEDS)
    assert (np.abs(freq - target) <= 5 * se).all(), np.abs(freq - target).max()      # (se == 0: the frequency is exact)
    for r in range(R["num_rows"]):
        lo, hi = lc.row_of(R, r)
        mean, want = freq[lo:hi].sum(), target[lo:hi].sum()
        row_se = np.sqrt((target[lo:hi] * (1 - target[lo:hi])).sum() / LAW_SEEDS)   # distinct neighbours: independent
        assert abs(mean - want) <= 5 * row_se


@pytest.mark.parametrize("k", [1, 5, 10])
def test_uniform_law(k):
    R = lc.small_graph()
    deg = np.diff(R["indptr"])
    target = np.repeat(np.minimum(1.0, k / np.maximum(deg, 1)), deg)
    freq = keep_frequencies(R, k)
    check_law(R, freq, target)
    # every row's mean kept count: min(k, d), by the sums above
    assert np.allclose(np.add.reduceat(np.append(target, 0), R["indptr"][:-1])[deg > 0], np.minimum(k, deg)[deg > 0])


@pytest.mark.parametrize("k", [1, 5, 10])
def test_weighted_law(k):
    R = lc.small_graph()
    rng = np.random.default_rng(4)
    prob = np.exp(rng.uniform(-2.0, 2.0, len(R["indices"])))
    prob[rng.integers(0, len(prob), 15)] = 0.0
    seeds = np.arange(R["num_rows"])
    c = lc.host_scale(R, seeds, k, prob, use_data=False)
    deg = np.diff(R["indptr"])
    with np.errstate(invalid="ignore"):
        target = np.where(prob > 0, np.minimum(1.0, np.repeat(c, deg) * prob), 0.0)
    check_law(R, keep_frequencies(R, k, prob=prob, c=c), target)
    # the expected kept count is k wherever more than k weights are positive
    for r in range(R["num_rows"]):
        lo, hi = lc.row_of(R, r)
        if (prob[lo:hi] > 0).sum() > k:
            assert abs(target[lo:hi].sum() - k) <= k * REL20


# ---- the scale -------------------------------------------------------------------------------------------
def one_row(weights):
    w = np.asarray(weights, dtype=np.float64)
    return dict(indptr=np.array([0, len(w)]), indices=np.arange(len(w), dtype=np.int64), data=None, num_rows=1,
                num_cols=max(1, len(w))), w


SCALE_ROWS = {
    "equal": (np.full(50, 0.375), 10),       # (a dyadic weight: the sum is exact in any order)
    "dominant": (np.concatenate([[1e6], np.full(99, 1.0)]), 10),
    "geometric": (2.0 ** -np.arange(40), 10),
    "geometric_slow": (1.5 ** -np.arange(200), 30),
    "messy": (np.concatenate([np.exp(np.random.default_rng(0).uniform(-3, 3, 300)), [0.0, -1.0, np.nan] * 5]), 10),
    "two_levels": (np.concatenate([np.full(7, 100.0), np.full(500, 0.01)]), 10),
}


@pytest.mark.parametrize("name", sorted(SCALE_ROWS))
def test_scale_solves_the_saturation_equation(name):
    weights, k = SCALE_ROWS[name]
    R, w = one_row(weights)
    c = lc.host_scale(R, np.array([0]), k, w, use_data=False)
    exact = lc.model_scale(R, np.array([0]), k, w, use_data=False)
    assert np.isfinite(c[0]) and c[0] > 0
    total = lc.saturation_sum(R, np.array([0]), c, w, use_data=False)[0]
    assert abs(total - k) <= k * REL20, (total, k)
    assert abs(c[0] - exact[0]) <= exact[0] * REL20
    if name == "equal":
        assert c[0] == k / w.sum()                # one pass: nothing saturates
    if name.startswith("geometric"):
        assert (c[0] * w >= 1).sum() >= 5       # several weights saturate: the first pass alone is not the answer
        assert abs(c[0] - k / w.sum()) > 0.5 * c[0]


def test_scale_special_rows():
    for weights, k, want in [
        ([1.0, 2.0, 3.0], 3, np.inf),                   # P <= k: every positive weight, p = 1
        ([1.0, 2.0, 0.0, -1.0, np.nan], 2, np.inf),     # P counts the positive weights only
        ([0.0, 0.0, 0.0], 2, np.inf),                   # all zero: P = 0 <= k, and nothing is positive
        ([1.0, np.inf, 2.0], 1, 0.0),                   # an infinite weight: nothing is kept
        ([1e308, 1e308, 1e308], 1, 0.0),                # a sum that overflows
        ([1.0, 2.0, 3.0], -1, np.inf),
    ]:
        R, w = one_row(weights)
        c = lc.host_scale(R, np.array([0]), k, w, use_data=False)
        assert c[0] == want, (weights, k, c)
        ptr, nbr, eid, imp = lc.host_pick(R, np.array([0]), k, 5, prob=w, c=c, use_data=False)
        kept = set(eid.numpy().tolist())
        assert kept == (set() if want == 0.0 else {i for i, x in enumerate(weights) if x > 0}), (weights, k)
    # fanout 0 keeps nothing
    R, w = one_row([1.0, 2.0, 3.0])
    c = lc.host_scale(R, np.array([0]), 0, w, use_data=False)
    assert int(lc.host_pick(R, np.array([0]), 0, 5, prob=w, c=c, use_data=False)[0][-1]) == 0


def test_scale_equals_the_exact_solve_on_the_ladder(graph, probs):
    seeds = seeds_of(graph, 65)
    for dtype in (np.float32, np.float64):
        prob = probs[dtype]
        for k in (1, 5, 10):
            c = lc.host_scale(graph, seeds, k, prob)
            exact = lc.model_scale(graph, seeds, k, prob)
            fin = np.isfinite(exact) & (exact > 0)
            assert np.array_equal(c[~fin], exact[~fin])
            assert (np.abs(c[fin] - exact[fin]) <= exact[fin] * REL20).all()
            total = lc.saturation_sum(graph, seeds, c, prob)
            assert (np.abs(total[fin] - k) <= k * REL20).all()


# ---- the C ABI -------------------------------------------------------------------------------------------
NEW = ["dgla_labor_workspace_bytes", "dgla_labor_scale", "dgla_labor_count", "dgla_labor_fill", "dgla_labor_scale_host",
       "dgla_labor_pick_host"]


def test_header_declares_and_library_exports_the_entry_points():
    from dgl_amd._lib import LIB

    header = open(os.path.join(ROOT, "include", "dgl_amd.h")).read()
    assert "Layer-neighbour sampling" in header
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(LIB, name), name


def align256(x):
    return (x + 255) // 256 * 256


# dgla_labor_workspace_bytes(id width, n): int64 offsets [n + 1], fp64 importance sums [n], the scan's block sums
WORKSPACE = {0: 0, 1: 768, 255: 4352, 256: 4608, 257: 4864, 65536: 1049088, 2 ** 20 + 1: 16780032}


def test_workspace_sizes_are_pinned():
    from dgl_amd._lib import LIB

    for n, want in WORKSPACE.items():
        for bits in (32, 64):
            got = LIB.dgla_labor_workspace_bytes(bits, n)
            assert got == want, (bits, n, got)
            assert got % 256 == 0
        if n:
            assert want == align256(8 * (n + 1)) + align256(8 * n) + align256(((n + 1 + 4095) // 4096 + 1) * 8)
    assert LIB.dgla_labor_workspace_bytes(16, 100) == 0
    assert LIB.dgla_labor_workspace_bytes(64, -1) == 0


def test_bad_arguments_fail_with_a_message():
    from dgl_amd import _capi
    from dgl_amd._lib import CSR, LIB

    R = lc.small_graph()
    csr = lc.host_csr_of(R, torch.int64)
    seeds = torch.arange(4)
    out = torch.zeros(5, dtype=torch.int64)
    c = torch.ones(4, dtype=torch.float64)
    prob = torch.ones(len(R["indices"]), dtype=torch.float32)
    ref = ctypes.byref

    def refused(rc, *words):
        assert rc == -1
        msg = LIB.dgla_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(LIB.dgla_labor_pick_host(None, None, 0, None, seeds.data_ptr(), 4, 2, 1, out.data_ptr(), None, None, None),
            "labor_pick_host", "csr is null")
    refused(LIB.dgla_labor_pick_host(ref(csr), None, 0, None, None, 4, 2, 1, out.data_ptr(), None, None, None), "seeds is null")
    refused(LIB.dgla_labor_pick_host(ref(csr), None, 0, None, seeds.data_ptr(), 4, 2, 1, None, None, None, None),
            "out_indptr is null")
    refused(LIB.dgla_labor_pick_host(ref(csr), None, 0, None, seeds.data_ptr(), -1, 2, 1, out.data_ptr(), None, None, None),
            "negative size")
    refused(LIB.dgla_labor_pick_host(ref(csr), prob.data_ptr(), 0, None, seeds.data_ptr(), 4, 2, 1, out.data_ptr(), None, None,
                                     None), "c is null")
    refused(LIB.dgla_labor_pick_host(ref(csr), prob.data_ptr(), 2, c.data_ptr(), seeds.data_ptr(), 4, 2, 1, out.data_ptr(),
                                     None, None, None), "float32 or float64")
    refused(LIB.dgla_labor_scale_host(ref(csr), None, 0, seeds.data_ptr(), 4, 2, c.data_ptr()), "labor_scale_host", "prob is null")
    refused(LIB.dgla_labor_scale_host(ref(csr), prob.data_ptr(), 0, seeds.data_ptr(), 4, 2, None), "c is null")
    narrow = CSR(csr.num_rows, csr.num_cols, csr.nnz, 16, csr.indptr, csr.indices, csr.data)
    refused(LIB.dgla_labor_pick_host(ref(narrow), None, 0, None, seeds.data_ptr(), 4, 2, 1, out.data_ptr(), None, None, None),
            "int32 or int64")
    refused(LIB.dgla_labor_scale_host(ref(narrow), prob.data_ptr(), 0, seeds.data_ptr(), 4, 2, c.data_ptr()), "int32 or int64")
    no_ptr = CSR(csr.num_rows, csr.num_cols, csr.nnz, 64, None, csr.indices, csr.data)
    refused(LIB.dgla_labor_pick_host(ref(no_ptr), None, 0, None, seeds.data_ptr(), 4, 2, 1, out.data_ptr(), None, None, None),
            "indptr is null")
    # the device entry points refuse the same arguments before any launch (no GPU is touched)
    refused(LIB.dgla_labor_count(None, None, 0, None, None, 0, 2, 1, None, None, None, 0, None), "labor_count", "csr is null")
    refused(LIB.dgla_labor_count(ref(narrow), None, 0, None, seeds.data_ptr(), 4, 2, 1, out.data_ptr(), out.data_ptr(), None, 0,
                                 None), "int32 or int64")
    refused(LIB.dgla_labor_count(ref(csr), None, 0, None, seeds.data_ptr(), 4, 2, 1, None, None, None, 0, None),
            "out_indptr / total are null")
    refused(LIB.dgla_labor_count(ref(csr), None, 0, None, seeds.data_ptr(), 4, 2, 1, out.data_ptr(), out.data_ptr(), None, 0,
                                 None), "workspace of 768 bytes required")
    refused(LIB.dgla_labor_fill(ref(csr), None, 0, None, seeds.data_ptr(), 4, 2, 1, 10, None, None, None, None, 0, None),
            "labor_fill", "are null")
    refused(LIB.dgla_labor_fill(ref(csr), None, 0, None, seeds.data_ptr(), 4, 2, 1, -1, None, None, None, None, 0, None),
            "negative capacity")
    refused(LIB.dgla_labor_scale(None, None, 0, None, 0, 2, None, None), "labor_scale", "csr is null")
    # the Python wrappers check what the C side cannot see
    with pytest.raises(_capi._lib.DGLAMDError, match="one value per edge"):
        _capi.labor_pick_host(csr, seeds, 2, 1, prob=prob[:-1].contiguous())
    with pytest.raises(_capi._lib.DGLAMDError, match="id type"):
        _capi.labor_pick_host(csr, seeds.int(), 2, 1)
    with pytest.raises(_capi._lib.DGLAMDError, match="one entry per seed"):
        _capi.labor_pick_host(csr, seeds, 2, 1, prob=prob, c=c[:2].contiguous())


def test_python_surface_refusals_need_no_gpu():
    import dgl_amd
    from dgl_amd import DGLAMDError

    g = dgl_amd.graph((torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])))
    assert dgl_amd.DGLGraph.sample_labors is dgl_amd.sampling.sample_labors
    assert dgl_amd.LaborSampler is dgl_amd.sampling.LaborSampler
    with pytest.raises(DGLAMDError, match="importance_sampling"):
        dgl_amd.sampling.sample_labors(g, [0], 2, importance_sampling=1)
    with pytest.raises(DGLAMDError, match="seed2_contribution"):
        dgl_amd.sampling.sample_labors(g, [0], 2, seed2_contribution=0.5)
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        g.sample_labors([0], 2)
    with pytest.raises(DGLAMDError, match="inbound"):
        dgl_amd.LaborSampler([2], edge_dir="out")
