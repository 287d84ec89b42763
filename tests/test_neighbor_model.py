"""The rule of dgla_sample_neighbors, dgla_sample_neighbors_weighted and dgla_to_block (include/dgl_amd.h) on its Python
model (tests/neighbor_cases.py) — runs without a GPU and without the library.

The device kernels of csrc/sampling.hip are held to this model bit for bit by tests/test_zzzzzzzzzzzz_gpu_neighbor.py,
so what is shown here about the model is shown about them: known answers (the model cannot drift silently), the law
of the uniform and of the weighted picks on fixed seeds (deterministic: the statistics are numbers, not samples of a
run), the key gaps that make the without-replacement comparison independent of the last bits of a logarithm, and that
each committed case table tells the true rule from nine specific defects."""
import math

import numpy as np
import pytest

from tests import neighbor_cases as nc
from tests.test_random_walk_host import KNOWN

Z_CAP = 4.5      # every cell; at most 1 500 cells in all: a correct rule exceeds it with probability about 1 %


# ---- known answers ------------------------------------------------------------------------------------
def test_generator_known_answers():
    for (seed, i, t, k), r, idx, _ in KNOWN:
        got = nc.mix64((nc.step_key(nc.walk_key(seed, i), t) + k) & nc.M64)
        assert got == r and nc.index(got, 40) == idx


POSITIONS = [
    ((0, 0, 40, 4, False), [24, 6, 19, 39]),
    ((0, 0, 40, 4, True), [26, 6, 20, 39]),
    ((42, 99999, 100000, 5, False), [78403, 29049, 26114, 63434, 22944]),
    ((2 ** 64 - 1, 2 ** 40 + 5, 1000, 6, True), [655, 368, 706, 155, 841, 875]),
    ((7, 12, 5, 4, False), [0, 2, 3, 4]),
    ((7, 12, 2, 1, False), [0]),
    ((7, 12, 3, 8, True), [0, 2, 2, 0, 0, 1, 2, 2]),
    ((21, 1, 9, 8, False), [1, 0, 3, 4, 5, 6, 7, 8]),
]
# deg = fanout + 1 at the dispatch boundaries and at the largest fanout: (first six slots, position left out)
LONG = [
    ((42, 7, 17, 16, False), [1, 2, 3, 4, 5, 6], 0),
    ((42, 7, 33, 32, False), [1, 2, 3, 4, 5, 6], 0),
    ((2 ** 64 - 1, 3, 34, 33, False), [0, 2, 3, 4, 5, 1], 18),
    ((21, 1, 129, 128, False), [1, 0, 3, 4, 5, 6], 44),
]


def test_uniform_known_answers():
    for (S, r, deg, f, rep), want in POSITIONS:
        assert nc.uniform_positions(S, r, deg, f, rep) == want, (S, r, deg, f, rep)
    for (S, r, deg, f, rep), head, missing in LONG:
        got = nc.uniform_positions(S, r, deg, f, rep)
        assert got[:6] == head and sorted(got + [missing]) == list(range(deg)), (S, r, deg, f)
    # the whole row in order: no fanout, or a row no longer than the fanout; an empty row with replacement
    assert nc.uniform_positions(5, 1, 7, -1, False) is None and nc.uniform_positions(5, 1, 7, 7, False) is None
    assert nc.uniform_positions(5, 1, 0, 3, True) == []


def test_weighted_and_block_known_answers():
    w = np.array([0.5, 0.0, 2.0, np.nan, 1.0, -1.0, 4.0, 0.25], dtype=np.float32)
    order, keys = nc.clock_order(42, 3, w)
    assert sorted(order) == [0, 2, 4, 6, 7] and keys == sorted(keys)
    assert order == WEIGHTED_ORDER and nc.replace_picks(42, 3, w, 8) == WEIGHTED_PICKS
    assert nc.replace_picks(42, 3, np.zeros(4), 8) == [] and nc.clock_order(42, 3, np.zeros(4)) == ([], [])
    local, nodes = nc.model_block([7, 2, 9], [5, 2, 11, 5, 7, 0, 9, 11])
    assert nodes.tolist() == [7, 2, 9, 0, 5, 11] and local.tolist() == [4, 1, 5, 4, 0, 3, 2, 5]
    local, nodes = nc.model_block([4], [])
    assert nodes.tolist() == [4] and local.tolist() == []


WEIGHTED_ORDER = [2, 6, 0, 4, 7]
WEIGHTED_PICKS = [6, 6, 6, 2, 4, 2, 4, 6]


# ---- the law of the uniform rule ------------------------------------------------------------------------
def position_counts(deg, f, N, S, replace):
    c = np.zeros(deg)
    for r in range(N):
        for p in nc.uniform_positions(S, r, deg, f, replace):
            c[p] += 1
    return c


def chi2_cap(dof):
    """The 1 - 1e-6 quantile of the chi-square law."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, dof))
    except ImportError:      # Wilson-Hilferty: chi2_p ~ dof (1 - 2 / (9 dof) + z_p sqrt(2 / (9 dof)))^3, z_p = 4.7534
        a = 2.0 / (9.0 * dof)
        return dof * (1.0 - a + 4.7534 * math.sqrt(a)) ** 3


@pytest.mark.parametrize("deg,f,N,S,recorded", [(40, 4, 6000, 7, 2.15), (70, 33, 4000, 21, 2.32), (33, 32, 4000, 22, 2.75),
                                                (17, 16, 4000, 23, 2.13), (200, 128, 1500, 24, 3.07),
                                                (129, 128, 1500, 25, 3.64)])
def test_uniform_inclusion_is_binomial(deg, f, N, S, recorded):
    """Without replacement every position is in the sample of a row with probability f / deg, independently from row to
    row (node ids 0 .. N - 1): the count of a position is Binomial(N, f / deg)."""
    c = position_counts(deg, f, N, S, False)
    assert c.sum() == N * f
    p = f / deg
    z = np.abs(c - N * p) / math.sqrt(N * p * (1 - p))
    print("deg %d fanout %d: largest |z| = %.2f" % (deg, f, z.max()))
    assert z.max() <= Z_CAP
    assert abs(z.max() - recorded) < 0.005       # (the figure of the model when the test was written)


@pytest.mark.parametrize("deg,f,N,S,recorded", [(40, 4, 6000, 8, 48.7), (100, 40, 3000, 31, 103.8)])
def test_uniform_with_replacement_is_uniform(deg, f, N, S, recorded):
    c = position_counts(deg, f, N, S, True)
    e = N * f / deg
    x = float(((c - e) ** 2 / e).sum())
    print("deg %d fanout %d: chi2(%d) = %.1f, cap %.1f" % (deg, f, deg - 1, x, chi2_cap(deg - 1)))
    assert x < chi2_cap(deg - 1)
    assert abs(x - recorded) < 0.05


def test_chi2_cap_matches_its_approximation():
    for dof, want in ((39, 96.2), (99, 180.8)):      # (96.2: the cap tests/test_random_walk_host.py uses for 39 dof)
        a = 2.0 / (9.0 * dof)
        wh = dof * (1.0 - a + 4.7534 * math.sqrt(a)) ** 3
        assert abs(chi2_cap(dof) - wh) < 0.01 * wh and abs(chi2_cap(dof) - want) < 1.0


# ---- the law of the weighted rules ----------------------------------------------------------------------
def law_row(L):
    return nc.dyadic_row(np.random.default_rng(500 + L), L)


@pytest.mark.parametrize("L", [64, 65, 130, 200])
def test_weighted_with_replacement_follows_the_weights(L):
    w, N, f, S = law_row(L), 15000, 4, 11
    c = np.zeros(L)
    for r in range(N):
        for p in nc.replace_picks(S, r, w, f):
            c[p] += 1
    assert c.sum() == N * f and (c[w == 0] == 0).all()
    pos = w > 0
    p = w[pos] / w.sum()
    z = np.abs(c[pos] - N * f * p) / np.sqrt(N * f * p * (1 - p))
    print("length %d: largest |z| = %.2f over %d positive positions" % (L, z.max(), pos.sum()))
    assert z.max() <= Z_CAP


@pytest.mark.parametrize("L", [5, 64, 65, 130, 200])
def test_weighted_without_replacement_first_slot_follows_the_weights(L):
    """The smallest of independent exponential clocks of rates w_j belongs to j with probability w_j / sum w."""
    w, N, S = law_row(L), 8000, 12
    c = np.zeros(L)
    for r in range(N):
        c[nc.clock_order(S, r, w)[0][0]] += 1
    assert c.sum() == N and (c[w == 0] == 0).all()
    pos = w > 0
    p = w[pos] / w.sum()
    z = np.abs(c[pos] - N * p) / np.sqrt(N * p * (1 - p))
    print("length %d: largest |z| = %.2f over %d positive positions" % (L, z.max(), pos.sum()))
    assert z.max() <= Z_CAP


# ---- the committed tables ---------------------------------------------------------------------------------
def test_uniform_tables_hold_what_they_promise():
    for f in nc.FANOUTS:
        G = nc.uniform_graph(f)
        deg = np.diff(G["indptr"])
        assert set(nc.ladder(f)) <= set(deg.tolist()) and 200 <= G["num_rows"] <= 400
        for r in range(G["num_rows"]):
            row = G["indices"][G["indptr"][r]:G["indptr"][r + 1]]
            assert len(np.unique(row)) == len(row)
        assert sorted(G["eids"].tolist()) == list(range(len(G["indices"])))
        seeds, perm = nc.uniform_seeds(f)
        assert set(seeds.tolist()) == set(range(G["num_rows"])) and len(seeds) == G["num_rows"] + 1
        assert not np.array_equal(perm, np.arange(len(perm)))


def test_weighted_tables_hold_what_they_promise():
    G, w = nc.weighted_graph("dyadic")
    deg = np.diff(G["indptr"])
    assert set(nc.W_LENGTHS) <= set(deg.tolist())
    assert np.array_equal(w * 8, np.round(w * 8)) and w.min() == 0 and w.max() <= 8
    assert 0.25 < (w == 0).mean() < 0.45
    rows = [w[G["indptr"][r]:G["indptr"][r + 1]] for r in range(G["num_rows"])]
    assert all((x[-3:] == 0).all() for x in rows if len(x) >= 5)
    assert any(len(x) > 0 and (x == 0).all() for x in rows)
    assert any(np.nonzero(x)[0].tolist() == [64] for x in rows)
    G, w = nc.weighted_graph("generic")
    assert set(nc.W_LENGTHS) <= set(np.diff(G["indptr"]).tolist()) and 0.2 < (w == 0).mean() < 0.4
    for dtype in (np.float32, np.float64):
        G, w = nc.special_graph(dtype)
        fi = np.finfo(dtype)
        assert np.isnan(w[3]) and w[66] == -1 and np.signbit(w[11]) and w[11] == 0 and w[12] == 0
        assert np.isinf(w).sum() == 1 and w[nc.SPECIAL_INF] == np.inf
        assert (w == fi.smallest_subnormal).sum() == 1 and (w == fi.max).sum() == 1
        assert sorted(set(range(90)) - set(nc.positive_positions(w))) == sorted(nc.SPECIAL_NEVER)


@pytest.mark.parametrize("kind", ["dyadic", "generic"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_clock_keys_of_the_tables_are_far_apart(kind, dtype):
    """What the device comparison without replacement rests on: among the first picks + 1 keys of every row, adjacent
    keys differ by more than 1e-9 relative, so a device logarithm a few ulp off cannot reorder them."""
    G, w_pos = nc.weighted_graph(kind)
    w_pos = w_pos.astype(dtype)
    smallest = math.inf
    for S in nc.W_SEEDS:
        for r in range(G["num_rows"]):
            w = nc.row_weights(G, w_pos, r, use_eids=False)
            smallest = min(smallest, nc.min_key_gap(S, r, w, nc.MAX_FANOUT))
    print("%s %s: smallest relative key gap %.3g" % (kind, np.dtype(dtype).name, smallest))
    assert smallest > 1e-9


def test_block_tables_hold_what_they_promise():
    for n in nc.B_NODES:
        cases = nc.block_cases(n)
        assert [len(src) for _, _, src in cases[:2 * len(nc.B_NNZ)]] == [v for v in nc.B_NNZ for _ in nc.B_SEEDS]
        for name, seeds, src in cases:
            assert len(np.unique(seeds)) == len(seeds) and len(seeds) in (1, min(300, n - 10))
            assert len(src) == 0 or (0 <= src.min() and src.max() < n)
            if name.startswith("nnz") and len(src) >= 2:
                assert 0 in src and n - 1 in src
            if name == "all_seeds":
                assert np.isin(src, seeds).all()
            if name == "disjoint":
                assert not np.isin(src, seeds).any()
            local, nodes = nc.model_block(seeds, src)
            assert np.array_equal(nodes[local], src) and len(np.unique(nodes)) == len(nodes)
            assert np.array_equal(nodes[:len(seeds)], seeds) and (np.diff(nodes[len(seeds):]) > 0).all()


# ---- the cases discriminate -------------------------------------------------------------------------------
def uniform_differs(bug):
    """A committed uniform case whose model output changes under the defect, or None."""
    for f in nc.FANOUTS:
        G, (seeds, _) = nc.uniform_graph(f), nc.uniform_seeds(f)
        for fanout, replace in nc.uniform_modes(f):
            true = nc.expected_uniform(f, fanout, replace, 42)
            wrong = nc.model_uniform(G, seeds, fanout, replace, 42, bug=bug)
            if not all(np.array_equal(a, b) for a, b in zip(true, wrong)):
                return f, fanout, replace
    return None


def weighted_differs(bug, kind, replace, use_eids=False):
    G, w_pos = nc.weighted_graph(kind)
    seeds = nc.weighted_seeds(G)
    prob = nc.prob_by_eid(G, w_pos, use_eids, np.float64)
    for fanout in nc.W_FANOUTS:
        true = nc.model_weighted(G, prob, seeds, fanout, replace, 42, use_eids)
        wrong = nc.model_weighted(G, prob, seeds, fanout, replace, 42, use_eids, bug=bug)
        assert all(np.array_equal(a, b) for a, b in zip(true, nc.expected_weighted(kind, np.float64, fanout, replace, 42)))
        if not all(np.array_equal(a, b) for a, b in zip(true, wrong)):
            return kind, fanout
    return None


def block_differs(bug):
    for n in nc.B_NODES:
        for name, seeds, src in nc.block_cases(n):
            true, wrong = nc.model_block(seeds, src), nc.model_block(seeds, src, bug=bug)
            if not all(np.array_equal(a, b) for a, b in zip(true, wrong)):
                return n, name
    return None


def test_the_cases_tell_the_defects_apart():
    """Model against model: a kernel with one of these defects would fail the equality tests on the device."""
    # (a) the weight of the chunks already passed is not carried: dyadic rows, with replacement (byte equality there)
    assert weighted_differs("no_chunk_carry", "dyadic", True)
    # (b) the exponential-clock scan ignores positions >= 64
    assert weighted_differs("scan_stops_at_64", "dyadic", False) and weighted_differs("scan_stops_at_64", "generic", False)
    # (c) Floyd substitutes j - 1 on a duplicate; (e) the draw slot is k + 1; (f) keyed by seed position
    for bug in ("floyd_j_minus_one", "slot_plus_one", "key_by_seed_position"):
        assert uniform_differs(bug), bug
    # (d) equal keys by descending position: two +inf weights have the key 0 both (the model-only table)
    for dtype in (np.float32, np.float64):
        G, w = nc.special_graph(dtype, twin_inf=True)
        true, wrong = nc.clock_order(42, 0, w)[0], nc.clock_order(42, 0, w, bug="ties_descending")[0]
        assert true[:2] == [20, nc.SPECIAL_INF] and wrong[:2] == [nc.SPECIAL_INF, 20] and true[2:] == wrong[2:]
    # (g) prob read by position instead of by edge id: the cases with an edge-id map
    for kind, replace in (("dyadic", True), ("dyadic", False), ("generic", False)):
        assert weighted_differs("prob_by_position", kind, replace, use_eids=True)
    # (h) new nodes in first-appearance order; (i) ranks off by one from element 16 384 of the sorted ids on
    assert block_differs("first_appearance") and block_differs("rank_off_from_16384")
