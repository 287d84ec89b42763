"""node2vec walks (include/dgl_amd.h "node2vec walks", csrc/node2vec_step.h) through the HOST walker — runs without a GPU.

dgla_node2vec_walk_host compiles the one definition of the step rule that node2vec_walk_kernel compiles for the device,
so what is pinned here is pinned for the kernel too (tests/test_zzzzzzzz_gpu_node2vec.py checks device == host bit for
bit).  The checker is an independent restatement of the rule in plain Python integers and floats, written below from the
text of the header: classes from sets of successors (no bisection), Python's own fp64 multiply and add (two roundings).

Exact: host walker == model (uniform, fp32 / fp64 weights, int32 / int64, with and without an edge-id map, steps 0 / 1 /
7 / 40, five (p, q)) together with the walker's counters; p == q == 1 equals dgla_random_walk_host.  The model's own
counters show that the fixed graph exercises every path (three classes, several attempts, the scan at both ends of K's
clamp); the scan's rounding fallback is driven by a stand-alone case with subnormal weights.  Properties, the law of
the second step against the exact node2vec probabilities (upper 1e-6 quantile of the chi-square law), the reference's own
property check, the C ABI's refusals and the Python surface.
Reference: python/dgl/sampling/node2vec_randomwalk.py, src/graph/sampling/randomwalks/node2vec_randomwalk.h."""
import bisect
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.test_random_walk_host import (SEEDS, cdf_of, check_properties, chi2, csr_from_coo, draw, host_walk, messy_weights,
                                         mulhi, uniform)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
PQ = [(1.0, 1.0), (0.25, 4.0), (4.0, 0.25), (0.5, 2.0), (1000.0, 0.001)]
MODERATE = PQ[1:4]
K_MIN, K_MAX = 8, 1024
CHI2_1E6 = {3: 30.7, 4: 33.4, 5: 35.9, 6: 38.3}      # upper 1e-6 quantiles of the chi-square law


# ---- the model of the rule, in Python integers and floats ------------------------------------------
def pmix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pstep_key(seed, i, t):
    return pmix((pmix((seed & M64) ^ ((i * 0xD1B54A32D192ED03) & M64)) + t) & M64)


def pdraw(step_key, k):
    return pmix((step_key + k) & M64)


def pindex(r, n):
    return (r * n) >> 64


def puniform(r):
    return (r >> 11) * 2.0 ** -53


def accept_probs(p, q):
    ip, iq = 1.0 / p, 1.0 / q
    m = max(ip, 1.0, iq)
    return ip / m, 1.0 / m, iq / m


class Model:
    """One relation as Python lists; succ[x] = the set of successors of x (the class test without a bisection)."""

    def __init__(self, R):
        self.indptr = [int(v) for v in R["indptr"]]
        self.indices = [int(v) for v in R["indices"]]
        self.data = None if R["data"] is None else [int(v) for v in R["data"]]
        self.cdf = None if R["cdf"] is None else [float(v) for v in R["cdf"]]
        self.n = R["num_rows"]
        self.succ = [set(self.indices[self.indptr[r]:self.indptr[r + 1]]) for r in range(self.n)]

    def klass(self, x, prev):
        return 0 if x == prev else (1 if prev in self.succ[x] else 2)

    def pick(self, lo, hi, r):
        """Rules 3 / 4 of the first-order step: the candidate position, or -1."""
        if self.cdf is None:
            return lo + pindex(r, hi - lo)
        total = self.cdf[hi - 1]
        if not total > 0 or not math.isfinite(total):
            return -1
        x = puniform(r) * total
        k = bisect.bisect_right(self.cdf, x, lo, hi)
        if k == hi:
            k = bisect.bisect_left(self.cdf, total, lo, hi)
        return k

    def walk(self, seeds, steps, seed, p, q):
        a = accept_probs(p, q)
        n = len(seeds)
        traces = np.full((n, steps + 1), -1, dtype=np.int64)
        eids = np.full((n, steps), -1, dtype=np.int64)
        c = dict(steps=0, attempts=0, scans=0, scan_k=[], fallbacks=0, accepted=[0, 0, 0], max_attempts=0,
                 per_t=np.zeros((steps + 1, 3), dtype=np.int64))
        for i, s in enumerate(seeds):
            s = int(s)
            traces[i, 0] = s
            if not 0 <= s < self.n:
                continue
            curr, prev = s, -1
            for t in range(steps):
                key = pstep_key(seed, i, t)
                lo, hi = self.indptr[curr], self.indptr[curr + 1]
                if hi == lo:
                    break
                if t == 0:
                    pos = self.pick(lo, hi, pdraw(key, 0))
                else:
                    pos = self.second_order(a, key, prev, lo, hi, c, t)
                if pos < 0:
                    break
                traces[i, t + 1] = self.indices[pos]
                eids[i, t] = pos if self.data is None else self.data[pos]
                prev, curr = curr, self.indices[pos]
        return traces, eids, c

    def second_order(self, a, key, prev, lo, hi, c, t):
        deg = hi - lo
        K = min(max(deg, K_MIN), K_MAX)
        before = c["attempts"]
        for k in range(K):
            pos = self.pick(lo, hi, pdraw(key, 2 * k))
            if pos < 0:
                return -1
            c["attempts"] += 1
            cls = self.klass(self.indices[pos], prev)
            if puniform(pdraw(key, 2 * k + 1)) < a[cls]:
                c["steps"] += 1
                c["accepted"][cls] += 1
                c["max_attempts"] = max(c["max_attempts"], k + 1)
                c["per_t"][t] += (1, c["attempts"] - before, 0)
                return pos
        c["scans"] += 1
        c["scan_k"].append(K)
        g = []
        S = 0.0
        for j in range(lo, hi):
            d = 1.0 if self.cdf is None else self.cdf[j] - (self.cdf[j - 1] if j > lo else 0.0)
            gj = d * a[self.klass(self.indices[j], prev)]      # one rounding
            g.append(gj)
            S = S + gj                                         # and another
        if not S > 0:
            c["per_t"][t] += (0, c["attempts"] - before, 1)
            return -1
        x = puniform(pdraw(key, 2 * K)) * S
        run, pos = 0.0, -1
        for j, gj in enumerate(g):
            run = run + gj
            if run > x:
                pos = lo + j
                break
        if pos < 0:
            c["fallbacks"] += 1
            pos = lo + max(j for j, gj in enumerate(g) if gj > 0)
        c["steps"] += 1
        c["accepted"][self.klass(self.indices[pos], prev)] += 1
        c["per_t"][t] += (1, c["attempts"] - before, 1)
        return pos


def test_scalar_generator_is_the_array_generator():
    for seed, i, t, k in ((0, 0, 0, 0), (7, 3, 2, 1), (42, 1000000, 79, 2047), (2 ** 64 - 1, 2 ** 40 + 5, 3, 16)):
        r = pdraw(pstep_key(seed, i, t), k)
        assert r == int(draw(seed, i, t, k))
        assert pindex(r, 1100) == int(mulhi(r, 1100)) and puniform(r) == float(uniform(r))


# ---- the host walker ---------------------------------------------------------------------------
def member_of(R):
    m = np.array(R["indices"], dtype=np.int64)
    ip = R["indptr"]
    for r in range(R["num_rows"]):
        m[ip[r]:ip[r + 1]].sort()
    return m


def host_n2v(R, seeds, steps, seed, p, q, idtype=torch.int64, return_eids=True, stats=False, member=None):
    from dgl_amd import _capi

    def t_(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(idtype)

    csr = _capi.host_csr(t_(R["indptr"]), t_(R["indices"]), t_(R["data"]), R["num_cols"])
    cdf = None if R["cdf"] is None else torch.from_numpy(np.ascontiguousarray(R["cdf"]))
    out = _capi.node2vec_walk_host(csr, cdf, t_(member_of(R) if member is None else member),
                                   torch.as_tensor(np.asarray(seeds), dtype=idtype), steps, p, q, rng_seed=seed,
                                   return_eids=return_eids, stats=stats)
    assert out[0].dtype == idtype
    res = (out[0].numpy().astype(np.int64), None if out[1] is None else out[1].numpy().astype(np.int64))
    return res + (out[2],) if stats else res


# ---- the graph ---------------------------------------------------------------------------------
N = 300
GRAPH_SEED = 11


def layout(n):
    """Where the special nodes of node2vec_graph(n) are: everything below n - 100 is the random part."""
    return dict(base=n - 100, t_nodes=np.arange(n - 100, n - 40), cliques=[range(n - 40 + 6 * k, n - 34 + 6 * k) for k in range(4)],
                dead=[n - 16, n - 15, n - 14], one=n - 13, p_node=n - 10, hub=n - 9, isolated=n - 1)


def node2vec_graph(presorted, n=N, e=1500, big_hub=0):
    """A random graph on the first n - 100 nodes with its reverse edges, duplicate edges and self-loops; four 6-cliques
    (three of them closed, one tied to the random part); dead ends with and without in-edges, a row of degree 1; a hub
    row of 1100 edges into 60 nodes, each of which has an edge to `p_node`, whose only out-edge leads to the hub — so a
    walk from p_node stands on the hub with every candidate in class 1.  `big_hub` adds that many out-edges to one
    node of the random part (a multigraph row)."""
    L = layout(n)
    base, t_nodes = L["base"], L["t_nodes"]
    rng = np.random.default_rng(GRAPH_SEED)
    s, d = rng.integers(0, base, e), rng.integers(0, base, e)
    src, dst = [s, d], [d, s]
    for c in L["cliques"]:
        a, b = zip(*[(u, v) for u in c for v in c if u != v])
        src.append(np.array(a)), dst.append(np.array(b))
    tie, last = rng.integers(0, base, 6), np.array(L["cliques"][3])
    src += [last, tie]
    dst += [tie, last]
    dup = rng.integers(0, e, 40)
    src.append(s[dup]), dst.append(d[dup])
    loops = rng.integers(0, base, 12)
    src.append(loops), dst.append(loops)
    into_dead = rng.integers(0, base, 9)
    src.append(into_dead), dst.append(np.repeat(L["dead"], 3))
    src.append(np.array([L["one"], L["p_node"]])), dst.append(np.array([0, L["hub"]]))
    src.append(np.full(1100, L["hub"])), dst.append(rng.choice(t_nodes, 1100))
    src.append(t_nodes), dst.append(np.full(60, L["p_node"]))
    src.append(np.repeat(t_nodes, 3)), dst.append(rng.integers(0, base, 180))
    if big_hub:
        src.append(np.full(big_hub, base // 2)), dst.append(rng.integers(0, base, big_hub))
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    o = np.argsort(src, kind="stable") if presorted else rng.permutation(len(src))
    src, dst = src[o], dst[o]
    R = csr_from_coo(src, dst, n, n)
    assert (R["data"] is None) == presorted
    deg = np.diff(R["indptr"])
    assert deg[L["hub"]] > K_MAX and deg[L["one"]] == 1 and (deg[L["dead"]] == 0).all() and deg[L["isolated"]] == 0
    assert ((deg > 1) & (deg < K_MIN)).any() and deg.max() >= max(big_hub, 1100)
    return R, len(src)


def walk_seeds(n=N, count=150):
    """Many walks from p_node and the cliques, repeats, dead ends, ids outside the graph, and random nodes."""
    L = layout(n)
    rng = np.random.default_rng(2)
    fixed = [L["p_node"]] * 40 + [c[0] for c in L["cliques"]] * 6 + \
        [L["hub"], L["hub"], L["one"], L["one"], L["dead"][0], L["isolated"], -1, n, 2 ** 31 - 1, 10, 10]
    return np.concatenate([np.array(fixed), rng.integers(0, n - 16, count)])


class Cases:
    """Graphs, weights and the model's 40-step walks, each computed once and shared (never modified).  A walk of fewer
    steps is a prefix of a longer one: a pick depends on (seed, walk, step, slot) and on the walk so far only."""

    def __init__(self):
        self.graphs, self.models = {}, {}
        self.seeds = walk_seeds()

    def graph(self, presorted, weights):
        key = (presorted, weights)
        if key not in self.graphs:
            R, ne = node2vec_graph(presorted)
            prob = None
            if weights is not None:
                prob = messy_weights(ne, np.random.default_rng(5), np.float32 if weights == "f32" else np.float64)
                R = dict(R, cdf=cdf_of(R, prob))
            self.graphs[key] = (R, prob, Model(R))
        return self.graphs[key]

    def model(self, presorted, weights, pq, seed=21):
        key = (presorted, weights, pq, seed)
        if key not in self.models:
            self.models[key] = self.graph(presorted, weights)[2].walk(self.seeds, 40, seed, *pq)
        return self.models[key]


@pytest.fixture(scope="module")
def cases():
    return Cases()


# ---- exact --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pq", PQ)
@pytest.mark.parametrize("presorted", [False, True])
@pytest.mark.parametrize("weights", [None, "f32", "f64"])
def test_host_walker_equals_model(cases, weights, presorted, pq):
    R, prob, _ = cases.graph(presorted, weights)
    mt, me, c = cases.model(presorted, weights, pq)
    for idtype in (torch.int32, torch.int64):
        seeds = cases.seeds.astype(np.int32 if idtype == torch.int32 else np.int64)
        for steps in (0, 1, 7, 40):
            tr, ev, stats = host_n2v(R, seeds, steps, 21, *pq, idtype=idtype, stats=True)
            assert tr.shape == (len(seeds), steps + 1) and ev.shape == (len(seeds), steps)
            assert np.array_equal(tr, mt[:, :steps + 1]) and np.array_equal(ev, me[:, :steps]), (idtype, steps)
            assert stats == c["per_t"][:steps].sum(0).tolist(), (idtype, steps)
    assert stats == [c["steps"], c["attempts"], c["scans"]]
    check_properties([R], [0] * 40, tr, ev, 21, None, [prob])
    assert (tr[:, -1] >= 0).any() and (tr[:, 1] == -1).any()
    assert host_n2v(R, seeds, 7, 21, *pq, return_eids=False)[1] is None


def test_the_graph_exercises_every_path(cases):
    """Asserted on the MODEL: a graph that does not reach the classes, the repeated attempts and the scan fails here."""
    steps, accepted = 0, np.zeros(3)
    for pq in MODERATE:
        c = cases.model(False, None, pq)[2]
        steps += c["steps"]
        accepted += c["accepted"]
        assert c["max_attempts"] >= 2
    print("moderate (p, q): steps", steps, "accepted per class", accepted.tolist())
    assert steps > 5000 and (accepted >= 0.01 * steps).all()
    c = cases.model(False, None, PQ[4])[2]
    print("(1000, 0.001): scans", c["scans"], "of", c["steps"], "steps; K at the scans", sorted(set(c["scan_k"])))
    assert c["scans"] >= 100
    assert K_MIN in c["scan_k"] and K_MAX in c["scan_k"]          # both ends of K's clamp reach the scan
    for w in ("f32", "f64"):
        assert cases.model(False, w, PQ[4])[2]["scans"] >= 100


def test_scan_rounding_fallback():
    """u * S rounds up to S only among subnormal numbers.  0 -> 1 is forced; the row of 1 holds two edges of weight
    2000 * 2^-1074 whose ends both lead back to 0 (class 1, a1 = 1e-3): g = 2 units each, S = 4 units, and a draw above
    7/8 puts x at S, so no running sum exceeds it and the scan takes the last position with mass."""
    tiny = 2000 * 5e-324
    R = csr_from_coo([0, 1, 1, 2, 3, 1], [1, 2, 3, 0, 0, 3], 4, 4)
    prob = np.array([1.0, tiny, tiny, 1.0, 1.0, 0.0])
    R["cdf"] = cdf_of(R, prob)
    seeds = np.zeros(400, dtype=np.int64)
    mt, me, c = Model(R).walk(seeds, 2, 3, 1000.0, 0.001)
    print("scans", c["scans"], "fallbacks", c["fallbacks"])
    assert c["scans"] >= 300 and c["fallbacks"] >= 20
    for idtype in (torch.int32, torch.int64):
        tr, ev, stats = host_n2v(R, seeds, 2, 3, 1000.0, 0.001, idtype=idtype, stats=True)
        assert np.array_equal(tr, mt) and np.array_equal(ev, me) and stats == [c["steps"], c["attempts"], c["scans"]]
    assert set(me[:, 1]) == {1, 2}       # the zero-weight edge 5 is the row's last position and is never the fallback


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("presorted", [False, True])
@pytest.mark.parametrize("weights", [None, "f32", "f64"])
def test_p_q_one_is_the_first_order_walk(cases, weights, presorted, idtype):
    R, prob, _ = cases.graph(presorted, weights)
    seeds = cases.seeds.astype(np.int32 if idtype == torch.int32 else np.int64)
    for steps, seed in ((1, 5), (7, 2 ** 63 + 11), (40, 9)):
        tr, ev, stats = host_n2v(R, seeds, steps, seed, 1.0, 1.0, idtype=idtype, stats=True)
        ht, he = host_walk([R], [0] * steps, seeds, seed, None, idtype)
        assert np.array_equal(tr, ht) and np.array_equal(ev, he)
        assert stats[1] == stats[0] and stats[2] == 0                # one attempt per step, never the scan


# ---- distribution ---------------------------------------------------------------------------------
def forced_graph():
    """12 nodes.  0 -> 1 and 6 -> 7 are the only out-edges of 0 and 6, so prev and curr of the second step are forced.
    Row of 1: 0 (class 0), 2 twice, 3 and the self-loop 1 (class 1: 2 -> 0, 3 -> 0, 1 -> 0 exist), 4 and 5 (class 2).
    Row of 7: 6 (class 0), 8 twice, 9, 10, 11 and the self-loop 7, all with an edge to 6 (class 1): no class 2."""
    src = [0, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 7, 7, 7, 7, 7, 7, 8, 9, 10, 11]
    dst = [1, 0, 2, 2, 3, 1, 4, 5, 0, 0, 4, 2, 7, 6, 8, 8, 9, 10, 11, 7, 6, 6, 6, 6]
    return csr_from_coo(src, dst, 12, 12)


def exact_law(R, prob, curr, prev, p, q):
    """(edge ids of curr's row, exact node2vec probabilities)."""
    m = Model(R)
    a = accept_probs(p, q)
    lo, hi = m.indptr[curr], m.indptr[curr + 1]
    eid = np.arange(lo, hi) if m.data is None else np.array(m.data[lo:hi])
    w = np.ones(hi - lo) if prob is None else np.asarray(prob, dtype=np.float64)[eid]
    mass = np.array([w[j] * a[m.klass(m.indices[lo + j], prev)] for j in range(hi - lo)])
    return eid, mass / mass.sum()


def pooled_chi2(counts, expected):
    """Chi-square with the cells of expectation < 5 pooled into the smallest other cell; returns (value, dof)."""
    small = expected < 5
    if small.any() and not small.all():
        k = np.nonzero(~small)[0][np.argmin(expected[~small])]
        counts, expected = counts.astype(np.float64), expected.copy()
        counts[k] += counts[small].sum()
        expected[k] += expected[small].sum()
        counts, expected = counts[~small], expected[~small]
    return chi2(counts, expected), len(expected) - 1


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("start,pq,served", [(0, (0.5, 2.0), "rejection"), (0, (1000.0, 0.001), "both"),
                                             (6, (1000.0, 0.001), "scan")])
def test_second_step_follows_the_node2vec_law(seed, weighted, start, pq, served):
    R = forced_graph()
    prob = None
    if weighted:
        prob = np.array([1, 2, 3, 1, 4, 2, 5, 1, 1, 1, 1, 1, 1, 3, 1, 2, 5, 4, 2, 1, 1, 1, 1, 1], dtype=np.float32)
        R["cdf"] = cdf_of(R, prob)
    walks = 200000
    tr, ev, stats = host_n2v(R, np.full(walks, start), 2, seed, *pq, stats=True)
    assert (tr[:, 1] == start + 1).all() and stats[0] == walks
    eid, law = exact_law(R, prob, start + 1, start, *pq)
    counts = np.array([(ev[:, 1] == e).sum() for e in eid])
    assert counts.sum() == walks and len(eid) == 7
    share = stats[2] / stats[0]
    print("attempts per step %.3f, share of steps served by the scan %.4f" % (stats[1] / stats[0], share))
    # row of 1 holds class 2 (a2 = 1 at (1000, 0.001)), so rejection still serves there; the row of 7 does not
    assert {"rejection": share < 0.05, "both": 0.01 < share < 0.9, "scan": share > 0.95}[served]
    x, dof = pooled_chi2(counts, walks * law)
    print("counts", counts.tolist(), "expected", np.round(walks * law, 1).tolist(), "chi2(%d) = %.2f" % (dof, x))
    assert x < CHI2_1E6[dof]


# ---- the reference's own property check -----------------------------------------------------------
def test_reference_property_check():
    """tests/python/common/sampling/test_sampling.py test_node2vec: its two graphs, prob = [3, 0, 3, 3, 3], p = q = 1,
    four steps; every hop is an edge with that edge id and the zero-weight edge is never taken."""
    g1 = csr_from_coo([0, 1, 2], [1, 2, 0], 3, 3)
    tr, ev = host_n2v(g1, [0, 1, 2, 0, 1, 2], 4, 1, 1.0, 1.0)
    check_properties([g1], [0] * 4, tr, ev, 1)
    assert (tr >= 0).all()
    g2 = csr_from_coo([0, 1, 1, 2, 3], [1, 2, 3, 0, 0], 4, 4)
    prob = np.array([3, 0, 3, 3, 3], dtype=np.float32)
    g2["cdf"] = cdf_of(g2, prob)
    for p, q in PQ:
        tr, ev = host_n2v(g2, [0, 1, 2, 3, 0, 1, 2, 3], 4, 1, p, q)
        check_properties([g2], [0] * 4, tr, ev, 1, None, [prob])
        assert (tr >= 0).all() and not (ev == 1).any()


# ---- C ABI ---------------------------------------------------------------------------------------
NEW = ["dgla_csr_sorted_columns_workspace_bytes", "dgla_csr_sorted_columns", "dgla_node2vec_walk", "dgla_node2vec_walk_host"]


def test_header_declares_and_library_exports_the_entry_points():
    from dgl_amd import _lib

    with open(os.path.join(ROOT, "include", "dgl_amd.h")) as fh:
        hdr = fh.read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(_lib.LIB, name), name
    assert "#define DGLA_ABI_VERSION 2" in hdr
    # the header quotes the rule of csrc/node2vec_step.h in full
    with open(os.path.join(ROOT, "dgl_amd", "csrc", "node2vec_step.h")) as fh:
        step = fh.read()
    squeeze = lambda s: " ".join(re.sub(r"^\s*(//|\*)", "", line).strip() for line in s.splitlines())
    rule = step[step.index("// Setting."):step.index("#pragma once")]
    assert len(rule.splitlines()) > 30 and squeeze(rule) in squeeze(hdr)
    assert "K = min(max(deg, 8), 1024)" in rule and "kN2vMinAttempts = 8, kN2vMaxAttempts = 1024" in step
    assert "#pragma clang fp contract(off)" in step and '#include "random_walk_step.h"' in step
    for name in ("rw_mix64", "rw_walk_key", "rw_step_key", "rw_draw", "rw_index", "rw_uniform", "rw_pick_weighted"):
        assert not re.search(r"\b%s\s*\([^)]*\)\s*\{" % name, step), name + " is defined again instead of included"


def test_bad_arguments_fail_with_a_message():
    from dgl_amd import _capi, _lib

    def csr(n_rows, n_cols, dt=torch.int64):
        return _capi.host_csr(torch.zeros(n_rows + 1, dtype=dt), torch.zeros(0, dtype=dt), None, n_cols)

    seeds = torch.zeros(2, dtype=torch.int64)
    none = torch.zeros(0, dtype=torch.int64)
    with pytest.raises(_lib.DGLAMDError, match="num_rows 3 != num_cols 4"):
        _capi.node2vec_walk_host(csr(3, 4), None, none, seeds, 3, 1.0, 1.0)
    for p, q in ((0.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (1.0, float("inf")), (1e-320, 1.0), (1e300, 1e-300)):
        with pytest.raises(_lib.DGLAMDError, match="p and q must be finite and > 0"):
            _capi.node2vec_walk_host(csr(3, 3), None, none, seeds, 3, p, q)
    with pytest.raises(_lib.DGLAMDError, match="id type"):
        _capi.node2vec_walk_host(csr(3, 3), None, none, seeds.int(), 3, 1.0, 1.0)
    with pytest.raises(_lib.DGLAMDError, match="member"):
        _capi.node2vec_walk_host(csr(3, 3), None, none.int(), seeds, 3, 1.0, 1.0)
    tr, ev = _capi.node2vec_walk_host(csr(3, 3), None, none, seeds, 3, 1.0, 1.0)
    assert tr.tolist() == [[0, -1, -1, -1]] * 2 and ev.tolist() == [[-1] * 3] * 2
    # the raw entries refuse NULL arrays, and the device entry refuses before it touches the GPU
    err = lambda: _lib.LIB.dgla_last_error().decode()
    full = _capi.host_csr(torch.tensor([0, 1, 2]), torch.tensor([1, 0]), None, 2)
    ref = ctypes.byref
    out = torch.zeros(8, dtype=torch.int64)
    L = _lib.LIB
    assert L.dgla_node2vec_walk_host(None, None, None, seeds.data_ptr(), 2, 3, 1.0, 1.0, 0, out.data_ptr(), None, None) == -1
    assert "csr is null" in err()
    assert L.dgla_node2vec_walk_host(ref(full), None, None, seeds.data_ptr(), 2, 3, 1.0, 1.0, 0, out.data_ptr(), None, None) == -1
    assert "member" in err()
    assert L.dgla_node2vec_walk(ref(full), None, full._keep[1].data_ptr(), None, 2, 3, 1.0, 1.0, 0, out.data_ptr(), None, None) == -1
    assert "seeds / traces are null" in err()
    assert L.dgla_node2vec_walk(ref(full), None, full._keep[1].data_ptr(), seeds.data_ptr(), 2, 3, 0.0, 1.0, 0, out.data_ptr(),
                                None, None) == -1 and "p and q" in err()
    assert L.dgla_csr_sorted_columns(None, None, None, 0, None) == -1 and "csr is null" in err()
    assert L.dgla_csr_sorted_columns_workspace_bytes(ref(full)) > 0
    assert L.dgla_csr_sorted_columns(ref(full), out.data_ptr(), None, 0, None) == -1 and "workspace" in err()


# ---- Python surface ------------------------------------------------------------------------------
def test_argument_errors_before_any_launch():
    import dgl_amd
    from dgl_amd import sampling

    assert dgl_amd.node2vec_random_walk is sampling.node2vec_random_walk
    g1 = dgl_amd.graph(([0, 1, 1, 2, 3], [1, 2, 3, 0, 0]))
    g2 = dgl_amd.heterograph({("user", "follow", "user"): ([0, 1], [1, 0]), ("user", "view", "item"): ([0, 1], [0, 1])})
    with pytest.raises(dgl_amd.DGLError, match="Node2vec only support homogeneous graph"):
        sampling.node2vec_random_walk(g2, [0, 1], 1, 1, 4)
    with pytest.raises(dgl_amd.DGLError, match="data type"):
        sampling.node2vec_random_walk(g1, torch.tensor([0, 1], dtype=torch.int32), 1, 1, 4)
    g1.edata["short"] = torch.ones(5, 2)
    with pytest.raises(dgl_amd.DGLError, match="one value per edge"):
        sampling.node2vec_random_walk(g1, [0, 1], 1, 1, 4, prob="short")
    with pytest.raises(dgl_amd.DGLError, match="one value per edge"):
        sampling.node2vec_random_walk(g1, [0, 1], 1, 1, 4, prob=torch.ones(4))
    for p, q in ((0, 1), (1, -1), (float("nan"), 1), (1, float("inf"))):
        with pytest.raises(dgl_amd.DGLError, match="finite and > 0"):
            sampling.node2vec_random_walk(g1, [0, 1], p, q, 4)
    with pytest.raises(dgl_amd.DGLError, match="no CPU fallback"):     # valid arguments, a graph that is not on a GPU
        sampling.node2vec_random_walk(g1, [0, 1], 1, 1, 4)
