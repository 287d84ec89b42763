"""Random walks (include/dgl_amd.h "random walks", csrc/random_walk_step.h) through the HOST walker — runs without a GPU.

dgla_random_walk_host compiles the one definition of the step rule that random_walk_kernel compiles for the device, so
what is pinned here is pinned for the kernel too (tests/test_zzzzzz_gpu_random_walk.py checks device == host bit for bit).
The checker is an independent numpy restatement of the rule, written below from the text of the header.

Exact: generator known answers; host walker == numpy model (uniform, weighted, mixed metapath, scalar and stepwise
restart, int32 / int64, with and without an edge-id map).  Properties: every hop is an edge of its relation with that
edge id, -1 only trails, halts only at dead ends or restart draws, unusable weights never traversed.  Distributions on
fixed seeds against the upper 1e-6 quantile of the chi-square law.  API surface of dgl_amd.sampling.random_walk /
pack_traces.  Reference: python/dgl/sampling/randomwalks.py, src/graph/sampling/randomwalks/."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
SEEDS = (7, 8, 42)


# ---- the numpy model of the rule ---------------------------------------------------------------
def mix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def draw(seed, i, t, k):
    """r(seed, i, t, k) for arrays (or scalars) of walk indices."""
    with np.errstate(over="ignore"):
        i = np.asarray(i, dtype=U64)
        a = mix64(U64(seed & (2 ** 64 - 1)) ^ (i * U64(0xD1B54A32D192ED03)))
        return mix64(mix64(a + U64(t)) + U64(k))


def mulhi(r, n):
    """(r * n) >> 64 by 32-bit limbs."""
    r, n = np.asarray(r, dtype=U64), np.asarray(n, dtype=U64)
    m = U64(0xFFFFFFFF)
    rl, rh, nl, nh = r & m, r >> U64(32), n & m, n >> U64(32)
    with np.errstate(over="ignore"):
        mid = (rl * nl >> U64(32)) + (rh * nl & m) + (rl * nh & m)
        return rh * nh + (rh * nl >> U64(32)) + (rl * nh >> U64(32)) + (mid >> U64(32))


def uniform(r):
    return (np.asarray(r, dtype=U64) >> U64(11)).astype(np.float64) * 2.0 ** -53


def csr_from_coo(src, dst, num_rows, num_cols):
    """Out-edge CSR of a COO in edge-id order: a stable sort by source; no edge-id map when already sorted."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    indptr = np.zeros(num_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=num_rows), out=indptr[1:])
    data = None if np.array_equal(order, np.arange(len(src))) else order.astype(np.int64)
    return dict(indptr=indptr, indices=dst[order], data=data, cdf=None, num_rows=num_rows, num_cols=num_cols)


def usable(prob):
    w = np.asarray(prob, dtype=np.float64)
    return np.where(w > 0, w, 0.0)      # negative and NaN -> 0


def cdf_of(rel, prob):
    """Sequential fp64 running sum per row of w' in CSR position order (prob is indexed by EDGE ID)."""
    nnz = len(rel["indices"])
    eid = rel["data"] if rel["data"] is not None else np.arange(nnz)
    w = usable(prob)[eid]
    out = np.zeros(nnz, dtype=np.float64)
    ip = rel["indptr"]
    for r in range(rel["num_rows"]):
        out[ip[r]:ip[r + 1]] = np.cumsum(w[ip[r]:ip[r + 1]])
    return out


def model_walk(rels, metapath, seeds, seed, restart=None):
    """The rule of the header, step by step.  restart: None, a float, or an array with one entry per step."""
    seeds = np.asarray(seeds, dtype=np.int64)
    n, steps = len(seeds), len(metapath)
    traces = np.full((n, steps + 1), -1, dtype=np.int64)
    eids = np.full((n, steps), -1, dtype=np.int64)
    traces[:, 0] = seeds
    walk = np.arange(n)
    curr = seeds.copy()
    alive = np.ones(n, dtype=bool)
    if steps:
        alive &= (seeds >= 0) & (seeds < rels[metapath[0]]["num_rows"])
    for t, m in enumerate(metapath):
        R = rels[m]
        if restart is not None:
            p_t = float(restart) if np.isscalar(restart) else float(np.asarray(restart)[t])   # fp32 -> double
            alive &= ~(uniform(draw(seed, walk, t, 1)) < p_t)
        c = np.where(alive, curr, 0)
        lo, hi = R["indptr"][c], R["indptr"][c + 1]
        alive &= hi > lo
        r0 = draw(seed, walk, t, 0)
        pos = np.zeros(n, dtype=np.int64)
        if R["cdf"] is None:
            deg = np.where(alive, hi - lo, 1)
            pos = lo + mulhi(r0, deg).astype(np.int64)
        else:
            u = uniform(r0)
            for i in np.nonzero(alive)[0]:
                row = R["cdf"][lo[i]:hi[i]]
                total = row[-1]
                if not (total > 0) or not np.isfinite(total):
                    alive[i] = False
                    continue
                x = u[i] * total
                k = int(np.searchsorted(row, x, side="right"))      # first cdf > x
                if k == len(row):
                    k = int(np.searchsorted(row, total, side="left"))   # first cdf == total
                pos[i] = lo[i] + k
        a = np.nonzero(alive)[0]
        nxt = R["indices"][pos[a]]
        traces[a, t + 1] = nxt
        eids[a, t] = pos[a] if R["data"] is None else R["data"][pos[a]]
        curr[a] = nxt
    return traces, eids


# ---- the host walker ---------------------------------------------------------------------------
def host_walk(rels, metapath, seeds, seed, restart=None, idtype=torch.int64, return_eids=True):
    from dgl_amd import _capi

    def t_(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(idtype)

    table = []
    for R in rels:
        csr = _capi.host_csr(t_(R["indptr"]), t_(R["indices"]), t_(R["data"]), R["num_cols"])
        table.append((csr, None if R["cdf"] is None else torch.from_numpy(R["cdf"])))
    kw = {}
    if restart is not None:
        if np.isscalar(restart):
            kw["restart_prob"] = float(restart)
        else:
            kw["restart_steps"] = torch.from_numpy(np.ascontiguousarray(restart))
    tr, ev = _capi.random_walk_host(table, list(metapath), torch.as_tensor(np.asarray(seeds), dtype=idtype), rng_seed=seed,
                                    return_eids=return_eids, **kw)
    assert tr.dtype == idtype
    return tr.numpy().astype(np.int64), None if ev is None else ev.numpy().astype(np.int64)


def check_properties(rels, metapath, traces, eids, seed, restart=None, probs=None):
    """Integer work only.  probs[m]: the EDGE-ID indexed weights of relation m (None = uniform)."""
    n, steps = eids.shape
    assert traces.shape == (n, steps + 1)
    dead = traces == -1
    assert (dead[:, 1:-1] <= dead[:, 2:]).all(), "a node after a -1"
    assert ((eids == -1) == dead[:, 1:]).all()
    walk = np.arange(n)
    for t, m in enumerate(metapath):
        R = rels[m]
        nnz = len(R["indices"])
        src_of_pos = np.repeat(np.arange(R["num_rows"]), np.diff(R["indptr"]))
        eid_of_pos = R["data"] if R["data"] is not None else np.arange(nnz)
        pos_of_eid = np.empty(nnz, dtype=np.int64)
        pos_of_eid[eid_of_pos] = np.arange(nnz)
        went = ~dead[:, t + 1]
        p = pos_of_eid[eids[went, t]]
        assert np.array_equal(src_of_pos[p], traces[went, t]) and np.array_equal(R["indices"][p], traces[went, t + 1])
        w_eid = np.ones(nnz) if probs is None or probs[m] is None else usable(probs[m])
        assert (w_eid[eids[went, t]] > 0).all(), "a zero / negative / NaN weight was traversed"
        # halts: a node without usable out-edges, a restart draw, or (step 0) a seed outside the graph
        halted = dead[:, t + 1] & (~dead[:, t] if t else np.ones(n, dtype=bool))
        node = traces[halted, t]
        inside = (node >= 0) & (node < R["num_rows"])
        strength = np.bincount(src_of_pos, weights=w_eid[eid_of_pos], minlength=R["num_rows"])
        ok = ~inside
        ok[inside] = ~(strength[node[inside]] > 0)
        if restart is not None:
            p_t = float(restart) if np.isscalar(restart) else float(np.asarray(restart)[t])
            ok |= uniform(draw(seed, walk[halted], t, 1)) < p_t
        assert ok.all(), "a walk halted at a node with usable out-edges and without a restart draw"


# ---- graphs ------------------------------------------------------------------------------------
def skewed_graph(n, e, hub, rng, presorted=False):
    """Out-degrees skewed (src = min(floor(U^3 n), n-1)) so that some nodes have no out-edge, plus one hub row."""
    src = np.minimum(np.floor(rng.random(e) ** 3 * n), n - 1).astype(np.int64)
    src = np.concatenate([src, np.full(hub, n // 2, dtype=np.int64)])
    dst = rng.integers(0, n, size=len(src))
    if presorted:
        o = np.argsort(src, kind="stable")
        src, dst = src[o], dst[o]
    return src, dst


def messy_weights(count, rng, dtype=np.float32):
    w = rng.random(count).astype(dtype) + dtype(0.05)
    w[rng.random(count) < 0.1] = 0
    w[rng.random(count) < 0.03] = -1
    w[rng.random(count) < 0.03] = np.nan
    return w


def chi2(counts, expected):
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


# ---- exact --------------------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), 0x238275bc38fcbe91, 5, 0.13870941014555427),
         ((7, 3, 2, 1), 0xfbc3e871920ad92b, 39, 0.9834580685874629),
         ((42, 1000000, 79, 0), 0xd27dc01212f09285, 32, 0.8222312969327865),
         ((2 ** 64 - 1, 2 ** 40 + 5, 3, 1), 0x1d89e72052ada5c6, 4, 0.11538548030028162)]


def test_generator_known_answers():
    for (seed, i, t, k), r, idx, u in KNOWN:
        got = draw(seed, i, t, k)
        assert int(got) == r
        assert int(mulhi(got, 40)) == idx == (r * 40) >> 64
        assert float(uniform(got)) == u
    # ... and the library computes the same stream: node 0 with 40 successors, walk 0, step 0, seed 0 -> position 5;
    # walk 3 at step 2 under seed 7 restarts exactly when p > 0.98345...
    star = csr_from_coo(np.zeros(40, dtype=np.int64), np.arange(40), 40, 40)
    tr, ev = host_walk([star], [0], [0], 0)
    assert tr.tolist() == [[0, 5]] and ev.tolist() == [[5]]
    loop = csr_from_coo([0], [0], 1, 1)
    for p, alive in ((0.9834580685874629, True), (0.983458068587463, False)):
        tr, _ = host_walk([loop], [0, 0, 0], [0, 0, 0, 0], 7, restart=np.array([0.0, 0.0, p]))
        assert (tr[3, 3] == 0) == alive and tr[3, 2] == 0


@pytest.fixture(scope="module")
def skewed():
    rng = np.random.default_rng(5)
    out = {}
    for presorted in (False, True):
        src, dst = skewed_graph(300, 4000, 700, rng, presorted)
        R = csr_from_coo(src, dst, 300, 300)
        assert (R["data"] is None) == presorted and (np.diff(R["indptr"]) == 0).any()
        out[presorted] = (R, messy_weights(len(src), rng, np.float32), messy_weights(len(src), rng, np.float64))
    return out


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("presorted", [False, True])
@pytest.mark.parametrize("weights", [None, "f32", "f64"])
@pytest.mark.parametrize("restart", [None, 0.2, "steps32", "steps64"])
def test_host_walker_equals_numpy_model(skewed, idtype, presorted, weights, restart):
    R, w32, w64 = skewed[presorted]
    prob = {None: None, "f32": w32, "f64": w64}[weights]
    R = dict(R, cdf=None if prob is None else cdf_of(R, prob))
    steps = 9
    if restart == "steps32":
        restart = np.array([0, 0.5, 0.1, 0, 0.3, 0, 0, 0.9, 0.05], dtype=np.float32)
    elif restart == "steps64":
        restart = np.array([0.1, 0, 0.3, 0, 0.3, 1e-3, 0, 0.2, 0.05], dtype=np.float64)
    seeds = np.concatenate([np.random.default_rng(1).integers(0, 300, size=700), [150, 150, 299, 300, -1, 10 ** 6]])
    for seed in (3, 2 ** 63 + 11):
        tr, ev = host_walk([R], [0] * steps, seeds, seed, restart, idtype)
        mt, me = model_walk([R], [0] * steps, seeds.astype(np.int32 if idtype == torch.int32 else np.int64), seed, restart)
        assert np.array_equal(tr, mt) and np.array_equal(ev, me)
        check_properties([R], [0] * steps, tr, ev, seed, restart, [prob])
    assert (tr[:, -1] >= 0).any() and (tr[:, 1] == -1).any()     # some walks finish, some die at once


def hetero_rels(rng, n_user=60, n_item=40):
    """user -follow-> user, user -view-> item, item -viewed-by-> user; `view` carries weights."""
    f = csr_from_coo(rng.integers(0, n_user, 300), rng.integers(0, n_user, 300), n_user, n_user)
    v = csr_from_coo(rng.integers(0, n_user, 250), rng.integers(0, n_item, 250), n_user, n_item)
    b = csr_from_coo(rng.integers(0, n_item, 200), rng.integers(0, n_user, 200), n_item, n_user)
    wv = messy_weights(250, rng)
    v["cdf"] = cdf_of(v, wv)
    return [f, v, b], [None, wv, None]


@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_mixed_metapath_equals_numpy_model(idtype):
    rels, probs = hetero_rels(np.random.default_rng(9))
    path = [0, 1, 2] * 2
    seeds = np.arange(200) % 60
    for restart in (None, np.array([0, 0.5, 0, 0, 0.5, 0], dtype=np.float32)):
        tr, ev = host_walk(rels, path, seeds, 11, restart, idtype)
        mt, me = model_walk(rels, path, seeds, 11, restart)
        assert np.array_equal(tr, mt) and np.array_equal(ev, me)
        check_properties(rels, path, tr, ev, 11, restart, probs)
    # without eids; zero steps; zero seeds
    assert host_walk(rels, path, seeds, 11, None, idtype, return_eids=False)[1] is None
    tr, ev = host_walk(rels, [], seeds, 11, None, idtype)
    assert tr.shape == (200, 1) and ev.shape == (200, 0) and np.array_equal(tr[:, 0], seeds)
    tr, ev = host_walk(rels, path, np.zeros(0, dtype=np.int64), 11, None, idtype)
    assert tr.shape == (0, 7) and ev.shape == (0, 6)


# ---- distributions -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_pick_is_uniform(seed):
    star = csr_from_coo(np.zeros(40, dtype=np.int64), np.arange(40), 40, 40)
    tr, _ = host_walk([star], [0], np.zeros(6000, dtype=np.int64), seed)
    x = chi2(np.bincount(tr[:, 1], minlength=40), np.full(40, 150.0))
    print("chi2(39) =", x)
    assert x < 96.2


@pytest.mark.parametrize("seed", SEEDS)
def test_weighted_pick_follows_the_weights(seed):
    R = csr_from_coo(np.zeros(8, dtype=np.int64), np.arange(8), 8, 8)
    w = np.arange(8, dtype=np.float32)
    R["cdf"] = cdf_of(R, w)
    tr, ev = host_walk([R], [0], np.zeros(28000, dtype=np.int64), seed)
    counts = np.bincount(ev[:, 0], minlength=8)
    print("counts =", counts.tolist())
    assert counts[0] == 0
    if seed == 7:
        assert counts.tolist() == [0, 939, 2009, 2913, 4065, 5056, 6002, 7016]
    x = chi2(counts[1:], 1000.0 * w[1:])
    print("chi2(6) =", x)
    assert x < 38.3


@pytest.mark.parametrize("seed", SEEDS)
def test_two_step_walks_are_uniform_over_cells(seed):
    src, dst = zip(*[(a, b) for a in range(5) for b in range(5) if a != b])
    K5 = csr_from_coo(src, dst, 5, 5)
    tr, _ = host_walk([K5], [0, 0], np.zeros(20000, dtype=np.int64), seed)
    cells = np.bincount(tr[:, 1] * 5 + tr[:, 2], minlength=25)
    reach = [a * 5 + b for a in range(1, 5) for b in range(5) if a != b]
    assert len(reach) == 16 and cells.sum() == cells[reach].sum() == 20000
    x = chi2(cells[reach], np.full(16, 1250.0))
    print("chi2(15) =", x)
    assert x < 56.5


@pytest.mark.parametrize("seed", SEEDS)
def test_restart_survival_rate(seed):
    cyc = csr_from_coo(np.arange(16), (np.arange(16) + 1) % 16, 16, 16)
    seeds = np.arange(20000) % 16
    tr, _ = host_walk([cyc], [0] * 10, seeds, seed, 0.25)
    for t in range(10):
        before, after = (tr[:, t] >= 0).sum(), (tr[:, t + 1] >= 0).sum()
        dev = abs(after / before - 0.75)
        print("step %d: alive %d -> %d, deviation %.4f, bar %.4f" % (t, before, after, dev, 5 * np.sqrt(0.1875 / before)))
        assert dev <= 5 * np.sqrt(0.1875 / before)
    tr2, _ = host_walk([cyc], [0] * 10, seeds, seed, np.full(10, 0.25, dtype=np.float32))
    assert np.array_equal(tr, tr2)


# ---- C ABI ---------------------------------------------------------------------------------------
NEW = ["dgla_random_walk_cdf_workspace_bytes", "dgla_random_walk_cdf", "dgla_random_walk_workspace_bytes",
       "dgla_random_walk", "dgla_random_walk_host"]


def test_header_declares_and_library_exports_the_entry_points():
    from dgl_amd import _lib

    with open(os.path.join(ROOT, "include", "dgl_amd.h")) as fh:
        hdr = fh.read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(_lib.LIB, name), name
    assert "dgla_walk_relation" in code and "#define DGLA_ABI_VERSION 2" in hdr
    # the header carries the rule in the words of csrc/random_walk_step.h
    with open(os.path.join(ROOT, "dgl_amd", "csrc", "random_walk_step.h")) as fh:
        step = fh.read()
    squeeze = lambda s: " ".join(re.sub(r"^\s*(//|\*)", "", line).strip() for line in s.splitlines())
    for phrase in ("r(seed,i,t,k) = mix64( mix64( mix64(seed ^ (i * 0xD1B54A32D192ED03)) + t ) + k )",
                   "If there is none (rounding), pos is the first position with cdf[pos] == total.",
                   "A seed outside [0, num_rows of rels[metapath[0]]) halts at once and touches no memory through that id.",
                   "w'(pos) == 0 implies cdf[pos] == cdf[pos-1]"):
        assert phrase in squeeze(hdr) and phrase in squeeze(step), phrase


def test_bad_arguments_fail_with_a_message():
    from dgl_amd import _capi, _lib

    def csr(n_rows, n_cols, dt=torch.int64):
        return _capi.host_csr(torch.zeros(n_rows + 1, dtype=dt), torch.zeros(0, dtype=dt), None, n_cols)

    seeds = torch.zeros(2, dtype=torch.int64)
    err = lambda: _lib.LIB.dgla_last_error().decode()
    a, b = csr(3, 4), csr(4, 3)
    with pytest.raises(_lib.DGLAMDError, match="null or empty"):
        _capi.random_walk_host([], [], seeds)
    with pytest.raises(_lib.DGLAMDError, match="mixed id widths"):
        _capi.random_walk_host([(a, None), (csr(4, 3, torch.int32), None)], [0, 1], seeds)
    with pytest.raises(_lib.DGLAMDError, match="out of range"):
        _capi.random_walk_host([(a, None), (b, None)], [0, 2], seeds)
    with pytest.raises(_lib.DGLAMDError, match="does not chain"):
        _capi.random_walk_host([(a, None), (b, None)], [0, 0], seeds)
    tr, _ = _capi.random_walk_host([(a, None), (b, None)], [0, 1, 0], seeds)
    assert tr.tolist() == [[0, -1, -1, -1]] * 2
    # the device entry refuses a missing workspace before it touches the GPU: 17 relations / 257 steps exceed the
    # kernel arguments
    assert _lib.LIB.dgla_random_walk_workspace_bytes(16, 256) == 0
    sq = csr(3, 3)
    for nrel, steps in ((17, 4), (1, 257)):
        need = _lib.LIB.dgla_random_walk_workspace_bytes(nrel, steps)
        assert need > 0
        args, tr, ev, keep = _capi._walk_args([(sq, None)] * nrel, [0] * steps, seeds, 0.0, None, 0, True)
        assert _lib.LIB.dgla_random_walk(*args, None, 0, None) == -1 and "workspace" in err()
        assert _lib.LIB.dgla_random_walk(*args, tr.data_ptr(), need - 1, None) == -1 and "workspace" in err()


# ---- Python surface ------------------------------------------------------------------------------
def _hetero():
    import dgl_amd

    return dgl_amd.heterograph({("user", "follow", "user"): ([0, 1, 1, 2, 3], [1, 2, 3, 0, 0]),
                                ("user", "view", "item"): ([0, 0, 1, 2, 3, 3], [0, 1, 1, 2, 2, 1]),
                                ("item", "viewed-by", "user"): ([0, 1, 1, 2, 2, 1], [0, 0, 1, 2, 3, 3])})


def test_argument_errors_and_types():
    import dgl_amd
    from dgl_amd import sampling

    g2 = _hetero()
    g1 = dgl_amd.graph(([0, 1, 1, 2, 3], [1, 2, 3, 0, 0]))
    with pytest.raises(dgl_amd.DGLError, match="metapath not specified and the graph is not homogeneous."):
        sampling.random_walk(g2, [0, 1], length=4)
    with pytest.raises(ValueError, match="Please specify either the metapath or the random walk length."):
        sampling.random_walk(g1, [0, 1])
    with pytest.raises(TypeError, match="restart_prob should be float or Tensor."):
        sampling.random_walk(g1, [0, 1], length=4, restart_prob=1)
    with pytest.raises(dgl_amd.DGLError, match="does not chain"):
        sampling.random_walk(g2, [0, 1], metapath=["follow", "view", "view"])
    with pytest.raises(dgl_amd.DGLError, match="one entry per step"):
        sampling.random_walk(g1, [0, 1], length=4, restart_prob=torch.tensor([0.5, 0.5]))
    with pytest.raises(dgl_amd.DGLError, match="data type"):
        sampling.random_walk(g1, torch.tensor([0, 1], dtype=torch.int32), length=4)
    path, types = sampling._walk_plan(g2, ["follow", "view", "viewed-by"] * 2, None)
    user, item = g2.get_ntype_id("user"), g2.get_ntype_id("item")
    assert types == [user, user, item, user, user, item, user]
    assert path == [g2.get_etype_id(e) for e in ["follow", "view", "viewed-by"] * 2]
    assert sampling._walk_plan(g1, None, 3) == ([0, 0, 0], [0, 0, 0, 0])


def test_cpu_graph_is_refused():
    import dgl_amd
    from dgl_amd import sampling

    g1 = dgl_amd.graph(([0, 1, 1, 2, 3], [1, 2, 3, 0, 0]))
    with pytest.raises(dgl_amd.DGLError, match="no CPU fallback"):
        sampling.random_walk(g1, [0, 1], length=4)
    with pytest.raises(dgl_amd.DGLError, match="no CPU fallback"):
        sampling.random_walk(_hetero(), [0, 1], metapath=["follow", "view", "viewed-by"], prob="p")


def test_pack_traces():
    from dgl_amd.sampling import pack_traces

    traces = torch.tensor([[0, 1, -1, -1, -1, -1, -1], [0, 1, 1, 3, 0, 0, 0]])
    types = torch.tensor([0, 0, 1, 0, 0, 1, 0])
    vids, vtypes, lengths, offsets = pack_traces(traces, types)
    assert vids.tolist() == [0, 1, 0, 1, 1, 3, 0, 0, 0] and vtypes.tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 0]
    assert lengths.tolist() == [2, 7] and offsets.tolist() == [0, 2]
    full = torch.tensor([[4, 5, 6], [7, 8, 9], [1, 1, 1]], dtype=torch.int32)
    vids, vtypes, lengths, offsets = pack_traces(full, torch.tensor([0, 1, 0], dtype=torch.int32))
    assert vids.tolist() == [4, 5, 6, 7, 8, 9, 1, 1, 1] and vtypes.tolist() == [0, 1, 0] * 3
    assert lengths.tolist() == [3, 3, 3] and offsets.tolist() == [0, 3, 6] and vids.dtype == torch.int32
