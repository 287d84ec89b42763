"""Graphs, the numpy model and the host-function wrappers of the layer-neighbour sampling tests
(tests/test_labor_host.py, tests/test_zzzzzzzzzz_gpu_labor.py).

The model is an independent restatement of the rule of csrc/labor_step.h written from its text: the variate with the
numpy generator of tests/test_random_walk_host.py (Python-integer semantics on uint64 arrays), the uniform test by the
32-bit-limb multiply-high, the weighted test and the importances by whole-array fp64 arithmetic, the scale by an exact
solve over the sorted weights (no iteration)."""
import numpy as np
import torch

from tests.test_random_walk_host import draw, mulhi, uniform, usable

# degrees around every fanout the tests use (k - 1, k, k + 1 for k in 1, 5, 10), around the 16- and 64-lane steps of
# the kernels, several 64-position steps, and one hub past 2^16
DEGREES = [0, 1, 2, 4, 5, 6, 9, 10, 11, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025, 70000]
NUM_NBR = 3000        # neighbour ids: the long rows must repeat some (a multigraph), the short ones share many


def labor_graph(pad_rows=0, seed=5):
    """CSR (rows = the seed side) with one row per entry of DEGREES, then a multigraph row, then `pad_rows` empty rows
    (they pull the mean degree under the kernels' 16-lane threshold).  With an edge-id map (a permutation)."""
    rng = np.random.default_rng(seed)
    rows = []
    for d in DEGREES:
        rows.append(rng.integers(0, NUM_NBR, d) if d > 500 else rng.choice(NUM_NBR // 10, d, replace=False))
    rows.append(np.array([5, 5, 5, 7, 7, 9, 11, 5, 13, 7, 17, 19, 23, 29, 31, 37, 5, 41, 43, 47, 53, 59]))   # duplicates
    deg = [len(r) for r in rows] + [0] * pad_rows
    indptr = np.zeros(len(deg) + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate(rows).astype(np.int64)
    data = rng.permutation(len(indices)).astype(np.int64)
    return dict(indptr=indptr, indices=indices, data=data, num_rows=len(deg), num_cols=NUM_NBR)


def small_graph(seed=11):
    """A few hundred edges, no duplicate inside a row (so a row's keep flags are independent): the law tests."""
    rng = np.random.default_rng(seed)
    deg = [0, 1, 3, 5, 6, 8, 12, 20, 33, 64, 70, 90]
    rows = [rng.choice(120, d, replace=False) for d in deg]
    indptr = np.zeros(len(deg) + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate(rows).astype(np.int64)
    return dict(indptr=indptr, indices=indices, data=rng.permutation(len(indices)).astype(np.int64), num_rows=len(deg),
                num_cols=120)


def seeds_for(R, n, rng):
    """n seeds of labor_graph: the hub first, then every other real row, so that every degree class is hit when n
    allows (n = 1: the hub alone); then repeats of the rows below the hub (seeds listed twice), the last row of the graph and, from 64
    seeds on, two ids outside the graph (rows of degree 0 that touch no memory)."""
    real = len(DEGREES) + 1
    hub = DEGREES.index(max(DEGREES))
    order = np.array([hub] + [r for r in range(real) if r != hub])
    base = order[:min(n, real)]
    extra = rng.integers(0, hub, n - len(base))
    if len(extra) >= 3:
        extra[0] = R["num_rows"] - 1
    if n >= 64:
        extra[1], extra[2] = -1, R["num_rows"]
    return np.concatenate([base, extra]).astype(np.int64)


def messy_prob(nnz, rng, dtype=np.float32):
    """Weights by EDGE ID: mostly positive over three decades, some zero, negative and NaN."""
    w = np.exp(rng.uniform(-3.0, 4.0, nnz))
    kind = rng.integers(0, 20, nnz)
    w[kind == 0] = 0.0
    w[kind == 1] = -1.0
    w[kind == 2] = np.nan
    return w.astype(dtype)


# ---- the model ---------------------------------------------------------------------------------------
def variate(seed, t):
    return draw(seed, t, 0, 0)


def row_of(R, s):
    if s < 0 or s >= R["num_rows"]:
        return 0, 0
    return int(R["indptr"][s]), int(R["indptr"][s + 1])


def edge_ids(R, lo, hi, use_data):
    return R["data"][lo:hi] if use_data else np.arange(lo, hi, dtype=np.int64)


def model_scale(R, seeds, k, prob, use_data=True):
    """c per seed by an exact solve: with the positive weights sorted descending, the number m of saturated ones is the
    first m with c = (k - m) / (sum of the rest), c * w[m] < 1 (and c * w[m - 1] >= 1 by construction)."""
    out = np.zeros(len(seeds))
    for i, s in enumerate(seeds):
        lo, hi = row_of(R, int(s))
        w = usable(prob[edge_ids(R, lo, hi, use_data)])
        w = np.sort(w[w > 0])[::-1]
        with np.errstate(over="ignore"):
            W = w.sum()
        if not np.isfinite(W):
            out[i] = 0.0
        elif k < 0 or len(w) <= k:
            out[i] = np.inf
        else:
            tail = np.cumsum(w[::-1])[::-1]          # tail[m] = sum of w[m:]
            for m in range(k):
                c = (k - m) / tail[m]
                if c * w[m] < 1:
                    break
            out[i] = c
    return out


def model_pick(R, seeds, k, seed, prob=None, c=None, use_data=True):
    """(indptr, nbr, eids, importances or None) of the rule."""
    indptr, nbr, eid, imp = [0], [], [], []
    for i, s in enumerate(seeds):
        lo, hi = row_of(R, int(s))
        t = R["indices"][lo:hi]
        e = edge_ids(R, lo, hi, use_data)
        d = hi - lo
        if d == 0:
            keep = np.zeros(0, dtype=bool)
        elif prob is None:
            keep = np.ones(d, dtype=bool) if (k < 0 or d <= k) else mulhi(variate(seed, t), d) < np.uint64(k)
        else:
            w = usable(prob[e])
            with np.errstate(invalid="ignore", over="ignore"):
                p = np.minimum(1.0, c[i] * w)
                keep = (w > 0) & (c[i] > 0) & (uniform(variate(seed, t)) < p)
            a = w[keep] / p[keep]
            if keep.any():
                imp.append(a * (keep.sum() / a.sum()))
        nbr.append(t[keep])
        eid.append(e[keep])
        indptr.append(indptr[-1] + int(keep.sum()))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    return (np.array(indptr, dtype=np.int64), cat(nbr).astype(np.int64), cat(eid).astype(np.int64),
            None if prob is None else cat(imp).astype(np.float64))


# ---- the host functions ------------------------------------------------------------------------------
def tensors_of(R, idtype, use_data=True, device="cpu"):
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(idtype).to(device)
    return t_(R["indptr"]), t_(R["indices"]), (t_(R["data"]) if use_data else None)


def host_csr_of(R, idtype, use_data=True):
    from dgl_amd import _capi

    return _capi.host_csr(*tensors_of(R, idtype, use_data), R["num_cols"])


def host_pick(R, seeds, k, seed, prob=None, c=None, idtype=torch.int64, use_data=True):
    from dgl_amd import _capi

    csr = host_csr_of(R, idtype, use_data)
    s = torch.from_numpy(np.ascontiguousarray(seeds)).to(idtype)
    p = None if prob is None else torch.from_numpy(prob)
    cc = None if c is None else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64))
    return _capi.labor_pick_host(csr, s, k, seed, prob=p, c=cc)


def host_scale(R, seeds, k, prob, idtype=torch.int64, use_data=True):
    from dgl_amd import _capi

    csr = host_csr_of(R, idtype, use_data)
    s = torch.from_numpy(np.ascontiguousarray(seeds)).to(idtype)
    return _capi.labor_scale_host(csr, torch.from_numpy(prob), s, k).numpy()


def saturation_sum(R, seeds, c, prob, use_data=True):
    """sum_q min(1, c_i w'(q)) per seed, in fp64."""
    out = np.zeros(len(seeds))
    for i, s in enumerate(seeds):
        lo, hi = row_of(R, int(s))
        w = usable(prob[edge_ids(R, lo, hi, use_data)])
        out[i] = np.minimum(1.0, c[i] * w[w > 0]).sum()
    return out
