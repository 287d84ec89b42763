"""Point sets, the numpy model and the call wrappers of the point-cloud tests (tests/test_knn_host.py,
tests/test_zzzzzzzzzzz_gpu_knn.py).

The model is an independent restatement of the rule of csrc/knn_step.h written from its TEXT, not from the header:
whole-array distances in a wider type (fp64; long double for fp64 operands of the generic part), NaN as +inf, then a
stable sort by distance (stable over ascending ids = the key (d, id)).  Farthest points follow the three numbered
steps of the rule."""
import numpy as np
import torch

QUERY_TILE, DATA_TILE = 64, 32     # the kernel's tiles (pinned against dgla_knn_tile_sizes by test_knn_host.py)
MAX_K = 64                         # kKnnMaxK
FPS_LDS_ROWS = 4096                # farthest points: mind lives in LDS up to here

TORCH = {np.float32: torch.float32, np.float64: torch.float64}


# ---- point sets ----------------------------------------------------------------------------------------
def lattice(rng, n, D):
    """Multiples of 1/4 in [-4, 4]: every difference, square and sum of up to 257 squares is exact in fp32."""
    return rng.integers(-16, 17, (n, D)).astype(np.float64) / 4.0


def _case(name, D, k, x_segs, y_segs=None, x=None, y=None, seed=0):
    rng = np.random.default_rng(seed + 1000 * D + k)
    if x is None:
        x = lattice(rng, sum(x_segs), D)
    if y_segs is not None and y is None:
        y = lattice(rng, sum(y_segs), D)
    return dict(name=name, D=D, k=k, x_segs=list(x_segs), y_segs=None if y_segs is None else list(y_segs), x=x, y=y)


def exact_cases():
    """Lattice inputs: host == model for ids AND distance bits, whatever the order of accumulation."""
    Q, T = QUERY_TILE, DATA_TILE
    cases = [
        # segment lengths 1, k, k + 1, one below / at / above the data tile and the query tile, twice a tile plus one
        _case("ladder_k1_d3", 3, 1, [1, 2, T - 1, T, T + 1, Q - 1, Q, Q + 1, 2 * Q + 1]),
        _case("ladder_k2_d4", 4, 2, [2, 3, T + 1, Q, 2 * T + 1]),
        _case("ladder_k20_d1", 1, 20, [20, 21, Q + 1]),
        # x != y, unequal segments, an empty query segment, an empty data segment, a data segment shorter than k
        _case("xy_k20_d5", 5, 20, [20, 21, 7, Q, 0, 40], [5, 0, 3, Q + 1, 2, 1]),
        _case("kmax_d1", 1, MAX_K, [MAX_K, MAX_K + 1, 2 * Q + 1]),
        _case("kmax_d3_xy", 3, MAX_K, [MAX_K + 5, 2 * MAX_K], [Q + 1, 3]),
        _case("wide_d64", 64, 20, [70, 33], [Q + 1, 10]),
        _case("wider_d257", 257, 2, [40, 3], [17, 2]),
    ]
    # all points coincident: the ids in ascending order
    cases.append(_case("coincident", 3, 20, [100], x=np.full((100, 3), 1.25)))
    # duplicates on both sides of a data-tile boundary (the nearest rows of their own point, at distance 0)
    x = lattice(np.random.default_rng(7), 70, 3)
    x[T - 2:T + 2] = [0.5, -1.0, 2.0]
    x[2 * T - 1:2 * T + 1] = [0.5, -1.0, 2.0]
    cases.append(_case("dup_tile_boundary", 3, 5, [70], x=x))
    cases.append(_case("dup_tile_boundary_xy", 3, 6, [70], [2], x=x, y=np.array([[0.5, -1.0, 2.0], [0.5, -1.0, 2.25]])))
    return cases


def generic_cases():
    """randn inputs: distances within the bound of a chain of D fused steps, no closer point left out."""
    out = []
    for D, segs in ((3, [150, 40]), (64, [130]), (257, [70])):
        rng = np.random.default_rng(50 + D)
        out.append(dict(name="randn_d%d" % D, D=D, k=8, x_segs=segs, y_segs=None, x=rng.standard_normal((sum(segs), D)),
                        y=None))
    rng = np.random.default_rng(99)
    out.append(dict(name="randn_xy_d5", D=5, k=4, x_segs=[200, 90], y_segs=[70, 33], x=rng.standard_normal((290, 5)),
                    y=rng.standard_normal((103, 5))))
    return out


def special_case():
    """NaN and +-inf coordinates among lattice points (x != y): a NaN distance orders as +inf, behind every finite one,
    by ascending id."""
    rng = np.random.default_rng(3)
    x, y = lattice(rng, 40, 3), lattice(rng, 6, 3)
    x[3, 1] = np.nan
    x[9] = np.inf
    x[17, 0] = -np.inf
    x[33, 2] = np.nan
    y[1, 0] = np.nan          # every distance NaN: the ids in ascending order
    y[2] = np.inf             # inf - inf = NaN against row 9, +inf against the rest
    y[4, 0] = -np.inf
    return dict(name="nan_inf", D=3, k=38, x_segs=[40], y_segs=[6], x=x, y=y)


def offsets(segs):
    return [0] + [int(v) for v in np.cumsum(segs)]


# ---- the model -----------------------------------------------------------------------------------------
def model_knn(case, dtype, wide=np.float64):
    """(ids [2, k * ny] int64, dist [k * ny] in `wide`) of the rule for the operands rounded to `dtype`."""
    x = case["x"].astype(dtype).astype(wide)
    y = x if case["y"] is None else case["y"].astype(dtype).astype(wide)
    xo = offsets(case["x_segs"])
    yo = xo if case["y_segs"] is None else offsets(case["y_segs"])
    k, ny = case["k"], y.shape[0]
    ids = np.full((2, ny * k), -1, dtype=np.int64)
    dist = np.full(ny * k, np.inf, dtype=wide)
    for s in range(len(xo) - 1):
        seg = x[xo[s]:xo[s + 1]]
        for q in range(yo[s], yo[s + 1]):
            with np.errstate(invalid="ignore", over="ignore"):
                t = y[q][None, :] - seg
                d = (t * t).sum(axis=1)
            d[np.isnan(d)] = np.inf
            order = np.argsort(d, kind="stable")[:k]
            ids[0, q * k:(q + 1) * k] = q
            ids[1, q * k:q * k + len(order)] = xo[s] + order
            dist[q * k:q * k + len(order)] = d[order]
    return ids, dist


def model_distances(case, dtype, wide):
    """All distances of a single-segment view: d[q][i] in `wide`, per segment as a list of (q0, x0, matrix)."""
    x = case["x"].astype(dtype).astype(wide)
    y = x if case["y"] is None else case["y"].astype(dtype).astype(wide)
    xo = offsets(case["x_segs"])
    yo = xo if case["y_segs"] is None else offsets(case["y_segs"])
    out = []
    for s in range(len(xo) - 1):
        t = y[yo[s]:yo[s + 1], None, :] - x[None, xo[s]:xo[s + 1], :]
        out.append((yo[s], xo[s], (t * t).sum(axis=2)))
    return out


def model_fps(pos, npoints, start):
    """(B, npoints) of the rule; pos (B, N, D) in fp64."""
    B, N, _ = pos.shape
    out = np.zeros((B, npoints), dtype=np.int64)
    for b in range(B):
        mind = np.full(N, np.inf)
        cur = int(start[b])
        out[b, 0] = cur
        for t in range(1, npoints):
            with np.errstate(invalid="ignore", over="ignore"):
                d = ((pos[b] - pos[b, cur]) ** 2).sum(axis=1)
            lower = d < mind                     # (a NaN distance lowers nothing)
            mind[lower] = d[lower]
            mind[cur] = -1.0
            cur = int(np.argmax(mind))           # the first of the largest
            out[b, t] = cur
    return out


# ---- the entry points ----------------------------------------------------------------------------------
def run_knn(case, dtype, idtype, device=None):
    """(ids, dist) of dgla_knn_host (device None) or dgla_knn, as numpy."""
    from dgl_amd import _capi

    t_ = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a.astype(dtype)))
    x, y = t_(case["x"]), t_(case["y"])
    xo = offsets(case["x_segs"])
    yo = None if case["y_segs"] is None else offsets(case["y_segs"])
    if device is None:
        ids, dist = _capi.knn_host(x, xo, case["k"], y, yo, idtype=idtype, with_dist=True)
    else:
        ids, dist = _capi.knn(x.to(device), xo, case["k"], None if y is None else y.to(device), yo, idtype=idtype,
                              with_dist=True)
    return ids.cpu().numpy(), dist.cpu().numpy()


def fps_clouds():
    """name -> (pos (B, N, D) fp64 lattice, starts to try)."""
    rng = np.random.default_rng(21)
    square = np.array([[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.5, 0.5]]])
    return {
        "lattice_b3_n50": (lattice(rng, 150, 3).reshape(3, 50, 3), [0, 17, 49]),
        "lattice_n300_d5": (lattice(rng, 300, 5).reshape(1, 300, 5), [0, 299]),      # more rows than threads
        "coincident": (np.full((2, 9, 3), -0.75), list(range(9))),
        "square": (square, list(range(5))),
        "nan_rows": (_with_nan(lattice(rng, 24, 3).reshape(2, 12, 3)), [0, 4, 11]),
    }


def _with_nan(pos):
    pos[0, 4, 1] = np.nan
    pos[0, 9, 0] = np.nan
    pos[1, 0, 2] = np.nan
    return pos


def run_fps(pos, npoints, start, dtype, device=None):
    from dgl_amd import _capi

    p = torch.from_numpy(np.ascontiguousarray(pos.astype(dtype)))
    s = torch.as_tensor(np.asarray(start, dtype=np.int64))
    if device is None:
        return _capi.fps_host(p, npoints, s).numpy()
    return _capi.fps(p.to(device), npoints, s.to(device)).cpu().numpy()
