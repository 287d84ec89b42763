"""Shared by the neighbour-matching tests: an independent numpy model of the rule of include/dgl_amd.h "Graph matching"
(written from the header's text, whole rounds at a time over the entry list, not from csrc/matching_step.h) and the table
of bi-directed graphs the host and device tests run."""
import numpy as np

M64 = (1 << 64) - 1
BLUE_T = int(0.53406 * 2.0 ** 64)          # floor(0.53406 * 2^64)
HASH_SALT = 0x6D61746368696E67
WALK_MUL = 0xD1B54A32D192ED03
NONE, SINGLE = -1, -2
SEEDS = (0, 1, 0xDEADBEEFCAFEF00D)
FORMS = ("none", "f32", "f64", "ones", "special")


def mix64(z):
    """splitmix64 finaliser with its increment, on uint64 arrays (arithmetic mod 2^64)."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def colours(seed, n, t):
    """BLUE flags of nodes 0 .. n - 1 in round t."""
    v = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        walk = mix64(np.uint64(seed & M64) ^ (v * np.uint64(WALK_MUL)))
        return mix64(mix64(walk + np.uint64(t)) + np.uint64(0)) < np.uint64(BLUE_T)


def edge_hash(seed, u, v):
    a, b = np.minimum(u, v).astype(np.uint64), np.maximum(u, v).astype(np.uint64)
    with np.errstate(over="ignore"):
        return mix64(mix64(np.uint64((seed ^ HASH_SALT) & M64) ^ (a * np.uint64(WALK_MUL))) + b)


def _best_per_row(rows, cols, w, h, sel, n):
    """best[u] = the column of the selected entry of row u with the largest (w, h), the smaller column on a full tie;
    -1 for a row with no selected entry."""
    idx = np.flatnonzero(sel)
    best = np.full(n, -1, dtype=np.int64)
    if idx.size:
        order = idx[np.lexsort((cols[idx], ~h[idx], -w[idx], rows[idx]))]
        first = np.ones(order.size, dtype=bool)
        first[1:] = rows[order][1:] != rows[order][:-1]
        best[rows[order][first]] = cols[order][first]
    return best


def model(indptr, indices, data, weight, seed, max_rounds=256, trace=None):
    """(label, rounds) of the rule; raises RuntimeError at the round cap.  `trace` (a list) receives per round
    ``dict(active, blue, prop, picks)`` with `picks` the {RED u: v} pairs of the round."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n = indptr.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    cols = indices
    eid = np.arange(cols.size, dtype=np.int64) if data is None else np.asarray(data, dtype=np.int64)
    if weight is None:
        w = np.zeros(cols.size)
    else:
        x = np.asarray(weight, dtype=np.float64)[eid]
        w = np.where(x > 0, x, 0.0)                       # negative and NaN count as 0
    valid = (cols != rows) & (cols >= 0) & (cols < n)
    safe = np.where(valid, cols, 0)
    h = edge_hash(seed, rows, safe)
    label = np.full(n, -1, dtype=np.int64)
    prop = np.full(n, NONE, dtype=np.int64)
    t = 0
    while True:
        active = label < 0
        if not active.any():
            return label, t
        if t == max_rounds:
            raise RuntimeError("round cap")
        blue = colours(seed, n, t)
        live = valid & active[rows] & active[safe]        # entries between two active nodes
        has_nb = np.bincount(rows[live], minlength=n) > 0
        best = _best_per_row(rows, safe, w, h, live & blue[rows] & ~blue[safe], n)
        new = np.where(~has_nb, SINGLE, np.where(blue & (best >= 0), best, NONE))
        prop = np.where(active, new, prop)
        # respond
        label[active & (prop == SINGLE)] = np.flatnonzero(active & (prop == SINGLE))
        offered = live & ~blue[rows] & blue[safe] & (prop[safe] == rows)
        pick = _best_per_row(rows, safe, w, h, offered, n)
        us = np.flatnonzero(pick >= 0)
        vs = pick[us]
        assert np.unique(vs).size == vs.size               # a BLUE node proposed to one node only
        label[us] = label[vs] = np.minimum(us, vs)
        if trace is not None:
            trace.append(dict(active=active, blue=blue, prop=prop.copy(), picks=dict(zip(us.tolist(), vs.tolist()))))
        t += 1


# ---- graphs -----------------------------------------------------------------------------------------
def csr_of(n, src, dst, shuffle_seed=None):
    """CSR of the entry list (src[i] -> dst[i]), edge i keeping id i.  With `shuffle_seed` the entries of a row stand in a
    random order and `data` maps positions to edge ids; without it they stand in list order and `data` is None when the
    list is already sorted by source."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    ids = np.arange(src.size)
    if shuffle_seed is not None:
        ids = np.random.default_rng(shuffle_seed).permutation(src.size)
    order = ids[np.argsort(src[ids], kind="stable")]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=indptr[1:])
    data = None if np.array_equal(order, np.arange(src.size)) else order
    return dict(n=n, indptr=indptr, indices=dst[order], data=data, nnz=int(src.size))


def both_ways(pairs):
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([a[:, 0], a[:, 1]]), np.concatenate([a[:, 1], a[:, 0]])


def path_pairs(n, start=0):
    return [(start + i, start + i + 1) for i in range(n - 1)]


def grid_pairs(r, c):
    at = lambda i, j: i * c + j
    return [(at(i, j), at(i, j + 1)) for i in range(r) for j in range(c - 1)] + \
           [(at(i, j), at(i + 1, j)) for i in range(r - 1) for j in range(c)]


def random_pairs(n, m, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = a != b
    return sorted(set(zip(np.minimum(a, b)[keep].tolist(), np.maximum(a, b)[keep].tolist())))


def _degree_pairs():
    """hubs of degree 1, 15, 16, 17, 63, 64, 65 (each over fresh leaves of degree 1) and node 0 of degree 0"""
    pairs, nxt = [], 1
    for d in (1, 15, 16, 17, 63, 64, 65):
        hub = nxt
        pairs += [(hub, hub + 1 + i) for i in range(d)]
        nxt = hub + d + 1
    return nxt, pairs


def _case(name, n, pairs, shuffle=None, extra=None, plain=False):
    src, dst = both_ways(pairs)
    if extra is not None:                                   # further directed entries (self-loops)
        src, dst = np.concatenate([src, extra[0]]), np.concatenate([dst, extra[1]])
    if plain:                                               # edge id == position: the CSR has no `data`
        order = np.argsort(src, kind="stable")
        src, dst = src[order], dst[order]
    c = csr_of(n, src, dst, shuffle)
    c["name"] = name
    return c


def cases():
    out = [
        _case("path3", 3, path_pairs(3), plain=True),
        _case("path257", 257, path_pairs(257), shuffle=1),
        _case("star300", 301, [(0, i) for i in range(1, 301)], shuffle=2),
        _case("grid16x16", 256, grid_pairs(16, 16), shuffle=3),
        _case("clique70", 70, [(i, j) for i in range(70) for j in range(i + 1, 70)], plain=True),
        _case("components", 18, path_pairs(5) + [(7 + i, 7 + (i + 1) % 6) for i in range(6)], shuffle=4),
    ]
    n, pairs = _degree_pairs()
    out.append(_case("degrees", n, pairs, shuffle=5))
    multi = path_pairs(10) * 2 + [(3, 4), (0, 9), (0, 9)]
    out.append(_case("multigraph", 10, multi, shuffle=6))
    loops = np.array([0, 3, 3, 6, 9, 12, 25], dtype=np.int64)      # node 25 has a self-loop and nothing else
    out.append(_case("selfloops", 26, grid_pairs(5, 5), shuffle=7, extra=(loops, loops)))
    for n in (255, 256, 257):
        out.append(_case("random%d" % n, n, random_pairs(n, 3 * n, n), shuffle=n))
    return out


def weights(case, form):
    """One weight per EDGE ID (None for the unweighted form); symmetric forms where both directions must agree are built
    by the tests themselves."""
    m = case["nnz"]
    rng = np.random.default_rng(m + len(form))
    if form == "none":
        return None
    if form == "f32":
        return rng.random(m, dtype=np.float32)
    if form == "f64":
        return rng.random(m)
    if form == "ones":
        return np.ones(m, dtype=np.float32)
    assert form == "special"
    w = rng.integers(1, 4, m).astype(np.float64)                      # many ties
    for i, v in enumerate((0.0, -1.0, np.nan, np.inf)):
        w[i::7][: max(1, m // 14)] = v
    return w


def entry_set(case):
    rows = np.repeat(np.arange(case["n"]), np.diff(case["indptr"]))
    return set(zip(rows.tolist(), case["indices"].tolist()))


def check_properties(case, label):
    """The five consequences of the rule that the header states (the first, purity, is the equality with the model)."""
    label = np.asarray(label, dtype=np.int64)
    n = case["n"]
    assert label.shape == (n,) and (label >= 0).all() and (label < n).all()
    assert np.array_equal(label[label], label) and (label <= np.arange(n)).all()
    sizes = np.bincount(label, minlength=n)
    assert sizes.max(initial=0) <= 2
    entries = entry_set(case)
    for i in np.flatnonzero(label != np.arange(n)):
        assert (int(i), int(label[i])) in entries or (int(label[i]), int(i)) in entries
    single = sizes[label] == 1
    for u, v in entries:                                              # (every case of the table is symmetric)
        assert u == v or not (single[u] and single[v]), (u, v)
