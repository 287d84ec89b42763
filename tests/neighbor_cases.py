"""Graphs, the Python model and the call wrappers of the neighbour-sampling and block-building tests
(tests/test_neighbor_model.py, tests/test_zzzzzzzzzzzz_gpu_neighbor.py).

The model is an independent restatement of the rule that include/dgl_amd.h quotes beside dgla_sample_neighbors,
dgla_sample_neighbors_weighted and dgla_to_block, written from that TEXT: Python integers for the generator and for
Floyd's subset rule, math.log and one fp64 division for the exponential-clock keys followed by a plain sort, a running
fp64 sum and a bisection for the picks with replacement, numpy set operations for the block.  Nothing here walks a row
in chunks of 64 or lane by lane; the `bug=` forms are deliberate defects of the model (what a wrong kernel would
compute), used by tests/test_neighbor_model.py to show that the committed cases tell them apart."""
import bisect
import functools
import math
from fractions import Fraction

import numpy as np
import torch

from tests.test_random_walk_host import mix64 as mix64_np

M64 = (1 << 64) - 1
U64 = np.uint64
MAX_FANOUT = 128                    # kMaxFanout
CLOCK_STRIDE = 0x5851F42D4C957F2D   # key of position j: walk_key + CLOCK_STRIDE * (j + 1)
SLOT_STRIDE = 0x2545F4914F6CDD1D    # target of slot t:  walk_key + SLOT_STRIDE * (t + 1)
NP_I = {torch.int32: np.int32, torch.int64: np.int64}


# ---- the generator (csrc/random_walk_step.h), on Python integers ----------------------------------------
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def walk_key(seed, i):
    return mix64((seed & M64) ^ ((i * 0xD1B54A32D192ED03) & M64))


def step_key(wk, t):
    return mix64((wk + t) & M64)


def index(r, n):
    return (r * n) >> 64


# ---- the uniform rule ----------------------------------------------------------------------------------
def uniform_positions(S, r, deg, fanout, replace, bug=None):
    """Positions inside the row of node `r`, slot by slot; None = the whole row in order."""
    if fanout < 0 or (not replace and deg <= fanout):
        return None
    if deg == 0:
        return []
    wk = walk_key(S, r)
    shift = 1 if bug == "slot_plus_one" else 0
    if replace:
        return [index(step_key(wk, k + shift), deg) for k in range(fanout)]
    out, held = [], set()
    for m in range(fanout):
        j = deg - fanout + m
        t = index(step_key(wk, m + shift), j + 1)
        if t in held:
            t = j - 1 if bug == "floyd_j_minus_one" else j
        held.add(t)
        out.append(t)
    return out


def model_uniform(G, seeds, fanout, replace, S, bug=None):
    """(out_indptr, global CSR positions of the slots), int64."""
    indptr = [0]
    gpos = []
    for i, r in enumerate(seeds):
        r = int(r)
        start, deg = int(G["indptr"][r]), int(G["indptr"][r + 1] - G["indptr"][r])
        pos = uniform_positions(S, i if bug == "key_by_seed_position" else r, deg, fanout, replace, bug)
        pos = np.arange(deg, dtype=np.int64) if pos is None else np.asarray(pos, dtype=np.int64)
        gpos.append(start + pos)
        indptr.append(indptr[-1] + len(pos))
    return np.asarray(indptr, dtype=np.int64), (np.concatenate(gpos) if gpos else np.zeros(0, dtype=np.int64))


def gather(G, gpos, use_eids):
    """(src, eids) of the slots at the global positions `gpos`."""
    return G["indices"][gpos], (G["eids"][gpos] if use_eids else gpos.copy())


# ---- the weighted rules --------------------------------------------------------------------------------
def row_weights(G, prob, r, use_eids, bug=None):
    """The weights of row r by POSITION, in prob's own type (prob is indexed by edge id)."""
    start, end = int(G["indptr"][r]), int(G["indptr"][r + 1])
    if use_eids and bug != "prob_by_position":
        return prob[G["eids"][start:end]]
    return prob[start:end]


def positive_positions(w):
    with np.errstate(invalid="ignore"):
        return [int(j) for j in np.nonzero(w > 0)[0]]      # NaN, negatives and +-0 are not positive


def clock_keys(S, r, w, pos):
    """key_j = -ln(u_j) / (double) w_j of the positive positions `pos`, in fp64 with math.log."""
    if not pos:
        return []
    wk = walk_key(S, r)
    with np.errstate(over="ignore"):
        rr = mix64_np(U64(wk) + U64(CLOCK_STRIDE) * (np.asarray(pos, dtype=U64) + U64(1)))
    u = ((rr >> U64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    return [-math.log(a) / float(w[j]) for a, j in zip(u.tolist(), pos)]


def clock_order(S, r, w, bug=None):
    """Every positive position of the row in ascending (key, position): slot t of any fanout is entry t.
    Also the sorted keys."""
    pos = positive_positions(w)
    if bug == "scan_stops_at_64":
        pos = [j for j in pos if j < 64]
    keys = clock_keys(S, r, w, pos)
    tie = -1 if bug == "ties_descending" else 1
    order = sorted(range(len(pos)), key=lambda q: (keys[q], tie * pos[q]))
    return [pos[q] for q in order], [keys[q] for q in order]


def slot_target(S, r, t, total):
    rr = mix64((walk_key(S, r) + SLOT_STRIDE * (t + 1)) & M64)
    return (float(rr >> 11) + 0.5) * 2.0 ** -53 * total


def replace_picks(S, r, w, fanout, bug=None):
    """Slots with replacement: the first positive position whose inclusive prefix reaches the slot's target."""
    pos = positive_positions(w)
    if not pos:
        return []
    prefix, total = [], 0.0
    for j in pos:
        total += float(w[j])
        prefix.append(total)
    out = []
    for t in range(fanout):
        target = slot_target(S, r, t, total)
        if bug == "no_chunk_carry":      # a prefix that restarts at every 64-position boundary past the first
            q = next((q for q, j in enumerate(pos)
                      if prefix[q] - (_before(prefix, pos, j - j % 64) if j >= 64 else 0.0) >= target), len(pos))
        else:
            q = bisect.bisect_left(prefix, target)
        out.append(pos[min(q, len(pos) - 1)])
    return out


def _before(prefix, pos, boundary):
    q = bisect.bisect_left(pos, boundary)
    return prefix[q - 1] if q else 0.0


def model_weighted(G, prob, seeds, fanout, replace, S, use_eids, bug=None, order_cache=None):
    """(out_indptr, global positions).  order_cache: dict shared between fanouts (the clock order of a row does not
    depend on the fanout)."""
    indptr, gpos = [0], []
    for i, r in enumerate(seeds):
        r = int(r)
        start = int(G["indptr"][r])
        w = row_weights(G, prob, r, use_eids, bug)
        if replace:
            pos = replace_picks(S, r, w, fanout, bug)
        else:
            if order_cache is not None and r in order_cache:
                order = order_cache[r]
            else:
                order = clock_order(S, r, w, bug)[0]
                if order_cache is not None:
                    order_cache[r] = order
            count = min(fanout, len(positive_positions(w)))
            pos = (order + [0] * count)[:count]           # (only a defective scan leaves slots unfilled)
        gpos.append(start + np.asarray(pos, dtype=np.int64))
        indptr.append(indptr[-1] + len(pos))
    return np.asarray(indptr, dtype=np.int64), (np.concatenate(gpos) if gpos else np.zeros(0, dtype=np.int64))


def exact_prefix(w, pos):
    """The exact inclusive prefix sums of the positive weights, each rounded once (what math.fsum of the head gives)."""
    out, acc = [], Fraction(0)
    for j in pos:
        acc += Fraction(float(w[j]))
        out.append(float(acc))
    return out


def min_key_gap(S, r, w, picks):
    """Smallest relative difference of adjacent keys among the first picks + 1 of the row (inf: fewer than two)."""
    keys = clock_order(S, r, w)[1][:picks + 1]
    gaps = [(b - a) / b for a, b in zip(keys, keys[1:])]
    return min(gaps) if gaps else math.inf


# ---- the block rule ------------------------------------------------------------------------------------
def model_block(seeds, src, bug=None):
    """(local_src, src_nodes) of the rule; num_src = len(src_nodes)."""
    seeds, src = np.asarray(seeds, dtype=np.int64), np.asarray(src, dtype=np.int64)
    new = np.setdiff1d(src, seeds)                       # ascending, each once
    if bug == "first_appearance":
        rest = src[~np.isin(src, seeds)]
        _, first = np.unique(rest, return_index=True)
        new = rest[np.sort(first)]
    src_nodes = np.concatenate([seeds, new])
    local = np.full(int(src_nodes.max()) + 1 if len(src_nodes) else 1, -1, dtype=np.int64)
    local[new] = len(seeds) + np.arange(len(new))
    if bug == "rank_off_from_16384":                      # new nodes whose run starts at element >= 16 384 of sorted src
        late = np.searchsorted(np.sort(src), new, side="left") >= 16384
        local[new[late]] += 1
    local[seeds] = np.arange(len(seeds))
    return local[src], src_nodes


# ---- graphs --------------------------------------------------------------------------------------------
def _csr(rows, num_cols, rng):
    deg = [len(r) for r in rows]
    indptr = np.zeros(len(deg) + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, dtype=np.int64)
    return dict(indptr=indptr, indices=indices, eids=rng.permutation(len(indices)).astype(np.int64),
                num_rows=len(deg), num_cols=num_cols)


FANOUTS = [1, 2, 15, 16, 17, 32, 33, 64, 127, 128]   # 16|17, 32|33: the position-array dispatch; 128: kMaxFanout
CALL_SEEDS = [0, 42, 2 ** 64 - 1]
UNIFORM_COLS = 100003


def ladder(f):
    return [0, 1, f - 1, f, f + 1, 2 * f, 2 * f + 1, 1000, 100000]


@functools.lru_cache(maxsize=None)
def uniform_graph(f):
    """One row of every ladder length for fanout f (deg = f + 1: Floyd's last step draws from the whole row), then 200
    short rows around f; neighbour ids distinct within a row."""
    rng = np.random.default_rng(1000 + f)
    short = ladder(f)[:7]
    lens = ladder(f) + [short[k] for k in rng.integers(0, 7, 120)] + [int(v) for v in rng.integers(0, 3 * f + 3, 80)]
    lens = [lens[k] for k in rng.permutation(len(lens))]
    return _csr([rng.choice(UNIFORM_COLS, L, replace=False) for L in lens], UNIFORM_COLS, rng)


@functools.lru_cache(maxsize=None)
def uniform_seeds(f):
    """Every row in a shuffled order with one node listed twice, and a permutation of that list."""
    G = uniform_graph(f)
    rng = np.random.default_rng(2000 + f)
    seeds = rng.permutation(G["num_rows"]).astype(np.int64)
    long_row = int(np.argmax(np.diff(G["indptr"])))
    seeds = np.insert(seeds, len(seeds) // 2, long_row)            # the 100 000-edge node twice
    perm = rng.permutation(len(seeds))
    return seeds, perm


@functools.lru_cache(maxsize=None)
def expected_uniform(f, fanout, replace, S):
    return model_uniform(uniform_graph(f), uniform_seeds(f)[0], fanout, replace, S)


def uniform_modes(f):
    return [(f, False), (f, True), (-1, False)]


W_LENGTHS = [0, 1, 5, 63, 64, 65, 127, 128, 129, 200, 1000]
W_FANOUTS = [1, 7, 64, 128]
W_SEEDS = [42, 2 ** 64 - 1]
W_COLS = 1009
W_COPIES = 3


def dyadic_row(rng, L):
    """Multiples of 1/8 in [0, 8], about 30 % zero, the last three positions zero: every partial sum is exact."""
    w = rng.integers(1, 65, L) / 8.0
    w[rng.random(L) < 0.3] = 0.0
    if L >= 5:
        w[0] = max(w[0], 0.125)
        w[-3:] = 0.0
    return w


def generic_row(rng, L):
    w = rng.random(L)
    w[rng.random(L) < 0.3] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def weighted_graph(kind):
    """(graph, weights by POSITION in fp64).  kind: "dyadic" or "generic"."""
    rng = np.random.default_rng({"dyadic": 31, "generic": 32}[kind])
    lens = [L for L in W_LENGTHS for _ in range(W_COPIES)]
    make = dyadic_row if kind == "dyadic" else generic_row
    ws = [make(rng, L) for L in lens]
    if kind == "dyadic":
        ws.append(np.zeros(70))                       # all zero
        one = np.zeros(100)
        one[64] = 2.5                                 # a single positive edge, the first of the second chunk
        ws.append(one)
    G = _csr([rng.choice(W_COLS, len(w), replace=False) for w in ws], W_COLS, rng)
    return G, np.concatenate(ws)


def special_graph(dtype, twin_inf=False):
    """One row of 90 lattice weights with the special values among them; twin_inf adds a second +inf (equal keys)."""
    rng = np.random.default_rng(33)
    w = (rng.integers(1, 65, 90) / 8.0).astype(dtype)
    fi = np.finfo(dtype)
    w[3], w[66] = np.nan, -1.0
    w[11], w[12], w[40] = -0.0, 0.0, 0.0
    w[70] = np.inf
    w[25], w[68] = fi.smallest_subnormal, fi.max      # (one largest value: two of them would sum to +inf in fp64)
    if twin_inf:
        w[20] = np.inf
    G = _csr([rng.choice(W_COLS, 90, replace=False)], W_COLS, rng)
    return G, w


SPECIAL_NEVER = [3, 66, 11, 12, 40]
SPECIAL_INF = 70


def prob_by_eid(G, w_pos, use_eids, dtype):
    """The weights of the positions as the `prob` array of the call: indexed by edge id."""
    w = w_pos.astype(dtype)
    if not use_eids:
        return w
    prob = np.empty_like(w)
    prob[G["eids"]] = w
    return prob


def weighted_seeds(G):
    rng = np.random.default_rng(4000 + G["num_rows"])
    seeds = rng.permutation(G["num_rows"]).astype(np.int64)
    return np.insert(seeds, 5, int(np.argmax(np.diff(G["indptr"]))))     # a 1000-edge node twice


_ORDERS = {}


def expected_weighted(kind, dtype, fanout, replace, S):
    """Global positions of the model; they do not depend on the id width or on the edge-id map, since `prob` is built
    from the weights by position."""
    key = (kind, dtype, fanout, replace, S)
    if key not in _ORDERS:
        G, w_pos = weighted_graph(kind)
        cache = _ORDERS.setdefault(("order", kind, dtype, S), {})
        _ORDERS[key] = model_weighted(G, w_pos.astype(dtype), weighted_seeds(G), fanout, replace, S, use_eids=False,
                                      order_cache=cache)
    return _ORDERS[key]


B_NNZ = [0, 1, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 32767, 32768, 40000]
B_NODES = [50, 5000, 2 ** 20 + 3]         # heavy duplication, ordinary, sparse
B_SEEDS = [1, 300]


def block_case(nnz, num_nodes, num_seeds, kind="random"):
    """(seeds, src).  Seeds are distinct, so a graph of 50 nodes gets 40 of them where 300 are asked for.  kind:
    "random" (ids 0 and num_nodes - 1 present from two edges on), "all_seeds", "disjoint"."""
    rng = np.random.default_rng(nnz * 7 + num_nodes * 13 + num_seeds)
    ns = min(num_seeds, num_nodes - 10)
    seeds = rng.choice(num_nodes, ns, replace=False).astype(np.int64)
    if kind == "all_seeds":
        src = seeds[rng.integers(0, ns, nnz)]
    elif kind == "disjoint":
        others = np.setdiff1d(np.arange(num_nodes), seeds)
        src = others[rng.integers(0, len(others), nnz)]
    else:
        src = rng.integers(0, num_nodes, nnz).astype(np.int64)
        if nnz >= 2:
            a, b = rng.choice(nnz, 2, replace=False)
            src[a], src[b] = 0, num_nodes - 1
    return seeds, src.astype(np.int64)


def block_cases(num_nodes):
    """(name, seeds, src) of every block case of a node count."""
    out = [("nnz%d_seeds%d" % (nnz, ns), *block_case(nnz, num_nodes, ns)) for nnz in B_NNZ for ns in B_SEEDS]
    for kind in ("all_seeds", "disjoint"):
        out.append((kind, *block_case(1025, num_nodes, 300, kind)))
    return out


# ---- the entry points ----------------------------------------------------------------------------------
def device_csr(G, idtype, use_eids, dev):
    from dgl_amd import _capi

    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(idtype).to(dev)
    return _capi.make_csr(t_(G["indptr"]), t_(G["indices"]), t_(G["eids"]) if use_eids else None, G["num_cols"])


def _trim(indptr, src, eids):
    indptr = indptr.cpu().numpy()
    total = int(indptr[-1])
    return indptr, src[:total].cpu().numpy(), eids[:total].cpu().numpy()


def run_uniform(csr, seeds, fanout, replace, S, idtype, dev):
    """(out_indptr, src[:total], eids[:total]) of dgla_sample_neighbors as numpy arrays of the id type."""
    from dgl_amd import _capi

    s = torch.from_numpy(np.ascontiguousarray(seeds)).to(idtype).to(dev)
    return _trim(*_capi.sample_neighbors(csr, s, fanout, replace=replace, rng_seed=S))


def run_weighted(csr, prob, seeds, fanout, replace, S, idtype, dev):
    from dgl_amd import _capi

    s = torch.from_numpy(np.ascontiguousarray(seeds)).to(idtype).to(dev)
    p = torch.from_numpy(np.ascontiguousarray(prob)).to(dev)
    return _trim(*_capi.sample_neighbors_weighted(csr, p, s, fanout, replace=replace, rng_seed=S))


def run_block(seeds, src, node_map, idtype, dev, padded):
    """(local_src, src_nodes[:num_src], num_src): through to_block (key width from the node count), or through
    to_block_padded without a node count (keys of the full 31 / 63 bits)."""
    from dgl_amd import _capi

    s = torch.from_numpy(np.ascontiguousarray(seeds)).to(idtype).to(dev)
    e = torch.from_numpy(np.ascontiguousarray(src)).to(idtype).to(dev)
    if padded:
        local, nodes, num = _capi.to_block_padded(s, None, e, node_map, fill=0, num_nodes=0)
        k = int(num.item())
        nodes = nodes[:k]
    else:
        local, nodes, k = _capi.to_block(s, e, node_map)
    return local.cpu().numpy(), nodes.cpu().numpy(), k
