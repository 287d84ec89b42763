"""Shared by the tag-sort / biased-sampling tests: the table of graphs, tags and sampler calls that the host and device
tests run, and an independent Python model.

The sort model is Python's stable ``sorted(range(deg), key=tag)`` per row; the sampler model is the counting rule (how
many picks a seed yields) in plain Python.  Neither builds a histogram, a cursor or a scan, so they cannot share a
mistake with csrc/biased_step.h."""
import numpy as np

# every unit class and chunk boundary of the sort: 16 / 64 / 256 lanes, and one hub for the workgroup pass
LADDER = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 3000)
TAGS = (1, 2, 3, 16, 17, 64, 65, 256)          # 256 is the first T whose T + 1 counters no longer fit in LDS
PATTERNS = ("equal", "alternating", "descending", "empty-tags", "random")
FANOUTS = (0, 1, 2, 16, 17, 64, 65, -1, 3500)  # 3500 exceeds every degree
BIASES = ("zero-tag", "all-zero", "nan", "dominant", "uniform")


# ---- the model --------------------------------------------------------------------------------------
def sort_model(case):
    """(indices, data, tag_pos) of the sorted CSR, as lists."""
    T = case["T"]
    indices, data, tag_pos = [], [], []
    for r in range(case["n"]):
        lo, hi = int(case["indptr"][r]), int(case["indptr"][r + 1])
        eid = [q if case["data"] is None else int(case["data"][q]) for q in range(lo, hi)]
        tags = [int(case["tag"][e]) for e in eid]
        order = sorted(range(hi - lo), key=lambda k: tags[k])
        indices += [int(case["indices"][lo + k]) for k in order]
        data += [eid[k] for k in order]
        tag_pos.append([sum(1 for t in tags if t < j) for j in range(T + 1)])
    return indices, data, tag_pos


def positive(bias):
    return [bool(b > 0) and np.isfinite(b) for b in bias]       # NaN > 0 is False


def picks_model(tag_pos_row, bias, fanout, replace):
    P = sum(tag_pos_row[t + 1] - tag_pos_row[t] for t, ok in enumerate(positive(bias)) if ok)
    if fanout < 0:
        return P
    if replace:
        return fanout if P > 0 else 0
    return min(fanout, P)


# ---- the table --------------------------------------------------------------------------------------
def _tags(pattern, T, rank, rng):
    if pattern == "equal":
        return np.full(rank.shape, T - 1)
    if pattern == "alternating":
        return (rank % 2) * (T - 1)
    if pattern == "descending":
        return T - 1 - rank % T
    if pattern == "empty-tags":                                   # odd tags stay empty
        return rng.integers(0, (T + 1) // 2, rank.shape) * 2
    return rng.integers(0, T, rank.shape)


def bias_of(kind, T, dtype):
    b = np.linspace(0.5, 2.0, T)
    if kind == "zero-tag":
        b[0] = 0.0
    elif kind == "all-zero":
        b[:] = 0.0
    elif kind == "nan":
        b[T // 2] = np.nan
    elif kind == "dominant":
        b[T - 1] = 1e6
    return b.astype(dtype)


def _calls(n, degrees, k):
    """(seeds, fanout, replace, bias kind, bias dtype, rng seed) of one case; the long fanouts run on a few seeds."""
    every = list(range(n))
    hub = int(np.argmax(degrees))
    few = [hub, 0, 1, n - 1, hub, 5 % n]
    lists = (every, few + few, list(reversed(every)), [])
    calls = []
    for i, fanout in enumerate(FANOUTS):
        for replace in (False, True):
            j = k + 2 * i + replace
            seeds = lists[j % 4] if 0 <= fanout <= 17 else (few, [], list(reversed(few)))[j % 3]
            calls.append((seeds, fanout, replace, BIASES[j % 5], ("f4", "f8")[j % 2], 1000 + j))
    return calls


def cases():
    rng = np.random.default_rng(21)
    out = []
    shapes = (("ladder", list(LADDER)),                                   # mean degree 323: the 64-lane unit and the hub
              ("short", [d % 18 for d in range(400)] + [3000]))           # mean degree 16: the 16-lane unit and the hub
    for k, (T, (shape, degrees)) in enumerate((T, s) for T in TAGS for s in shapes):
        n = len(degrees)
        indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
        nnz = int(indptr[-1])
        rank = np.arange(nnz) - np.repeat(indptr[:-1], degrees)
        mode = ("null", "identity", "permuted")[k % 3]
        data = None if mode == "null" else (np.arange(nnz) if mode == "identity" else rng.permutation(nnz)).astype(np.int64)
        pattern = PATTERNS[k % 5]
        tag = np.empty(nnz, dtype=("i4", "i8")[k % 2])
        tag[np.arange(nnz) if data is None else data] = _tags(pattern, T, rank, rng)      # indexed by EDGE ID
        out.append({"name": "%s-T%d-%s-%s" % (shape, T, pattern, mode), "n": n, "nnz": nnz, "T": T, "indptr": indptr,
                    "indices": rng.integers(0, n, nnz).astype(np.int64), "data": data, "tag": tag, "degrees": degrees,
                    "calls": _calls(n, degrees, k)})
    return out
