"""Shared by the select_topk tests: the table of graphs, weights and calls that the host and device tests run, and an
independent Python model of the rule.

The model sorts a row with Python's ``sorted`` on the tuple (NaN last, weight as a Python float or int, edge id) and takes
a prefix.  It compares VALUES with Python's own float and int comparison (so -0.0 == 0.0 without a special case) and
decodes fp16 / bf16 with ``struct``; it never builds the integer key of csrc/topk_step.h, so it cannot share a mistake
with it."""
import struct

import numpy as np

MAX_PICKS = 1024
KS = (1, 2, 7, 8, 64, 1000, 1024, -1, 0)
DTYPES = ("f4", "f8", "f2", "bf16", "i4", "i8")     # bf16 weights travel as their uint16 bit patterns


# ---- the model --------------------------------------------------------------------------------------
def value_of(dt, raw):
    """The Python value (float or int) of one stored weight."""
    if dt == "bf16":
        return struct.unpack("<f", struct.pack("<I", int(raw) << 16))[0]
    if dt == "f2":
        return struct.unpack("<e", struct.pack("<H", int(np.float16(raw).view(np.uint16))))[0]
    if dt in ("f4", "f8"):
        return float(raw)
    return int(raw)


def sort_key(value, eid, ascending):
    if isinstance(value, float) and value != value:
        return (1, 0, eid)                      # NaN loses in both directions
    return (0, value if ascending else -value, eid)


def row_order(case, dt, weight, ascending, row):
    """[(neighbour, edge id)] of the whole row, best first."""
    lo, hi = int(case["indptr"][row]), int(case["indptr"][row + 1])
    entries = []
    for q in range(lo, hi):
        e = q if case["data"] is None else int(case["data"][q])
        entries.append((sort_key(value_of(dt, weight[e]), e, ascending), int(case["indices"][q]), e))
    entries.sort(key=lambda t: t[0])
    return [(nbr, e) for _, nbr, e in entries]


class Model:
    """The full order of every row of (case, weight, direction), computed once; a call is a prefix per seed."""

    def __init__(self, case, dt, weight, ascending):
        self.rows = [row_order(case, dt, weight, ascending, r) for r in range(case["n"])]

    def select(self, seeds, k):
        indptr, nbr, eids = [0], [], []
        for s in seeds:
            row = self.rows[s]
            picks = len(row) if k < 0 else min(k, len(row))
            nbr += [a for a, _ in row[:picks]]
            eids += [b for _, b in row[:picks]]
            indptr.append(len(nbr))
        return indptr, nbr, eids


# ---- the table --------------------------------------------------------------------------------------
LADDER = (0, 1, 2, 3, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 999, 1000, 1001, 1023, 1024, 1025, 5000)


def _graph(name, degrees, permuted, rng):
    n = len(degrees)
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, n, nnz).astype(np.int64)
    data = rng.permutation(nnz).astype(np.int64) if permuted else None
    return {"name": name + ("-permuted" if permuted else "-identity"), "n": n, "nnz": nnz, "indptr": indptr,
            "indices": indices, "data": data, "degrees": list(degrees)}


def _along_rows(case, per_position):
    """A weight array (indexed by EDGE ID) whose value at CSR position q is per_position[q]."""
    w = np.empty(case["nnz"], dtype=per_position.dtype)
    w[np.arange(case["nnz"]) if case["data"] is None else case["data"]] = per_position
    return w


def bf16_bits(f32):
    return (np.asarray(f32, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _weights(case, rng):
    nnz = case["nnz"]
    pos = np.arange(nnz)
    start = np.repeat(case["indptr"][:-1], case["degrees"])
    rank = pos - start                                   # the position within the row
    dup = rng.integers(-3, 4, nnz)                       # heavy duplication: 7 values
    out = {}
    for dt in ("f4", "f8", "f2", "i4", "i8"):
        out["dups/" + dt] = (dt, dup.astype(dt))
    out["dups/bf16"] = ("bf16", bf16_bits(dup))
    out["equal/f4"] = ("f4", np.full(nnz, 2.5, dtype="f4"))
    out["equal/i8"] = ("i8", np.full(nnz, -7, dtype="i8"))
    for dt in ("f4", "f8", "i4", "i8"):                  # strictly ascending along the row: every entry beats the threshold
        out["ascending/" + dt] = (dt, _along_rows(case, rank.astype(dt)))
    for dt in ("f4", "f8"):
        out["descending/" + dt] = (dt, _along_rows(case, (-rank).astype(dt)))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 65504.0, 1e-7, -1e-7])
    pick = special[rng.integers(0, len(special), nnz)]
    with np.errstate(over="ignore"):
        for dt in ("f4", "f8", "f2"):
            out["specials/" + dt] = (dt, pick.astype(dt))
    neg_nan = pick.astype("f4")
    neg_nan[::5] = np.frombuffer(struct.pack("<I", 0xFFC00001), dtype="f4")[0]      # a NaN with its sign bit set
    out["specials-negative-nan/f4"] = ("f4", neg_nan)
    out["specials/bf16"] = ("bf16", bf16_bits(pick))
    big = np.array([2 ** 63 - 1, -(2 ** 63 - 1), -2 ** 63, 0, 1, -1, 2 ** 31, -2 ** 31 - 1], dtype="i8")
    out["extremes/i8"] = ("i8", big[rng.integers(0, len(big), nnz)])
    small = np.array([2 ** 31 - 1, -2 ** 31, 0, 1, -1], dtype="i4")
    out["extremes/i4"] = ("i4", small[rng.integers(0, len(small), nnz)])
    close = (1.0 + rng.integers(0, 64, nnz) * 2.0 ** -14).astype("f4")     # 64 fp32 values, 2^-14 apart
    out["collide/f2"] = ("f2", close.astype("f2"))                        # fp16 keeps 2^-10: they collide after rounding
    out["collide/bf16"] = ("bf16", bf16_bits(close))
    sub = (rng.integers(-8, 9, nnz) * 2.0 ** -24).astype("f2")            # fp16 subnormals
    out["subnormal/f2"] = ("f2", sub)
    return out


def _calls(case, rng):
    n = case["n"]
    every = list(range(n))
    fits = [r for r in every if case["degrees"][r] <= MAX_PICKS]
    calls = [(every if k >= 0 else fits, k) for k in KS]
    calls.append(([fits[-1], 0, fits[-1], fits[-1], 1][: max(1, min(5, n))], 7))    # a seed listed three times
    calls.append((list(reversed(fits)) + fits[:3], -1))
    calls.append(([], 8))
    calls.append(([], -1))
    calls.append((fits, 5000))                                                      # k above the limit, rows that fit
    return calls


def cases():
    rng = np.random.default_rng(20)
    out = []
    for permuted in (False, True):
        out.append(_graph("ladder", LADDER, permuted, rng))                          # mean degree 543: the wide classes
        out.append(_graph("short", [d % 41 for d in range(160)], permuted, rng))     # mean degree 20, rows up to 40
        out.append(_graph("tiny", [d % 18 for d in range(90)], permuted, rng))       # rows up to 17: k = -1 fits 16 lanes
    for c in out:
        c["weights"] = _weights(c, rng)
        c["calls"] = _calls(c, rng)
    return out


def torch_weight(dt, w):
    import torch

    if dt == "bf16":
        return torch.from_numpy(w.view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(w))
