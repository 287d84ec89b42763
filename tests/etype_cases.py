"""Shared by the per-edge-type sampling tests: the table of graphs, edge-type offsets and sampler calls that the host and
device tests run, and an independent Python model.

The model never bisects: it groups a row's entries by type with a list comprehension and counts.  It cannot share a
mistake with csrc/etype_step.h."""
import math

import numpy as np
import torch

DEGREES = (0, 1, 15, 16, 17, 63, 64, 65, 3000)      # every chunk boundary of both group widths, and one hub
TYPES = (1, 2, 16, 17, 64, 65, 1024)                # 16 | 17: the group width changes; 64 | 65: a second chunk; the limit
PROBS = (None, "f4", "f8", "mask")


def entries(case, u):
    """[(row-relative position, edge id)] of row u."""
    lo, hi = int(case["indptr"][u]), int(case["indptr"][u + 1])
    return [(q - lo, q if case["data"] is None else int(case["data"][q])) for q in range(lo, hi)]


def weight_of(case, prob, t, e):
    """The weight of edge id e of type t under the per-type list `prob` (None: uniform)."""
    if prob is None or prob[t] is None:
        return 1.0
    w = float(prob[t][e - case["off"][t]])
    return w if w > 0 and math.isfinite(w) else 0.0


def model(case, seeds, fanout, replace, prob):
    """Per seed, per type: (the edge ids of the type's entries in position order, those with a positive weight, the
    number of picks)."""
    out, grouped = [], case.setdefault("_grouped", {})     # (the grouping of a row is computed once per case)
    for u in seeds:
        if u not in grouped:
            row = entries(case, u) if 0 <= u < case["n"] else []
            grouped[u] = [[e for _, e in row if case["off"][t] <= e < case["off"][t + 1]] for t in range(case["T"])]
        per = []
        for t, f in enumerate(fanout):
            ids = grouped[u][t]
            pos = [e for e in ids if weight_of(case, prob, t, e) > 0]
            per.append((ids, pos, len(pos) if f < 0 else ((f if pos else 0) if replace else min(f, len(pos)))))
        out.append(per)
    return out


def prob_of(case, kind):
    """The per-type weight list of one kind: every third type stays None; zeros and NaNs among the weights."""
    if kind is None:
        return None
    rng = np.random.default_rng(case["T"])
    out = []
    for t in range(case["T"]):
        m = case["off"][t + 1] - case["off"][t]
        if t % 3 == 2:
            out.append(None)
        elif kind == "mask":
            out.append(torch.from_numpy(rng.integers(0, 2, m).astype(bool)))
        else:
            w = rng.choice(np.array([0.0, np.nan, 0.5, 1.0, 3.0, 7.5]), m)
            out.append(torch.from_numpy(w.astype(kind)))
    return out


def cases():
    rng = np.random.default_rng(22)
    indptr = np.concatenate([[0], np.cumsum(DEGREES)]).astype(np.int64)
    n, nnz = len(DEGREES), int(indptr[-1])
    out = []
    for k, T in enumerate(TYPES):
        # the cuts of the id space: repeated values are types with an empty id range; rows list ascending types
        off = np.sort(np.concatenate([[0], rng.integers(0, nnz + 1, T - 1), [nnz]])).astype(np.int64) if T > 1 else np.array([0, nnz])
        if T >= 16:
            off[5] = off[4]                                   # (at least one empty id range)
        mode = ("null", "identity", "permuted")[k % 3]
        data = None if mode == "null" else np.arange(nnz, dtype=np.int64)
        if mode == "permuted":                                # ids shuffled WITHIN a type: rows stay ordered by type
            for t in range(T):
                data[off[t]:off[t + 1]] = off[t] + rng.permutation(off[t + 1] - off[t])
        big = int(min(max(DEGREES), np.diff(off).max())) + 1  # above every n_t
        mix = (0, 1, 2, 32, 33, -1, big)
        fanout = [mix[(t + k) % 7] for t in range(T)]
        seeds = list(range(n)) + [n - 1, 0, n + 3, -1, 4]     # every row, repeats, and two seeds outside the graph
        calls = [(seeds, fanout, replace, kind, 2200 + 10 * k + j) for j, (replace, kind) in
                 enumerate((r, p) for r in (False, True) for p in PROBS)]
        out.append({"name": "T%d-%s" % (T, mode), "n": n, "nnz": nnz, "T": T, "indptr": indptr, "off": off.tolist(),
                    "indices": rng.integers(0, n, nnz).astype(np.int64), "data": data, "calls": calls})
    return out
