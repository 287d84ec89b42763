#!/usr/bin/env python
"""Neighbour-matching timings (csrc/matching.hip) with the HIP-event protocol of benchmarks/bench_labor.py: medians of
10 calls after 3 warm-up calls, timed on the stream with events (the calls synchronise themselves: they read back).

    python benchmarks/bench_neighbor_matching.py [--out profiles/r16/neighbor_matching.jsonl]

Graphs, all bi-directed, int32 ids, no edge-id map:
  c2      the C2-shaped graph of tests/graphgen.py (ogbn-products size, uniform) with every edge in both directions
          (mean degree 50: a wavefront per row)
  grid    a 2-D grid of --grid x --grid nodes (degree <= 4: 16 lanes per row)
  batch   --graphs disjoint random graphs of 64 nodes each, as a pooling model batches them (16 lanes per row)
Forms: unweighted, and fp32 weights by edge id.  Cases per graph and form:

  neighbor_matching   `_capi.neighbor_matching` with relabelling, the output and scratch allocation included, at the
                      library's default batch of rounds between read-backs; `ms_batch_<b>` the same at other batch sizes;
                      `noop_round_ms` = (ms at batch 64 - ms at batch rounds + 1) / (63 - rounds), both one batch and
                      one read-back: a round in which every row is inactive, two launches that read label once.
                      (rounds - 2) * noop_round_ms bounds from above what a GLOBAL compaction of the active list
                      between rounds could still save.
  torch_matching      the same rule composed from torch round by round (colours and hashes as int64 arithmetic, the best
                      key per row by scatter_reduce amax / amin over the candidate entries, one .any() read-back per
                      round): the yardstick.  `equals_kernel`: its labels are the kernel's, bit for bit.

`rounds`, `readbacks` and `row_entries_per_round` (entries of the rows active at the start of the round: what propose
streams at most, a RED row leaves at its first active neighbour) come from the torch composition's trace.
`model_bytes` is the byte model of DESIGN.md 3.17, counted from that trace and not from counters: per round, b bytes of
label per node and phase (the activity test), and for the rows that stream (propose: the active rows; respond: the active
RED rows that have an active neighbour) 2 b per row for indptr plus 2 b per entry (the id and one gather), b = 4.
`graph_passes` = the entries streamed over all rounds and phases / nnz.  `stream_fraction` = model_bytes / call time /
7.1 TB/s: the whole call (allocation, launches and read-backs included) over the read-only stream rate the README
records, not a kernel's share of peak.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dgl_amd  # noqa: E402,F401
from dgl_amd import _capi  # noqa: E402
from tests.graphgen import C2_EDGES, C2_NODES, synth_csr  # noqa: E402

STREAM_RATE = 7.1e12
MIN64 = -(1 << 63)


def timeit(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for k in range(reps):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    ts = [ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]
    return float(np.median(ts)), float(np.min(ts))


# ---- the rule in torch (int64 arithmetic wraps mod 2^64) --------------------------------------------
def _s64(c):
    return c - (1 << 64) if c >= (1 << 63) else c


def _lsr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def mix64(z):
    z = z + _s64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def colours(seed, ids, t):
    draw = mix64(mix64(mix64(_s64(seed) ^ (ids * _s64(0xD1B54A32D192ED03))) + t) + 0)
    return (draw ^ MIN64) < (_s64(0x88b827fa1a0cf000) ^ MIN64)           # unsigned compare


def edge_hash(seed, u, v):
    a, b = torch.minimum(u, v), torch.maximum(u, v)
    h = mix64(mix64(_s64(seed ^ 0x6D61746368696E67) ^ (a * _s64(0xD1B54A32D192ED03))) + b)
    return h ^ MIN64                                                      # signed order == the unsigned order of h


def best_per_row(rows, cols, w, h, sel, n):
    """The column of the selected entry of every row with the largest (w, h), the smaller column on a full tie; -1."""
    idx = torch.nonzero(sel).reshape(-1)
    r = rows[idx]
    if w is not None:
        top = torch.full((n,), -1.0, dtype=w.dtype, device=r.device).scatter_reduce_(0, r, w[idx], "amax")
        idx = idx[w[idx] == top[r]]
        r = rows[idx]
    top = torch.full((n,), MIN64, dtype=torch.int64, device=r.device).scatter_reduce_(0, r, h[idx], "amax")
    idx = idx[h[idx] == top[r]]
    r = rows[idx]
    low = torch.full((n,), n, dtype=torch.int64, device=r.device).scatter_reduce_(0, r, cols[idx], "amin")
    return torch.where(low == n, -1, low)


def torch_matching(n, rows, cols, valid, w, h, seed, trace=None):
    """(label, rounds); rows / cols are the int64 entry list, w the clamped weights per entry or None, h the hashes."""
    dev = rows.device
    ids = torch.arange(n, device=dev)
    label = torch.full((n,), -1, dtype=torch.int64, device=dev)
    prop = torch.full((n,), -1, dtype=torch.int64, device=dev)
    t = 0
    while True:
        active = label < 0
        if not bool(active.any()):                                       # the read-back of the round
            return label, t
        blue = colours(seed, ids, t)
        live = valid & active[rows] & active[cols]
        has_nb = torch.zeros(n, dtype=torch.bool, device=dev)
        has_nb[rows[live]] = True
        best = best_per_row(rows, cols, w, h, live & blue[rows] & ~blue[cols], n)
        new = torch.where(~has_nb, -2, torch.where(blue & (best >= 0), best, -1))
        prop = torch.where(active, new, prop)
        single = active & (prop == -2)
        label = torch.where(single, ids, label)
        pick = best_per_row(rows, cols, w, h, live & ~blue[rows] & blue[cols] & (prop[cols] == rows), n)
        us = torch.nonzero(pick >= 0).reshape(-1)
        vs = pick[us]
        m = torch.minimum(us, vs)
        label[us] = m
        label[vs] = m
        if trace is not None:
            trace.append((active, active & ~blue & has_nb))
        t += 1


# ---- graphs -----------------------------------------------------------------------------------------
def csr_from_pairs(n, a, b, dev):
    """int32 CSR of the entries a -> b and b -> a (a, b int64 tensors on the device), rows in stable order."""
    src, dst = torch.cat([a, b]), torch.cat([b, a])
    order = torch.argsort(src, stable=True)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    return indptr.to(torch.int32), dst[order].to(torch.int32).contiguous()


def make_graph(name, args, dev):
    if name == "c2":
        g = synth_csr(args.nodes, args.nodes, args.edges, "U", device=dev, with_eids=False, sort_cols=False)
        deg = (g["indptr"][1:] - g["indptr"][:-1]).long()
        a = torch.repeat_interleave(torch.arange(args.nodes, device=dev), deg)
        return args.nodes, csr_from_pairs(args.nodes, a, g["indices"].long(), dev)
    if name == "grid":
        s = args.grid
        at = torch.arange(s * s, device=dev).reshape(s, s)
        a = torch.cat([at[:, :-1].reshape(-1), at[:-1, :].reshape(-1)])
        b = torch.cat([at[:, 1:].reshape(-1), at[1:, :].reshape(-1)])
        return s * s, csr_from_pairs(s * s, a, b, dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    k, m = 64, 192                                                        # nodes and edges per small graph
    base = torch.arange(args.graphs, device=dev).repeat_interleave(m) * k
    a = torch.randint(0, k, (args.graphs * m,), device=dev, generator=gen)
    b = torch.randint(0, k, (args.graphs * m,), device=dev, generator=gen)
    keep = a != b
    return args.graphs * k, csr_from_pairs(args.graphs * k, (base + a)[keep], (base + b)[keep], dev)


def bench_graph(name, args, dev, lines):
    n, (indptr, indices) = make_graph(name, args, dev)
    nnz = int(indices.shape[0])
    csr = _capi.make_csr(indptr, indices, None, n)
    deg = (indptr[1:] - indptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(n, device=dev), deg)
    cols = indices.long()
    valid = rows != cols
    seed, b = 7, 4
    h = edge_hash(seed, rows, cols)
    gen = torch.Generator(device=dev).manual_seed(1)
    weight = torch.rand(nnz, device=dev, generator=gen)                   # fp32, by edge id (= CSR position: no map)

    def emit(rec):
        rec.update(graph=name, nodes=n, entries=nnz, mean_degree=nnz / n, lanes_per_row=16 if nnz // n <= 32 else 64,
                   gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for form, wt in (("unweighted", None), ("weighted_f32", weight)):
        run = lambda batch=0: _capi.neighbor_matching(csr, wt, seed, relabel=True, batch_rounds=batch)
        ms, best = timeit(run)
        _, rounds = run()
        label, _ = _capi.neighbor_matching(csr, wt, seed)
        by_batch = {bb: timeit(lambda bb=bb: run(bb))[0] for bb in sorted({1, 4, 16, 64, rounds + 1})}
        noop = (by_batch[64] - by_batch[rounds + 1]) / (63 - rounds) if rounds < 63 else None
        w_entry = None if wt is None else wt.clamp(min=0).double()
        trace = []
        t_label, t_rounds = torch_matching(n, rows, cols, valid, w_entry, h, seed, trace)
        tms, tbest = timeit(lambda: torch_matching(n, rows, cols, valid, w_entry, h, seed), reps=3, warm=1)
        per_round, streamed, model = [], 0, 0
        for active, red_rows in trace:
            p, r = int(deg[active].sum()), int(deg[red_rows].sum())
            per_round.append(p)
            streamed += p + r
            model += 2 * n * b + 2 * b * (int(active.sum()) + int(red_rows.sum())) + 2 * b * (p + r)
        model += 2 * n * b + 3 * n * b                                    # init of label and prop; flag, rank gather, out
        default_batch = 8
        emit(dict(case="neighbor_matching", form=form, ms=ms, ms_min=best, rounds=rounds,
                  readbacks=rounds // default_batch + 1,
                  **{"ms_batch_%d" % bb: v for bb, v in by_batch.items()}, noop_round_ms=noop,
                  compaction_upper_bound_ms=None if noop is None else max(rounds - 2, 0) * noop,
                  clusters=int(torch.unique(label).numel()), row_entries_per_round=per_round,
                  graph_passes=streamed / max(nnz, 1), model_bytes=model,
                  stream_fraction=model / (ms * 1e-3) / STREAM_RATE, entries_per_s=nnz / (ms * 1e-3),
                  workspace_bytes=int(_capi.LIB.dgla_neighbor_matching_workspace_bytes(32, n))))
        emit(dict(case="torch_matching", form=form, ms=tms, ms_min=tbest, rounds=t_rounds, readbacks=t_rounds + 1,
                  equals_kernel=bool(t_rounds == rounds and torch.equal(t_label.to(label.dtype), label)),
                  ratio_torch_over_kernel=tms / ms))
    del rows, cols, h, valid
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs-to-run", nargs="+", default=["c2", "grid", "batch"])
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbor_matching needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []
    for name in args.graphs_to_run:
        bench_graph(name, args, dev, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
