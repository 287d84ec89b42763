#!/usr/bin/env python
"""node2vec walk timings (csrc/node2vec.hip) with the HIP-event protocol of benchmarks/bench_random_walk.py: medians of 10
calls after 3 warm-up calls, one JSON line per case.

    python benchmarks/bench_node2vec.py [--walks 1000000] [--steps 32] [--out profiles/r12/node2vec.jsonl]

The graph is the C2 shape (tests/graphgen.py) made symmetric: every edge and its reverse, int32 ids, as the out-edge CSR
without an edge-id map.  Cases: the one-off membership-list build (dgla_csr_sorted_columns); `random_walk` on the same
graph in the same run, uniform and weighted — the yardstick; node2vec walks, uniform and weighted, at (p, q) = (1, 1),
(0.25, 4), (4, 0.25) and (100, 0.01).  What is timed is `_capi.node2vec_walk` (output allocation + one kernel launch); a
step is one hop a walk actually made.

`attempts_per_step` and `scan_share` come from dgla_node2vec_walk_host with `stats` on the first --sample walks (the
device kernel keeps no counters): candidates drawn per second-order step, and the share of those steps that fell through
to the exact scan.

`requests_per_step` is the MODEL of line requests a lane issues per hop, counted from the code, not measured: per
attempt one `indices` gather, the candidate's indptr pair and ceil(log2 deg(x)) probes of the membership list (plus,
weighted, the row total and the ceil(log2 deg(curr)) probes of the CDF); per step the trace store.  It charges every
attempt its class test; the kernel skips the pair and the probes when the acceptance draw decides without the class (at
(1, 1) always), so the model is an upper count there.  `model_fraction` compares steps/s with 55.5 G requests/s (what the
g-SpMM merge kernel sustains, README.md) divided by that count — a yardstick nobody has measured for this access pattern,
not a peak.  `ratio_to_random_walk` is the time of the node2vec call over the time of `random_walk` with the same
weights: at (1, 1) both make the same picks, so that ratio is the cost of the second-order machinery.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dgl_amd import _capi  # noqa: E402
from tests.graphgen import C2_EDGES, C2_NODES, synth_csr  # noqa: E402

REQUEST_RATE = 55.5e9
PQ = [(1.0, 1.0), (0.25, 4.0), (4.0, 0.25), (100.0, 0.01)]


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


def symmetric_csr(nodes, edges, dev):
    g = synth_csr(nodes, nodes, edges, "U", device=dev, with_eids=False, sort_cols=False)
    deg = (g["indptr"][1:] - g["indptr"][:-1]).long()
    row = torch.repeat_interleave(torch.arange(nodes, device=dev, dtype=torch.int32), deg, output_size=edges)
    col = g["indices"].to(torch.int32)
    indptr, indices, _ = _capi.coo_to_csr(torch.cat([row, col]), torch.cat([col, row]), None, nodes, nodes)
    return indptr, indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--sample", type=int, default=20000, help="walks the host walker repeats for the counters")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_node2vec needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    indptr, indices = symmetric_csr(args.nodes, args.edges, dev)
    nnz = int(indices.shape[0])
    gen = torch.Generator(device=dev).manual_seed(1)
    prob = torch.rand(nnz, device=dev, generator=gen)
    seeds = torch.randint(0, args.nodes, (args.walks,), device=dev, generator=gen).to(torch.int32)
    deg = (indptr[1:] - indptr[:-1]).long()
    csr = _capi.make_csr(indptr, indices, None, args.nodes)
    lines = []

    def emit(rec):
        rec.update(walks=args.walks, steps=args.steps, nodes=args.nodes, edges=nnz, gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    ms, best = timeit(lambda: _capi.csr_sorted_columns(csr))
    emit(dict(case="membership_build", ms=ms, ms_min=best, edges_per_s=nnz / (ms * 1e-3),
              workspace_bytes=int(_capi.LIB.dgla_csr_sorted_columns_workspace_bytes(_capi.ctypes.byref(csr)))))
    member = _capi.csr_sorted_columns(csr)
    cdf = _capi.random_walk_cdf(csr, prob)
    # the host side of the counters: the same arrays on the CPU
    sample = min(args.sample, args.walks)
    h_csr = _capi.host_csr(indptr.cpu(), indices.cpu(), None, args.nodes)
    h_member, h_cdf, h_seeds = member.cpu(), cdf.cpu(), seeds[:sample].cpu().contiguous()

    base = {}
    for weighted in (False, True):
        rels = [(csr, cdf if weighted else None)]
        run = lambda: _capi.random_walk(rels, [0] * args.steps, seeds, rng_seed=7, return_eids=False)
        ms, best = timeit(run)
        hops = int((run()[0][:, 1:] >= 0).sum())
        base[weighted] = ms
        emit(dict(case="random_walk", weighted=weighted, ms=ms, ms_min=best, hops=hops, steps_per_s=hops / (ms * 1e-3)))

    for weighted in (False, True):
        for p, q in PQ:
            c = cdf if weighted else None
            run = lambda: _capi.node2vec_walk(csr, c, member, seeds, args.steps, p, q, rng_seed=7, return_eids=False)
            ms, best = timeit(run)
            traces, _ = run()
            made = traces[:, 1:] >= 0
            hops = int(made.sum())
            ht, _, stats = _capi.node2vec_walk_host(h_csr, h_cdf if weighted else None, h_member, h_seeds, args.steps, p,
                                                    q, rng_seed=7, return_eids=False, stats=True)
            same = bool(torch.equal(ht, traces[:sample].cpu()))
            attempts = stats[1] / max(1, stats[0])
            d_next = deg[traces[:, 1:][made].long()].double().clamp(min=1)
            per_attempt = 2.0 + float(torch.ceil(torch.log2(d_next)).mean())
            if weighted:
                d_curr = deg[traces[:, :-1][made].long()].double().clamp(min=1)
                per_attempt += 1.0 + float(torch.ceil(torch.log2(d_curr)).mean())
            req = attempts * per_attempt + 1.0
            rate = hops / (ms * 1e-3)
            emit(dict(case="node2vec", weighted=weighted, p=p, q=q, ms=ms, ms_min=best, hops=hops, steps_per_s=rate,
                      attempts_per_step=attempts, scan_share=stats[2] / max(1, stats[0]), sample_walks=sample,
                      sample_equals_host=same, requests_per_step=req, model_steps_per_s=REQUEST_RATE / req,
                      model_fraction=rate * req / REQUEST_RATE, ratio_to_random_walk=ms / base[weighted]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
