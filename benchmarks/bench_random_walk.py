#!/usr/bin/env python
"""Random-walk timings (csrc/random_walk.hip) with the HIP-event protocol of benchmarks/bench_ops.py: medians of 10 calls
after 3 warm-up calls, one JSON line per case.

    python benchmarks/bench_random_walk.py [--walks 1000000] [--steps 32] [--out profiles/r10/random_walk.jsonl]

The graph is the C2 shape (tests/graphgen.py: 2 449 029 nodes, 61 859 140 edges, log-normal out-degrees with a 17 500-edge
tail, uniform successors), used as the out-edge CSR.  Cases: uniform and weighted walks, with and without the edge-id
map, with and without the edge-id output; plus the one-off CDF build.  What is timed is `_capi.random_walk` (output
allocation + one kernel launch); a step is one hop a walk actually made (walks that reach a node without out-edges stop).

`requests_per_step` is the MODEL of 64-byte-or-larger line requests a lane issues per hop, counted from the code, not
measured: the indptr pair (1), indices[pos] (1), the trace store (1); + 1 for the edge-id map, + 1 for the edge-id output;
the weighted step adds the row total and the bisection's probes, 1 + ceil(log2(deg)) on the degrees the walks actually
visited.  `model_fraction` compares steps/s with 55.5 G requests/s (what the g-SpMM merge kernel sustains, README.md)
divided by that count — a yardstick nobody has measured for this access pattern, not a peak.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_random_walk needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    g = synth_csr(args.nodes, args.nodes, args.edges, "U", device=dev, with_eids=True, sort_cols=False)
    gen = torch.Generator(device=dev).manual_seed(1)
    prob = torch.rand(args.edges, device=dev, generator=gen)
    seeds = torch.randint(0, args.nodes, (args.walks,), device=dev, generator=gen).to(g["indptr"].dtype)
    deg = (g["indptr"][1:] - g["indptr"][:-1]).long()
    lines = []

    def emit(rec):
        rec.update(walks=args.walks, steps=args.steps, nodes=args.nodes, edges=args.edges, gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for with_map in (False, True):
        csr = _capi.make_csr(g["indptr"], g["indices"], g["eids"] if with_map else None, args.nodes)
        ms, best = timeit(lambda: _capi.random_walk_cdf(csr, prob))
        emit(dict(case="cdf_build", edge_id_map=with_map, ms=ms, ms_min=best, edges_per_s=args.edges / (ms * 1e-3)))
        cdf = _capi.random_walk_cdf(csr, prob)
        for weighted in (False, True):
            for want_eids in (False, True):
                rels = [(csr, cdf if weighted else None)]
                run = lambda: _capi.random_walk(rels, [0] * args.steps, seeds, rng_seed=7, return_eids=want_eids)
                ms, best = timeit(run)
                traces, _ = run()
                made = traces[:, 1:] >= 0
                hops = int(made.sum())
                req = 3.0 + (1.0 if with_map else 0.0) + (1.0 if want_eids else 0.0)
                if weighted:
                    d = deg[traces[:, :-1][made].long()].double()
                    req += 1.0 + float(torch.ceil(torch.log2(d)).mean())
                rate = hops / (ms * 1e-3)
                emit(dict(case="weighted" if weighted else "uniform", edge_id_map=with_map, eids_out=want_eids, ms=ms,
                          ms_min=best, hops=hops, steps_per_s=rate, requests_per_step=req,
                          model_steps_per_s=REQUEST_RATE / req, model_fraction=rate * req / REQUEST_RATE))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
