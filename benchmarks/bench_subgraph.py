#!/usr/bin/env python
"""Node-induced subgraph timings (csrc/subgraph.hip) on the C2-shaped graph of tests/graphgen.py (ogbn-products size,
uniform, int32 ids, in-edge CSR without an edge-id map).

    python benchmarks/bench_subgraph.py [--nodes-selected 1000 10000 100000] [--out profiles/r17/subgraph.jsonl]

Every case is timed as a WHOLE CALL, host work, allocations and read-backs included (wall clock around a device
synchronisation; the median of --reps calls after --warm), against the torch `node_subgraph` on the same node set in the
same run, and the two results are asserted identical (edges, ids, features).

  induced_rows     `transforms._induced_rows` on n distinct random nodes
  khop_in          `khop_in_subgraph` (1 000 seeds, k = 2); the yardstick is `node_subgraph` on the node set it found, so
                   the hop expansion is on the kernel's side of the comparison only (`ms_induced_only` leaves it out)
  shadow           one `ShaDowKHopSampler([10, 10])` step at batch 1 000; the yardstick as for khop_in

`model_bytes` is the byte model 2 passes x (sum of the selected nodes' in-degrees) x (id bytes + one 4-byte gather request
per entry), counted from the degrees; `stream_fraction` = model_bytes / call time / 7.1 TB/s, the read-only stream rate
the README records: the whole call over that rate, not a kernel's share of peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dgl_amd as dgl  # noqa: E402
from dgl_amd import transforms  # noqa: E402
from dgl_amd.graph_index import GraphIndex, Relation  # noqa: E402
from tests.graphgen import C2_EDGES, C2_NODES, synth_csr  # noqa: E402
from tests.subgraph_cases import same_graph  # noqa: E402

STREAM_RATE = 7.1e12


def timeit(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes-selected", type=int, nargs="+", default=[1_000, 10_000, 100_000])
    ap.add_argument("--batch", type=int, default=1_000)
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_subgraph needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    n = args.nodes
    c = synth_csr(n, n, args.edges, "U", device=dev, with_eids=False, sort_cols=False)
    indptr, indices = c["indptr"].to(torch.int32), c["indices"].to(torch.int32)
    rel = Relation(n, n, csc=(indptr, indices, None), idtype=torch.int32, device=dev)
    g = dgl.DGLGraph(GraphIndex([n], [(0, 0)], [rel]), ["_N"], [("_N", "_E", "_N")])
    nnz = int(indices.shape[0])
    gen = torch.Generator(device=dev).manual_seed(1)
    g.ndata["x"] = torch.rand(n, 8, device=dev, generator=gen)
    g.edges()                                        # the COO of the torch path, built once outside the timings
    deg = (indptr[1:] - indptr[:-1]).long()
    b = 4
    lines = []

    def emit(rec):
        rec.update(nodes=n, edges=nnz, mean_degree=nnz / n, lanes_per_row=16 if nnz // n <= 32 else 64, id_bytes=b,
                   gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def against_torch(case, ids, ms, best, got, extra):
        D = int(deg[ids.long()].sum())
        tms, tbest = timeit(lambda: transforms.node_subgraph(g, ids), args.reps, args.warm)
        same_graph(got, transforms.node_subgraph(g, ids))
        model = 2 * D * (b + 4)
        emit(dict(case=case, selected=int(ids.shape[0]), ms=ms, ms_min=best, torch_ms=tms, torch_ms_min=tbest,
                  ratio_torch_over_kernel=tms / ms, rows_read=D, kept_edges=got.num_edges(), identical=True,
                  model_bytes=model, stream_fraction=model / (ms * 1e-3) / STREAM_RATE, **extra))

    for k in args.nodes_selected:
        ids = torch.randperm(n, device=dev, generator=gen)[:k].to(torch.int32)
        run = lambda: transforms._induced_rows(g, {"_N": ids})
        ms, best = timeit(run, args.reps, args.warm)
        against_torch("induced_rows", ids, ms, best, run(), {})

    seeds = torch.randperm(n, device=dev, generator=gen)[:args.batch].to(torch.int32)
    run = lambda: dgl.khop_in_subgraph(g, seeds, 2)
    ms, best = timeit(run, args.reps, args.warm)
    got = run()[0]
    ids = got.ndata["_ID"]
    ims, _ = timeit(lambda: transforms._induced_rows(g, {"_N": ids}), args.reps, args.warm)
    against_torch("khop_in", ids, ms, best, got, dict(seeds=args.batch, k=2, ms_induced_only=ims))

    sampler = dgl.ShaDowKHopSampler([10, 10], seed=3)
    ms, best = timeit(lambda: sampler.sample(g, seeds), args.reps, args.warm)
    ids, _, got = sampler.sample(g, seeds)
    ims, _ = timeit(lambda: transforms._induced_rows(g, {"_N": ids}), args.reps, args.warm)
    against_torch("shadow", ids, ms, best, got, dict(seeds=args.batch, fanouts=[10, 10], ms_induced_only=ims))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
