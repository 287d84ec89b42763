#!/usr/bin/env python
"""Link-prediction batch timings (csrc/exclude.hip) on the C2-shaped graph (ogbn-products size, uniform, int32 ids) made
symmetric: E / 2 random edges followed by their reverses, so that edge e + E / 2 is the reverse of edge e.

    python benchmarks/bench_edge_prediction.py [--batches 1000 10000] [--out profiles/r18/edge_prediction.jsonl]

Per batch of seed edges, with ``NeighborSampler([15, 10])``, ``PerSourceUniform(1)`` and ``exclude="reverse_id"``:

  sample           the whole ``as_edge_prediction_sampler(...).sample(g, eids)`` call: pair and negative graph, compaction,
                   the exclusion set, two sampled layers with the filter, the blocks.  Host work, allocations and
                   read-backs included.
  filter           ``_capi.frontier_exclude`` alone on the outer layer's frontier (fanout 15 over the batch's nodes) against
                   ``torch.isin`` + boolean-mask indexing producing the same three arrays, after asserting them identical.
                   ``model_bytes`` = read nnz x 2 ids, write the survivors x 2 ids; ``stream_fraction`` = model_bytes / call
                   time / 7.1 TB/s: the whole call over the stream rate, not a kernel's share of peak.
  compact          ``compact_graphs([pair, neg])`` (whole call) and its core ``_capi.compact_nodes`` against
                   ``torch.unique(return_inverse=True)`` over the same end points, after asserting them identical.

Every time is wall clock around a device synchronisation: the median (and minimum) of --reps windows after --warm, a
window being --inner back-to-back calls for the two short cases (filter, compact core).
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
from dgl_amd import _capi, dataloading  # noqa: E402
from dgl_amd.sampling import _node_map  # noqa: E402
from tests.graphgen import C2_EDGES, C2_NODES  # noqa: E402

STREAM_RATE = 7.1e12


def timeit(fn, reps, warm, inner=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / inner)
    return float(np.median(ts)), float(np.min(ts))


def torch_filter(indptr, src, eids, n_e, x):
    keep = ~torch.isin(eids[:n_e], x)
    kept = torch.zeros(n_e + 1, dtype=indptr.dtype, device=indptr.device)
    kept[1:] = torch.cumsum(keep, 0)
    return kept[indptr.long()], src[:n_e][keep], eids[:n_e][keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1_000, 10_000])
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--fanouts", type=int, nargs="+", default=[15, 10])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_prediction needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    n, half = args.nodes, args.edges // 2
    E = 2 * half
    gen = torch.Generator(device=dev).manual_seed(18)
    u = torch.randint(0, n, (half,), device=dev, generator=gen, dtype=torch.int32)
    v = torch.randint(0, n, (half,), device=dev, generator=gen, dtype=torch.int32)
    g = dgl.graph((torch.cat([u, v]), torch.cat([v, u])), num_nodes=n, idtype=torch.int32, device=dev)
    rev = ((torch.arange(E, device=dev) + half) % E).to(torch.int32)
    rel = g._graph.relations[0]
    indptr, indices, emap = rel.csc()                  # built once, outside the timings
    csr = _capi.make_csr(indptr, indices, emap, n)
    lines = []

    def emit(rec):
        rec.update(nodes=n, edges=E, fanouts=args.fanouts, id_bytes=4, gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    neg = dgl.negative_sampler.PerSourceUniform(1)
    for batch in args.batches:
        eids = torch.randperm(E, device=dev, generator=gen)[:batch].to(torch.int32)
        es = dataloading.as_edge_prediction_sampler(dgl.NeighborSampler(args.fanouts, seed=1), exclude="reverse_id",
                                                    reverse_eids=rev, negative_sampler=neg)
        ms, best = timeit(lambda: es.sample(g, eids), args.reps, args.warm)
        input_nodes, pair, ngraph, blocks = es.sample(g, eids)
        x = _capi.exclude_set(eids, E, reverse=rev)
        leaked = sum(int(torch.isin(b.edata[dgl.EID], x).sum()) for b in blocks)
        plain = dataloading.as_edge_prediction_sampler(dgl.NeighborSampler(args.fanouts, seed=1), negative_sampler=neg)
        pms, _ = timeit(lambda: plain.sample(g, eids), args.reps, args.warm)
        emit(dict(case="sample", batch=batch, ms=ms, ms_min=best, ms_without_exclusion=pms, seed_nodes=pair.num_nodes(),
                  input_nodes=int(input_nodes.shape[0]), block_edges=[b.num_edges() for b in blocks],
                  excluded_edges_in_blocks=leaked))

        # the filter alone, on the outer layer's frontier
        seeds = pair.ndata[dgl.NID]
        f_indptr, f_src, f_eids = _capi.sample_neighbors(csr, seeds, args.fanouts[-1], False, 1)
        n_e = int(f_indptr[-1])
        got = _capi.frontier_exclude(f_indptr, f_src, f_eids, x)
        want = torch_filter(f_indptr, f_src, f_eids, n_e, x)
        kept = int(got[0][-1])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1][:kept], want[1]) and torch.equal(got[2][:kept], want[2])
        fms, fbest = timeit(lambda: _capi.frontier_exclude(f_indptr, f_src, f_eids, x), args.reps, args.warm, args.inner)
        tms, tbest = timeit(lambda: torch_filter(f_indptr, f_src, f_eids, n_e, x), args.reps, args.warm, args.inner)
        model = (2 * n_e + 2 * kept) * 4
        emit(dict(case="filter", batch=batch, rows=int(seeds.shape[0]), nnz=n_e, kept=kept, n_x=int(x.shape[0]), ms=fms,
                  ms_min=fbest, torch_ms=tms, torch_ms_min=tbest, ratio_torch_over_kernel=tms / fms, identical=True,
                  model_bytes=model, stream_fraction=model / (fms * 1e-3) / STREAM_RATE))

        # compaction of the pair and the negative graph
        pu, pv = g.find_edges(eids)
        nu, nv = neg(g, eids)
        pg = dgl.graph((pu, pv), num_nodes=n, idtype=torch.int32, device=dev)
        ng = dgl.graph((nu, nv), num_nodes=n, idtype=torch.int32, device=dev)
        ends = torch.cat([pu, pv, nu, nv]).contiguous()
        none = torch.empty(0, dtype=torch.int32, device=dev)
        node_map = _node_map(pg, dev)
        local, nodes = _capi.compact_nodes(none, ends, node_map)
        t_nodes, t_inv = torch.unique(ends, return_inverse=True)
        assert torch.equal(nodes, t_nodes) and torch.equal(local.long(), t_inv)
        gms, gbest = timeit(lambda: dgl.compact_graphs([pg, ng]), args.reps, args.warm)
        cms, cbest = timeit(lambda: _capi.compact_nodes(none, ends, node_map), args.reps, args.warm, args.inner)
        ums, ubest = timeit(lambda: torch.unique(ends, return_inverse=True), args.reps, args.warm, args.inner)
        emit(dict(case="compact", batch=batch, end_points=int(ends.shape[0]), nodes_kept=int(nodes.shape[0]),
                  ms_compact_graphs=gms, ms_compact_graphs_min=gbest, ms=cms, ms_min=cbest, torch_ms=ums, torch_ms_min=ubest,
                  ratio_torch_over_kernel=ums / cms, identical=True))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
