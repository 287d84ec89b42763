#!/usr/bin/env python
"""Layer-neighbour (LABOR-0) sampling timings (csrc/labor.hip) with the HIP-event protocol of
benchmarks/bench_negative_sampling.py: medians of 10 calls after 3 warm-up calls, timed on the stream with events.

    python benchmarks/bench_labor.py [--seeds 10000 100000] [--fanout 10] [--out profiles/r14/labor.jsonl]

Graph: the C2-shaped graph of tests/graphgen.py (ogbn-products size, uniform, int32 ids) as an in-edge CSR without an
edge-id map (mean degree 25: the kernels give a row 16 lanes), at every number of seeds; then `dense`, the same number
of edges over an eighth of the nodes (mean degree 202: a wavefront per row), at the largest number of seeds, so that each
group width has a workload.  The seeds are distinct random nodes.  Cases, per graph and number of seeds:

  labor_uniform      `_capi.labor_sample` without weights: count, the scan, one read-back of the total, fill, with the
                     output and workspace allocation; `sample_equals_host` compares the first --sample seeds' rows with
                     dgla_labor_pick_host
  labor_scale        `_capi.labor_scale` (fp32 weights by edge id): the per-seed scale alone
  labor_weighted     `_capi.labor_sample` with those weights and the scale given: count, scan, read-back, fill
  sample_neighbors   `_capi.sample_neighbors` at the same seeds and fanout — the sampler LABOR stands next to
  torch_labor        the uniform rule composed from torch: one `torch.rand` variate per node, the seeds' rows expanded
                     with repeat_interleave, keep = r[neighbour] < k / degree, boolean selection, a cumsum for the
                     offsets — the yardstick (the same law, not the same picks)

`distinct_sources` is the number of distinct neighbour ids in the result: what LABOR is for.  It is reported for LABOR and
for sample_neighbors at the same seeds and fanout.

`model_bytes` is the byte model of DESIGN.md 3.15, counted from the degrees and not from counters: D = the seeds' degrees
summed, D_long = the same over rows longer than the fanout, K = kept entries, b = 4 (int32 ids), n seeds.
    uniform   (D_long + D) b   [ids: count skips rows it keeps whole, fill reads every row]   + 2 K b   + n (3 b + 24)
    weighted  2 D b + 2 D 4    [ids and weights, count + fill]                                + K (2 b + 4) + n (3 b + 40)
    scale     2 D 4            [weights: the first sweep and ONE saturation pass; more passes re-read cached lines]
`stream_fraction` = model_bytes / call time / 7.1 TB/s, the read-only stream rate the README records.  It is the whole
call over that rate (allocation, four launches and one host synchronisation included), not a kernel's share of peak.
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


def bench_graph(args, dev, label, nodes, seed_counts, lines):
    """Every case on one uniform graph of `nodes` nodes and args.edges edges, at each number of seeds."""
    g = synth_csr(nodes, nodes, args.edges, "U", device=dev, with_eids=False, sort_cols=False)
    indptr, indices = g["indptr"].to(torch.int32), g["indices"].to(torch.int32)
    nnz = int(indices.shape[0])
    csr = _capi.make_csr(indptr, indices, None, nodes)
    h_csr = _capi.host_csr(indptr.cpu(), indices.cpu(), None, nodes)
    deg = (indptr[1:] - indptr[:-1]).long()
    gen = torch.Generator(device=dev).manual_seed(1)
    prob = torch.rand(nnz, device=dev, generator=gen) + 0.05       # fp32, by edge id (= CSR position: no map)
    h_prob = prob.cpu()
    k, b = args.fanout, 4

    def emit(rec):
        rec.update(graph=label, mean_degree=nnz / nodes, lanes_per_row=16 if nnz // nodes <= 32 else 64, nodes=nodes,
                   edges=nnz, fanout=k, gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for n in seed_counts:
        seeds = torch.randperm(nodes, device=dev, generator=gen)[:n].to(torch.int32).contiguous()
        d = deg[seeds.long()]
        D, D_long = int(d.sum()), int(d[d > k].sum())
        small = min(args.sample, n)
        h_seeds = seeds[:small].cpu()

        def rows_equal(got, want):
            m = int(want[0][-1])
            return bool(torch.equal(got[0][:small + 1].cpu(), want[0]) and torch.equal(got[1][:m].cpu(), want[1])
                        and torch.equal(got[2][:m].cpu(), want[2])
                        and (want[3] is None or torch.equal(got[3][:m].cpu(), want[3])))

        # ---- uniform ----
        run = lambda: _capi.labor_sample(csr, seeds, k, 7)
        ms, best = timeit(run)
        got = run()
        K = int(got[0][-1])
        same = rows_equal(got, _capi.labor_pick_host(h_csr, h_seeds, k, 7))
        model = (D_long + D) * b + 2 * K * b + n * (3 * b + 24)
        labor_distinct = int(torch.unique(got[1]).numel())
        emit(dict(case="labor_uniform", seeds=n, ms=ms, ms_min=best, seeds_per_s=n / (ms * 1e-3), neighbours_read=D,
                  neighbours_per_s=D / (ms * 1e-3), kept=K, distinct_sources=labor_distinct, sample_seeds=small,
                  sample_equals_host=same, model_bytes=model, stream_fraction=model / (ms * 1e-3) / STREAM_RATE,
                  workspace_bytes=int(_capi.LIB.dgla_labor_workspace_bytes(32, n))))

        # ---- weighted ----
        ms_c, best_c = timeit(lambda: _capi.labor_scale(csr, prob, seeds, k))
        c = _capi.labor_scale(csr, prob, seeds, k)
        h_c = _capi.labor_scale_host(h_csr, h_prob, h_seeds, k)
        fin = torch.isfinite(h_c)
        rel = float(((c[:small].cpu() - h_c)[fin].abs() / h_c[fin]).max()) if bool(fin.any()) else 0.0
        model_c = 2 * D * 4 + n * (3 * b + 8)
        emit(dict(case="labor_scale", seeds=n, ms=ms_c, ms_min=best_c, seeds_per_s=n / (ms_c * 1e-3), neighbours_read=D,
                  max_rel_diff_to_host=rel, model_bytes=model_c, stream_fraction=model_c / (ms_c * 1e-3) / STREAM_RATE))
        run = lambda: _capi.labor_sample(csr, seeds, k, 7, prob=prob, c=c)
        ms, best = timeit(run)
        got = run()
        Kw = int(got[0][-1])
        same = rows_equal(got, _capi.labor_pick_host(h_csr, h_seeds, k, 7, prob=h_prob, c=c[:small].cpu()))
        model = 2 * D * b + 2 * D * 4 + Kw * (2 * b + 4) + n * (3 * b + 40)
        emit(dict(case="labor_weighted", seeds=n, ms=ms, ms_min=best, seeds_per_s=n / (ms * 1e-3), neighbours_read=D,
                  neighbours_per_s=D / (ms * 1e-3), kept=Kw, kept_per_seed=Kw / n,
                  distinct_sources=int(torch.unique(got[1]).numel()), sample_seeds=small, sample_equals_host=same,
                  model_bytes=model, stream_fraction=model / (ms * 1e-3) / STREAM_RATE, ms_with_scale=ms + ms_c))

        # ---- the yardsticks ----
        run = lambda: _capi.sample_neighbors(csr, seeds, k, False, 7)
        nms, nbest = timeit(run)
        ptr, src, _ = run()
        ns_distinct = int(torch.unique(src[:int(ptr[-1])]).numel())
        emit(dict(case="sample_neighbors", seeds=n, ms=nms, ms_min=nbest, seeds_per_s=n / (nms * 1e-3),
                  kept=int(ptr[-1]), distinct_sources=ns_distinct, labor_distinct_sources=labor_distinct,
                  ratio_labor_over_neighbors_distinct=labor_distinct / max(ns_distinct, 1),
                  ratio_labor_over_neighbors_ms=lines[-3]["ms"] / nms))

        starts = indptr[:-1][seeds.long()].long()

        def torch_labor():
            r = torch.rand(nodes, device=dev)
            offs = torch.zeros(n + 1, dtype=torch.long, device=dev)
            offs[1:] = torch.cumsum(d, 0)
            total = int(offs[-1])
            pos = torch.repeat_interleave(starts - offs[:-1], d, output_size=total) + torch.arange(total, device=dev)
            nbr = indices[pos]
            thr = torch.repeat_interleave((k / d.clamp(min=1).double()).float(), d, output_size=total)
            keep = r[nbr.long()] < thr
            kept_ptr = torch.zeros(n + 1, dtype=torch.long, device=dev)
            if total:     # kept entries up to the end of every row (an empty row repeats the count before it)
                kept_ptr[1:] = torch.where(offs[1:] > 0, torch.cumsum(keep, 0)[(offs[1:] - 1).clamp(min=0)], 0)
            return kept_ptr, nbr[keep], pos[keep]

        tms, tbest = timeit(torch_labor)
        t_kept = int(torch_labor()[1].numel())
        emit(dict(case="torch_labor", seeds=n, ms=tms, ms_min=tbest, kept=t_kept, ratio_torch_over_kernel=tms / lines[-4]["ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--fanout", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--sample", type=int, default=2000, help="seeds the host function repeats for the comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_labor needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []
    # the C2 shape (mean degree 25: 16 lanes per row), then the same edges over 1 / 8 of the nodes (mean degree 200: a
    # wavefront per row) at the largest number of seeds, so that each group width of the kernels has a workload
    bench_graph(args, dev, "c2", args.nodes, args.seeds, lines)
    bench_graph(args, dev, "dense", max(1, args.nodes // 8), [max(args.seeds)], lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
