#!/usr/bin/env python
"""Tag sort and tag-biased sampling timings (csrc/biased.hip): whole calls on the wall clock, each against its yardsticks
in the same run.

    python benchmarks/bench_biased.py [--out profiles/r21/biased.jsonl]

Shapes: the C2-shaped graph (ogbn-products size, uniform, int32 ids, the in-edge CSR with its edge-id map) and the same
edges over an eighth of the nodes (mean degree 202); uniform random edge tags, T in {4, 64}; bias rising from 0.5 to 2.

Sort (C2-shaped graph): dgla_sort_csr_by_tag against the rule as a torch composition, a stable sort on (row, tag) and a
bincount; its result is asserted identical.

Sampler (both graphs, all nodes and 100 000 seeds, fanout in {5, 10, 50}, without replacement) against

  weighted   dgla_sample_neighbors_weighted with prob = bias[tag] at the same fanout: the same law, every edge of the row
             read once per pick;
  uniform    dgla_sample_neighbors at the same fanout: what a pick costs without any weight;
  host       what the reference forces on a GPU graph: the sorted CSR and the offsets to the CPU,
             dgla_sample_neighbors_biased_host there, the picks back.  Taken for the 100 000-seed cases only (the host twin
             runs the lane scan in software and is seconds long).

The device result is asserted identical to the host twin on a sample of --check seeds in every case.  Every time is wall
clock around a device synchronisation: the median (and minimum) of --reps calls after --warm.  Kernel-only times are not
taken.
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
from dgl_amd import _capi  # noqa: E402
from tests.graphgen import C2_EDGES, C2_NODES  # noqa: E402


def timeit(fn_, reps, warm):
    for _ in range(warm):
        fn_()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn_()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def torch_sort(fmt, tag, T):
    """(indices, data, tag_pos) of the sort rule as a torch composition."""
    indptr, indices, data = fmt
    n = indptr.shape[0] - 1
    row = torch.repeat_interleave(torch.arange(n, device=indptr.device), (indptr[1:] - indptr[:-1]).long(),
                                  output_size=indices.shape[0])
    key = row * T + tag[data.long()].long()
    order = torch.argsort(key, stable=True)
    counts = torch.bincount(key, minlength=n * T).reshape(n, T)
    tag_pos = torch.cat([counts.new_zeros(n, 1), torch.cumsum(counts, 1)], 1).to(indptr.dtype)
    return indices[order], data[order], tag_pos


def host_path(indptr, srt, cols, bias, seeds, fanout):
    csr = _capi.host_csr(indptr.cpu(), srt[0].cpu(), srt[1].cpu(), cols)
    out = _capi.sample_neighbors_biased_host(csr, srt[2].cpu(), bias.cpu(), seeds.cpu(), fanout, False, 21)
    return tuple(t.to(bias.device) for t in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--seeds", type=int, default=100000)
    ap.add_argument("--check", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--yard-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_biased needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(rec):
        rec["gpu"] = name
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    gen = torch.Generator(device=dev).manual_seed(21)
    E = args.edges
    for graph, N in (("c2", args.nodes), ("c2_eighth", max(1, args.nodes // 8))):
        u = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
        v = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
        fmt = dgl.graph((u, v), num_nodes=N, idtype=torch.int32, device=dev)._graph.relations[0].csc()
        del u, v
        csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], N)
        every = torch.arange(N, device=dev, dtype=torch.int32)
        some = torch.randperm(N, device=dev, generator=gen)[: min(args.seeds, N)].to(torch.int32)
        ws = torch.empty(_capi.sample_neighbors_biased_workspace_bytes(torch.int32, N), dtype=torch.uint8, device=dev)
        for T in (4, 64):
            tag = torch.randint(0, T, (E,), device=dev, generator=gen, dtype=torch.int32)
            bias = torch.linspace(0.5, 2.0, T, device=dev)
            srt = _capi.sort_csr_by_tag(csr, tag, T)
            if graph == "c2":
                want = torch_sort(fmt, tag, T)
                assert all(torch.equal(a, b) for a, b in zip(srt, want))
                del want
                ms, best = timeit(lambda: _capi.sort_csr_by_tag(csr, tag, T), args.reps, args.warm)
                tms, tbest = timeit(lambda: torch_sort(fmt, tag, T), args.yard_reps, 1)
                emit(dict(case="sort_%s_T%d" % (graph, T), nodes=N, edges=E, T=T, ms=ms, ms_min=best, torch_ms=tms,
                          torch_ms_min=tbest, ratio_torch_over_device=tms / ms, identical_to_torch=True, kernel_only_ms=None))
            sorted_csr = _capi.make_csr(fmt[0], srt[0], srt[1], N)
            prob = bias[tag.long()].contiguous()
            for which, seeds in (("all", every), ("seeds", some)):
                for fanout in (5, 10, 50):
                    ours = lambda: _capi.sample_neighbors_biased(sorted_csr, srt[2], bias, seeds, fanout, False, 21, ws=ws)
                    sample = seeds[: args.check].contiguous()
                    got = _capi.sample_neighbors_biased(sorted_csr, srt[2], bias, sample, fanout, False, 21)
                    want = host_path(fmt[0], srt, N, bias, sample, fanout)
                    assert all(torch.equal(a[: b.shape[0]], b) for a, b in zip(got, want))
                    picks = int(ours()[0][-1])
                    ms, best = timeit(ours, args.reps, args.warm)
                    wms, wbest = timeit(lambda: _capi.sample_neighbors_weighted(csr, prob, seeds, fanout, False, 21), args.reps, args.warm)
                    ums, ubest = timeit(lambda: _capi.sample_neighbors(csr, seeds, fanout, False, 21), args.reps, args.warm)
                    hms = None
                    if which == "seeds":
                        hms, _ = timeit(lambda: host_path(fmt[0], srt, N, bias, seeds, fanout), 1, 0)
                    emit(dict(case="sample_%s_%s_T%d_f%d" % (graph, which, T, fanout), nodes=N, edges=E, T=T, fanout=fanout,
                              seeds=int(seeds.shape[0]), picks=picks, ms=ms, ms_min=best, weighted_ms=wms, weighted_ms_min=wbest,
                              uniform_ms=ums, uniform_ms_min=ubest, host_path_ms=hms, ratio_weighted_over_device=wms / ms,
                              ratio_uniform_over_device=ums / ms, ratio_host_over_device=None if hms is None else hms / ms,
                              identical_to_host_on_sample=int(sample.shape[0]), kernel_only_ms=None))
            del srt, sorted_csr, prob, tag
        del fmt, csr
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
