#!/usr/bin/env python
"""Per-edge-type neighbour sampling timings (csrc/etype.hip): whole calls on the wall clock, each against its yardsticks
in the same run.

    python benchmarks/bench_etype.py [--out profiles/r22/etype.jsonl]

Shape: the C2-shaped graph (ogbn-products size, uniform, int32 ids, the in-edge CSR with its edge-id map), its edge ids cut
into T in {4, 64} equal types, rows sorted by type.  All nodes and 100 000 seeds, fan-out 5 and 10 per type, without
replacement, against

  hetero   dgl_amd.sampling.sample_neighbors with a dict fan-out on the equivalent heterograph (one relation per type);
  biased   dgla_sample_neighbors_biased at the same T with equal biases and fan-out f * T: one draw over all types;
  host     what the reference forces on a GPU graph: the CSR to the CPU, dgla_sample_etype_neighbors_host there, the picks
           back.  Taken for the 100 000-seed cases only.

Also timed: the one-off sort of etype_sorted=False (per-edge type + tag sort).  The device result is asserted identical to
the host twin on a sample of --check seeds in every case.  Every time is wall clock around a device synchronisation: the
median (and minimum) of --reps calls after --warm.  Kernel times alone are not taken.
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


def host_path(fmt, cols, off, fanout, seeds):
    csr = _capi.host_csr(*[t.cpu() for t in fmt], cols)
    table = _capi.EtypeTable(off)
    out = _capi.sample_etype_neighbors_host(csr, table, table.fanouts(fanout), seeds.cpu(), False, 22)
    return tuple(t.to(seeds.device) for t in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--seeds", type=int, default=100000)
    ap.add_argument("--check", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_etype needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(rec):
        rec["gpu"] = name
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    gen = torch.Generator(device=dev).manual_seed(22)
    N, E = args.nodes, args.edges
    u = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
    v = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
    fmt = dgl.graph((u, v), num_nodes=N, idtype=torch.int32, device=dev)._graph.relations[0].csc()
    csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], N)
    every = torch.arange(N, device=dev, dtype=torch.int32)
    some = torch.randperm(N, device=dev, generator=gen)[: min(args.seeds, N)].to(torch.int32)
    ws = torch.empty(_capi.sample_etype_neighbors_workspace_bytes(torch.int32, N), dtype=torch.uint8, device=dev)
    bws = torch.empty(_capi.sample_neighbors_biased_workspace_bytes(torch.int32, N), dtype=torch.uint8, device=dev)
    for T in (4, 64):
        off = [E * t // T for t in range(T + 1)]
        table = _capi.EtypeTable(off, dev)

        def sort_once():
            tag = torch.bucketize(torch.arange(E, device=dev), table.offsets[1:], right=True)
            return _capi.sort_csr_by_tag(csr, tag, T)

        srt = sort_once()
        ms, best = timeit(sort_once, 3, 1)
        emit(dict(case="sort_T%d" % T, nodes=N, edges=E, T=T, ms=ms, ms_min=best, kernel_only_ms=None))
        sorted_fmt = (fmt[0], srt[0], srt[1])
        sorted_csr = _capi.make_csr(*sorted_fmt, N)
        bias = torch.ones(T, device=dev)
        hg = dgl.heterograph({("_N", "e%d" % t, "_N"): (u[off[t]:off[t + 1]], v[off[t]:off[t + 1]]) for t in range(T)},
                             num_nodes_dict={"_N": N}, idtype=torch.int32, device=dev)
        for which, seeds in (("all", every), ("seeds", some)):
            for f in (5, 10):
                fan = table.fanouts([f] * T)
                cap = int(seeds.shape[0]) * f * T
                ours = lambda: _capi.sample_etype_neighbors(sorted_csr, table, fan, seeds, False, 22, ws=ws, capacity=cap)
                sample = seeds[: args.check].contiguous()
                got = _capi.sample_etype_neighbors(sorted_csr, table, fan, sample, False, 22)
                want = host_path(sorted_fmt, N, off, [f] * T, sample)
                assert all(torch.equal(a[: b.shape[0]], b) for a, b in zip(got, want))
                picks = int(ours()[0][-1])
                ms, best = timeit(ours, args.reps, args.warm)
                bms, bbest = timeit(lambda: _capi.sample_neighbors_biased(sorted_csr, srt[2], bias, seeds, f * T, False, 22, ws=bws),
                                    args.reps, args.warm)
                hetero = lambda: dgl.sampling.sample_neighbors(hg, {"_N": seeds}, {"e%d" % t: f for t in range(T)}, seed=22)
                tms, tbest = timeit(hetero, 3, 1)
                hms = None
                if which == "seeds":
                    hms, _ = timeit(lambda: host_path(sorted_fmt, N, off, [f] * T, seeds), 1, 0)
                emit(dict(case="sample_%s_T%d_f%d" % (which, T, f), nodes=N, edges=E, T=T, fanout=f, seeds=int(seeds.shape[0]),
                          picks=picks, ms=ms, ms_min=best, biased_ms=bms, biased_ms_min=bbest, hetero_ms=tms, hetero_ms_min=tbest,
                          host_path_ms=hms, ratio_biased_over_device=bms / ms, ratio_hetero_over_device=tms / ms,
                          ratio_host_over_device=None if hms is None else hms / ms,
                          identical_to_host_on_sample=int(sample.shape[0]), kernel_only_ms=None))
        del srt, sorted_csr, sorted_fmt, hg
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
