#!/usr/bin/env python
"""select_topk timings (csrc/topk.hip): whole calls on the wall clock, each against three yardsticks in the same run.

    python benchmarks/bench_select_topk.py [--out profiles/r20/select_topk.jsonl]

Shapes: the C2-shaped graph (ogbn-products size, uniform, int32 ids, fp32 weights, the in-edge CSR with its edge-id map)
and the same edges over an eighth of the nodes (mean degree 202); k in {5, 10, 50}; all nodes and 100 000 seeds.

Yardsticks:

  weighted   dgla_sample_neighbors_weighted without replacement at fanout k: the same reads, but once per pick.  Its
             picks are random, so only the time is compared.
  torch      the rule as a torch composition: the frontier of the seeds expanded, three stable sorts (edge id, weight,
             row), rank < k.  Its result is asserted identical.
  host       what the reference forces on a GPU graph: CSR and weights to the CPU, dgla_select_topk_host there, the picks
             back.  Its result is asserted identical.

Every time is wall clock around a device synchronisation: the median (and minimum) of --reps calls after --warm (the host
path: --host-reps calls, no warm-up; it is seconds long).  Kernel-only times are not taken.

Byte model of the device call, written down here: every entry of a selected row costs one edge id (id bytes, streamed) and
one weight gather (4 bytes, one request); every pick is written twice (neighbour and edge id) and gathers its neighbour:

    model_bytes = E_sel x (id + 4) + picks x 3 x id        requests = E_sel

``gather_fraction`` = requests / call time / 55.5 G requests/s and ``stream_fraction`` = model_bytes / call time /
7.1 TB/s: the whole call over the rates measured on this pool, not a kernel's share of peak.
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

STREAM_RATE = 7.1e12
GATHER_RATE = 55.5e9


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


def torch_rule(fmt, w, seeds, k):
    """(indptr, nbr, eids) of the rule as a torch composition: a segmented sort of the frontier."""
    indptr, indices, data = fmt
    s = seeds.long()
    lo = indptr[s].long()
    deg = indptr[s + 1].long() - lo
    start = torch.cumsum(deg, 0) - deg
    total = int(deg.sum())
    row = torch.repeat_interleave(torch.arange(s.shape[0], device=s.device), deg, output_size=total)
    pos = torch.arange(total, device=s.device) - start[row] + lo[row]
    e = data[pos].long()
    o = torch.argsort(e, stable=True)
    o = o[torch.argsort(w[e[o]], descending=True, stable=True)]
    o = o[torch.argsort(row[o], stable=True)]
    keep = (torch.arange(total, device=s.device) - start[row]) < k        # (row[o] == row: the last sort is by row)
    o = o[keep]
    picks = torch.clamp(deg, max=k)
    out_indptr = torch.cat([picks.new_zeros(1), torch.cumsum(picks, 0)]).to(indptr.dtype)
    return out_indptr, indices[pos[o]], data[pos[o]]


def host_path(fmt, cols, w, seeds, k):
    """What the reference does for a GPU graph: everything to the CPU, the rule there, the picks back."""
    csr = _capi.host_csr(*[t.cpu() for t in fmt], cols)
    out = _capi.select_topk_host(csr, w.cpu(), seeds.cpu(), k)
    return tuple(t.to(w.device) for t in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--seeds", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--yard-reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select_topk needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []
    gen = torch.Generator(device=dev).manual_seed(20)
    E = args.edges
    w = torch.rand(E, device=dev, generator=gen) + 0.125          # positive: the weighted sampler can pick every edge
    for graph, N in (("c2", args.nodes), ("c2_eighth", max(1, args.nodes // 8))):
        u = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
        v = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
        g = dgl.graph((u, v), num_nodes=N, idtype=torch.int32, device=dev)
        fmt = g._graph.relations[0].csc()
        del u, v
        csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], N)
        deg = (fmt[0][1:] - fmt[0][:-1]).long()
        every = torch.arange(N, device=dev, dtype=torch.int32)
        some = torch.randperm(N, device=dev, generator=gen)[: min(args.seeds, N)].to(torch.int32)
        ws = torch.empty(_capi.select_topk_workspace_bytes(torch.int32, N), dtype=torch.uint8, device=dev)
        for which, seeds in (("all", every), ("seeds", some)):
            e_sel = int(deg[seeds.long()].sum())
            for k in (5, 10, 50):
                ours = lambda: _capi.select_topk(csr, w, seeds, k, workspace=ws)
                got = ours()
                total = int(got[0][-1])
                want_t = torch_rule(fmt, w, seeds, k)
                want_h = host_path(fmt, N, w, seeds, k)
                for want in (want_t, want_h):
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1][:total], want[1]) \
                        and torch.equal(got[2][:total], want[2])
                del want_t, want_h, got
                ms, best = timeit(ours, args.reps, args.warm)
                wms, wbest = timeit(lambda: _capi.sample_neighbors_weighted(csr, w, seeds, k, False, 20), args.reps, args.warm)
                tms, tbest = timeit(lambda: torch_rule(fmt, w, seeds, k), args.yard_reps, 1)
                hms, hbest = timeit(lambda: host_path(fmt, N, w, seeds, k), args.host_reps, 0)
                model = e_sel * (4 + 4) + total * 3 * 4
                rec = dict(case="%s_%s_k%d" % (graph, which, k), nodes=N, edges=E, seeds=int(seeds.shape[0]), k=k, id_bytes=4,
                           weight="fp32", entries_of_selected_rows=e_sel, picks=total, ms=ms, ms_min=best,
                           weighted_ms=wms, weighted_ms_min=wbest, torch_ms=tms, torch_ms_min=tbest, host_path_ms=hms,
                           host_path_ms_min=hbest, ratio_weighted_over_device=wms / ms, ratio_torch_over_device=tms / ms,
                           ratio_host_over_device=hms / ms, identical_to_torch=True, identical_to_host=True,
                           model_bytes=model, gather_fraction=e_sel / (ms * 1e-3) / GATHER_RATE,
                           stream_fraction=model / (ms * 1e-3) / STREAM_RATE, kernel_only_ms=None,
                           gpu=torch.cuda.get_device_name(0))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
        del g, fmt, csr
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
