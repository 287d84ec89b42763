#!/usr/bin/env python
"""Negative-sampling timings (csrc/negative_sampling.hip) with the HIP-event protocol of benchmarks/bench_random_walk.py:
medians of 10 calls after 3 warm-up calls, timed on the stream with events.

    python benchmarks/bench_negative_sampling.py [--samples 1000000] [--out profiles/r13/negative_sampling.jsonl]

Graph: the C2-shaped graph of tests/graphgen.py (ogbn-products size, uniform, int32 ids) as an out-edge CSR without an
edge-id map.  Cases:

  membership_build   dgla_csr_sorted_columns, once per relation (the list node2vec_random_walk shares)
  negative_sample    `_capi.negative_sample` (output + workspace allocation and every launch), replace on and off, with the
                     slots the public function would draw; `sample_equals_host` compares the first --sample slots' worth
                     of the result with dgla_negative_sample_host
  torch_sampling     the same task composed from torch: randint + searchsorted in the sorted edge keys (sorted ONCE,
                     outside the timing) + boolean selection (+ unique without replacement) — the yardstick
  has_edges_kernel   `_capi.csr_has_edges` at --pairs pairs, half of them edges, on int32 id tensors prepared in advance:
                     the kernel call alone (output allocation + one launch)
  has_edges_between  `DGLGraph.has_edges_between` on a GPU graph holding the same edges, same pairs: the method as a user
                     calls it (id conversion, the relation's cached csr struct and membership list, the kernel call)
  torch_has_edges    the lines DGLGraph.has_edges_between ran before (a sort of all edge keys per call) — the yardstick

`requests_per_slot` is a model, not a counter: a slot makes `trials` trials — the expected number, computed from the
graph's density as sum over t < T of reject^t with reject = nnz / (R C) + 1 / R — each one gather of the row's indptr
pair and a bisection of ceil(log2(deg + 1)) gathers in the membership list; the outputs are streamed.
`model_slots_per_s` = 55.5 G requests/s over that number, `model_fraction` the measured share of it.  55.5 G requests/s
is the rate the g-SpMM merge kernel sustains, the figure the other sampling benchmarks use: it is not a peak
measured for this access pattern.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dgl_amd  # noqa: E402
from dgl_amd import _capi  # noqa: E402
from dgl_amd.sampling import NEGATIVE_SAMPLING_TRIALS, _negative_redundancy  # noqa: E402
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
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--sample", type=int, default=100000, help="slots the host function repeats for the comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_negative_sampling needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    g = synth_csr(args.nodes, args.nodes, args.edges, "U", device=dev, with_eids=False, sort_cols=False)
    indptr, indices = g["indptr"].to(torch.int32), g["indices"].to(torch.int32)
    nnz = int(indices.shape[0])
    csr = _capi.make_csr(indptr, indices, None, args.nodes)
    deg = (indptr[1:] - indptr[:-1]).long()
    lines = []

    def emit(rec):
        rec.update(nodes=args.nodes, edges=nnz, gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    ms, best = timeit(lambda: _capi.csr_sorted_columns(csr))
    emit(dict(case="membership_build", ms=ms, ms_min=best, edges_per_s=nnz / (ms * 1e-3)))
    member = _capi.csr_sorted_columns(csr)
    h_csr = _capi.host_csr(indptr.cpu(), indices.cpu(), None, args.nodes)
    h_member = member.cpu()

    # ---- sampling ----
    k = args.samples
    n_slots = int(k * (1 + _negative_redundancy(k, nnz, args.nodes * args.nodes)))
    T = NEGATIVE_SAMPLING_TRIALS
    # edge keys of the torch composition, sorted once
    row = torch.repeat_interleave(torch.arange(args.nodes, device=dev), deg, output_size=nnz)
    keys = torch.sort(row * args.nodes + indices.long())[0]
    # the model's bisection depth: a uniform source node
    depth = float(torch.ceil(torch.log2(deg.double() + 1)).mean())
    for replace in (True, False):
        run = lambda: _capi.negative_sample(csr, member, n_slots, k, T, True, replace, rng_seed=7)
        ms, best = timeit(run)
        src, dst, count = run()
        small = min(args.sample, n_slots)
        hs, hd, hc = _capi.negative_sample_host(h_csr, h_member, small, small, T, True, replace, rng_seed=7)
        hc = int(hc)
        # the first `small` slots give a prefix of the result (slot order), as long as the request is not cut before it
        same = bool(hc <= int(count) and torch.equal(hs[:hc], src[:hc].cpu()) and torch.equal(hd[:hc], dst[:hc].cpu()))
        reject = nnz / (args.nodes * args.nodes) + 1.0 / args.nodes       # an edge or a self-loop
        trials = sum(reject ** t for t in range(T))                        # expected trials of a slot, at most T
        req = trials * (1.0 + depth)
        rate = n_slots / (ms * 1e-3)
        emit(dict(case="negative_sample", replace=replace, samples=k, n_slots=n_slots, trials=T, count=int(count), ms=ms,
                  ms_min=best, slots_per_s=rate, sample_slots=small, sample_equals_host=same, requests_per_slot=req,
                  model_slots_per_s=REQUEST_RATE / req, model_fraction=rate * req / REQUEST_RATE,
                  workspace_bytes=int(_capi.LIB.dgla_negative_sample_workspace_bytes(32, n_slots))))

        def torch_run():
            u = torch.randint(0, args.nodes, (n_slots,), device=dev)
            v = torch.randint(0, args.nodes, (n_slots,), device=dev)
            want = u * args.nodes + v
            at = torch.searchsorted(keys, want).clamp(max=nnz - 1)
            ok = (keys[at] != want) & (u != v)
            want = want[ok]
            if not replace:
                want = torch.unique(want)
            want = want[:k]
            return want // args.nodes, want % args.nodes

        tms, tbest = timeit(torch_run)
        emit(dict(case="torch_sampling", replace=replace, samples=k, n_slots=n_slots, ms=tms, ms_min=tbest,
                  ratio_torch_over_kernel=tms / ms))

    # ---- the edge lookup ----
    n = args.pairs
    gen = torch.Generator(device=dev).manual_seed(1)
    pick = torch.randint(0, nnz, (n // 2,), device=dev, generator=gen)
    u = torch.cat([row[pick].to(torch.int32), torch.randint(0, args.nodes, (n - n // 2,), device=dev, generator=gen).to(torch.int32)])
    v = torch.cat([indices[pick], torch.randint(0, args.nodes, (n - n // 2,), device=dev, generator=gen).to(torch.int32)])
    run = lambda: _capi.csr_has_edges(csr, member, u, v)
    ms, best = timeit(run)
    got = run()
    src_all, dst_all = row.to(torch.int32), indices
    g = dgl_amd.graph((src_all, dst_all), num_nodes=args.nodes, idtype=torch.int32, device=dev)
    method = lambda: g.has_edges_between(u, v)
    method()                    # first use: the relation's CSR and membership list
    mms, mbest = timeit(method)
    method_same = bool(torch.equal(method(), got))

    def torch_has_edges():      # DGLGraph.has_edges_between before the kernel
        n_dst = max(args.nodes, 1)
        key = torch.sort(src_all.long() * n_dst + dst_all.long())[0]
        want = u.long() * n_dst + v.long()
        at = torch.searchsorted(key, want).clamp(max=key.numel() - 1)
        return key[at] == want

    tms, tbest = timeit(torch_has_edges)
    same = bool(torch.equal(got, torch_has_edges()))
    req = 1.0 + float(torch.ceil(torch.log2(deg[u.long()].double() + 1)).mean())
    emit(dict(case="has_edges_kernel", pairs=n, ms=ms, ms_min=best, pairs_per_s=n / (ms * 1e-3), hits=int(got.sum()),
              equals_torch=same, requests_per_pair=req, model_pairs_per_s=REQUEST_RATE / req,
              model_fraction=n / (ms * 1e-3) * req / REQUEST_RATE))
    emit(dict(case="has_edges_between", pairs=n, ms=mms, ms_min=mbest, pairs_per_s=n / (mms * 1e-3),
              equals_kernel=method_same))
    emit(dict(case="torch_has_edges", pairs=n, ms=tms, ms_min=tbest, ratio_torch_over_kernel=tms / ms,
              ratio_torch_over_method=tms / mms))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
