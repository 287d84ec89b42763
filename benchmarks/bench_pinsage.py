#!/usr/bin/env python
"""PinSAGE neighbour-selection timings (csrc/pinsage.hip) with the HIP-event protocol of benchmarks/bench_ops.py: medians
of 10 calls after 3 warm-up calls, one JSON line per case.

    python benchmarks/bench_pinsage.py [--segments 100000] [--out profiles/r11/pinsage.jsonl]

Cases:
  * the selection alone (`_capi.select_pinsage_neighbors_padded`: output allocation + one kernel launch, and
    `_capi.select_pinsage_neighbors`: + scan, one read of the total, compaction) at `--segments` segments of
    S in {30, 600, 4096} samples, k = 10, int32 and int64 ids.  A segment's ids are drawn with a cubic skew from a pool
    of 4 S ids of its own and 10 % of them are -1 (walks that died);
  * the whole sampler (`RandomWalkNeighborSampler`: walks + column slice + selection + the result graph) on the C2-shaped
    graph of benchmarks/bench_random_walk.py, the reference's documented setting 200 walks x 3 traversals, 10 neighbours;
  * in the same run the baseline: the same rule as a torch composition (row sort, unique_consecutive with counts on
    segment-tagged keys, a second sort on (segment, count, id), rank < k), checked for equality with the kernel's result
    before it is timed;
  * `control`: an operator this file's subject does not touch (g-SpMM through `sparse.spmm`), for the run's noise.

`gb_per_s` is the BYTE MODEL over the median time: num_dst * S * i read, plus what is written (at most 3 * num_dst * k * i;
the padded form writes 2 * num_dst * k' * i + 2 * num_dst * i) — bytes the algorithm needs, not counter readings.
`stream_fraction` compares it with 7.1 TB/s, the read-only streaming peak measured for this project (README.md).
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
from dgl_amd import _capi, sampling  # noqa: E402
from dgl_amd import sparse as dglsp  # noqa: E402
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


def torch_select(src, dst, S, k):
    """The rule as a torch composition, for ids below 2^32 and fewer than 2^17 segments; int64 inside."""
    n = src.shape[0] // S
    rows = src.view(n, S).long().sort(dim=1).values
    seg = torch.arange(n, device=src.device).unsqueeze(1).expand(n, S)
    keep = rows >= 0
    key, cnt = torch.unique_consecutive((seg[keep] << 32) | rows[keep], return_counts=True)   # (segment, id) ascending
    seg_u, ids = key >> 32, key & 0xFFFFFFFF
    order = torch.argsort((seg_u << 45) | ((S - cnt) << 32) | (0xFFFFFFFF - ids))              # count, id descending
    seg_u, ids, cnt = seg_u[order], ids[order], cnt[order]
    first = torch.searchsorted(seg_u, torch.arange(n, device=src.device))
    top = torch.arange(seg_u.shape[0], device=src.device) - first[seg_u] < k
    d = dst.view(n, S)[:, 0].long()
    return ids[top].to(src.dtype), d[seg_u[top]].to(src.dtype), cnt[top].to(src.dtype)


def make_traces(n, S, idtype, gen, dev):
    pool = 4 * S
    ids = (torch.rand((n, S), device=dev, generator=gen) ** 3 * pool).long()
    ids += (torch.arange(n, device=dev) * 7919 % 1_000_003).unsqueeze(1)          # every segment's own id range
    ids[torch.rand((n, S), device=dev, generator=gen) < 0.1] = -1
    dst = torch.arange(n, device=dev).repeat_interleave(S)
    return ids.reshape(-1).to(idtype), dst.to(idtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="*", default=[30, 600, 4096])
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--seeds", type=int, default=10_000, help="seed nodes of the whole-sampler case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pinsage needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    lines = []

    def emit(rec):
        rec.update(gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def control(tag):
        n = 100_000
        cg = torch.Generator().manual_seed(0)
        A = dglsp.from_coo(torch.randint(0, n, (n * 10,), generator=cg).to(dev), torch.randint(0, n, (n * 10,), generator=cg).to(dev),
                           torch.randn(n * 10, generator=cg).to(dev), (n, n))
        x = torch.randn(n, 64, device=dev)
        ms, best = timeit(lambda: dglsp.spmm(A, x))
        emit(dict(case="control spmm uniform n=%d F=64 (%s)" % (n, tag), ms=ms, ms_min=best))

    control("start")
    n, k = args.segments, args.k
    for idtype in (torch.int32, torch.int64):
        i = 4 if idtype == torch.int32 else 8
        for S in args.sizes:
            src, dst = make_traces(n, S, idtype, gen, dev)
            kp = min(k, S)
            got = _capi.select_pinsage_neighbors(src, dst, S, k)
            want = torch_select(src, dst, S, k)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), "the torch composition and the kernel disagree"
            kept = got[0].shape[0]
            read = n * S * i
            for case, fn, written in (
                    ("select_padded", lambda: _capi.select_pinsage_neighbors_padded(src, dst, S, k), (2 * n * kp + 2 * n) * i),
                    ("select_compact", lambda: _capi.select_pinsage_neighbors(src, dst, S, k), 3 * kept * i),
                    ("torch_composition", lambda: torch_select(src, dst, S, k), 3 * kept * i)):
                ms, best = timeit(fn)
                rate = (read + written) / (ms * 1e-3)
                emit(dict(case=case, idtype=str(idtype).split(".")[-1], segments=n, S=S, k=k, kept=kept, ms=ms, ms_min=best,
                          bytes_read=read, bytes_written=written, gb_per_s=rate / 1e9, stream_fraction=rate / STREAM_RATE))
            del src, dst, got, want
    # the whole sampler on the C2-shaped graph (out-edge CSR -> COO -> graph; the formats are built before the timed region)
    c = synth_csr(args.nodes, args.nodes, args.edges, "U", device=dev, with_eids=False, sort_cols=False)
    deg = (c["indptr"][1:] - c["indptr"][:-1]).long()
    rows = torch.arange(args.nodes, device=dev, dtype=c["indices"].dtype).repeat_interleave(deg)
    g = dgl_amd.graph((rows, c["indices"]), num_nodes=args.nodes)
    walks, traversals = 200, 3
    sampler = sampling.RandomWalkNeighborSampler(g, traversals, 0.5, walks, k)
    seeds = torch.randint(0, args.nodes, (args.seeds,), device=dev, generator=gen).to(g.idtype)
    S = walks * traversals

    def torch_sampler():
        paths, _ = sampling.random_walk(g, seeds.repeat_interleave(walks), metapath=sampler.full_metapath,
                                        restart_prob=sampler.restart_prob, seed=7)
        src = paths[:, 1:].reshape(-1)
        return torch_select(src, paths[:, 0].repeat_interleave(traversals), S, k)

    f = sampler(seeds, seed=7)
    u, v = f.edges()
    want = torch_sampler()
    assert torch.equal(u, want[0]) and torch.equal(v, want[1]) and torch.equal(f.edata["weights"], want[2])
    i = 4 if g.idtype == torch.int32 else 8
    for case, fn in (("sampler", lambda: sampler(seeds, seed=7)), ("sampler_torch_selection", torch_sampler),
                     ("walks_only", lambda: sampling.random_walk(g, seeds.repeat_interleave(walks), metapath=sampler.full_metapath,
                                                                 restart_prob=sampler.restart_prob, seed=7))):
        ms, best = timeit(fn)
        emit(dict(case=case, idtype=str(g.idtype).split(".")[-1], seeds=args.seeds, walks=walks, traversals=traversals, k=k,
                  nodes=args.nodes, edges=args.edges, edges_out=int(u.shape[0]), ms=ms, ms_min=best,
                  seeds_per_s=args.seeds / (ms * 1e-3)))
    control("end")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
