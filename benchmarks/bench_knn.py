#!/usr/bin/env python
"""Point-cloud graph timings (csrc/knn.hip) with the HIP-event protocol of bench_labor.py: every case warmed up, then
timed call by call between events on the current stream; the median and the minimum are reported.

    python benchmarks/bench_knn.py [--out profiles/r15/knn.jsonl] [--reps 30]

Shapes (the ones EdgeConv / DGCNN and PointNet++ run):
  clouds_d3 / clouds_d64   32 clouds x 1024 points, D = 3 / 64, k = 20
  big_d3                   one cloud of 100 000 points, D = 3, k = 16
  fps                      farthest_point_sampler, 32 x 1024 x 3 -> 256

Cases per k-NN shape, all in the same run:
  knn            `dgl_amd.knn` (the self-query; one launch, the (2, k N) id tensor)
  knn_graph      `dgl_amd.knn_graph` (the same launch + building the DGLGraph)
  torch_topk     the composition a user has without the kernel, the reference's "bruteforce-blas": `torch.cdist` + `topk`
                 per cloud (batched; the big cloud in blocks of 8192 query rows, since the full matrix is 40 GB)
`same_sets` is the fraction of queries whose neighbour SET equals torch's (ties and cdist's own rounding aside it is 1);
`host_equal` compares the first 64 queries of the first cloud with dgla_knn_host, bit for bit.

Model, counted from the shapes, not from counters: pairs = sum over clouds of n^2; fma = pairs * Dp with
Dp = D rounded up to the kernel's column chunk (4 for D <= 4, else 16); tile_bytes = (query tiles of 64) * n * D * 4, the
data-row bytes all workgroups read (from L2 after the first touch); `fma_rate` = fma / call time and `fma_fraction` =
that over the fp32 vector FMA rate (256 CUs * 128 lanes * 2.4 GHz = 78.6 T fma/s).  Whole calls, not kernel shares."""
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
from dgl_amd.geometry import farthest_point_sampler  # noqa: E402

FMA_RATE = 256 * 128 * 2.4e9


def timeit(fn, reps, warm=3):
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


def torch_topk(x, k, block=8192):
    """(B, N, k) neighbour ids inside each cloud: cdist + topk, query rows in blocks when the matrix would not fit."""
    B, N, _ = x.shape
    if N <= block:
        return torch.topk(torch.cdist(x, x), k, dim=-1, largest=False)[1]
    out = [torch.topk(torch.cdist(x[:, lo:lo + block], x), k, dim=-1, largest=False)[1] for lo in range(0, N, block)]
    return torch.cat(out, dim=1)


def torch_fps(pos, npoints, start):
    """The textbook loop in torch, batched over the clouds: 3 launches and more per sample."""
    B, N, _ = pos.shape
    mind = torch.full((B, N), float("inf"), device=pos.device, dtype=pos.dtype)
    out = torch.empty((B, npoints), dtype=torch.int64, device=pos.device)
    cur = start.clone()
    rows = torch.arange(B, device=pos.device)
    for t in range(npoints):
        out[:, t] = cur
        d = ((pos - pos[rows, cur].unsqueeze(1)) ** 2).sum(-1)
        mind = torch.minimum(mind, d)
        cur = mind.argmax(dim=1)
    return out


def bench_knn(name, B, N, D, k, reps, dev, emit):
    gen = torch.Generator(device=dev).manual_seed(15)
    x = torch.randn(B, N, D, device=dev, generator=gen)
    flat, segs = x.reshape(B * N, D), [N] * B
    C = 4 if D <= 4 else 16
    pairs = B * N * N
    model = dict(pairs=pairs, fma=pairs * ((D + C - 1) // C * C), tile_bytes=B * ((N + 63) // 64) * N * D * 4,
                 out_bytes=B * N * k * 16)
    base = dict(shape=name, clouds=B, points=N, dim=D, k=k, **model)

    run = lambda: dgl_amd.knn(k, flat, segs)
    ms, best = timeit(run, reps)
    got = run()[1].view(B, N, k) - (torch.arange(B, device=dev) * N).view(B, 1, 1)
    want = torch_topk(x, k)
    same = float((torch.sort(got, -1)[0] == torch.sort(want, -1)[0]).all(-1).float().mean())
    h = _capi.knn_host(x[0].cpu().contiguous(), [0, N], k, x[0, :64].cpu().contiguous(), [0, 64], with_dist=True)
    d = _capi.knn(x[0].contiguous(), [0, N], k, x[0, :64].contiguous(), [0, 64], with_dist=True)
    host_equal = bool(torch.equal(h[0], d[0].cpu()) and h[1].numpy().tobytes() == d[1].cpu().numpy().tobytes())
    emit(dict(base, case="knn", ms=ms, ms_min=best, fma_rate=model["fma"] / (ms * 1e-3),
              fma_fraction=model["fma"] / (ms * 1e-3) / FMA_RATE, same_sets=same, host_equal=host_equal))
    knn_ms = ms
    ms, best = timeit(lambda: dgl_amd.knn_graph(x if B > 1 else flat, k), reps)
    emit(dict(base, case="knn_graph", ms=ms, ms_min=best))
    ms, best = timeit(lambda: torch_topk(x, k), max(3, reps // 2))
    emit(dict(base, case="torch_topk", ms=ms, ms_min=best, matrix_bytes=B * N * min(N, 8192) * 4,
              ratio_torch_over_knn=ms / knn_ms))


def bench_fps(B, N, D, npoints, reps, dev, emit):
    gen = torch.Generator(device=dev).manual_seed(16)
    pos = torch.rand(B, N, D, device=dev, generator=gen)
    start = torch.zeros(B, dtype=torch.int64, device=dev)
    base = dict(shape="fps", clouds=B, points=N, dim=D, npoints=npoints, fma=B * N * npoints * D)
    run = lambda: farthest_point_sampler(pos, npoints, start_idx=0)
    ms, best = timeit(run, reps)
    got = run()
    same = float((got == torch_fps(pos, npoints, start)).all(-1).float().mean())
    host_equal = bool(torch.equal(got[:2].cpu(), _capi.fps_host(pos[:2].cpu().contiguous(), npoints, start[:2].cpu())))
    emit(dict(base, case="fps", ms=ms, ms_min=best, us_per_sample=ms * 1e3 / npoints, same_as_torch_loop=same,
              host_equal=host_equal))
    fps_ms = ms
    ms, best = timeit(lambda: torch_fps(pos, npoints, start), max(3, reps // 2))
    emit(dict(base, case="torch_fps_loop", ms=ms, ms_min=best, ratio_torch_over_fps=ms / fps_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "knn.jsonl"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--big", type=int, default=100000, help="points of the single large cloud")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        rec.update(gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    bench_knn("clouds_d3", 32, 1024, 3, 20, args.reps, dev, emit)
    bench_knn("clouds_d64", 32, 1024, 64, 20, args.reps, dev, emit)
    bench_knn("big_d3", 1, args.big, 3, 16, args.reps, dev, emit)
    bench_fps(32, 1024, 3, 256, args.reps, dev, emit)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
