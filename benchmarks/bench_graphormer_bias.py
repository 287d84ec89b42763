#!/usr/bin/env python
"""Graphormer attention bias timings (csrc/graphormer_bias.hip): the fused operator against the torch composition of
the same formula (``fused=False``: index the edge features with the paths, einsum, divide, embedding) in the same run.

    python benchmarks/bench_graphormer_bias.py [--out profiles/r24/graphormer_bias.jsonl]

Inputs: B = --graphs padded blocks of N x N pairs, N = 32 and 128, taken from ``shortest_dist`` on batched molecule-like
graphs (bench_shortest_dist.py's generator); paths cut or padded to L = 5; d = 16; H = 8 and 32; fp32 and bf16.  The two
routes are asserted equal within the test's bar before anything is timed.

Every time is taken with device events around whole calls that end in a device synchronise, after --warm calls: the
median, minimum and maximum of --reps.  ``fwd`` is the forward under no_grad, ``fwd_bwd`` the forward and the backward
to edge_feat, the path table and the spatial table.

Byte model (what a pass must move; T is read from cache): forward = P (L ids + 1 distance) id bytes + P H values
written; backward = the same ids and distances + P H cotangents read + the tables written.  ``*_stream_fraction`` = that
over the measured time of the whole call over the measured 7.1 TB/s stream rate, not a kernel's share of peak."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

import dgl_amd as dgl  # noqa: E402
from bench_shortest_dist import STREAM_RATE, molecules, timeit  # noqa: E402
from dgl_amd import ops  # noqa: E402

L, D, MAX_DIST = 5, 16, 8


def blocks(graphs, atoms, dev, rng):
    """dist (B, N, N), paths (B, N, N, L) and the edge count of a batch of molecule-like graphs."""
    dists, pathss, edges, chunk = [], [], 0, 8                                    # (all pairs of 8 graphs at a time)
    for _ in range(0, graphs, chunk):
        src, dst = molecules(chunk, atoms, rng)
        n = chunk * atoms
        g = dgl.graph((torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)), num_nodes=n, idtype=torch.int32, device=dev)
        dist, paths = dgl.shortest_dist(g, return_paths=True)
        idx = torch.arange(n, device=dev).reshape(chunk, atoms)
        dists.append(dist[idx[:, :, None], idx[:, None, :]])                        # the diagonal blocks
        paths = paths[idx[:, :, None], idx[:, None, :]]
        if paths.shape[-1] < L:
            paths = torch.nn.functional.pad(paths, (0, L - paths.shape[-1]), value=-1)
        paths = paths[..., :L]
        pathss.append(torch.where(paths >= 0, paths + edges, paths))
        edges += int(src.size)
    return torch.cat(dists).contiguous(), torch.cat(pathss).contiguous(), edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_graphormer_bias needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(24)
    lines = []
    for atoms in (32, 128):
        dist, paths, E = blocks(args.graphs, atoms, dev, rng)
        P = dist.numel()
        for H in (8, 32):
            for dtype in (torch.float32, torch.bfloat16):
                torch.manual_seed(24)
                X, W, S = (torch.randn(shape, device=dev).to(dtype).requires_grad_()
                           for shape in ((E, D), (L * H, D), (MAX_DIST + 2, H)))
                cot = torch.randn(dist.shape + (H,), device=dev).to(dtype)

                def run(fused, backward):
                    if not backward:
                        with torch.no_grad():
                            return ops.graphormer_bias(dist, paths, X, W, S, padding_idx=0, fused=fused)
                    X.grad = W.grad = S.grad = None
                    ops.graphormer_bias(dist, paths, X, W, S, padding_idx=0, fused=fused).backward(cot)

                # equal within the test's bar first: 2^-22 (|q| + |s|) + one ulp of the store, the composition's own
                # fp32 rounding of a sum of L * d products on top (its einsum is not exact on random values)
                a, b = run(True, False).double(), run(False, False).double()
                u = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}[dtype]
                mag = (X.detach().double().abs().max() * W.detach().double().abs().max() * D * L + S.detach().double().abs().max())
                assert float((a - b).abs().max()) <= float((2.0 ** -22 + 2 * u + L * D * 2.0 ** -24) * mag), (atoms, H, dtype)
                item, idb = X.element_size(), dist.element_size()
                fwd_bytes = P * (L + 1) * idb + P * H * item
                bwd_bytes = P * (L + 1) * idb + P * H * item + (E * L * H + (MAX_DIST + 2) * H) * item
                rec = dict(graphs=args.graphs, atoms=atoms, pairs=P, edges=E, L=L, d=D, H=H, dtype=str(dtype).split(".")[1],
                           gpu=torch.cuda.get_device_name(0), fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes,
                           composition_path_data_bytes=P * L * D * item)
                for name, fused in (("fused", True), ("composed", False)):
                    rec[name + "_fwd"] = timeit(lambda: run(fused, False), args.reps, args.warm)
                    rec[name + "_fwd_bwd"] = timeit(lambda: run(fused, True), args.reps, args.warm)
                rec["fwd_speedup"] = rec["composed_fwd"]["ms"] / rec["fused_fwd"]["ms"]
                rec["fwd_bwd_speedup"] = rec["composed_fwd_bwd"]["ms"] / rec["fused_fwd_bwd"]["ms"]
                rec["fwd_stream_fraction"] = fwd_bytes / STREAM_RATE * 1e3 / rec["fused_fwd"]["ms"]
                rec["fwd_bwd_stream_fraction"] = (fwd_bytes + bwd_bytes) / STREAM_RATE * 1e3 / rec["fused_fwd_bwd"]["ms"]
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
