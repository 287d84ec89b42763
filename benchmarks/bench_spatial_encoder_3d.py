#!/usr/bin/env python
"""3D spatial encoding timings (csrc/spatial_encoder3d.hip): the fused operator against the reference's sequence in
plain torch (``fused=False``: cdist, Gaussian, linear, GELU, linear) in the same process, the two routes alternating.

    python benchmarks/bench_spatial_encoder_3d.py [--out profiles/r26/spatial_encoder_3d.jsonl]

Shapes (B, N, K, H): (64, 128, 128, 32), (256, 32, 128, 8) (small molecules), (8, 512, 128, 32); fp32 and bf16 weights;
node types given.  ``fwd`` is the forward under no_grad, ``fwd_bwd`` the forward and the backward to the six parameter
tensors, means, stds and the four pair vectors.  Every time is taken with device events around whole calls, after --warm
calls: the median, minimum and maximum of --reps.

Byte model (what a pass must move): forward = the (B, N, N, H) result; backward = the cotangent once plus one fp32 per
pair written and read twice.  ``*_stream_fraction`` = that over the time of the whole call over the measured 7.1 TB/s
stream rate.  ``out_diff`` is max |fused - composed| / max |composed| of the result at the timed size."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from bench_shortest_dist import STREAM_RATE, timeit  # noqa: E402
from dgl_amd import ops  # noqa: E402

SHAPES = [(64, 128, 128, 32), (256, 32, 128, 8), (8, 512, 128, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spatial_encoder_3d needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []
    for B, N, K, H in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(26)
            coord = 3 * torch.rand(B, N, 3, device=dev)
            small = [3 * torch.rand(K, device=dev), 3 * torch.rand(K, device=dev)]                     # means, stds
            weights = [((2 * torch.rand(shape, device=dev) - 1) * K ** -0.5).to(dtype) for shape in ((K, K), (K,), (H, K), (H,))]
            pair = [torch.rand(B, N, device=dev) + 0.5, torch.rand(B, N, device=dev) + 0.5,
                    torch.rand(B, N, device=dev) - 0.5, torch.rand(B, N, device=dev) - 0.5]
            cot = torch.randn(B, N, N, H, device=dev).to(dtype)
            leaves = [t.requires_grad_() for t in small + weights + pair]

            def run(fused, backward):
                if not backward:
                    with torch.no_grad():
                        return ops.spatial_encoder_3d(coord, *small, *weights, *pair, fused=fused)
                for t in leaves:
                    t.grad = None
                ops.spatial_encoder_3d(coord, *small, *weights, *pair, fused=fused).backward(cot)

            a, b = run(True, False).float(), run(False, False).float()
            out_bytes = B * N * N * H * cot.element_size()
            rec = dict(B=B, N=N, K=K, H=H, dtype=str(dtype).split(".")[1], gpu=torch.cuda.get_device_name(0),
                       out_diff=float((a - b).abs().max() / b.abs().max()), fwd_bytes=out_bytes, bwd_bytes=out_bytes + 12 * B * N * N)
            del a, b
            for what, backward in (("fwd", False), ("fwd_bwd", True)):       # the two routes alternate
                for name, fused in (("fused", True), ("composed", False)):
                    rec["%s_%s" % (name, what)] = timeit(lambda: run(fused, backward), args.reps, args.warm)
            rec["fwd_speedup"] = rec["composed_fwd"]["ms"] / rec["fused_fwd"]["ms"]
            rec["fwd_bwd_speedup"] = rec["composed_fwd_bwd"]["ms"] / rec["fused_fwd_bwd"]["ms"]
            rec["fwd_stream_fraction"] = rec["fwd_bytes"] / STREAM_RATE * 1e3 / rec["fused_fwd"]["ms"]
            rec["fwd_bwd_stream_fraction"] = (rec["fwd_bytes"] + rec["bwd_bytes"]) / STREAM_RATE * 1e3 / rec["fused_fwd_bwd"]["ms"]
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
