#!/usr/bin/env python
"""Biased attention timings (csrc/biased_attention.hip): the fused operator against the reference's sequence in plain
torch (``fused=False``: bmm, add, masked fill, softmax, bmm) in the same process, the two routes alternating.

    python benchmarks/bench_biased_attention.py [--out profiles/r25/biased_attention.jsonl]

Shapes (B, N, H, D): (64, 128, 32, 24), (16, 100, 8, 64) (the reference's docstring), (256, 32, 8, 64) (small molecules),
(8, 512, 8, 64); fp32 and bf16; bias and mask present; no dropout.  ``fwd`` is the forward under no_grad, ``fwd_bwd`` the
forward and the backward to q, k, v and the bias.  Every time is taken with device events around whole calls, after
--warm calls: the median, minimum and maximum of --reps.  ``sdpa`` is ``F.scaled_dot_product_attention`` on the bias
permuted to (B, H, N, N) with the mask folded in, the permute inside the timing (informative; forward only).

Byte model (what a pass must move): forward = q, k, v, out + the bias + the mask; backward = q, k, v, out, dout, dq, dk,
dv + the bias and dbias once + the mask.  ``*_stream_fraction`` = that over the time of the whole call over the measured
7.1 TB/s stream rate.  The last lines are the errors of the test cases on both routes (tests/battn_cases.py)."""
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
from tests.battn_cases import CASES, NAMES, errors, formula, inputs, outputs  # noqa: E402

SHAPES = [(64, 128, 32, 24), (16, 100, 8, 64), (256, 32, 8, 64), (8, 512, 8, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_biased_attention needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []
    for B, N, H, D in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            torch.manual_seed(25)
            q, k, v, cot = (torch.randn(B, N, H, D, device=dev).to(dtype) for _ in range(4))
            bias = torch.randn(B, N, N, H, device=dev).to(dtype)
            mask = torch.rand(B, N, N, device=dev) < 0.2
            mask[:, :, 0] = False
            leaves = [t.requires_grad_() for t in (q, k, v, bias)]

            def run(fused, backward):
                if not backward:
                    with torch.no_grad():
                        return ops.biased_attention(q, k, v, bias, mask, fused=fused)
                for t in leaves:
                    t.grad = None
                ops.biased_attention(q, k, v, bias, mask, fused=fused).backward(cot)

            def sdpa():
                with torch.no_grad():
                    b = bias.permute(0, 3, 1, 2).masked_fill(mask[:, None], float("-inf"))
                    return torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), b)

            item = q.element_size()
            fwd_bytes = 4 * B * N * H * D * item + B * N * N * (H * item + 1)
            bwd_bytes = 8 * B * N * H * D * item + B * N * N * (2 * H * item + 1)
            rec = dict(B=B, N=N, H=H, D=D, dtype=str(dtype).split(".")[1], gpu=torch.cuda.get_device_name(0),
                       fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes)
            for what, backward in (("fwd", False), ("fwd_bwd", True)):       # the two routes alternate
                for name, fused in (("fused", True), ("composed", False)):
                    rec["%s_%s" % (name, what)] = timeit(lambda: run(fused, backward), args.reps, args.warm)
            rec["sdpa_fwd"] = timeit(sdpa, args.reps, args.warm)
            rec["fwd_speedup"] = rec["composed_fwd"]["ms"] / rec["fused_fwd"]["ms"]
            rec["fwd_bwd_speedup"] = rec["composed_fwd_bwd"]["ms"] / rec["fused_fwd_bwd"]["ms"]
            rec["fwd_stream_fraction"] = fwd_bytes / STREAM_RATE * 1e3 / rec["fused_fwd"]["ms"]
            rec["fwd_bwd_stream_fraction"] = (fwd_bytes + bwd_bytes) / STREAM_RATE * 1e3 / rec["fused_fwd_bwd"]["ms"]
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    for case in CASES:                                                       # the errors of the test cases, both routes
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            c = inputs(case, dtype)
            ref = outputs(lambda q, k, v, b, m: formula(q, k, v, b, m, case[3] ** -0.5), c, torch.float64, "cpu")
            rec = dict(case=case, dtype=str(dtype).split(".")[1])
            for name, fused in (("e_fused", True), ("e_composed", False)):
                got = outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, fused=fused), c, dtype, dev)
                rec[name] = dict(zip(NAMES, errors(got, ref)))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
