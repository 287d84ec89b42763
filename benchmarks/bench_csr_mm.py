#!/usr/bin/env python
"""Sparse x sparse timings (csrc/csr_mm.hip) with the HIP-event protocol of benchmarks/bench_ops.py: medians of 10 calls
after 3 warm-up calls, one JSON line per shape.

    python benchmarks/bench_csr_mm.py [--label this] [--out profiles/r9/csr_mm.jsonl]

What is timed is `dgl_amd.sparse.spspmm` — it exists on trees with and without the kernels (there: the torch composition
expand -> unique -> index_add), so two trees are compared by running this file from each, alternately on one GPU, two runs
each.  Shapes: A.A^T and A.A on a uniform-random graph of 100 k nodes with average degree 10 and on one with a power-law
degree tail, the reference test's 500 x 600 x 700 case, and (only where the package has it) the two-operand sum at 1 M edges
each.  `control` is an operator neither tree's change touches (g-SpMM through `sparse.spmm` on the uniform graph): the spread
of its medians across runs is the noise floor a gap has to exceed before a shape counts as faster.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dgl_amd import sparse as dglsp  # noqa: E402


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


def simple_coo(rows, cols, n_cols):
    key = torch.unique(rows.long() * n_cols + cols.long())   # a simple graph: duplicates merged
    return key // n_cols, key % n_cols


def uniform_graph(n, deg, gen):
    return simple_coo(torch.randint(0, n, (n * deg,), generator=gen), torch.randint(0, n, (n * deg,), generator=gen), n)


def power_law_graph(n, deg, gen):
    # destination ids drawn with density ~ x^-0.5 over the id range (a heavy tail of popular columns), sources with the
    # same law through an independent permutation: hub rows and hub columns, the same edge count as the uniform graph
    def draw():
        return (torch.rand(n * deg, generator=gen, dtype=torch.float64) ** 2 * n).long().clamp_(max=n - 1)

    perm = torch.randperm(n, generator=gen)
    return simple_coo(perm[draw()], draw(), n)


def matrix(rows, cols, shape, dev, gen, dtype=torch.float32):
    p = torch.randperm(rows.shape[0], generator=gen)   # shuffled: the CSR carries an edge-id map
    val = torch.randn(rows.shape[0], generator=gen).to(dtype)
    return dglsp.from_coo(rows[p].to(dev), cols[p].to(dev), val.to(dev), shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--degree", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = []

    def emit(shape, ms, ms_min, **kw):
        r = {"label": args.label, "shape": shape, "ms_median": round(ms, 4), "ms_min": round(ms_min, 4)}
        r.update(kw)
        lines.append(r)
        print(json.dumps(r), flush=True)

    n = args.nodes
    graphs = {"uniform": uniform_graph(n, args.degree, gen), "power_law": power_law_graph(n, args.degree, gen)}
    for name, (r, c) in graphs.items():
        A = matrix(r, c, (n, n), dev, gen)
        At = A.t()
        for what, rhs in (("A.At", At), ("A.A", A)):
            C = dglsp.spspmm(A, rhs)   # (also builds the operands' formats outside the timed region)
            ms, mn = timeit(lambda: dglsp.spspmm(A, rhs))
            emit("%s %s n=%d" % (name, what, n), ms, mn, nnz_a=A.nnz, nnz_c=C.nnz)
        if name == "uniform":
            x = torch.randn(n, 64, device=dev)
            ms, mn = timeit(lambda: dglsp.spmm(A, x))
            emit("control spmm uniform n=%d F=64" % n, ms, mn, nnz_a=A.nnz)
    ra, ca = simple_coo(torch.randint(0, 500, (9000,), generator=gen), torch.randint(0, 600, (9000,), generator=gen), 600)
    rb, cb = simple_coo(torch.randint(0, 600, (9000,), generator=gen), torch.randint(0, 700, (9000,), generator=gen), 700)
    A, B = matrix(ra, ca, (500, 600), dev, gen), matrix(rb, cb, (600, 700), dev, gen)
    C = dglsp.spspmm(A, B)
    ms, mn = timeit(lambda: dglsp.spspmm(A, B))
    emit("500x600x700, 9000 draws", ms, mn, nnz_a=A.nnz, nnz_c=C.nnz)

    from dgl_amd import sparse_kernels
    if hasattr(sparse_kernels, "_csrsum"):
        from dgl_amd.graph_index import GraphIndex
        m = 1_000_000
        ops = []
        for _ in range(2):
            r, c = simple_coo(torch.randint(0, n, (m,), generator=gen), torch.randint(0, n, (m,), generator=gen), n)
            S = matrix(r, c, (n, n), dev, gen)
            ops.append((GraphIndex([n, n], [(0, 1)], [S._rel.reverse()]), S.val))
        gs, ws = [o[0] for o in ops], [o[1] for o in ops]
        gc, _ = sparse_kernels._csrsum(gs, ws)
        ms, mn = timeit(lambda: sparse_kernels._csrsum(gs, ws))
        emit("sum of two, 1 M draws each, n=%d" % n, ms, mn, nnz_c=gc.num_edges(0))
    else:
        lines.append({"label": args.label, "shape": "sum of two, 1 M draws each, n=%d" % n, "ms_median": None,
                      "note": "this tree has no csrsum"})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
