#!/usr/bin/env python
"""dgl.shortest_dist timings (csrc/shortest_dist.hip): all-pairs `dist` and `dist + paths` on the device, against the
reference's route in the same run (copy the graph to the host, scipy's shortest_path, copy dist back; taken only when
scipy imports, and without the reference's Python loop over the pairs that rebuilds the paths).

    python benchmarks/bench_shortest_dist.py [--out profiles/r18/shortest_dist.jsonl]

Graphs, seeded, of a size a graph-transformer batch has:

  molecules   --mols random molecule-like graphs of --atoms nodes each in one batch: a random tree plus as many extra
              bonds again, every bond in both directions (mean degree about 4).  Distances stay inside a molecule, so most
              pairs are unreachable and L is a molecule's diameter.
  dense       the same node count with 16 uniform random in-edges per node: every pair is reachable in a few levels.

Every time is taken with device events around whole calls that end in a device synchronise, after --warm calls: the
median, minimum and maximum of --reps.  `dist` is ONE kernel and no read-back; `dist + paths` is the three kernels, the
read-back of L (8 bytes) and the allocation of `paths`.  ``lds`` / ``global`` are the two homes of the search's masks
(max_lds_nodes = 1 forces the workspace form); both are asserted equal to the host twin first.

Traffic: ``dist_bytes`` = S x N x 8 and ``paths_bytes`` = S x N x L x 8 are what the call must write.  The write of
dist alone bounds the time below by dist_bytes / 7.1 TB/s (``dist_floor_ms``); ``dist_floor_fraction`` = that floor over
the measured call time, the whole call over the stream rate, not a kernel's share of peak.  With one workgroup per 64
sources, N / 64 workgroups write dist: a batch of 4 096 nodes occupies 64 of the device's CUs.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dgl_amd as dgl  # noqa: E402
from dgl_amd import _capi  # noqa: E402

STREAM_RATE = 7.1e12


def timeit(fn_, reps, warm):
    for _ in range(warm):
        fn_()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn_()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))


def molecules(mols, atoms, rng):
    src, dst = [], []
    for m in range(mols):
        child = np.arange(1, atoms)
        parent = (rng.random(atoms - 1) * child).astype(np.int64)
        a, b = np.r_[child, rng.integers(0, atoms, atoms)], np.r_[parent, rng.integers(0, atoms, atoms)]
        src += [a + m * atoms, b + m * atoms]
        dst += [b + m * atoms, a + m * atoms]
    return np.concatenate(src), np.concatenate(dst)


def scipy_route(g):
    """What the reference does for `dist`: the CSR to the host, scipy, the distances back."""
    from scipy import sparse

    indptr, indices = (t.cpu().numpy() for t in g._graph.relations[0].csr()[:2])
    n = g.num_nodes()
    adj = sparse.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    dist = sparse.csgraph.shortest_path(adj, unweighted=True, directed=True)
    dist[np.isinf(dist)] = -1
    return torch.from_numpy(dist.astype(np.int64)).to(g.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=128)
    ap.add_argument("--atoms", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shortest_dist needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(18)
    n = args.mols * args.atoms
    graphs = {"molecules": molecules(args.mols, args.atoms, rng),
              "dense": (rng.integers(0, n, 16 * n), np.repeat(np.arange(n), 16))}
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    lines = []
    for case, (src, dst) in graphs.items():
        g = dgl.graph((torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)), num_nodes=n, idtype=torch.int32, device=dev)
        fmt = [t.contiguous() for t in g._graph.relations[0].csc()]
        csr = _capi.make_csr(*fmt, n)
        want = _capi.shortest_dist_host(_capi.host_csr(*[t.cpu() for t in fmt], n), None, True)
        ws = torch.empty(_capi.shortest_dist_workspace_bytes(torch.int32, n, n), dtype=torch.uint8, device=dev)
        L = int(want[1].shape[2])
        rec = dict(case=case, nodes=n, edges=int(src.size), sources=n, L=L, reachable_pairs=int((want[0] >= 0).sum()),
                   dist_bytes=n * n * 8, paths_bytes=n * n * L * 8, workspace_bytes=ws.numel(), gpu=torch.cuda.get_device_name(0),
                   lds_per_workgroup=torch.cuda.get_device_properties(0).shared_memory_per_block)
        for form, lds in (("lds", None), ("global", 1)):
            got = _capi.shortest_dist(csr, None, True, ws=ws, max_lds_nodes=lds)
            assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), (case, form)
            del got
            rec["dist_" + form] = timeit(lambda: _capi.shortest_dist(csr, None, False, ws=ws, max_lds_nodes=lds), args.reps, args.warm)
            rec["dist_paths_" + form] = timeit(lambda: _capi.shortest_dist(csr, None, True, ws=ws, max_lds_nodes=lds), args.reps, args.warm)
        rec["dist_floor_ms"] = rec["dist_bytes"] / STREAM_RATE * 1e3
        rec["dist_floor_fraction"] = rec["dist_floor_ms"] / rec["dist_lds"]["ms"]
        rec["written_GBps_dist_paths"] = (rec["dist_bytes"] + rec["paths_bytes"]) / rec["dist_paths_lds"]["ms"] / 1e6
        if have_scipy:
            assert torch.equal(scipy_route(g).cpu(), want[0])
            rec["scipy_route_dist"] = timeit(lambda: scipy_route(g), 3, 1)
        else:
            rec["scipy_route_dist"] = "not measured: scipy does not import"
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del g, csr, ws, want
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
