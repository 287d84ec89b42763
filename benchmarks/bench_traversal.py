#!/usr/bin/env python
"""Graph traversal timings (csrc/traversal.hip): whole calls on the wall clock, each against what the reference does for
a GPU graph in the same run: copy the CSR to the host, run the sequential-order rule there (the host twin
dgla_traverse_host), copy the frontiers back.

    python benchmarks/bench_traversal.py [--out profiles/r19/traversal.jsonl]

Shapes:

  trees_topo       a batch of 256 random trees of 30 - 60 nodes, edges child -> parent, topological_nodes_generator: the
                   TreeLSTM shape.  Launches and read-backs dominate here.
  c2_bfs_1 / _1000 bfs_nodes_generator from 1 and from 1 000 sources on the C2-shaped graph (ogbn-products size, uniform,
                   int32 ids).
  c2_dag_topo      topological_nodes_generator on a random DAG of the C2 size (every edge from the smaller to the larger id).
  trees_prop       prop_nodes_topo with copy_u / sum on the batch of trees, against the same sweep over frontiers that
                   took the host path.

Every time is wall clock around a device synchronisation: the median (and minimum) of --reps calls after --warm.  The
formats (CSR and CSC) are built once, outside the timings, for both paths.  The two paths are asserted identical first.

Per record: ``levels`` (frontiers expanded), ``launches_per_level`` (4 + two scans, a scan being 1 launch up to 32 768
rows and 3 above; the mean over the levels), ``read_backs`` (one per level, plus frontier 0 of the topological order), and
a byte model of the device path, written down here:

    model_bytes = E x 3 x (id + 8)          every expanded entry is loaded in the mark, count and fill passes and each
                                            pass gathers the target's 8-byte key
                + E x 2 x 8 + E x 16        topological only: count[v] in the two select passes, and the two atomics
                + R x 4 x 3 x id            every frontier row: its id and two indptr entries in the 4 row passes
                + R x 6 x 8                 the row lengths / kept counts, written, scanned and read

with E the entries expanded and R the frontier rows over all levels.  ``stream_fraction`` = model_bytes / call time /
7.1 TB/s: the whole call over the stream rate, not a kernel's share of peak.
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
import dgl_amd.function as fn  # noqa: E402
from dgl_amd import _capi  # noqa: E402
from tests.graphgen import C2_EDGES, C2_NODES  # noqa: E402
from tests.traversal_cases import random_trees  # noqa: E402

STREAM_RATE = 7.1e12
SCAN_SMALL = 32768


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


def host_path(g, mode, sources, reverse=False):
    """What the reference does for a GPU graph: the CSR goes to the host, the queue-order rule runs there, the frontiers
    come back."""
    rel = g._graph.relations[0]
    walk, other = ("csc", "csr") if reverse else ("csr", "csc")
    cpu = lambda fmt: _capi.host_csr(*[None if t is None else t.cpu() for t in getattr(rel, fmt)()], rel.num_dst)
    csr = cpu(walk)
    opposite = cpu(other) if mode == _capi.TRAVERSE_TOPO_NODES else None
    src = None if sources is None else sources.cpu()
    ids, sections = _capi.traverse_host(mode, csr, opposite, src)
    return tuple(torch.split(ids.to(g.device), sections))


def shape_record(g, frontiers, topo, id_bytes):
    """levels, launches, read-backs and the byte model of one traversal, from its frontiers."""
    rel = g._graph.relations[0]
    deg = rel.out_degrees().long()
    rows = [int(f.shape[0]) for f in frontiers]
    R = sum(rows)
    E = int(deg[torch.cat(frontiers).long()].sum()) if frontiers else 0
    scans = [1 if m + 1 <= SCAN_SMALL else 3 for m in rows]
    model = E * 3 * (id_bytes + 8) + (E * 32 if topo else 0) + R * 12 * id_bytes + R * 48
    return dict(levels=len(rows), largest_frontier=max(rows, default=0), frontier_rows=R, entries_expanded=E,
                launches_per_level=float(np.mean([4 + 2 * s for s in scans])) if rows else 0.0,
                read_backs=len(rows) + (1 if topo else 0), model_bytes=model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=C2_NODES)
    ap.add_argument("--edges", type=int, default=C2_EDGES)
    ap.add_argument("--trees", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_traversal needs a ROCm GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        rec.update(gpu=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def compare(case, g, mode, sources, id_bytes, gen):
        topo = mode == _capi.TRAVERSE_TOPO_NODES
        got, want = gen(), host_path(g, mode, sources)
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
        ms, best = timeit(gen, args.reps, args.warm)
        hms, hbest = timeit(lambda: host_path(g, mode, sources), args.host_reps, 1)
        rec = shape_record(g, got, topo, id_bytes)
        rec.update(case=case, nodes=g.num_nodes(), edges=g.num_edges(), id_bytes=id_bytes, ms=ms, ms_min=best, host_path_ms=hms,
                   host_path_ms_min=hbest, ratio_host_over_device=hms / ms, identical=True,
                   stream_fraction=rec["model_bytes"] / (ms * 1e-3) / STREAM_RATE)
        emit(rec)
        return got

    # (a) the TreeLSTM shape
    n, src, dst, _ = random_trees(args.trees, 30, 60, 19)
    t = lambda a: torch.from_numpy(a).to(device=dev, dtype=torch.int64)
    g = dgl.graph((t(src), t(dst)), num_nodes=n, device=dev)
    rel = g._graph.relations[0]
    rel.csr(), rel.csc()
    compare("trees_topo", g, _capi.TRAVERSE_TOPO_NODES, None, 8, lambda: dgl.topological_nodes_generator(g))

    # (d) the sweep over it
    def sweep(frontiers_of):
        g.ndata["h"] = torch.ones(n, 1, device=dev)
        g.prop_nodes(frontiers_of(), fn.copy_u("h", "m"), fn.sum("m", "h"))
        return g.ndata["h"]

    on_device = lambda: sweep(lambda: dgl.topological_nodes_generator(g))
    on_host = lambda: sweep(lambda: host_path(g, _capi.TRAVERSE_TOPO_NODES, None))
    assert torch.equal(on_device(), on_host())
    ms, best = timeit(on_device, args.reps, args.warm)
    hms, hbest = timeit(on_host, args.reps, args.warm)
    emit(dict(case="trees_prop", nodes=n, edges=int(src.size), id_bytes=8, ms=ms, ms_min=best, host_path_ms=hms,
              host_path_ms_min=hbest, ratio_host_over_device=hms / ms, identical=True,
              levels=len(dgl.topological_nodes_generator(g))))
    del g

    # (b) BFS on the C2-shaped graph
    N, E = args.nodes, args.edges
    gen = torch.Generator(device=dev).manual_seed(19)
    u = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
    v = torch.randint(0, N, (E,), device=dev, generator=gen, dtype=torch.int32)
    g = dgl.graph((u, v), num_nodes=N, idtype=torch.int32, device=dev)
    g._graph.relations[0].csr()
    for k in (1, 1000):
        s = torch.randperm(N, device=dev, generator=gen)[:k].to(torch.int32)
        compare("c2_bfs_%d" % k, g, _capi.TRAVERSE_BFS_NODES, s, 4, lambda s=s: dgl.bfs_nodes_generator(g, s))
    del g

    # (c) the topological order of a random DAG of that size
    keep = u != v
    lo, hi = torch.minimum(u, v)[keep], torch.maximum(u, v)[keep]
    g = dgl.graph((lo, hi), num_nodes=N, idtype=torch.int32, device=dev)
    rel = g._graph.relations[0]
    rel.csr(), rel.csc()
    compare("c2_dag_topo", g, _capi.TRAVERSE_TOPO_NODES, None, 4, lambda: dgl.topological_nodes_generator(g))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
