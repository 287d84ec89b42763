"""GAT attention block through ``dgl_amd.nn.gat_attention`` on 16-bit operands and on head widths that are not a power of
two: the default route (the fused kernel where ``gat_attention_applies``) and the composed operators (``fused=False``).

Only the public API is used, so the same script runs on a tree whose fused kernel takes fp32 power-of-two widths only
(there the default route composes for every other case): run it on both trees on one GPU, alternating, and compare the
``default`` lines.  Graphs and byte model are those of benchmarks/hot_path_variants.py: C3 (169 343 nodes, 2 501 829
edges) forward and forward + backward, C2 size (2 449 029 nodes, 61 859 140 edges) forward, both behind a random
edge-id map.  Algorithmic bytes of the forward: E * (H*D*s + H*s + i) + N * (H*D*s + 2*H*4) + (N + 1) * i with s the
element size; forward + backward counts three such passes.

One JSON line per case: ms median / min over >= 10 timed calls after warm-up, algorithmic bytes, fraction of 8 TB/s,
hbm_roofline_evidence (the gathered operand exceeds the 256 MiB cache), a SHA-256 of the result bytes (same bits on
both trees for the fp32 power-of-two controls) and the commit id given with --commit.

    python benchmarks/bench_gat_attention.py --commit $(git rev-parse --short HEAD) [--scale 1] [--reps 10]

``--train`` times the TRAINING rows instead (profiles/r8/gat_attention_dropout.jsonl): forward and forward + backward at
C3 and at C2 size, H8 D8 and H8 D32, fp32 and bf16, attention dropout p = 0.6, each three ways: ``fused_p0`` (the fused
kernel without dropout, the control: it runs on a tree without the ``attn_drop`` keyword too, so this tree and its parent
can alternate on one GPU), ``fused_drop`` (the fused kernel with the mask evaluated in registers, a fresh seed per call)
and ``composed_drop`` (the four operators with ``F.dropout`` on the (E, H) weights).  A
dropout pass reads the edge-id map once more than the byte model above: + E * i bytes per pass.
"""
import argparse
import hashlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK = 8000.0
CACHE_BYTES = 256 << 20
C3_NODES, C3_EDGES = 169_343, 2_501_829
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# (dtype, H, D, kind): controls = what the fused kernel took before the set was widened
CASES = ([("fp32", 8, 8, "control"), ("fp32", 8, 32, "control")] +
         [(t, 8, d, "new") for t in ("bf16", "fp16") for d in (8, 32, 64)] +
         [("fp32", 2, 12, "new"), ("fp32", 1, 47, "new")])


def _time(fn, reps, warm=3):
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


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def _dgl_graph(g, dev):
    from dgl_amd.graph_index import GraphIndex, Relation
    from dgl_amd.heterograph import DGLGraph

    n = g["num_rows"]
    rel = Relation(n, g["num_cols"], csc=(g["indptr"], g["indices"], g["eids"]), idtype=g["indptr"].dtype, device=dev)
    return DGLGraph(GraphIndex([n], [(0, 0)], [rel]), ["_N"], [("_N", "_E", "_N")])


def _emit(args, case, ms_mn, nbytes, e, gathered, **kw):
    ms, mn = ms_mn
    rec = {"case": case, "commit": args.commit, "ms": ms, "ms_min": mn, "reps": args.reps, "edges": int(e),
           "alg_bytes": int(nbytes), "achieved_GBps": nbytes / (ms * 1e-3) / 1e9,
           "roofline_frac": nbytes / (ms * 1e-3) / 1e9 / PEAK, "hbm_roofline_evidence": bool(gathered > CACHE_BYTES),
           "device": torch.cuda.get_device_name(0)}
    rec.update(kw)
    print(json.dumps(rec), flush=True)


def run(args):
    import dgl_amd as dgl
    from tests.graphgen import C2_EDGES, C2_NODES, synth_csr

    dev = torch.device("cuda:0")
    i = 4
    routes = (("default", {}), ("composed", dict(fused=False)))
    for size in ("C3", "C2size"):
        if size == "C3":
            n, e = C3_NODES, C3_EDGES
            g = synth_csr(n, n, e, "U", seed=3, device=dev, with_eids=True)
        else:
            n, e = C2_NODES // args.scale, C2_EDGES // args.scale
            g = synth_csr(n, n, e, "U", seed=20250824, device=dev)
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            g["eids"] = torch.randperm(e, device=dev, generator=gen).to(torch.int32)
        dg = _dgl_graph(g, dev)
        for tname, h, d, kind in CASES:
            dt = DTYPES[tname]
            s = torch.finfo(dt).bits // 8
            torch.manual_seed(h * 100 + d)
            ps = [(torch.rand(n, h, d, device=dev) + 1).to(dt), torch.randn(n, h, 1, device=dev).to(dt),
                  torch.randn(n, h, 1, device=dev).to(dt)]
            up = torch.randn(n, h, d, device=dev).to(dt)
            nb = e * (h * d * s + h * s + i) + n * (h * d * s + 2 * h * 4) + (n + 1) * i
            applies = bool(dgl.ops.gat_attention_applies(dg, *ps))
            for route, kw in routes:
                if route == "composed" and not args.composed:
                    continue
                tag = "%s_H%d_D%d_eid_map_%s" % (tname, h, d, route)
                with torch.no_grad():
                    out = dgl.nn.gat_attention(dg, ps[0], ps[1], ps[2], 0.2, **kw)
                    t = _time(lambda: dgl.nn.gat_attention(dg, ps[0], ps[1], ps[2], 0.2, **kw), args.reps)
                _emit(args, "gat_attention_fwd_%s_%s" % (size, tag), t, nb, e, n * h * d * s, kind=kind, dtype=tname,
                      heads=h, dim=d, route=route, fused=applies and route == "default", sha256=_sha(out))
                del out
                if size != "C3":
                    continue
                qs = [p.clone().requires_grad_(True) for p in ps]

                def train():
                    for p in qs:
                        p.grad = None
                    dgl.nn.gat_attention(dg, qs[0], qs[1], qs[2], 0.2, **kw).backward(up)

                train()
                sha = _sha(*[p.grad for p in qs])
                t = _time(train, args.reps)
                _emit(args, "gat_attention_fwd_bwd_%s_%s" % (size, tag), t, 3 * nb, e, n * h * d * s, kind=kind, dtype=tname,
                      heads=h, dim=d, route=route, fused=applies and route == "default", sha256=sha)
                del qs
            del ps, up
        del dg, g
        torch.cuda.empty_cache()


TRAIN_CASES = [(t, 8, d) for t in ("fp32", "bf16") for d in (8, 32)]
TRAIN_P = 0.6


class _Seeds:
    """A fresh seed per call without a generator draw inside the timed region: ``int(seed)`` counts up."""

    def __init__(self):
        self.n = 0

    def __int__(self):
        self.n += 1
        return self.n


def run_train(args):
    import dgl_amd as dgl
    from tests.graphgen import C2_EDGES, C2_NODES, synth_csr

    dev = torch.device("cuda:0")
    i = 4
    routes = [("fused_p0", dict(fused=True), 0.0)]
    if "attn_drop" in inspect.signature(dgl.nn.gat_attention).parameters:
        routes += [("fused_drop", dict(fused=True, attn_drop=TRAIN_P, seed=_Seeds()), TRAIN_P),
                   ("composed_drop", dict(fused=False, attn_drop=TRAIN_P), TRAIN_P)]
    for size in ("C3", "C2size"):
        if size == "C3":
            n, e = C3_NODES, C3_EDGES
            g = synth_csr(n, n, e, "U", seed=3, device=dev, with_eids=True)
        else:
            n, e = C2_NODES // args.scale, C2_EDGES // args.scale
            g = synth_csr(n, n, e, "U", seed=20250824, device=dev)
            gen = torch.Generator(device=dev)
            gen.manual_seed(7)
            g["eids"] = torch.randperm(e, device=dev, generator=gen).to(torch.int32)
        dg = _dgl_graph(g, dev)
        for tname, h, d in TRAIN_CASES:
            dt = DTYPES[tname]
            s = torch.finfo(dt).bits // 8
            torch.manual_seed(h * 100 + d)
            ps = [(torch.rand(n, h, d, device=dev) + 1).to(dt), torch.randn(n, h, 1, device=dev).to(dt),
                  torch.randn(n, h, 1, device=dev).to(dt)]
            up = torch.randn(n, h, d, device=dev).to(dt)
            for route, kw, p in routes:
                nb = e * (h * d * s + h * s + i + (i if p else 0)) + n * (h * d * s + 2 * h * 4) + (n + 1) * i
                tag = "%s_H%d_D%d_eid_map_%s" % (tname, h, d, route)
                common = dict(dtype=tname, heads=h, dim=d, route=route, p=p, fused=route != "composed_drop")
                with torch.no_grad():
                    out = dgl.nn.gat_attention(dg, ps[0], ps[1], ps[2], 0.2, **kw)
                    t = _time(lambda: dgl.nn.gat_attention(dg, ps[0], ps[1], ps[2], 0.2, **kw), args.reps)
                _emit(args, "gat_attention_train_fwd_%s_%s" % (size, tag), t, nb, e, n * h * d * s,
                      sha256=None if p else _sha(out), **common)
                del out
                qs = [q.clone().requires_grad_(True) for q in ps]

                def train():
                    for q in qs:
                        q.grad = None
                    dgl.nn.gat_attention(dg, qs[0], qs[1], qs[2], 0.2, **kw).backward(up)

                train()
                sha = None if p else _sha(*[q.grad for q in qs])
                t = _time(train, args.reps)
                _emit(args, "gat_attention_train_fwd_bwd_%s_%s" % (size, tag), t, 3 * nb, e, n * h * d * s, sha256=sha, **common)
                del qs
            del ps, up
        del dg, g
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default="unknown", help="commit id of the tree, copied into every line")
    ap.add_argument("--reps", type=int, default=10, help="timed calls per case (>= 10)")
    ap.add_argument("--scale", type=int, default=1, help="divide the C2-size graph by this")
    ap.add_argument("--composed", action="store_true", help="also time fused=False")
    ap.add_argument("--train", action="store_true", help="time the training rows (attention dropout) instead")
    args = ap.parse_args()
    args.reps = max(10, args.reps)
    (run_train if args.train else run)(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
