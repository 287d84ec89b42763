#!/usr/bin/env python
"""Run the REFERENCE'S OWN parametrised operator suites against this package (VERDICT r4 Next #2).

The suites are not ours and are not committed: ``--prepare`` copies the handful of files below from
``/root/reference/tests`` into ``scratch/ref_tests/`` (git-ignored; it travels to the GPU box with the
snapshot, where ``/root/reference`` does not exist).  A run then

  * aliases ``dgl`` -> ``dgl_amd`` (plus ``dgl.function / ops / backend / nn / base / convert``), provides the
    reference's ``tests/backend`` shim from its own files on top of ``shim_backend.py``, and a 20-line stand-in
    for ``networkx.erdos_renyi_graph`` when networkx is not installed (it is not, here);
  * executes the selected test functions UNMODIFIED under pytest with ``DGLTESTDEV=gpu``;
  * writes one json line per reference test id — outcome, seconds — to ``--out`` (commit under profiles/).

What the suites compare: every built-in message / reduce pair against the same computation written as
user-defined functions (edge batches + degree bucketing, dgl_amd/udf.py), forward and gradients, at the
reference's own tolerances (rtol = atol = 1e-4; tests/python/common/ops/test_ops.py:87-181).
"""
import argparse
import json
import os
import shutil
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEST = os.path.join(ROOT, "scratch", "ref_tests")
FILES = [
    "python/common/ops/test_ops.py",
    "python/common/ops/test_edge_softmax.py",
    "python/common/test_heterograph-kernel.py",
    "utils/__init__.py", "utils/checks.py", "utils/graph_cases.py",
    "backend/__init__.py", "backend/backend_unittest.py", "backend/pytorch/__init__.py",
]
SPARSE_FILES = ["python/pytorch/sparse/" + f for f in (
    "__init__.py", "utils.py", "test_broadcast.py", "test_elementwise_op.py", "test_elementwise_op_sp.py", "test_matmul.py",
    "test_matrix_op.py", "test_reduction.py", "test_sddmm.py", "test_softmax.py", "test_sparse_matrix.py",
    "test_unary_op.py")]
MP_FILES = ["python/common/test_heterograph-update-all.py", "python/common/test_heterograph-apply-edges.py",
            "python/common/test_heterograph-specialization.py", "python/common/test_readout.py",
            "python/common/transforms/test_to_block.py"]
SAMPLING_FILE = "python/common/sampling/test_sampling.py"
SAMPLING_SELECT = ["test_sample_neighbors_noprob", "test_sample_neighbors_prob", "test_sample_neighbors_outedge",
                   "test_sample_neighbors_with_0deg", "test_global_uniform_negative_sampling"]
NN_FILE = "python/pytorch/nn/test_nn.py"
NN_SELECT = ["test_graph_conv0", "test_graph_conv", "test_graph_conv_e_weight", "test_graph_conv_e_weight_norm",
             "test_graph_conv_bi", "test_sage_conv", "test_sage_conv_bi", "test_sage_conv2", "test_gat_conv",
             "test_gat_conv_bi", "test_rgcn", "test_rgcn_default_nbasis", "test_hetero_conv", "test_hetero_linear",
             "test_hetero_embedding", "test_typed_linear"]
# the reference's own LAYER files (python/dgl/nn/pytorch/...), imported unmodified as dgl.nn.pytorch.* on top of the alias:
# dgl_amd ships no layer code of its own (VERDICT r5 Next #8)
LAYER_FILES = ["conv/graphconv.py", "conv/sageconv.py", "conv/gatconv.py", "conv/relgraphconv.py", "linear.py", "hetero.py",
               "utils.py"]
LAYER_DEST = os.path.join(DEST, "_dgl_layers", "dgl", "nn", "pytorch")
SELECT = {
    "python/common/ops/test_ops.py": ["test_spmm", "test_half_spmm", "test_sddmm", "test_segment_reduce",
                                      "test_segment_mm", "test_gather_mm_idx_b"],
    "python/common/ops/test_edge_softmax.py": ["test_edge_softmax", "test_edge_softmax_unidirectional"],
    "python/common/test_heterograph-kernel.py": ["test_copy_src_reduce", "test_copy_edge_reduce",
                                                 "test_all_binary_builtins", "test_mean_zero_degree"],
}


def prepare(src):
    for f in FILES + SPARSE_FILES + [NN_FILE, SAMPLING_FILE] + MP_FILES:
        d = os.path.join(DEST, f)
        os.makedirs(os.path.dirname(d), exist_ok=True)
        shutil.copyfile(os.path.join(src, f), d)
    lsrc = os.path.join(os.path.dirname(os.path.abspath(src)), "python", "dgl", "nn", "pytorch")
    for f in LAYER_FILES:
        d = os.path.join(LAYER_DEST, f)
        os.makedirs(os.path.dirname(d), exist_ok=True)
        shutil.copyfile(os.path.join(lsrc, f), d)
    print("copied %d test files from %s and %d layer files from %s to %s" % (
        len(FILES + SPARSE_FILES + MP_FILES) + 2, src, len(LAYER_FILES), lsrc, DEST))


class _NxGraph:
    """The three calls dgl.from_networkx makes on nx.erdos_renyi_graph's result."""

    def __init__(self, n, pairs):
        self._n, self._pairs = n, pairs

    def number_of_nodes(self):
        return self._n

    def edges(self):
        return list(self._pairs)

    def is_directed(self):
        return False


def _install_networkx_stub():
    try:
        import networkx  # noqa: F401
        return "networkx"
    except ImportError:
        pass
    import numpy as np

    nx = types.ModuleType("networkx")

    def erdos_renyi_graph(n, p, seed=None, directed=False):
        rng = np.random.RandomState(seed if seed is not None else 4242)
        iu = np.triu_indices(n, 1)
        keep = rng.rand(iu[0].shape[0]) < p
        return _NxGraph(n, list(zip(iu[0][keep].tolist(), iu[1][keep].tolist())))

    def path_graph(n):
        return _NxGraph(n, [(i, i + 1) for i in range(n - 1)])

    nx.erdos_renyi_graph = erdos_renyi_graph
    nx.path_graph = path_graph
    nx.Graph = _NxGraph
    sys.modules["networkx"] = nx
    return "stub"


def install_aliases():
    """``import dgl`` -> dgl_amd, with the submodules the suites import by name."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch

    import dgl_amd
    import shim_backend

    dgl = types.ModuleType("dgl")
    dgl.__dict__.update({k: v for k, v in dgl_amd.__dict__.items() if not k.startswith("__")})
    dgl.__path__ = []                                  # a package: `import dgl.function as fn` resolves via sys.modules
    dgl.backend = shim_backend
    dgl.nn = types.ModuleType("dgl.nn")
    dgl.nn.__all__ = []
    dgl.nn.__path__ = []
    dgl.nn.functional = types.ModuleType("dgl.nn.functional")
    dgl.nn.functional.edge_softmax = dgl_amd.ops.edge_softmax
    sys.modules["dgl.nn.functional"] = dgl.nn.functional

    def _absent(name):
        def f(*a, **k):
            raise NotImplementedError("dgl.%s is outside the hot path and not part of dgl_amd" % name)
        return f

    part = types.ModuleType("dgl.partition")            # `import dgl.partition` at the top of test_to_block.py (unused there)
    dgl.partition = part
    sys.modules["dgl.partition"] = part
    for name in ("shortest_dist",):                      # imported by name at the top of test_nn.py, used by tests not run here
        if not hasattr(dgl, name):
            setattr(dgl, name, _absent(name))
    base = types.ModuleType("dgl.base")
    base.is_internal_column = lambda name: name.startswith("_")
    base.DGLError, base.NID, base.EID, base.NTYPE, base.ETYPE = dgl_amd.DGLError, "_ID", "_ID", "_TYPE", "_TYPE"
    dgl.base = base
    convert = types.ModuleType("dgl.convert")
    convert.heterograph, convert.graph = dgl_amd.heterograph, dgl_amd.graph
    dgl.convert = convert
    ops = types.ModuleType("dgl.ops")
    ops.__dict__.update({k: v for k, v in dgl_amd.ops.__dict__.items() if not k.startswith("__")})
    ops.segment_reduce, ops.gather_mm, ops.segment_mm = dgl_amd.segment_reduce, dgl_amd.gather_mm, dgl_amd.segment_mm
    dgl.ops = ops

    def seed(val):
        torch.manual_seed(val)

    dgl.seed = seed
    shim_backend.cuda = lambda: torch.device("cuda:0")
    dgl.sparse = dgl_amd.sparse                       # one module here, a package of thin wrappers there
    if not hasattr(dgl_amd.sparse, "__path__"):
        dgl_amd.sparse.__path__ = []
    for sub in ("matmul", "sparse_matrix", "sddmm", "softmax", "reduction", "elementwise_op", "elementwise_op_sp",
                "broadcast", "unary_op"):
        sys.modules["dgl.sparse." + sub] = dgl_amd.sparse
    for name, mod in (("dgl", dgl), ("dgl.backend", shim_backend), ("dgl.nn", dgl.nn), ("dgl.base", base),
                      ("dgl.convert", convert), ("dgl.ops", ops), ("dgl.function", dgl_amd.function),
                      ("dgl.sparse", dgl_amd.sparse)):
        sys.modules[name] = mod
    _install_reference_layers(dgl, base, convert)
    return _install_networkx_stub()


def _install_reference_layers(dgl, base, convert):
    """dgl.nn.pytorch = the reference's own layer files (copied by --prepare), imported through the alias.  What they
    import besides torch: dgl.function, dgl.base.DGLError / dgl_warning, dgl.utils.expand_as_pair / check_eq_shape,
    dgl.transforms.reverse, dgl.convert.block_to_graph, dgl.heterograph.DGLBlock, dgl.ops.gather_mm / segment_mm,
    dgl.nn.functional.edge_softmax, dgl.DGLGraph."""
    import importlib
    import warnings

    import dgl_amd

    pyt = types.ModuleType("dgl.nn.pytorch")
    if not os.path.isdir(LAYER_DEST):
        sys.modules["dgl.nn.pytorch"] = pyt              # the ops / sparse / mp suites do not need layers
        dgl.nn.pytorch = pyt
        return
    base.dgl_warning = lambda msg, *a, **k: warnings.warn(msg)
    utils = types.ModuleType("dgl.utils")

    def expand_as_pair(input_, g=None):
        if isinstance(input_, tuple):
            return input_
        if g is not None and g.is_block:
            if isinstance(input_, dict):
                return input_, {k: v[: g.number_of_dst_nodes(k)] for k, v in input_.items()}
            return input_, input_[: g.number_of_dst_nodes()]
        return input_, input_

    def check_eq_shape(input_):
        s, d = expand_as_pair(input_)
        if tuple(s.shape)[1:] != tuple(d.shape)[1:]:
            raise dgl_amd.DGLError("The feature shape of source nodes: {} should be equal to the feature shape of "
                                   "destination nodes: {}.".format(tuple(s.shape)[1:], tuple(d.shape)[1:]))

    utils.expand_as_pair, utils.check_eq_shape = expand_as_pair, check_eq_shape
    transforms = types.ModuleType("dgl.transforms")
    transforms.reverse = dgl_amd.reverse
    het = types.ModuleType("dgl.heterograph")

    class _BlockMeta(type):
        def __instancecheck__(cls, g):
            return isinstance(g, dgl_amd.DGLGraph) and bool(g.is_block)

    het.DGLBlock = _BlockMeta("DGLBlock", (), {})
    het.DGLGraph = dgl_amd.DGLGraph
    convert.block_to_graph = lambda g: g               # (EdgeWeightNorm only reads srcdata / dstdata / edata of it)
    dgl.utils, dgl.transforms, dgl.heterograph_module = utils, transforms, het
    for name, mod in (("dgl.utils", utils), ("dgl.transforms", transforms), ("dgl.heterograph", het)):
        sys.modules[name] = mod
    dgl.nn.__path__ = [os.path.dirname(LAYER_DEST)]
    pyt.__path__ = [LAYER_DEST]
    conv = types.ModuleType("dgl.nn.pytorch.conv")
    conv.__path__ = [os.path.join(LAYER_DEST, "conv")]
    sys.modules["dgl.nn.pytorch"], sys.modules["dgl.nn.pytorch.conv"] = pyt, conv
    dgl.nn.pytorch, pyt.conv = pyt, conv
    exported = {"conv.graphconv": ("GraphConv", "EdgeWeightNorm"), "conv.sageconv": ("SAGEConv",), "conv.gatconv": ("GATConv",),
                "conv.relgraphconv": ("RelGraphConv",), "linear": ("TypedLinear",),
                "hetero": ("HeteroGraphConv", "HeteroLinear", "HeteroEmbedding"), "utils": ("Sequential", "WeightBasis", "JumpingKnowledge", "LabelPropagation")}
    for sub, names in exported.items():
        m = importlib.import_module("dgl.nn.pytorch." + sub)
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(LAYER_DEST)), m.__file__
        for n in names:
            if hasattr(m, n):
                setattr(pyt, n, getattr(m, n))
                if sub.startswith("conv."):
                    setattr(conv, n, getattr(m, n))


def suite_targets(suite):
    if suite == "sparse":
        return [os.path.join(DEST, f) for f in SPARSE_FILES if os.path.basename(f).startswith("test_")]
    if suite == "mp":     # message passing on heterographs: update_all / apply_edges / pull / send_and_recv
        return [os.path.join(DEST, f) for f in MP_FILES]
    if suite == "sampling":
        return ["%s::%s" % (os.path.join(DEST, SAMPLING_FILE), n) for n in SAMPLING_SELECT]
    if suite == "nn":
        return ["%s::%s" % (os.path.join(DEST, NN_FILE), n) for n in NN_SELECT]
    return ["%s::%s" % (os.path.join(DEST, f), n) for f, names in SELECT.items() for n in names]


def short_id(nodeid):
    return nodeid.replace(DEST + "/", "").replace("scratch/ref_tests/", "")


class _Collect:
    def __init__(self):
        self.ids = []

    def pytest_collection_modifyitems(self, items):
        self.ids = [short_id(i.nodeid) for i in items]


class _Report:
    def __init__(self, path):
        self.rows, self.path = [], path

    def pytest_runtest_logreport(self, report):
        if report.when == "call" or (report.when == "setup" and report.outcome != "passed"):
            self.rows.append({"id": report.nodeid, "outcome": report.outcome, "seconds": round(report.duration, 4),
                              "detail": (str(report.longrepr)[-600:] if report.outcome == "failed" else "")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prepare", action="store_true", help="copy the suites from --src into scratch/ref_tests")
    ap.add_argument("--src", default="/root/reference/tests")
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "ref_suite.jsonl"))
    ap.add_argument("--device", default="gpu", choices=["gpu", "cpu"])
    ap.add_argument("--suite", default="ops", choices=["ops", "sparse", "nn", "mp", "sampling"],
                    help="ops: the operator suites (SELECT); sparse: tests/python/pytorch/sparse/*, every test")
    ap.add_argument("--collect", action="store_true", help="write the suite's test ids to scratch/ref_tests/ids_<suite>.json")
    ap.add_argument("-k", default=None)
    ap.add_argument("--maxfail", type=int, default=0)
    args = ap.parse_args()
    if args.prepare:
        prepare(args.src)
        return 0
    if args.collect:
        # the test ids of one suite, written next to the copied files: tests/test_zz_reference_suites.py parametrises over
        # them, so every reference test id shows up in the driver's own pytest count
        os.environ["DGLTESTDEV"] = args.device
        os.environ.setdefault("DGLBACKEND", "pytorch")
        install_aliases()
        sys.path.insert(0, DEST)
        import pytest

        col = _Collect()
        rc = pytest.main(["-q", "--collect-only", "-p", "no:cacheprovider", "--rootdir", DEST, "-c", os.devnull, "-W", "ignore"]
                         + suite_targets(args.suite), plugins=[col])
        with open(os.path.join(DEST, "ids_%s.json" % args.suite), "w") as fh:
            json.dump(col.ids, fh)
        print("collected %d ids of suite %s (pytest rc %d)" % (len(col.ids), args.suite, int(rc)))
        return 0 if col.ids else 1
    if not os.path.isdir(DEST):
        print("no scratch/ref_tests: run with --prepare in the container that has /root/reference")
        return 2
    os.environ["DGLTESTDEV"] = args.device
    os.environ.setdefault("DGLBACKEND", "pytorch")
    nx_kind = install_aliases()
    sys.path.insert(0, DEST)                          # `import backend`, `from utils import ...`
    import pytest

    rep = _Report(args.out)
    targets = suite_targets(args.suite)
    t0 = time.time()
    extra = ["-k", args.k] if args.k else []
    if args.maxfail:
        extra += ["--maxfail", str(args.maxfail)]
    rc = pytest.main(["-q", "-x" if False else "-p", "no:cacheprovider", "--rootdir", DEST, "-c", os.devnull,
                      "-W", "ignore"] + extra + targets, plugins=[rep])
    import torch

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    counts = {}
    per_test = {}
    for r in rep.rows:
        counts[r["outcome"]] = counts.get(r["outcome"], 0) + 1
        fn_name = r["id"].split("::")[-1].split("[")[0]
        d = per_test.setdefault(fn_name, {})
        d[r["outcome"]] = d.get(r["outcome"], 0) + 1
    with open(args.out, "w") as fh:
        fh.write(json.dumps({"summary": counts, "per_test_function": per_test, "pytest_rc": int(rc),
                             "seconds": round(time.time() - t0, 1), "device": args.device, "networkx": nx_kind,
                             "gpu": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
                             "note": "the reference's own test files, unmodified, `import dgl` -> dgl_amd"}) + "\n")
        for r in rep.rows:
            r["id"] = short_id(r["id"])
            fh.write(json.dumps(r) + "\n")
    print("reference suites:", counts, per_test, "->", args.out)
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
