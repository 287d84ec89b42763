"""The REFERENCE'S OWN test suites, unmodified, inside `pytest -m gpu` (VERDICT r5 Next #1b).

`tools/ref_suite/run.py --prepare --src <reference checkout>/tests` copies the suites' files into scratch/ref_tests/
(git-ignored) and `--collect --suite S --device cpu` writes their test ids; here every reference test id is one pytest test:
a session fixture runs each suite ONCE in a subprocess (`tools/ref_suite/run.py`: `import dgl` -> dgl_amd, the
reference's files executed as they are, DGLTESTDEV=gpu) and each id asserts its own outcome.  Suites:

  ops       tests/python/common/ops/test_ops.py (test_spmm, test_sddmm, test_half_spmm, test_segment_reduce, segment_mm,
            gather_mm), test_edge_softmax.py, test_heterograph-kernel.py (test_all_binary_builtins ...)   — the hot path
  mp        test_heterograph-update-all / -apply-edges / -specialization, test_readout, test_to_block
  nn        tests/python/pytorch/nn/test_nn.py (GraphConv, SAGEConv, GATConv, RelGraphConv, HeteroGraphConv, TypedLinear):
            the reference's own LAYER files imported unmodified over the alias (dgl_amd ships no layer code)
  sampling, sparse   the callers either side of the path

Named test_zz_* so that it runs after the package's own parity tests.  The reference's files are not part of this
repository, so on a checkout where they were never prepared it skips with a reason."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEST = os.path.join(ROOT, "scratch", "ref_tests")
SUITES = ("ops", "mp", "nn", "sampling", "sparse")
MIN_PASSED = {"ops": 2000, "mp": 150, "nn": 900, "sampling": 4, "sparse": 1200}
pytestmark = pytest.mark.gpu


def _ids(suite):
    try:
        with open(os.path.join(DEST, "ids_%s.json" % suite)) as fh:
            return json.load(fh)
    except OSError:
        return []


_RESULTS = {}


def _run(suite):
    if suite not in _RESULTS:
        out = os.path.join(ROOT, "gpurun_out", "ref_suite_%s.jsonl" % suite)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ref_suite", "run.py"), "--suite", suite, "--out", out],
                           cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
        rows, summary = {}, {}
        if os.path.exists(out):
            with open(out) as fh:
                lines = [json.loads(l) for l in fh if l.strip()]
            summary, rows = lines[0], {r["id"]: r for r in lines[1:]}
        _RESULTS[suite] = (p.returncode, summary, rows, p.stdout[-3000:])
    return _RESULTS[suite]


def _need():
    if not os.path.isdir(DEST):
        pytest.skip("scratch/ref_tests is absent: the reference's suites are prepared there by hand "
                    "(tools/ref_suite/run.py --prepare, then --collect per suite)")


@pytest.mark.parametrize("suite", SUITES)
def test_reference_suite_totals(dev, suite):
    """0 failed / errored, and at least as many passed as the suite has always had."""
    _need()
    rc, summary, rows, tail = _run(suite)
    counts = summary.get("summary", {})
    bad = {k: v for k, v in counts.items() if k not in ("passed", "skipped")}
    assert rc == 0 and not bad, "suite %s: rc %d, %s\n%s" % (suite, rc, counts, tail)
    assert counts.get("passed", 0) >= MIN_PASSED[suite], (suite, counts)
    assert len(rows) == len(_ids(suite)), "suite %s ran %d ids, build() collected %d" % (suite, len(rows), len(_ids(suite)))


def pytest_generate_tests(metafunc):
    if "ref_id" in metafunc.fixturenames:
        ids = [(s, i) for s in SUITES for i in _ids(s)]
        metafunc.parametrize("suite_of_id,ref_id", ids or [pytest.param("", "", marks=pytest.mark.skip(
            reason="scratch/ref_tests is absent (tools/ref_suite/run.py --prepare / --collect make it)"))],
            ids=[i for _, i in ids] or None)


def test_reference_id(dev, suite_of_id, ref_id):
    """One reference test id: the outcome the reference's own assertion produced on this package."""
    _need()
    _, _, rows, tail = _run(suite_of_id)
    r = rows.get(ref_id)
    assert r is not None, "%s did not run\n%s" % (ref_id, tail)
    if r["outcome"] == "skipped":
        pytest.skip("skipped by the reference's own test")
    assert r["outcome"] == "passed", "%s: %s\n%s" % (ref_id, r["outcome"], r.get("detail", ""))
