"""The torch composition of the Graphormer bias (fused=False, and CPU tensors) against the fp64 formula; needs no GPU."""
import pytest
import torch

from tests.test_zzzzzzzzzzzzzzzzzzzzzz_gpu_graphormer_bias import CASES, formula, inputs


@pytest.mark.parametrize("case", CASES[1:4], ids=lambda c: "P%d-Lp%d-L%d-H%d-d%d-E%d" % c)
def test_composition_on_the_cpu(case):
    from dgl_amd import ops
    from dgl_amd._lib import DGLAMDError

    max_len = case[2]
    c = inputs(case)
    q, s = formula(c["dist"], c["paths"], c["X"], c["W"], c["S"], max_len)
    X, W, S = (c[k].float() for k in ("X", "W", "S"))
    bar = 2.0 ** -22 * (q.abs() + s.abs())
    for fused in (None, False):
        out = ops.graphormer_bias(c["dist"], c["paths"], X, W, S, max_len=max_len, fused=fused)
        assert bool(((out.double() - (q + s)).abs() <= bar).all())
        out = ops.graphormer_bias_gather(c["dist"], c["paths"], X @ W.t(), S, max_len=max_len, fused=fused)
        assert bool(((out.double() - (q + s)).abs() <= bar).all())
    with pytest.raises(DGLAMDError, match="no CPU fallback"):
        ops.graphormer_bias(c["dist"], c["paths"], X, W, S, max_len=max_len, fused=True)
