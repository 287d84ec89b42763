"""Biased attention without a GPU: the composed route against the fp64 rule, the module's state-dict names, the host
dropout mask."""
import math

import pytest
import torch

from tests.battn_cases import CASES, errors, formula, inputs, outputs


@pytest.mark.parametrize("case", CASES[:3], ids=lambda c: "B%d-N%d-H%d-D%d" % c)
def test_composed_route_equals_the_formula(case):
    from dgl_amd import ops

    c = inputs(case, torch.float64)
    scale = case[3] ** -0.5
    ref = outputs(lambda q, k, v, b, m: formula(q, k, v, b, m, scale), c, torch.float64, "cpu")
    got = outputs(lambda q, k, v, b, m: ops.biased_attention(q, k, v, b, m, fused=False), c, torch.float64, "cpu")
    assert max(errors(got, ref)) <= 1e-12
    assert not ops.biased_attention_applies(c["q"], c["k"], c["v"], c["bias"], c["mask"])       # CPU tensors


def test_state_dict_key_names():
    from dgl_amd import nn

    m = nn.BiasedMHA(feat_size=16, num_heads=4)
    want = [p + s for p in ("q_proj", "k_proj", "v_proj", "out_proj") for s in (".weight", ".bias")]
    assert list(m.state_dict()) == want and "BiasedMHA" in nn.__all__
    assert list(nn.BiasedMHA(16, 4, bias=False).state_dict()) == want[::2]
    assert m(torch.randn(2, 5, 16), torch.randn(2, 5, 5, 4)).shape == (2, 5, 16)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_host_mask_share_and_seed(p):
    from dgl_amd import _capi

    B, H, N = 2, 3, 33
    keep = _capi.biased_attention_dropout_mask_host(7, p, B, H, N)
    assert keep.shape == (B, H, N, N) and keep.dtype == torch.uint8
    n = keep.numel()
    assert abs(float(keep.float().mean()) - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n)
    assert torch.equal(keep, _capi.biased_attention_dropout_mask_host(7, p, B, H, N))
    assert not torch.equal(keep, _capi.biased_attention_dropout_mask_host(8, p, B, H, N))
    assert bool(_capi.biased_attention_dropout_mask_host(7, 0.0, B, H, N).all())
