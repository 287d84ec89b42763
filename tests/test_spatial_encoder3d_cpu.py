"""The 3D spatial encoding without a GPU: the composed route against the rule of include/dgl_amd.h restated in fp64, the
module's parameters, and the refusals by name."""
import pytest
import torch

from tests.battn_cases import errors
from tests.se3d_cases import formula, inputs, module_outputs, outputs

DOC = (1, 4, 4, 8)       # the reference's docstring shape: B 1, N 4, K 4, H 8


@pytest.mark.parametrize("typed", [True, False])
def test_composed_route_is_the_rule(typed):
    from dgl_amd import ops

    c = inputs(DOC, torch.float64)
    ref = outputs(formula, c, torch.float64, "cpu", typed)
    got = outputs(lambda *a: ops.spatial_encoder_3d(*a, fused=False), c, torch.float64, "cpu", typed)
    assert max(errors(got, ref)) <= 1e-12
    through_module = module_outputs(DOC, c, torch.float64, "cpu", typed, None)
    assert errors(through_module[:1], ref[:1])[0] <= 1e-12
    if not typed:       # every pair takes row 0, the padding row: no gradient reaches the tables
        assert not through_module[1].any() and not through_module[2].any()


def test_state_dict_is_the_reference_one():
    from dgl_amd import nn

    m = nn.SpatialEncoder3d(4, 8, max_node_type=3)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "means": (4,), "stds": (4,), "linear_layer_1.weight": (4, 4), "linear_layer_1.bias": (4,),
        "linear_layer_2.weight": (8, 4), "linear_layer_2.bias": (8,), "gamma.weight": (9, 1), "beta.weight": (9, 1)}
    assert bool((m.gamma.weight == 1).all()) and bool((m.beta.weight == 0).all()) and "SpatialEncoder3d" in nn.__all__
    assert m(torch.rand(1, 4, 3), torch.tensor([[1, 0, 2, -1]])).shape == (1, 4, 4, 8)


def test_refusals():
    from dgl_amd import ops
    from dgl_amd._lib import DGLAMDError

    def call(K=4, H=8, fused=None, half=False):
        z = lambda *shape: torch.zeros(shape)
        return ops.spatial_encoder_3d(z(1, 4, 3), z(K), z(K), z(K, K), z(K), z(H, K).half() if half else z(H, K), z(H), fused=fused)

    for match, kw in (("spatial_encoder_3d: num_kernels 129", dict(K=129, fused=True)),
                      ("spatial_encoder_3d: num_heads 65", dict(H=65, fused=True)),
                      ("spatial_encoder_3d: operand dtypes differ", dict(half=True)),
                      ("spatial_encoder_3d: dgl_amd kernels run on a ROCm GPU", dict(fused=True))):
        with pytest.raises(DGLAMDError, match=match):
            call(**kw)
    assert call(K=129, H=65).shape == (1, 4, 4, 65)       # fused=None composes what the kernels refuse
