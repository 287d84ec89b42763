"""The 3D spatial encoding on the device (csrc/spatial_encoder3d.hip) against the rule of include/dgl_amd.h evaluated by
plain torch in fp64 on the CPU, on operands rounded to the case's dtype.  The bar is measured, not fixed: with e = max |x
- ref| / max |ref| per checked tensor (out and every gradient), e_fused <= 2 e_composed + u, where e_composed is the same
measure of ``fused=False`` on the same device inputs and u the unit roundoff of the dtype.  Case (4, 48, 32, 8) makes a
workgroup of the backward walk two tiles and the reduction add 256 partials; (1, 129, 8, 4) does the first for the forward."""
import pytest
import torch

from tests.battn_cases import errors
from tests.guarded import POISON_FLOAT, POISON_INDEX, guarded
from tests.se3d_cases import CASES, NAMES, formula, inputs, module_outputs, outputs, pair_vectors

pytestmark = pytest.mark.gpu

U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ids = dict(ids=lambda x: "B%d-N%d-K%d-H%d" % x if isinstance(x, tuple) else str(x).replace("torch.", ""))


def check(got, ref, comp, dtype, what, names=NAMES):
    for name, g, r, c in zip(names, got, ref, comp):
        assert bool(torch.isfinite(g).all()), (what, name)
        (e, e_comp), = zip(errors([g], [r]), errors([c], [r]))
        print(what, name, "e_fused %.3e e_composed %.3e" % (e, e_comp))
        assert e <= 2 * e_comp + U[dtype], (what, name, e, e_comp)


def against_the_rule(dev, case, c, dtype, typed, what):
    from dgl_amd import ops

    ref = outputs(formula, c, torch.float64, "cpu", typed)
    comp = outputs(lambda *a: ops.spatial_encoder_3d(*a, fused=False), c, dtype, dev, typed)
    got = outputs(lambda *a: ops.spatial_encoder_3d(*a, fused=True), c, dtype, dev, typed)
    check(got, ref, comp, dtype, what)
    modules = [module_outputs(case, c, dt, device, typed, fused)
               for dt, device, fused in ((dtype, dev, True), (torch.float64, "cpu", False), (dtype, dev, False))]
    check(*modules, dtype, what, ("module out", "gamma.weight", "beta.weight"))


@pytest.mark.parametrize("typed", [True, False], ids=["node_type", "None"])
@pytest.mark.parametrize("dtype", DTYPES, **ids)
@pytest.mark.parametrize("case", CASES, **ids)
def test_fused_against_the_fp64_rule(dev, case, dtype, typed):
    against_the_rule(dev, case, inputs(case, dtype), dtype, typed, (case, dtype, typed))


@pytest.mark.parametrize("dtype", DTYPES, **ids)
def test_coincident_points(dev, dtype):
    """Nodes 0, 1 and 7 of every batch share their coordinates (d = 0 off the diagonal too)."""
    c = dict(inputs(CASES[2], dtype))
    c["coord"] = c["coord"].clone()
    c["coord"][:, 1] = c["coord"][:, 7] = c["coord"][:, 0]
    against_the_rule(dev, CASES[2], c, dtype, True, ("coincident", dtype))


def test_two_runs_give_the_same_bits(dev):
    from dgl_amd import ops

    c = inputs(CASES[5], torch.bfloat16)
    runs = [outputs(lambda *a: ops.spatial_encoder_3d(*a, fused=True), c, torch.bfloat16, dev) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], **ids)
def test_guard_bands(dev, dtype):
    from dgl_amd import _capi

    B, N, K, H = case = CASES[2]
    c = inputs(case, dtype)
    f32 = lambda t: t.to(dev, torch.float32).contiguous()
    args = [f32(c["coord"]), [f32(t) for t in pair_vectors(c, True)], f32(c["means"]), f32(c["stds"])]
    args += [c[n].to(dev, dtype) for n in ("w1", "b1", "w2", "b2")]
    out = guarded(dev, (B, N, N, H), dtype, poison=POISON_FLOAT)
    grads = [guarded(dev, t.shape, t.dtype, poison=POISON_FLOAT) for t in args[4:] + args[2:4] + args[1]]
    ws = guarded(dev, _capi.spatial_encoder3d_workspace_bytes(B, N, K, H), torch.uint8, poison=POISON_INDEX)
    _capi.spatial_encoder3d_forward(*args, into=out.t)
    _capi.spatial_encoder3d_backward(*args, c["cot"].to(dev, dtype), into=[g.t for g in grads], ws=ws.t)
    for g, name in zip([out] + grads + [ws], NAMES + ("workspace",)):
        g.check(name)
    assert torch.equal(_capi.spatial_encoder3d_forward(*args), out.t)
    again = _capi.spatial_encoder3d_backward(*args, c["cot"].to(dev, dtype))
    assert all(torch.equal(a, g.t) for a, g in zip(again, grads))


def test_routing(dev):
    from dgl_amd import ops
    from dgl_amd._lib import DGLAMDError

    z = lambda *shape: torch.zeros(shape, device=dev)
    with pytest.raises(DGLAMDError, match="spatial_encoder_3d: num_kernels 129"):
        ops.spatial_encoder_3d(z(1, 4, 3), z(129), z(129), z(129, 129), z(129), z(2, 129), z(2), fused=True)
    with pytest.raises(DGLAMDError, match="spatial_encoder_3d: num_kernels 129"):
        from dgl_amd import _capi
        _capi.spatial_encoder3d_forward(z(1, 4, 3), [z(1, 4)] * 4, z(129), z(129), z(129, 129), z(129), z(2, 129), z(2))
    c = inputs(CASES[1], torch.float32)
    args = [c[n].to(dev, torch.float32) for n in ("coord", "means", "stds", "w1", "b1", "w2", "b2")]
    args[0].requires_grad_()
    with pytest.raises(DGLAMDError, match="spatial_encoder_3d: the gradient with respect to coord"):
        ops.spatial_encoder_3d(*args, fused=True)
    auto = ops.spatial_encoder_3d(*args)
    assert torch.equal(auto, ops.spatial_encoder_3d(*args, fused=False))
    auto.sum().backward()
    assert args[0].grad is not None and bool(torch.isfinite(args[0].grad).all())
    assert ops.spatial_encoder_3d(z(0, 4, 3), *args[1:], fused=True).shape == (0, 4, 4, 8)      # no pairs: no launch
