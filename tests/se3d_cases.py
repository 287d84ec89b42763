"""What the two 3D spatial encoding test files share: the cases, the rule of include/dgl_amd.h "3D spatial encoding" in
plain torch (evaluated in fp64 by the tests), and the runners that return the checked tensors."""
import torch

#        B  N    K    H
CASES = [(1, 1, 1, 1),       # degenerate
         (1, 5, 4, 8),       # 25 pairs, less than one tile
         (2, 33, 20, 3),     # K and H off every tile size; 2 178 pairs, tiles that cross rows and batches
         (1, 64, 128, 32),   # full K, the usual H
         (3, 17, 128, 64),   # the largest H
         (4, 48, 32, 8),     # 288 tiles: the backward's 256 workgroups take up to two, the reduction adds 256 partials
         (1, 129, 8, 4)]     # 521 tiles, the smallest N at which one of the forward's 512 workgroups takes two
NAMES = ("out", "w1", "b1", "w2", "b2", "means", "stds", "gamma_src", "gamma_tgt", "beta_src", "beta_tgt")
MAX_TYPE = 5
_inputs = {}


def inputs(case, dtype):
    """The case's fp64 CPU operands, built once: the weights rounded to `dtype`, everything else to fp32.  `state` is the
    module's state dict (random gamma / beta tables), `node_type` has padded nodes (-1)."""
    if (case, dtype) not in _inputs:
        B, N, K, H = case
        gen = torch.Generator().manual_seed(sum(case))
        u = lambda lo, hi, *shape: (torch.rand(shape, generator=gen, dtype=torch.float64) * (hi - lo) + lo)
        r = lambda t, dt=torch.float32: t.to(dt).double()
        bound = K ** -0.5                                        # nn.Linear's initialisation
        c = dict(coord=r(u(0, 3, B, N, 3)), means=r(u(0, 3, K)), stds=r(u(0, 3, K)),
                 w1=r(u(-bound, bound, K, K), dtype), b1=r(u(-bound, bound, K), dtype),
                 w2=r(u(-bound, bound, H, K), dtype), b2=r(u(-bound, bound, H), dtype),
                 gamma=r(u(0.5, 1.5, 2 * MAX_TYPE + 3, 1)), beta=r(u(-0.5, 0.5, 2 * MAX_TYPE + 3, 1)),
                 node_type=torch.randint(-1, MAX_TYPE, (B, N), generator=gen), cot=r(u(-1, 1, B, N, N, H), dtype))
        c["state"] = {"means": c["means"], "stds": c["stds"], "linear_layer_1.weight": c["w1"], "linear_layer_1.bias": c["b1"],
                      "linear_layer_2.weight": c["w2"], "linear_layer_2.bias": c["b2"], "gamma.weight": c["gamma"],
                      "beta.weight": c["beta"]}
        _inputs[(case, dtype)] = c
    return _inputs[(case, dtype)]


def pair_vectors(c, typed):
    """gamma_src, gamma_tgt, beta_src, beta_tgt (B, N): rows node_type + 2 and node_type + MAX_TYPE + 3, or row 0."""
    src, tgt = (c["node_type"] + 2, c["node_type"] + MAX_TYPE + 3) if typed else (torch.zeros_like(c["node_type"]),) * 2
    return [c[t][ids, 0] for t in ("gamma", "beta") for ids in (src, tgt)]


def formula(coord, means, stds, w1, b1, w2, b2, gs, gt, bs, bt):
    """The rule, term by term."""
    d = (coord[:, :, None, :] - coord[:, None, :, :]).pow(2).sum(-1).sqrt()
    x = (gs[:, :, None] + gt[:, None, :]) * d + (bs[:, :, None] + bt[:, None, :])
    sd = stds.abs() + 1e-2
    g = torch.exp(-0.5 * ((x[..., None] - means) / sd) ** 2) / ((2 * 3.14159) ** 0.5 * sd)
    z1 = g @ w1.t() + b1
    h = 0.5 * z1 * (1 + torch.erf(z1 / 2 ** 0.5))
    return h @ w2.t() + b2


def outputs(fn, c, dtype, device, typed=True):
    """NAMES: out and the ten gradients (fp64, CPU) of ``fn(coord, means, stds, w1, b1, w2, b2, *pair vectors)`` on
    the operands of `c` as leaves on `device`, the weights in `dtype`, with the cotangent of `c`."""
    small = torch.float64 if dtype == torch.float64 else torch.float32
    leaf = lambda t, dt: t.detach().clone().to(device=device, dtype=dt).requires_grad_()
    w = [leaf(c[n], dtype) for n in ("w1", "b1", "w2", "b2")]
    s = [leaf(t, small) for t in [c["means"], c["stds"]] + pair_vectors(c, typed)]
    out = fn(c["coord"].to(device=device, dtype=small), s[0], s[1], *w, *s[2:])
    out.backward(c["cot"].to(device=device, dtype=dtype))
    return [t.detach().double().cpu() for t in [out] + [x.grad for x in w + s]]


def module_outputs(case, c, dtype, device, typed, fused):
    """out and the gradients of the gamma and beta tables through dgl_amd.nn.SpatialEncoder3d with the state of `c`."""
    from dgl_amd import nn

    m = nn.SpatialEncoder3d(case[2], case[3], MAX_TYPE).double()
    m.load_state_dict(c["state"])
    m = m.to(device=device, dtype=torch.float64 if dtype == torch.float64 else torch.float32)
    m.linear_layer_1.to(dtype), m.linear_layer_2.to(dtype)          # (only the weights take the case's dtype)
    out = m(c["coord"].to(device=device, dtype=m.means.dtype), c["node_type"].to(device) if typed else None, fused=fused)
    out.backward(c["cot"].to(device=device, dtype=dtype))
    return [t.detach().double().cpu() for t in (out, m.gamma.weight.grad, m.beta.weight.grad)]
