"""What the two biased-attention test files share: the cases, the rule of include/dgl_amd.h "Biased attention" in plain
torch (evaluated in fp64 by the tests), and the error measure."""
import torch

#        B  N    H   D
CASES = [(1, 1, 1, 1),       # degenerate sizes
         (2, 33, 3, 24),     # one past a tile both ways; a head group with a tail; D padded to the K step; the batch stride
         (1, 65, 8, 64),     # several key tiles
         (2, 100, 4, 128),   # the widest head
         (1, 130, 32, 8)]    # five key tiles (of 32) of rescaling, many heads
NAMES = ("out", "dq", "dk", "dv", "dbias")
_inputs = {}


def inputs(case, dtype):
    """The case's fp64 CPU operands, already rounded to `dtype`, built once: q, k, v, bias, mask (>= 1 open key per
    row) and the cotangent."""
    if (case, dtype) not in _inputs:
        B, N, H, D = case
        gen = torch.Generator().manual_seed(sum(case))
        r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype).double()
        mask = torch.rand((B, N, N), generator=gen) < 0.3
        mask[:, torch.arange(N), torch.randint(0, N, (N,), generator=gen)] = False
        _inputs[(case, dtype)] = dict(q=r(B, N, H, D), k=r(B, N, H, D), v=r(B, N, H, D), bias=r(B, N, N, H), mask=mask,
                                      cot=r(B, N, H, D))
    return _inputs[(case, dtype)]


def formula(q, k, v, bias, mask, scale, keep=None, p=0.0):
    """The rule, rows without a finite score included: they give zeros.  `keep` is (B, H, N, N)."""
    s = torch.einsum("bihd,bjhd->bijh", q, k) * scale
    if bias is not None:
        s = s + bias
    if mask is not None:
        s = s.masked_fill(mask.to(torch.bool)[..., None], float("-inf"))
    dead = torch.isinf(s).all(dim=2, keepdim=True)
    w = torch.softmax(s.masked_fill(dead, 0.0), dim=2).masked_fill(dead, 0.0)
    if keep is not None:
        w = w * keep.permute(0, 2, 3, 1).to(w.dtype) / (1.0 - p)
    return torch.einsum("bijh,bjhd->bihd", w, v)


def outputs(fn, c, dtype, device, with_bias=True, with_mask=True):
    """[out, dq, dk, dv, dbias] (fp64, CPU; dbias None without a bias) of ``fn(q, k, v, bias, mask)`` on the operands
    of `c` as `dtype` leaves on `device`, with the cotangent of `c`."""
    leaf = lambda t: t.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    q, k, v = leaf(c["q"]), leaf(c["k"]), leaf(c["v"])
    bias = leaf(c["bias"]) if with_bias else None
    out = fn(q, k, v, bias, c["mask"].to(device) if with_mask else None)
    out.backward(c["cot"].to(device=device, dtype=dtype))
    return [t.detach().double().cpu() for t in (out, q.grad, k.grad, v.grad)] + [None if bias is None else bias.grad.double().cpu()]


def errors(got, ref):
    """max |x - ref| / max |ref| per checked tensor (the plain max |x| where the reference is all zero)."""
    return [None if r is None else float((g - r).abs().max() / (r.abs().max() if r.abs().max() > 0 else 1.0))
            for g, r in zip(got, ref)]
