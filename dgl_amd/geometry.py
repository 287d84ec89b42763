"""``dgl.geometry``: what the reference's geometry package runs on the GPU.

``farthest_point_sampler`` mirrors python/dgl/geometry/fps.py over csrc/knn.hip (the rule: include/dgl_amd.h
"Point-cloud graphs"): one workgroup per cloud, the whole sample loop in one launch, ties to the smaller row, the same
bytes on every run.  ``neighbor_matching`` is not here."""
import torch

from . import _capi
from ._lib import DGLAMDError as _DGLError

__all__ = ["farthest_point_sampler"]


def farthest_point_sampler(pos, npoints, start_idx=None, seed=None):
    """Farthest point sampling of every cloud of ``pos`` (B, N, C): (B, npoints) int64 row numbers inside each cloud,
    column 0 the start row.  Each further sample is the row farthest from the samples so far (squared Euclidean
    distance in ``pos``'s dtype, fp32 or fp64); ties go to the smaller row and no row is returned twice.

    ``start_idx`` (an int, checked like the reference: ``0 <= start_idx < N``) starts every cloud at that row.  Without
    it one start per cloud is drawn uniformly from ``[0, N)``: from a generator seeded with ``seed`` when given (the
    same ``seed`` gives the same result), else from torch's generator of ``pos``'s device.  There is no CPU path."""
    if pos.dim() != 3:
        raise _DGLError("farthest_point_sampler: pos must have shape (B, N, C), got %s" % (tuple(pos.shape),))
    B, N, _ = pos.shape
    if start_idx is None:
        gen = None
        if seed is not None:
            gen = torch.Generator(device=pos.device)
            gen.manual_seed(int(seed))
        start = torch.randint(0, max(N, 1), (B,), dtype=torch.int64, device=pos.device, generator=gen)
    else:
        if start_idx >= N or start_idx < 0:
            raise _DGLError("Invalid start_idx, expected 0 <= start_idx < {}, got {}".format(N, start_idx))
        start = torch.full((B,), int(start_idx), dtype=torch.int64, device=pos.device)
    return _capi.fps(pos.contiguous(), npoints, start)
