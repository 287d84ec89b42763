"""``dgl.geometry``: what the reference's geometry package runs on the GPU.

``farthest_point_sampler`` mirrors python/dgl/geometry/fps.py over csrc/knn.hip (the rule: include/dgl_amd.h
"Point-cloud graphs"): one workgroup per cloud, the whole sample loop in one launch, ties to the smaller row, the same
bytes on every run.

``neighbor_matching`` mirrors python/dgl/geometry/edge_coarsening.py over csrc/matching.hip (the rule: include/dgl_amd.h
"Graph matching"): the colour / propose / respond loop of Graclus and Metis coarsening as a pure function of
(graph, weights, seed), two launches per round and one word read back per batch of rounds."""
import torch

from . import _capi
from ._lib import DGLAMDError as _DGLError
from .sampling import _call_seed

__all__ = ["farthest_point_sampler", "neighbor_matching"]


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


def neighbor_matching(graph, e_weights=None, relabel_idx=True, seed=None):
    """Edge coarsening of Metis / Graclus on a homogeneous, bi-directed GPU graph: every node is matched with at most one
    neighbour (the heaviest free one when ``e_weights``, one non-negative value per edge, is given; ties and the
    unweighted form are broken at random), until no two unmatched nodes are adjacent.  Returns an ``(N,)`` tensor of the
    graph's idtype on its device: with ``relabel_idx`` consecutive cluster ids in ascending order of the cluster's
    smaller node, else that smaller node's id.  Self-loops take no part (the kernels skip them; no graph is rebuilt).

    ``seed=None`` draws the seed from torch's generator; the same ``seed`` gives the same result on every run.  A graph
    that is not bi-directed may never finish: after 256 rounds the call raises.  There is no CPU path."""
    if len(graph.canonical_etypes) != 1 or len(graph.ntypes) != 1:
        raise _DGLError("neighbor_matching: The graph used in graph node matching must be homogeneous")
    rel = graph._graph.relations[0]
    dev = graph.device
    if e_weights is not None:
        if not torch.is_tensor(e_weights) or e_weights.dim() == 0 or e_weights.numel() != rel.num_edges \
                or e_weights.shape[0] != rel.num_edges:
            raise _DGLError("neighbor_matching: e_weights must hold one value per edge of the graph (%d), got shape %s"
                            % (rel.num_edges, tuple(getattr(e_weights, "shape", ()))))
        if e_weights.device != dev:
            raise _DGLError("neighbor_matching: e_weights is on %s, the graph on %s" % (e_weights.device, dev))
        if not e_weights.is_floating_point():
            e_weights = e_weights.to(torch.float32)
        e_weights = e_weights.reshape(-1).contiguous()
    fmt = rel.csr()
    csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], rel.num_dst)    # (refuses a CPU graph: no CPU fallback)
    label, _ = _capi.neighbor_matching(csr, e_weights, _call_seed(seed), relabel=bool(relabel_idx))
    return label
