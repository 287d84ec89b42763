"""Negative samplers with the call shape of ``dgl.dataloading.negative_sampler``
(python/dgl/dataloading/negative_sampler.py): a sampler is called with the graph and the edge ids of a mini-batch (a
tensor, or a dict of edge type -> tensor on a graph with several edge types) and returns ``(src, dst)`` pairs (or a
dict of canonical edge type -> pairs).

``PerSourceUniform`` (alias ``Uniform``) keeps the source of every edge and draws ``k`` destinations for it: plain
torch, no kernel.  ``GlobalUniform`` draws both ends and guarantees that no pair is an edge: the device sampler of
:func:`dgl_amd.sampling.global_uniform_negative_sampling` (csrc/negative_sampling.hip)."""
from collections.abc import Mapping

import torch

from ._lib import DGLAMDError as _DGLError

__all__ = ["PerSourceUniform", "Uniform", "GlobalUniform"]


class _NegativeSampler:
    def _generate(self, g, eids, canonical_etype):
        raise NotImplementedError

    def __call__(self, g, eids):
        if isinstance(eids, Mapping):
            return {c: self._generate(g, ids, c) for c, ids in ((g.to_canonical_etype(k), v) for k, v in eids.items())}
        if len(g.canonical_etypes) != 1:
            raise _DGLError("please specify a dict of etypes and ids for graphs with multiple edge types")
        return self._generate(g, eids, g.canonical_etypes[0])


class PerSourceUniform(_NegativeSampler):
    """For every edge ``(u, v)`` of the batch, ``k`` pairs ``(u, v')`` with ``v'`` uniform over the destination node
    type: ``k * len(eids)`` pairs in the dtype and on the device of ``eids``, the ``k`` pairs of an edge next to each
    other.  A pair may be an edge."""

    def __init__(self, k):
        self.k = int(k)

    def _generate(self, g, eids, canonical_etype):
        eids = torch.as_tensor(eids)
        src, _ = g.find_edges(eids, etype=canonical_etype)
        src = src.to(device=eids.device, dtype=eids.dtype).repeat_interleave(self.k)
        dst = torch.randint(0, max(g.num_nodes(canonical_etype[2]), 1), (eids.shape[0] * self.k,), dtype=eids.dtype,
                            device=eids.device)
        return src, dst


Uniform = PerSourceUniform


class GlobalUniform(_NegativeSampler):
    """At most ``k * len(eids)`` pairs ``(u', v')``, both ends uniform over their node types, none of them an edge of
    the type (and no self-loop when ``exclude_self_loops``; distinct unless ``replace``).  ``redundancy`` and ``seed``
    are handed on to :func:`dgl_amd.sampling.global_uniform_negative_sampling`."""

    def __init__(self, k, exclude_self_loops=True, replace=False, redundancy=None, seed=None):
        self.k = int(k)
        self.exclude_self_loops = exclude_self_loops
        self.replace = replace
        self.redundancy = redundancy
        self.seed = seed

    def _generate(self, g, eids, canonical_etype):
        return g.global_uniform_negative_sampling(len(eids) * self.k, self.exclude_self_loops, self.replace,
                                                  canonical_etype, self.redundancy, self.seed)
