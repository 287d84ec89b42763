"""Edge-wise mini-batches for link prediction and edge classification, with the call shapes of ``dgl.dataloading``
(python/dgl/dataloading/base.py): ``find_exclude_eids``, ``EdgePredictionSampler`` and ``as_edge_prediction_sampler``.

A batch of seed edges becomes ``(input_nodes, pair_graph, blocks)`` or, with a negative sampler, ``(input_nodes,
pair_graph, neg_graph, blocks)``: the pair graph holds the seed edges (``edata[dgl.EID]`` = their ids) and the negative
graph the drawn pairs, both over ONE compact node space (:func:`dgl_amd.compact_graphs`); the blocks are the wrapped
node sampler's on that node space, with the seed edges (and, by mode, their reverses) dropped from every layer after
the picks (csrc/exclude.hip).  A ``DataLoader`` is not part of this module: iterate over batches of edge ids and call
``sampler.sample(g, eids)``.
"""
import inspect
from collections.abc import Mapping

import torch

from . import _capi, negative_sampler  # noqa: F401  (negative_sampler is re-exported, as in dgl.dataloading)
from ._lib import DGLAMDError as _DGLError
from .heterograph import graph as _graph, heterograph as _heterograph
from .sampling import (EID, NID, LaborSampler, NeighborSampler, SAINTSampler, ShaDowKHopSampler,  # noqa: F401
                       _mark_exclusion_set)
from .transforms import compact_graphs

__all__ = ["find_exclude_eids", "EdgePredictionSampler", "as_edge_prediction_sampler", "NeighborSampler", "LaborSampler",
           "ShaDowKHopSampler", "SAINTSampler", "negative_sampler"]


def _is_ids(x):
    return torch.is_tensor(x) or (isinstance(x, Mapping) and all(torch.is_tensor(v) for v in x.values()))


def _ids_on(g, c, ids):
    rel = g._graph.relations[g.get_etype_id(c)]
    return torch.as_tensor(ids).reshape(-1).to(device=rel.device, dtype=rel.idtype).contiguous(), rel


def _with_reverse_ids(g, c, ids, reverse):
    """``sort(ids ++ reverse[ids])`` of one relation: the set kernel on a GPU graph, its host twin on a CPU graph."""
    ids, rel = _ids_on(g, c, ids)
    reverse = torch.as_tensor(reverse).reshape(-1).to(device=rel.device, dtype=rel.idtype).contiguous()
    if reverse.shape[0] != rel.num_edges:
        raise _DGLError("find_exclude_eids: reverse_eids must map every edge of %s (%d), got %d entries"
                        % ((c,), rel.num_edges, reverse.shape[0]))
    if rel.device.type == "cuda":
        return _mark_exclusion_set(_capi.exclude_set(ids, rel.num_edges, reverse=reverse))
    x, flags = _capi.exclude_set_host(ids, rel.num_edges, reverse=reverse)
    if flags & _capi.EXCLUDE_OUT_OF_RANGE:
        raise _DGLError("find_exclude_eids: edge id out of range")
    return x


def find_exclude_eids(g, seed_edges, exclude, reverse_eids=None, reverse_etypes=None, output_device=None):
    """The edge ids to drop from the blocks of the batch ``seed_edges`` (ids, or a dict per edge type), by mode:

    None: nothing.  ``"self"``: the seed edges.  ``"reverse_id"``: the seed edges and, per edge type, the edges
    ``reverse_eids[seed]`` of the same type; the result is sorted and may hold an id twice.  ``"reverse_types"``: the
    seed edges of type ``t`` also under type ``reverse_etypes[t]`` with the same ids, two lists of one type merged by
    concatenation.  A callable: whatever it returns for ``seed_edges``.  A tensor or a dict of tensors: itself."""
    if exclude is None:
        out = None
    elif callable(exclude):
        out = exclude(seed_edges)
    elif _is_ids(exclude):
        out = exclude
    elif exclude == "self":
        out = seed_edges
    elif exclude == "reverse_id":
        if reverse_eids is None:
            raise _DGLError('find_exclude_eids: exclude="reverse_id" needs reverse_eids')
        if isinstance(seed_edges, Mapping):
            rev = {g.to_canonical_etype(k): v for k, v in reverse_eids.items()}
            out = {c: _with_reverse_ids(g, c, v, rev[c])
                   for c, v in ((g.to_canonical_etype(k), v) for k, v in seed_edges.items())}
        else:
            if len(g.canonical_etypes) != 1:
                raise _DGLError("please specify a dict of etypes and ids for graphs with multiple edge types")
            out = _with_reverse_ids(g, g.canonical_etypes[0], seed_edges, reverse_eids)
    elif exclude == "reverse_types":
        if reverse_etypes is None or not isinstance(seed_edges, Mapping):
            raise _DGLError('find_exclude_eids: exclude="reverse_types" needs reverse_etypes and a dict of seed edges')
        seeds = {g.to_canonical_etype(k): v for k, v in seed_edges.items()}
        out = dict(seeds)
        for k, v in reverse_etypes.items():
            k, v = g.to_canonical_etype(k), g.to_canonical_etype(v)
            if k in seeds:
                out[v] = torch.cat([out[v], seeds[k]]) if v in out else seeds[k]
    else:
        raise ValueError("unsupported mode {}".format(exclude))
    if out is not None and output_device is not None:
        out = {k: v.to(output_device) for k, v in out.items()} if isinstance(out, Mapping) else out.to(output_device)
    return out


class EdgePredictionSampler:
    """A node-wise sampler wrapped into an edge-wise one (dataloading/base.py EdgePredictionSampler); see
    :func:`as_edge_prediction_sampler`."""

    def __init__(self, sampler, exclude=None, reverse_eids=None, reverse_etypes=None, negative_sampler=None,
                 prefetch_labels=None):
        if len(inspect.getfullargspec(sampler.sample).args) < 4:        # self, g, indices, exclude_eids
            raise TypeError("This sampler does not support edge or link prediction; please add an"
                            "optional third argument for edge IDs to exclude in its sample() method.")
        self.sampler = sampler
        self.exclude = exclude
        self.reverse_eids = reverse_eids
        self.reverse_etypes = reverse_etypes
        self.negative_sampler = negative_sampler
        self.prefetch_labels = prefetch_labels or []    # accepted and ignored: there is no lazy feature loading here
        self.output_device = getattr(sampler, "output_device", None)

    @staticmethod
    def _pair_graph(g, pairs):
        """A graph on the node space of ``g`` with the (src, dst) pairs of ``pairs`` ({canonical edge type: pairs}) as
        edges; edge types without pairs stay empty."""
        dev, idt = g.device, g.idtype
        empty = torch.empty(0, dtype=idt, device=dev)
        data = {c: tuple(t.to(device=dev, dtype=idt) for t in pairs[c]) if c in pairs else (empty, empty)
                for c in g.canonical_etypes}
        if len(g.canonical_etypes) == 1 and len(g.ntypes) == 1:
            return _graph(data[g.canonical_etypes[0]], num_nodes=g.num_nodes(), idtype=idt, device=dev)
        return _heterograph(data, {n: g.num_nodes(n) for n in g.ntypes}, idtype=idt, device=dev)

    def sample(self, g, seed_edges):
        """``(input_nodes, pair_graph, blocks)``, or ``(input_nodes, pair_graph, neg_graph, blocks)`` with a negative
        sampler."""
        if isinstance(seed_edges, Mapping):
            seeds = {g.to_canonical_etype(k): torch.as_tensor(v).reshape(-1) for k, v in seed_edges.items()}
            seed_edges = seeds
        else:
            if len(g.canonical_etypes) != 1:
                raise _DGLError("please specify a dict of etypes and ids for graphs with multiple edge types")
            seed_edges = torch.as_tensor(seed_edges).reshape(-1)
            seeds = {g.canonical_etypes[0]: seed_edges}
        # the pair graph straight from the seed edges' end points (no unique over them: compaction renumbers)
        pair_graph = self._pair_graph(g, {c: g.find_edges(v.to(g.device), etype=c) for c, v in seeds.items()})
        if self.negative_sampler is not None:
            neg = self.negative_sampler(g, seed_edges)
            if not isinstance(neg, Mapping):
                if len(g.canonical_etypes) != 1:
                    raise _DGLError("graph has multiple or no edge types; please return a dict in negative sampler.")
                neg = {g.canonical_etypes[0]: neg}
            neg_graph = self._pair_graph(g, {g.to_canonical_etype(k): v for k, v in neg.items()})
            pair_graph, neg_graph = compact_graphs([pair_graph, neg_graph])
        else:
            pair_graph = compact_graphs(pair_graph)
        for c, v in seeds.items():
            pair_graph._edge_frames[pair_graph.get_etype_id(c)][EID] = v.to(device=g.device, dtype=g.idtype)
        if len(g.ntypes) == 1:
            seed_nodes = pair_graph.ndata[NID]
        else:
            seed_nodes = {n: pair_graph.nodes[n].data[NID] for n in g.ntypes}
        exclude_eids = find_exclude_eids(g, seed_edges, self.exclude, self.reverse_eids, self.reverse_etypes,
                                         self.output_device)
        input_nodes, _, blocks = self.sampler.sample(g, seed_nodes, exclude_eids)
        if self.negative_sampler is None:
            return input_nodes, pair_graph, blocks
        return input_nodes, pair_graph, neg_graph, blocks


def as_edge_prediction_sampler(sampler, exclude=None, reverse_eids=None, reverse_etypes=None, negative_sampler=None,
                               prefetch_labels=None):
    """``dgl.dataloading.as_edge_prediction_sampler``: an edge-wise sampler from a node-wise one.  For a batch of seed
    edges it runs ``sampler`` on their end points (and on the end points of the negative pairs, when
    ``negative_sampler`` is one of :mod:`dgl_amd.negative_sampler` or any callable of its shape) with the edges that
    ``exclude`` names dropped: see :func:`find_exclude_eids` for the modes, ``reverse_eids`` and ``reverse_etypes``.
    ``prefetch_labels`` is accepted and ignored."""
    return EdgePredictionSampler(sampler, exclude=exclude, reverse_eids=reverse_eids, reverse_etypes=reverse_etypes,
                                 negative_sampler=negative_sampler, prefetch_labels=prefetch_labels)
