"""Uniform neighbour sampling and message-flow blocks for mini-batch training.

Mirror of ``dgl.sampling.sample_neighbors`` (python/dgl/sampling/neighbor.py:222-395), ``dgl.to_block``
(python/dgl/transforms/functional.py) and ``dgl.dataloading.NeighborSampler.sample_blocks``
(python/dgl/dataloading/neighbor_sampler.py): the steps that run in front of the g-SpMM for every
mini-batch of GraphSAGE (BASELINE config 4).  The kernels are in csrc/sampling.hip; the blocks come out
with their in-edge CSR already built (rows = seeds), i.e. in the format the SpMM consumes — no COO
round trip.  Graphs with several relations (round 5): ``nodes`` / ``fanout`` / ``dst_nodes`` are given per
node / edge type as in the reference, every relation goes through the same two kernels, and a
block keeps one source and one destination node set per node type (R-GCN mini-batches).

``random_walk`` / ``pack_traces`` mirror ``dgl.sampling.random_walk`` / ``pack_traces``
(python/dgl/sampling/randomwalks.py:31-310) over csrc/random_walk.hip: metapath, weighted and restart walks.
``RandomWalkNeighborSampler`` / ``PinSAGESampler`` mirror python/dgl/sampling/pinsage.py:27-272: those walks followed by
the visit-count top-k of csrc/pinsage.hip.  ``node2vec_random_walk`` mirrors python/dgl/sampling/node2vec_randomwalk.py
over csrc/node2vec.hip: the bounded second-order step of csrc/node2vec_step.h.  ``global_uniform_negative_sampling`` mirrors
python/dgl/sampling/negative.py over csrc/negative_sampling.hip (the rule: csrc/negative_sample_step.h).  ``sample_labors`` /
``LaborSampler`` mirror python/dgl/sampling/labor.py and python/dgl/dataloading/labor_sampler.py over csrc/labor.hip:
layer-neighbour sampling, one variate per source node (the rule: csrc/labor_step.h).  ``select_topk`` mirrors
``dgl.sampling.select_topk`` (python/dgl/sampling/neighbor.py:880) over csrc/topk.hip: the k heaviest (or lightest) edges of
every node in one pass over its row (the rule: csrc/topk_step.h).
"""
import math

import torch

from . import _capi
from ._lib import DGLAMDError as _DGLError
from .graph_index import GraphIndex, Relation
from .heterograph import DGLGraph, heterograph as _heterograph

NID = "_ID"   # dgl.NID / dgl.EID
EID = "_ID"


def _call_seed(seed):
    """The seed of one call: ``seed=None`` draws it from torch's global CPU generator, an integer is taken as given."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


def _node_ids(nodes, device, idtype):
    """``nodes`` (ids, a list or one id) as a contiguous 1-D tensor of the graph's id type on its device."""
    return torch.as_tensor(nodes).reshape(-1).to(device=device, dtype=idtype).contiguous()


def _relation_slot(rel, name, keyed_tensors, build):
    """What ``build()`` returns, kept in ONE slot ``name`` on relation ``rel``: keyed by the address, ``_version``, shape,
    dtype and device of ``keyed_tensors`` and checked at every use (as ``static_features`` checks its promise), so an
    in-place write to one of them rebuilds it."""
    key = tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype, t.device) for t in keyed_tensors)
    slot = getattr(rel, name, None)
    if slot is None or slot[0] != key:
        slot = (key, build())
        setattr(rel, name, slot)
    return slot[1]


def _csc_of(g):
    rel = g._graph.relations[0]
    indptr, indices, eids = rel.csc()
    return rel, _capi.make_csr(indptr, indices, eids, rel.num_src), (indptr, indices, eids)


def _node_map(g, device, ntid=None):
    """Per-graph (per node type) dense node -> local-id scratch (int32, all -1 between calls)."""
    if ntid is None:
        m = getattr(g, "_sampling_node_map", None)
        if m is None or m.device != device:
            m = torch.full((g.num_nodes(),), -1, dtype=torch.int32, device=device)
            g._sampling_node_map = m
        return m
    maps = g.__dict__.setdefault("_sampling_node_maps", {})
    m = maps.get(ntid)
    if m is None or m.device != device:
        m = maps[ntid] = torch.full((max(1, g._graph.num_nodes(ntid)),), -1, dtype=torch.int32, device=device)
    return m


def _prob_of(prob, frame, rel, who):
    """The sampling weights of one relation as a contiguous float vector (None: uniform)."""
    if prob is None:
        return None
    p = frame[prob] if isinstance(prob, str) else prob
    # the kernels index `prob` by EDGE ID of g: anything else is an out-of-bounds device read
    # (reference: CHECK on the probability array's length, src/array/array.cc RowWiseSampling)
    if p.dim() == 0 or p.shape[0] != rel.num_edges or p.numel() != rel.num_edges:
        raise _DGLError("%s: prob must hold one value per edge of the graph (%d), got shape %s"
                        % (who, rel.num_edges, tuple(p.shape)))
    p = p.to(rel.device)
    return (p if p.dtype in (torch.float32, torch.float64) else p.float()).contiguous().reshape(-1)


def _per_etype(g, value, what):
    """``value`` (an int, or a dict keyed by edge type name / canonical edge type) -> one entry per relation."""
    if not isinstance(value, dict):
        return [value] * len(g.canonical_etypes)
    out = []
    for c in g.canonical_etypes:
        if c in value:
            out.append(value[c])
        elif c[1] in value:
            out.append(value[c[1]])
        else:
            raise _DGLError("%s is not given for edge type %s (a dict must name every edge type, neighbor.py:330-340)"
                            % (what, (c,)))
    return out


def _per_etype_ids(g, value):
    """``value`` (ids, or a dict keyed by edge type) -> one id tensor or None per relation."""
    if value is None:
        return [None] * len(g.canonical_etypes)
    if not isinstance(value, dict):
        if len(g.canonical_etypes) > 1:
            raise _DGLError("Must specify etype when the graph is not homogeneous.")
        value = {g.canonical_etypes[0]: value}
    out = [None] * len(g.canonical_etypes)
    for e, ids in value.items():
        out[g.get_etype_id(e)] = ids
    return out


class _ExclusionSets(list):
    """One sorted exclusion list (or None) per relation of a graph: what :func:`_exclusion_sets` builds once per batch."""


def _mark_exclusion_set(x):
    """Tags ``x`` as a sorted exclusion list (the output of ``_capi.exclude_set``), so that handing it on as
    ``exclude_eids`` does not sort it a second time.  The tag lives on this tensor object alone."""
    x._dgla_exclusion_set = True
    return x


def _exclusion_sets(g, exclude_edges):
    """``exclude_edges`` (ids, or a dict per edge type / canonical edge type) as one sorted list per relation on the
    graph's device (csrc/exclude.hip; one read-back of the flag word per relation that has a list).  An id outside the
    relation's edges is refused ("edge id out of range")."""
    if exclude_edges is None or isinstance(exclude_edges, _ExclusionSets):
        return exclude_edges
    out = _ExclusionSets()
    for etid, ids in enumerate(_per_etype_ids(g, exclude_edges)):
        rel = g._graph.relations[etid]
        if ids is None or torch.as_tensor(ids).numel() == 0:
            out.append(None)
        elif getattr(ids, "_dgla_exclusion_set", False) and ids.device == rel.device and ids.dtype == rel.idtype:
            out.append(ids)
        else:
            out.append(_capi.exclude_set(_node_ids(ids, rel.device, rel.idtype), rel.num_edges))
    return out


def _sample_neighbors_hetero(g, nodes, fanout, edge_dir, prob, replace, seed, excluded=None):
    """sample_neighbors on a graph with several relations (python/dgl/sampling/neighbor.py:300-395): relation by
    relation through the same kernels; a relation whose seed side has no nodes in ``nodes``, or whose fanout is 0, comes
    out empty.  The result keeps every node type and node count of ``g``."""
    if not isinstance(nodes, dict):
        if len(g.ntypes) != 1:
            raise _DGLError("Must specify node type when the graph is not homogeneous.")
        nodes = {g.ntypes[0]: nodes}
    for n in nodes:
        if n not in g.ntypes:
            raise _DGLError('Node type "{}" does not exist.'.format(n))
    fanouts = _per_etype(g, fanout, "fanout")
    rels = []
    picked = []
    for etid, (s_t, _, d_t) in enumerate(g.canonical_etypes):
        rel = g._graph.relations[etid]
        dev, idt = rel.device, rel.idtype
        seeds = nodes.get(d_t if edge_dir == "in" else s_t)
        f = int(fanouts[etid])
        if seeds is None or f == 0 or rel.num_edges == 0 or torch.as_tensor(seeds).numel() == 0:
            empty = torch.empty(0, dtype=idt, device=dev)
            rels.append(Relation(rel.num_src, rel.num_dst, empty, empty, idtype=idt, device=dev))
            picked.append(empty)
            continue
        seeds = _node_ids(seeds, dev, idt)
        fmt = rel.csc() if edge_dir == "in" else rel.csr()
        csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], rel.num_src if edge_dir == "in" else rel.num_dst)
        p = _prob_of(prob, g._edge_frames[etid], rel, "sample_neighbors")
        rng = int(seed) * 131 + etid
        if p is None:
            indptr, nbr, eids = _capi.sample_neighbors(csr, seeds, f, replace, rng)
        elif f < 0:         # every edge that CAN be picked: all of them, minus those of zero weight
            indptr, nbr, eids = _capi.sample_neighbors(csr, seeds, -1, False, rng)
        else:
            indptr, nbr, eids = _capi.sample_neighbors_weighted(csr, p, seeds, f, replace, rng)
        if excluded is not None and excluded[etid] is not None:     # sample first, then drop (sampling/utils.py EidExcluder)
            indptr, nbr, eids = _capi.frontier_exclude(indptr, nbr, eids, excluded[etid])
        n_e = int(indptr[-1])
        own = torch.repeat_interleave(seeds, (indptr[1:] - indptr[:-1]).long(), output_size=n_e)
        nbr, eids = nbr[:n_e], eids[:n_e]
        if p is not None and f < 0:
            keep_e = p[eids.long()] > 0
            own, nbr, eids = own[keep_e], nbr[keep_e], eids[keep_e]
        src, dst = (nbr.contiguous(), own) if edge_dir == "in" else (own, nbr.contiguous())
        rels.append(Relation(rel.num_src, rel.num_dst, src, dst, idtype=idt, device=dev))
        picked.append(eids)
    gi = g._graph
    out = DGLGraph(GraphIndex([gi.num_nodes(i) for i in range(len(g._ntypes))], list(gi.metagraph.edges), rels),
                   g._ntypes, g.canonical_etypes, src_ntypes=g._src_ntype_ids, dst_ntypes=g._dst_ntype_ids)
    for etid, e in enumerate(picked):
        out._edge_frames[etid][EID] = e
    return out


def sample_neighbors(g, nodes, fanout, edge_dir="in", prob=None, replace=False, seed=None, exclude_edges=None):
    """Frontier graph on the nodes of `g` holding, for every node in `nodes`, ``fanout`` of its
    inbound edges picked uniformly (all of them when it has fewer, or ``fanout == -1``).
    ``edata[dgl.EID]`` carries the original edge ids.

    ``exclude_edges`` (ids, or a dict keyed by edge type / canonical edge type) drops those edges from the frontier
    AFTER the picks (the reference's rule, sampling/utils.py EidExcluder: a row may come out shorter than its fanout):
    the filter of csrc/exclude.hip, on a GPU graph only.

    ``seed=None`` (default) draws a fresh stream for every call from torch's global CPU
    generator, like the reference's advancing global RNG (so ``torch.manual_seed`` makes a run
    reproducible); an explicit integer pins the picks of this call."""
    seed = _call_seed(seed)
    if edge_dir not in ("in", "out"):
        raise ValueError("edge_dir must be 'in' or 'out'")
    excluded = _exclusion_sets(g, exclude_edges)
    if len(g.canonical_etypes) != 1 or isinstance(nodes, dict) or isinstance(fanout, dict):
        return _sample_neighbors_hetero(g, nodes, fanout, edge_dir, prob, replace, seed, excluded)
    if edge_dir == "in":
        rel, csr, keep = _csc_of(g)
    else:  # outbound edges: the same kernel over the out-edge CSR (rows = source nodes)
        rel = g._graph.relations[0]
        keep = rel.csr()
        csr = _capi.make_csr(keep[0], keep[1], keep[2], rel.num_dst)
    if isinstance(prob, str):  # name of an edge feature, as in the reference
        prob = g.edata[prob]
    nodes = _node_ids(nodes, rel.device, rel.idtype)
    if prob is None:
        indptr, nbr, eids = _capi.sample_neighbors(csr, nodes, int(fanout), replace, int(seed))
    else:
        # the kernels index `prob` by EDGE ID of g: anything else is an out-of-bounds device read
        # (reference: CHECK on the probability array's length, src/array/array.cc RowWiseSampling)
        if prob.dim() == 0 or prob.shape[0] != rel.num_edges or prob.numel() != rel.num_edges:
            raise _DGLError("sample_neighbors: prob must hold one value per edge of the graph "
                            "(%d), got shape %s" % (rel.num_edges, tuple(prob.shape)))
        p = prob.to(rel.device)
        if p.dtype not in (torch.float32, torch.float64):
            p = p.float()
        p = p.contiguous().reshape(-1)
        if fanout < 0:      # every edge that CAN be picked: all of them, minus those of zero weight
            indptr, nbr, eids = _capi.sample_neighbors(csr, nodes, -1, False, int(seed))
        else:
            indptr, nbr, eids = _capi.sample_neighbors_weighted(csr, p, nodes, int(fanout), replace, int(seed))
    if excluded is not None and excluded[0] is not None:     # sample first, then drop
        indptr, nbr, eids = _capi.frontier_exclude(indptr, nbr, eids, excluded[0])
    n_e = int(indptr[-1])
    own = torch.repeat_interleave(nodes, (indptr[1:] - indptr[:-1]).long(), output_size=n_e)
    nbr, eids = nbr[:n_e], eids[:n_e]
    if prob is not None and fanout < 0:
        keep_e = p[eids.long()] > 0
        own, nbr, eids = own[keep_e], nbr[keep_e], eids[keep_e]
        n_e = int(eids.shape[0])
    src, dst = (nbr[:n_e].contiguous(), own) if edge_dir == "in" else (own, nbr[:n_e].contiguous())
    r = Relation(rel.num_src, rel.num_dst, src, dst, idtype=rel.idtype, device=rel.device)
    out = DGLGraph(GraphIndex([g.num_nodes()], [(0, 0)], [r]), ["_N"], [("_N", "_E", "_N")])
    out.edata[EID] = eids[:n_e]
    return out


def sample_neighbors_fused(g, nodes, fanout, edge_dir="in", prob=None, replace=False, seed=None, exclude_edges=None):
    """``sample_neighbors`` followed by ``to_block`` on the seeds (python/dgl/sampling/neighbor.py
    sample_neighbors_fused, a CPU-only fusion of the two there): the block of one sampling step, its edge ids those of
    ``g``.  ``exclude_edges`` is refused: use :func:`sample_neighbors` and :func:`to_block`."""
    if exclude_edges is not None:
        raise _DGLError("sample_neighbors_fused: exclude_edges is not supported; call sample_neighbors(exclude_edges=) "
                        "and to_block")
    if edge_dir != "in":
        raise _DGLError("sample_neighbors_fused: only inbound sampling yields a block whose destinations are the seeds")
    frontier = sample_neighbors(g, nodes, fanout, edge_dir=edge_dir, prob=prob, replace=replace, seed=seed)
    if isinstance(nodes, dict):
        seeds = {n: torch.as_tensor(v, device=g.device).reshape(-1) for n, v in nodes.items()}
    else:
        seeds = torch.as_tensor(nodes, device=g.device).reshape(-1)
    blk = to_block(frontier, seeds)
    for etid in range(len(g.canonical_etypes)):
        fe = frontier._edge_frames[etid][EID]
        blk._edge_frames[etid][EID] = fe[blk._edge_frames[etid][EID].long()]
    return blk


def _make_block(indptr, local_src, num_src, num_dst, idtype, device):
    rel = Relation(num_src, num_dst, csc=(indptr, local_src, None), idtype=idtype, device=device)
    rel.transient = True
    blk = DGLGraph(GraphIndex([num_src, num_dst], [(0, 1)], [rel]), ["_N", "_N"], [("_N", "_E", "_N")],
                   src_ntypes=[0], dst_ntypes=[1])
    blk.is_block = True
    return blk


def _renumber(seeds, src, g, dev, ntid=None):
    """Block-local ids of ``src`` with ``seeds`` first and the new sources after them in ascending order: the
    ``dgla_to_block`` kernel on the GPU; for a graph that lives on the CPU (graph construction in tests and data
    pipelines, where the reference runs its own CPU ``ToBlock``) the same convention in torch index arithmetic."""
    if dev.type == "cuda":
        return _capi.to_block(seeds, src, _node_map(g, dev, ntid))
    n_nodes = g.num_nodes() if ntid is None else g._graph.num_nodes(ntid)
    mark = torch.full((max(1, n_nodes),), -1, dtype=torch.long)
    mark[seeds.long()] = torch.arange(seeds.shape[0])
    new = torch.unique(src[mark[src.long()] < 0])
    mark[new.long()] = seeds.shape[0] + torch.arange(new.shape[0])
    return mark[src.long()].to(seeds.dtype), torch.cat([seeds, new.to(seeds.dtype)]), int(seeds.shape[0] + new.shape[0])


def _renumber_into(src_nodes, src, n_nodes):
    """Block-local ids of ``src`` when the block's source nodes are GIVEN (``to_block(..., src_nodes=)``)."""
    mark = torch.full((max(1, n_nodes),), -1, dtype=torch.long, device=src.device)
    mark[src_nodes.long()] = torch.arange(src_nodes.shape[0], device=src.device)
    local = mark[src.long()]
    if bool((local < 0).any()):
        raise _DGLError("to_block: src_nodes does not hold every source node of the frontier")
    return local.to(src_nodes.dtype), src_nodes, int(src_nodes.shape[0])


def _copy_block_features(g, blk, src_nodes, dst_nodes, induced):
    """Node / edge features of the frontier follow its nodes and edges into the block, behind the ids
    (utils.extract_node_subframes_for_block / extract_edge_subframes; the ids win over a feature of the same name)."""
    t = len(g.ntypes)
    for i, n in enumerate(g.ntypes):
        fr = g._node_frames[i]
        for key, val in fr.items():
            if key == NID:
                continue
            blk._node_frames[i][key] = val[src_nodes[n].long()]
            blk._node_frames[t + i][key] = val[dst_nodes[n].long()]
    for etid in range(len(g.canonical_etypes)):
        fr = g._edge_frames[etid]
        for key, val in fr.items():
            if key == EID:
                continue
            blk._edge_frames[etid][key] = val[induced[etid].long()]


def _default_dst_nodes(g):
    """``to_block(g)`` without destination nodes: per node type the nodes with an inbound edge, ascending
    (transforms/functional.py to_block: ``F.unique`` of the relations' destination ids)."""
    out = {}
    for c in g.canonical_etypes:
        out.setdefault(c[2], []).append(g.edges(etype=c)[1])
    return {n: (torch.unique(torch.cat(v)) if v else torch.empty(0, dtype=g.idtype, device=g.device)) for n, v in out.items()}


def to_block(g, dst_nodes=None, include_dst_in_src=True, src_nodes=None):
    """``dgl.to_block`` (python/dgl/transforms/functional.py to_block): the block's destination nodes are ``dst_nodes``
    in the given order (default: per type the nodes with an inbound edge, ascending); its source nodes start with them
    (``include_dst_in_src``) followed by the other sources in ascending order, or are ``src_nodes`` as given.
    ``srcdata / dstdata[dgl.NID]`` and ``edata[dgl.EID]`` hold the ids in ``g``; the features of ``g`` follow its nodes
    and edges into the block.  Every edge of ``g`` must point at one of ``dst_nodes``.  (:class:`NeighborSampler` then
    replaces ``edata[dgl.EID]`` by the ORIGINAL graph's edge ids, like neighbor_sampler.py:170-172.)"""
    if dst_nodes is None:
        dst_nodes = _default_dst_nodes(g)
        if len(g.ntypes) == 1:
            dst_nodes = dst_nodes.get(g.ntypes[0], torch.empty(0, dtype=g.idtype, device=g.device))
    return _to_block_hetero(g, dst_nodes, include_dst_in_src, src_nodes)


def _rows_of(rel, dst_nodes):
    """In-edges of ``dst_nodes`` (in that order) out of the relation's in-edge CSR: (block indptr, CSC positions)."""
    dev, idt = rel.device, rel.idtype
    indptr = rel.csc()[0]
    deg = (indptr[1:] - indptr[:-1])[dst_nodes.long()]
    total = int(deg.sum())
    if total != rel.num_edges:
        raise ValueError("to_block: some edges of the frontier do not end in dst_nodes")
    blk_ptr = torch.zeros(dst_nodes.shape[0] + 1, dtype=idt, device=dev)
    blk_ptr[1:] = torch.cumsum(deg, 0)
    starts = indptr[:-1][dst_nodes.long()].long()
    pos = torch.repeat_interleave(starts - blk_ptr[:-1].long(), deg.long(), output_size=total) + \
        torch.arange(total, device=dev)
    return blk_ptr, pos


def _to_block_hetero(g, dst_nodes, include_dst_in_src=True, given_src=None):
    """``dgl.to_block`` on a frontier with several node / edge types (python/dgl/transforms/functional.py to_block,
    src/graph/transform/cuda/cuda_to_block.cu): ``dst_nodes`` = {node type: ids}; per node type the block's source nodes
    start with that type's destination nodes (include_dst_in_src), followed by the new sources of EVERY relation leaving
    that type; one relation per edge type, rows = the destination nodes of its destination type."""
    if not isinstance(dst_nodes, dict):
        if len(g.ntypes) != 1:
            raise _DGLError("to_block: dst_nodes must be a dict of node type -> ids on a graph with several node types")
        dst_nodes = {g.ntypes[0]: dst_nodes}
    if g.is_block or len(set(g.ntypes)) != len(g.ntypes):
        raise _DGLError("to_block: the frontier must have one node space per type (not itself a block)")
    nts, cets = g.ntypes, g.canonical_etypes
    dev, idt = g.device, g.idtype
    dst = {n: torch.as_tensor(dst_nodes[n]).to(device=dev, dtype=idt).contiguous() if n in dst_nodes
           else torch.empty(0, dtype=idt, device=dev) for n in nts}
    rows, src_global, orig = [], [], []
    for etid, (s_t, _, d_t) in enumerate(cets):
        rel = g._graph.relations[etid]
        if rel.num_edges == 0 or dst[d_t].shape[0] == 0:
            # no destination node of this relation's destination type: the relation comes out empty and its sources are
            # not collected (src/graph/transform/to_block.cc:271-277)
            ptr = torch.zeros(dst[d_t].shape[0] + 1, dtype=idt, device=dev)
            pos = torch.empty(0, dtype=torch.long, device=dev)
        else:
            ptr, pos = _rows_of(rel, dst[d_t])
        indices, eids = rel.csc()[1], rel.csc()[2]
        rows.append(ptr)
        src_global.append(indices[pos].contiguous())
        orig.append(pos.to(idt) if eids is None else eids[pos])     # ids in g (no map: edge id == CSC position)
    src_nodes, local = {}, [None] * len(cets)
    for ntid, n in enumerate(nts):
        ets = [i for i, c in enumerate(cets) if c[0] == n]
        cat = torch.cat([src_global[i] for i in ets]) if ets else torch.empty(0, dtype=idt, device=dev)
        if given_src is not None:
            gs = given_src[n] if isinstance(given_src, dict) else given_src
            loc, sn, _ = _renumber_into(torch.as_tensor(gs).to(device=dev, dtype=idt), cat, g._graph.num_nodes(ntid))
        elif dst[n].shape[0] == 0 and cat.shape[0] == 0:
            src_nodes[n] = dst[n]
            for i in ets:
                local[i] = cat
            continue
        else:
            first = dst[n] if include_dst_in_src else dst[n][:0]
            loc, sn, _ = _renumber(first, cat, g, dev, ntid)
        src_nodes[n] = sn
        off = 0
        for i in ets:
            k = src_global[i].shape[0]
            local[i] = loc[off:off + k].contiguous()
            off += k
    t = len(nts)
    rels = []
    for etid, (s_t, _, d_t) in enumerate(cets):
        r = Relation(src_nodes[s_t].shape[0], dst[d_t].shape[0], csc=(rows[etid], local[etid], None), idtype=idt, device=dev)
        r.transient = True
        rels.append(r)
    meta = [(nts.index(c[0]), t + nts.index(c[2])) for c in cets]
    gidx = GraphIndex([src_nodes[n].shape[0] for n in nts] + [dst[n].shape[0] for n in nts], meta, rels)
    blk = DGLGraph(gidx, nts + nts, cets, src_ntypes=list(range(t)), dst_ntypes=list(range(t, 2 * t)))
    blk.is_block = True
    for i, n in enumerate(nts):
        blk._node_frames[i][NID] = src_nodes[n]
        blk._node_frames[t + i][NID] = dst[n]
    for etid in range(len(cets)):
        blk._edge_frames[etid][EID] = orig[etid]
    _copy_block_features(g, blk, src_nodes, dst, orig)
    return blk


class NeighborSampler:
    """``NeighborSampler([15, 10])``: one block per layer, built from the output nodes inwards
    (neighbor_sampler.py: sample_blocks).  ``sample_blocks(g, seed_nodes)`` returns
    ``(input_nodes, output_nodes, blocks)``; ``blocks[i].srcdata[dgl.NID]`` /
    ``dstdata[dgl.NID]`` / ``edata[dgl.EID]`` hold the original ids."""

    def __init__(self, fanouts, replace=False, seed=0, prob=None):
        self.fanouts = [f if isinstance(f, dict) else int(f) for f in fanouts]
        self.replace = bool(replace)
        self.seed = int(seed)
        self.prob = prob  # name of an edge feature holding sampling weights (the reference's `prob`)
        self.output_device = None
        self._calls = 0

    def sample(self, g, seed_nodes, exclude_eids=None):
        """``BlockSampler.sample`` of dataloading/base.py: :meth:`sample_blocks`, the signature that
        ``as_edge_prediction_sampler`` looks for."""
        return self.sample_blocks(g, seed_nodes, exclude_eids=exclude_eids)

    def _sample_blocks_hetero(self, g, seed_nodes, excluded=None):
        """Several relations: ``sample_neighbors`` + ``to_block`` per layer, as neighbor_sampler.py:150-175 composes
        them; fanouts may be dicts keyed by edge type."""
        if not isinstance(seed_nodes, dict):
            if len(g.ntypes) != 1:
                raise _DGLError("seed_nodes must be a dict of node type -> ids on a graph with several node types")
            seed_nodes = {g.ntypes[0]: seed_nodes}
        seeds = {n: torch.as_tensor(v).to(device=g.device, dtype=g.idtype).contiguous() for n, v in seed_nodes.items()}
        output_nodes = dict(seeds)
        blocks = []
        for layer, fanout in enumerate(reversed(self.fanouts)):
            rng = (self.seed * 1000003 + self._calls) * 64 + layer
            frontier = sample_neighbors(g, seeds, fanout, prob=self.prob, replace=self.replace, seed=rng,
                                        exclude_edges=excluded)
            blk = to_block(frontier, seeds)
            for etid in range(len(g.canonical_etypes)):          # ids of the ORIGINAL graph (neighbor_sampler.py:170-172)
                fe = frontier._edge_frames[etid][EID]
                blk._edge_frames[etid][EID] = fe[blk._edge_frames[etid][EID].long()]
            blocks.insert(0, blk)
            seeds = {n: blk.srcnodes[n].data[NID] for n in g.ntypes}
        self._calls += 1
        return seeds, output_nodes, blocks

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        """``exclude_eids`` (ids, or a dict per edge type): those edges are dropped from every layer's frontier after
        the picks (csrc/exclude.hip).  The set is sorted once per call; a layer with exclusion reads back the number of
        surviving picks and then the number of source nodes (two read-backs instead of the one of the plain path)."""
        excluded = _exclusion_sets(g, exclude_eids)
        if len(g.canonical_etypes) != 1 or len(g.ntypes) != 1 or isinstance(seed_nodes, dict):
            return self._sample_blocks_hetero(g, seed_nodes, excluded)
        x = excluded[0] if excluded is not None else None
        rel, csr, keep = _csc_of(g)
        dev, idt = rel.device, rel.idtype
        node_map = _node_map(g, dev)
        seeds = seed_nodes.to(device=dev, dtype=idt).contiguous()
        output_nodes = seeds
        blocks = []
        for layer, fanout in enumerate(reversed(self.fanouts)):
            rng = (self.seed * 1000003 + self._calls) * 64 + layer
            if self.prob is None:
                if x is not None or not (fanout > 0 and seeds.shape[0] > 0):
                    indptr, src, eids = _capi.sample_neighbors(csr, seeds, fanout, self.replace, rng)
            else:
                p = g.edata[self.prob] if isinstance(self.prob, str) else self.prob
                if p.dim() == 0 or p.shape[0] != rel.num_edges or p.numel() != rel.num_edges:
                    raise _DGLError("NeighborSampler: prob must hold one value per edge of the graph "
                                    "(%d), got shape %s" % (rel.num_edges, tuple(p.shape)))
                p = p.to(dev)
                p = (p if p.dtype in (torch.float32, torch.float64) else p.float()).contiguous().reshape(-1)
                indptr, src, eids = _capi.sample_neighbors_weighted(csr, p, seeds, fanout, self.replace, rng)
            n = seeds.shape[0]
            if x is not None:       # sample first, then drop (sampling/utils.py EidExcluder)
                indptr, src, eids = _capi.frontier_exclude(indptr, src, eids, x)
            if x is None and self.prob is None and fanout > 0 and n > 0:
                # ONE read-back per layer instead of two: renumber the whole fixed-size pick buffer
                # (its unused tail is filled with the first seed, which adds no node) and fetch the
                # number of picks and of source nodes together.  Same picks, same local ids.
                indptr, src, eids = _capi.sample_neighbors_padded(csr, seeds, None, fanout, self.replace, rng, None,
                                                                  sink_rows=1)
                local, src_nodes, num = _capi.to_block_padded(seeds, None, src, node_map, num_nodes=rel.num_src)
                n_e, num_src = (int(v) for v in torch.stack([indptr[n].long(), num[0]]).tolist())
                indptr, local, src_nodes = indptr[: n + 1], local[:n_e], src_nodes[:num_src]
            else:
                n_e = int(indptr[-1])   # one read-back here, one in to_block
                local, src_nodes, num_src = _capi.to_block(seeds, src[:n_e], node_map)
            blk = _make_block(indptr, local, num_src, seeds.shape[0], idt, dev)
            blk.srcdata[NID] = src_nodes
            blk.dstdata[NID] = seeds
            blk.edata[EID] = eids[:n_e]
            blocks.insert(0, blk)
            seeds = src_nodes
        self._calls += 1
        return seeds, output_nodes, blocks

    def sample_blocks_padded(self, g, seed_nodes, num_valid=None, exclude_eids=None):
        """Static-shape ``sample_blocks``: no size is read back, every tensor has a shape that depends
        only on ``len(seed_nodes)`` and the fanouts, so the call — and the training step around it —
        can be captured in one hipGraph (``torch.cuda.graph``) and replayed.

        ``seed_nodes`` has B slots of which the first ``num_valid`` (int64 device tensor, None = all)
        are real.  Layer by layer (output side first) a block has D destination SLOTS + 64 SINK rows
        and D + D * fanout source slots: real picks first, then the sink rows' edges (pointing at the
        real destination nodes in turn); source slots past the block's ``num_src`` (device tensor) are
        padding holding node 0.  Real rows are built exactly as :meth:`sample_blocks` builds them (same picks
        for the FIRST call of a fresh sampler; afterwards this method draws from its device-side counter's
        stream, :meth:`sample_blocks` from its host-side one); padded / sink rows produce values nobody reads.
        Every layer needs at least 64 pick slots (``slots * fanout >= 64``) — the sink rows' edges live there;
        a smaller batch is refused.  Returns ``(input_nodes,
        num_input, output_nodes, blocks)``; ``blocks[i].num_src_valid`` / ``.num_dst_valid`` are the
        device-side counts.  Each call advances a DEVICE-side draw counter (``self.counter``), so a
        replayed graph samples fresh neighbours.  ``exclude_eids`` is refused: dropping picks would move the sink rows'
        edges, a layout of its own."""
        if exclude_eids is not None:
            raise _DGLError("sample_blocks_padded: exclude_eids is not supported in the padded form; use sample_blocks")
        if len(g.canonical_etypes) != 1 or any(isinstance(f, dict) for f in self.fanouts):
            raise _DGLError("sample_blocks_padded: single-relation graphs only (one static shape per layer)")
        if min(self.fanouts) < 1:
            raise _DGLError("sample_blocks_padded needs positive fanouts")
        rel, csr, keep = _csc_of(g)
        dev, idt = rel.device, rel.idtype
        node_map = _node_map(g, dev)
        if getattr(self, "counter", None) is None or self.counter.device != dev:
            self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
        seeds = seed_nodes.to(device=dev, dtype=idt).contiguous()
        output_nodes, nv = seeds, num_valid
        p = None
        if self.prob is not None:
            p = g.edata[self.prob] if isinstance(self.prob, str) else self.prob
            if p.dim() == 0 or p.shape[0] != rel.num_edges or p.numel() != rel.num_edges:
                raise _DGLError("NeighborSampler: prob must hold one value per edge of the graph "
                                "(%d), got shape %s" % (rel.num_edges, tuple(p.shape)))
            p = p.to(dev)
            p = (p if p.dtype in (torch.float32, torch.float64) else p.float()).contiguous().reshape(-1)
        blocks = []
        for layer, fanout in enumerate(reversed(self.fanouts)):
            rng = (self.seed * 1000003) * 64 + layer
            if seeds.shape[0] * fanout < _capi.SINK_ROWS:
                raise _DGLError("sample_blocks_padded: %d slots x fanout %d leave fewer than %d pick slots for the "
                                "sink rows (a block would have more destination than source slots); use at least "
                                "%d seed slots" % (seeds.shape[0], fanout, _capi.SINK_ROWS,
                                                   -(-_capi.SINK_ROWS // fanout)))
            indptr, src, eids = _capi.sample_neighbors_padded(csr, seeds, nv, fanout, self.replace, rng,
                                                              self.counter, prob=p)
            local, src_nodes, num_src = _capi.to_block_padded(seeds, nv, src, node_map, num_nodes=rel.num_src)
            d = seeds.shape[0] + _capi.SINK_ROWS
            blk = _make_block(indptr, local, src_nodes.shape[0], d, idt, dev)
            blk.srcdata[NID] = src_nodes
            blk.dstdata[NID] = src_nodes[:d]
            blk.edata[EID] = eids
            blk.num_dst_valid, blk.num_src_valid = nv, num_src
            blocks.insert(0, blk)
            seeds, nv = src_nodes, num_src
        self.counter += 1
        return seeds, nv, output_nodes, blocks


# ---- layer-neighbour (LABOR) sampling ------------------------------------------------------------
def _labor_seed(random_seed):
    """``random_seed`` of :func:`sample_labors`: an int, a one-element int64 tensor, or None (drawn like every call seed)."""
    if torch.is_tensor(random_seed):
        if random_seed.numel() != 1:
            raise _DGLError("sample_labors: random_seed must be an int or a tensor with one element")
        random_seed = int(random_seed.reshape(-1)[0].item())
    return _call_seed(random_seed)


def sample_labors(g, nodes, fanout, edge_dir="in", prob=None, importance_sampling=0, random_seed=None,
                  seed2_contribution=0, copy_ndata=True, copy_edata=True, exclude_edges=None, output_device=None):
    """``dgl.sampling.sample_labors`` (python/dgl/sampling/labor.py): layer-neighbour sampling (LABOR-0, Balin and
    Catalyurek, arXiv:2210.13339).  Every node in ``nodes`` keeps about ``fanout`` of its inbound (``edge_dir="out"``:
    outbound) edges per edge type, all of them when it has no more or ``fanout == -1``; the random variate belongs to
    the NEIGHBOUR node, not to the edge, so seeds that share a neighbour keep or drop it together and the set of distinct
    neighbours comes out much smaller than :func:`sample_neighbors`' at the same fanout.

    ``nodes`` is an id tensor or a dict per node type, ``fanout`` an int or a dict per edge type, ``prob`` the name of an
    edge feature of unnormalised weights (relations that lack it sample uniformly; zero, negative and NaN weights are
    never kept).  ``random_seed`` (an int or a one-element int64 tensor; None draws one from torch's generator) fixes the
    variates: ALL relations of a call share it, so a node keeps its variate across edge types, and calls that belong to
    one batch should pass the same seed.  ``exclude_edges`` (ids, or a dict per edge type) drops those edges from the
    result after sampling, as the reference does on a GPU graph.

    Returns ``(frontier, importances)``: the frontier holds all nodes of ``g`` and the sampled edges, the original edge
    ids in ``edata[dgl.EID]``, the node features of ``g`` (the same tensors, ``copy_ndata``) and its edge features at the
    sampled edges (``copy_edata``); ``importances`` has one tensor per edge type with one weight per frontier edge,
    averaging 1 over the edges of a seed, such that ``fn.mean`` over the frontier is unbiased.  It is empty for a
    relation sampled uniformly, as in the reference.

    The picks run on the device (csrc/labor.hip; the rule: include/dgl_amd.h "Layer-neighbour sampling") and are a pure
    function of the arguments.  With weights the expected number of kept edges per seed is ``fanout``, the definition of
    the paper; the reference matches a variance target instead and keeps more.  Not supported, and refused:
    ``importance_sampling != 0`` (LABOR-i) and ``seed2_contribution != 0``."""
    if importance_sampling != 0:
        raise _DGLError("sample_labors: importance_sampling = %r is not supported: LABOR-i needs a per-neighbour maximum "
                        "over the seeds; only importance_sampling = 0 (LABOR-0) runs here" % (importance_sampling,))
    if seed2_contribution != 0:
        raise _DGLError("sample_labors: seed2_contribution = %r is not supported: the variates come from one seed; pass "
                        "seed2_contribution = 0" % (seed2_contribution,))
    if edge_dir not in ("in", "out"):
        raise ValueError("edge_dir must be 'in' or 'out'")
    if g.device.type != "cuda":
        raise _DGLError("sample_labors runs on a ROCm GPU; the graph is on %s (no CPU fallback)" % g.device)
    seed = _labor_seed(random_seed)
    if not isinstance(nodes, dict):
        if len(g.ntypes) != 1:
            raise _DGLError("Must specify node type when the graph is not homogeneous.")
        nodes = {g.ntypes[0]: nodes}
    for n in nodes:
        if n not in g.ntypes:
            raise _DGLError('Node type "{}" does not exist.'.format(n))
    fanouts = _per_etype(g, fanout, "fanout")
    excluded = _per_etype_ids(g, exclude_edges)
    rels, picked, importances = [], [], []
    for etid, (s_t, _, d_t) in enumerate(g.canonical_etypes):
        rel = g._graph.relations[etid]
        dev, idt = rel.device, rel.idtype
        frame = g._edge_frames[etid]
        p = _prob_of(prob, frame, rel, "sample_labors") if prob is not None and (not isinstance(prob, str) or prob in frame) \
            else None
        seeds = nodes.get(d_t if edge_dir == "in" else s_t)
        f = int(fanouts[etid])
        if seeds is None or f == 0 or rel.num_edges == 0 or torch.as_tensor(seeds).numel() == 0:
            own = nbr = eids = torch.empty(0, dtype=idt, device=dev)
            imp = torch.empty(0, dtype=torch.float32 if p is None else p.dtype, device=dev)
        else:
            seeds = _node_ids(seeds, dev, idt)
            fmt = rel.csc() if edge_dir == "in" else rel.csr()
            csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], rel.num_src if edge_dir == "in" else rel.num_dst)
            # the SAME seed for every relation: a node's variate is shared across edge types (labor.py:101-112)
            indptr, nbr, eids, imp = _capi.labor_sample(csr, seeds, f, seed, prob=p)
            own = torch.repeat_interleave(seeds, (indptr[1:] - indptr[:-1]).long(), output_size=int(eids.shape[0]))
            if imp is None:
                imp = torch.empty(0, dtype=torch.float32, device=dev)
            if excluded[etid] is not None:
                keep_e = ~torch.isin(eids, _node_ids(excluded[etid], dev, idt))
                own, nbr, eids = own[keep_e], nbr[keep_e], eids[keep_e]
                if p is not None:
                    imp = imp[keep_e]
        src, dst = (nbr.contiguous(), own) if edge_dir == "in" else (own, nbr.contiguous())
        rels.append(Relation(rel.num_src, rel.num_dst, src, dst, idtype=idt, device=dev))
        picked.append(eids)
        importances.append(imp)
    gi = g._graph
    out = DGLGraph(GraphIndex([gi.num_nodes(i) for i in range(len(g._ntypes))], list(gi.metagraph.edges), rels),
                   g._ntypes, g.canonical_etypes, src_ntypes=g._src_ntype_ids, dst_ntypes=g._dst_ntype_ids)
    if copy_ndata:      # the same tensors, as utils.extract_node_subframes(g, None) shares them
        for i, fr in enumerate(g._node_frames):
            for key, val in fr.items():
                out._node_frames[i][key] = val
    for etid, e in enumerate(picked):
        if copy_edata:
            for key, val in g._edge_frames[etid].items():
                if key != EID:
                    out._edge_frames[etid][key] = val[e.long()]
        out._edge_frames[etid][EID] = e
    if output_device is not None:
        out = out.to(output_device)
        importances = [w.to(output_device) for w in importances]
    return out, importances


DGLGraph.sample_labors = sample_labors


def select_topk(g, k, weight, nodes=None, edge_dir="in", ascending=False, copy_ndata=True, copy_edata=True,
                output_device=None):
    """``dgl.sampling.select_topk`` (python/dgl/sampling/neighbor.py:880): for every node in ``nodes`` the ``k`` inbound
    (``edge_dir="out"``: outbound) edges per edge type with the largest (``ascending``: smallest) weight, all of them
    when it has no more or ``k == -1``.

    ``k`` is an int or a dict that names every edge type; ``weight`` is the name of an edge feature with one element per
    edge (fp32, fp64, fp16, bf16, int32 or int64), which every edge type must have; ``nodes`` is an id tensor, a dict per
    node type, or None for all nodes.  A node listed twice is selected twice.

    Returns a graph with all nodes of ``g`` and only the selected edges, ordered by node in the given order and then by
    rank, best first; ``edata[dgl.EID]`` holds their ids in ``g``, the node features are those of ``g`` (the same
    tensors, ``copy_ndata``) and the edge features follow the selected edges (``copy_edata``).

    A GPU graph runs the kernels of csrc/topk.hip, a CPU graph the same rule compiled for the host
    (dgla_select_topk_host; the reference has the CPU form only).  The rule is written in include/dgl_amd.h, "Top-k
    neighbour selection": NaN loses in both directions and equal weights are ordered by edge id, which is one of the
    orders the reference's unstable sort may produce.  A node that would yield more than 1024 edges is refused."""
    who = "select_topk"
    if edge_dir not in ("in", "out"):
        raise ValueError("edge_dir must be 'in' or 'out'")
    if not isinstance(weight, str):
        raise _DGLError("%s: weight is the name of an edge feature, got %r" % (who, type(weight).__name__))
    if nodes is None:
        nodes = {n: torch.arange(g._graph.num_nodes(i)) for i, n in enumerate(g.ntypes)}
    elif not isinstance(nodes, dict):
        if len(g.ntypes) != 1:
            raise _DGLError("Must specify node type when the graph is not homogeneous.")
        nodes = {g.ntypes[0]: nodes}
    for n in nodes:
        if n not in g.ntypes:
            raise _DGLError('Node type "{}" does not exist.'.format(n))
    if isinstance(k, dict) and len(k) != len(g.canonical_etypes):
        raise _DGLError("K value must be specified for each edge type if a dict is provided.")
    ks = _per_etype(g, k, "k")
    weights = []
    for etid, c in enumerate(g.canonical_etypes):
        frame = g._edge_frames[etid]
        if weight not in frame:
            raise _DGLError('Edge weights "{}" do not exist for relation graph "{}".'.format(weight, c))
        weights.append(frame[weight])
    rels, picked = [], []
    for etid, (s_t, _, d_t) in enumerate(g.canonical_etypes):
        rel = g._graph.relations[etid]
        dev, idt = rel.device, rel.idtype
        w = weights[etid]
        if w.dim() == 0 or w.shape[0] != rel.num_edges or w.numel() != rel.num_edges:
            raise _DGLError('%s: edge weights "%s" of relation graph "%s" must have one element per edge (%d), got shape %s'
                            % (who, weight, g.canonical_etypes[etid], rel.num_edges, tuple(w.shape)))
        seeds = nodes.get(d_t if edge_dir == "in" else s_t)
        kk = int(ks[etid])
        if seeds is None or kk == 0 or rel.num_edges == 0 or torch.as_tensor(seeds).numel() == 0:
            own = nbr = eids = torch.empty(0, dtype=idt, device=dev)
        else:
            seeds = _node_ids(seeds, dev, idt)
            w = w.to(dev).reshape(-1).contiguous()
            fmt = rel.csc() if edge_dir == "in" else rel.csr()
            cols = rel.num_src if edge_dir == "in" else rel.num_dst
            if dev.type == "cuda":
                csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], cols)
                indptr, nbr, eids = _capi.select_topk(csr, w, seeds, kk, ascending)
            else:
                csr = _capi.host_csr(fmt[0].contiguous(), fmt[1].contiguous(), None if fmt[2] is None else fmt[2].contiguous(),
                                     cols)
                indptr, nbr, eids = _capi.select_topk_host(csr, w, seeds, kk, ascending)
            n_e = int(indptr[-1])
            own = torch.repeat_interleave(seeds, (indptr[1:] - indptr[:-1]).long(), output_size=n_e)
            nbr, eids = nbr[:n_e].contiguous(), eids[:n_e].contiguous()
        src, dst = (nbr, own) if edge_dir == "in" else (own, nbr)
        rels.append(Relation(rel.num_src, rel.num_dst, src, dst, idtype=idt, device=dev))
        picked.append(eids)
    gi = g._graph
    out = DGLGraph(GraphIndex([gi.num_nodes(i) for i in range(len(g._ntypes))], list(gi.metagraph.edges), rels),
                   g._ntypes, g.canonical_etypes, src_ntypes=g._src_ntype_ids, dst_ntypes=g._dst_ntype_ids)
    if copy_ndata:      # the same tensors, as utils.extract_node_subframes(g, None) shares them
        for i, fr in enumerate(g._node_frames):
            for key, val in fr.items():
                out._node_frames[i][key] = val
    for etid, e in enumerate(picked):
        if copy_edata:
            for key, val in g._edge_frames[etid].items():
                if key != EID:
                    out._edge_frames[etid][key] = val[e.long()]
        out._edge_frames[etid][EID] = e
    return out if output_device is None else out.to(output_device)


DGLGraph.select_topk = select_topk


class LaborSampler:
    """``dgl.dataloading.LaborSampler`` (python/dgl/dataloading/labor_sampler.py): one block per layer, built from the
    output nodes inwards; a layer is :func:`sample_labors` followed by :func:`to_block` on the seeds.
    ``sample_blocks(g, seed_nodes)`` returns ``(input_nodes, output_nodes, blocks)``; ``blocks[i].srcdata[dgl.NID]`` /
    ``dstdata[dgl.NID]`` / ``edata[dgl.EID]`` hold the original ids and, when ``prob`` names an edge feature,
    ``edata["edge_weights"]`` the importances.  ``layer_dependency=True`` samples every layer of a batch with one seed, so
    a node keeps its variate from layer to layer and the layers overlap more; ``False`` gives each layer its own seed.
    Successive calls advance the seeds, like :class:`NeighborSampler`; two samplers with the same ``seed`` agree."""

    def __init__(self, fanouts, edge_dir="in", prob=None, importance_sampling=0, layer_dependency=False, seed=0):
        if edge_dir != "in":
            raise _DGLError("LaborSampler: only inbound sampling yields blocks whose destinations are the seeds")
        self.fanouts = [f if isinstance(f, dict) else int(f) for f in fanouts]
        self.edge_dir = edge_dir
        self.prob = prob
        self.importance_sampling = importance_sampling
        self.layer_dependency = bool(layer_dependency)
        self.seed = int(seed)
        self.output_device = None
        self._calls = 0

    def sample(self, g, seed_nodes, exclude_eids=None):
        """``BlockSampler.sample`` of dataloading/base.py: :meth:`sample_blocks`, the signature that
        ``as_edge_prediction_sampler`` looks for."""
        return self.sample_blocks(g, seed_nodes, exclude_eids=exclude_eids)

    def sample_blocks(self, g, seed_nodes, exclude_eids=None):
        """``exclude_eids`` is handed to :func:`sample_labors` as ``exclude_edges`` for every layer."""
        as_dict = isinstance(seed_nodes, dict)
        if not as_dict:
            if len(g.ntypes) != 1:
                raise _DGLError("seed_nodes must be a dict of node type -> ids on a graph with several node types")
            seed_nodes = {g.ntypes[0]: seed_nodes}
        seeds = {n: torch.as_tensor(v).to(device=g.device, dtype=g.idtype).contiguous() for n, v in seed_nodes.items()}
        output_nodes = dict(seeds)
        blocks = []
        for layer, fanout in enumerate(reversed(self.fanouts)):
            rng = (self.seed * 1000003 + self._calls) * 64 + (0 if self.layer_dependency else layer)
            frontier, imps = sample_labors(g, seeds, fanout, edge_dir=self.edge_dir, prob=self.prob,
                                           importance_sampling=self.importance_sampling, random_seed=rng,
                                           copy_ndata=False, copy_edata=False, exclude_edges=exclude_eids)
            blk = to_block(frontier, seeds)
            for etid in range(len(g.canonical_etypes)):          # ids of the ORIGINAL graph (labor_sampler.py)
                fe = frontier._edge_frames[etid][EID]
                at = blk._edge_frames[etid][EID].long()
                blk._edge_frames[etid][EID] = fe[at]
                if self.prob is not None and imps[etid].shape[0] == fe.shape[0]:
                    blk._edge_frames[etid]["edge_weights"] = imps[etid][at]
            blocks.insert(0, blk)
            seeds = {n: blk.srcnodes[n].data[NID] for n in g.ntypes}
        self._calls += 1
        if as_dict:
            return seeds, output_nodes, blocks
        n = g.ntypes[0]
        return seeds[n], output_nodes[n], blocks


# ---- random walks ------------------------------------------------------------------------------
def _walk_cdf(rel, csr, w):
    """The CDF of relation ``rel`` under the edge weights ``w``: one :func:`_relation_slot`, keyed by the weight tensor."""
    def build():
        p = (w if w.dtype in (torch.float32, torch.float64) else w.float()).contiguous().reshape(-1)
        return _capi.random_walk_cdf(csr, p)
    return _relation_slot(rel, "_walk_cdf", (w,), build)


def _walk_plan(g, metapath, length):
    """``(edge type ids, node type id of every trace column)`` of a walk, with the reference's argument errors
    (randomwalks.py:170-184); a metapath whose node types do not chain is refused here, before any launch.  Host work."""
    if metapath is None:
        if len(g.canonical_etypes) > 1 or len(g.ntypes) > 1:
            raise _DGLError("metapath not specified and the graph is not homogeneous.")
        if length is None:
            raise ValueError("Please specify either the metapath or the random walk length.")
        metapath = [0] * int(length)
    else:
        metapath = [g.get_etype_id(e) for e in metapath]
    meta = g._graph.metagraph
    for t in range(1, len(metapath)):
        if meta.find_edge(metapath[t - 1])[1] != meta.find_edge(metapath[t])[0]:
            raise _DGLError("metapath does not chain: edge type %s ends in node type '%s', edge type %s starts from '%s'"
                            % (g.canonical_etypes[metapath[t - 1]], g.canonical_etypes[metapath[t - 1]][2],
                               g.canonical_etypes[metapath[t]], g.canonical_etypes[metapath[t]][0]))
    if metapath:
        types = [meta.find_edge(metapath[0])[0]] + [meta.find_edge(m)[1] for m in metapath]
    elif len(g.ntypes) == 1:
        types = [0]
    else:
        raise _DGLError("an empty metapath does not say which node type the walks start from")
    return metapath, types


def random_walk(g, nodes, *, metapath=None, length=None, prob=None, restart_prob=None, return_eids=False, seed=None):
    """``dgl.sampling.random_walk`` (python/dgl/sampling/randomwalks.py:31-226): one walk per entry of ``nodes`` along
    ``metapath`` (edge types; default ``length`` steps of the only edge type).  ``prob`` names an edge feature of
    unnormalised weights (relations that lack it walk uniformly; zero, negative and NaN weights are never taken),
    ``restart_prob`` is a float (the same halting probability before every step) or a tensor with one entry per step.
    Returns ``(traces, types)`` or ``(traces, eids, types)``: ``traces`` is ``(len(nodes), steps + 1)`` with -1 after a
    walk halted (no out-edge, or a restart draw), ``eids`` ``(len(nodes), steps)``, ``types`` the node type id of every
    column.  ``seed=None`` draws the call's seed from torch's generator (``torch.manual_seed`` makes a run
    reproducible); an integer pins the walks, whatever the launch geometry (the step rule: include/dgl_amd.h)."""
    metapath, types = _walk_plan(g, metapath, length)
    restart_steps, restart_scalar = None, 0.0
    if restart_prob is None:
        pass
    elif torch.is_tensor(restart_prob):
        restart_steps = restart_prob
        if restart_steps.dim() != 1 or restart_steps.shape[0] != len(metapath):
            raise _DGLError("restart_prob must hold one entry per step (%d), got shape %s"
                            % (len(metapath), tuple(restart_steps.shape)))
    elif isinstance(restart_prob, float):
        restart_scalar = restart_prob
    else:
        raise TypeError("restart_prob should be float or Tensor.")
    if torch.is_tensor(nodes) and nodes.dtype != g.idtype:
        raise _DGLError("Expect argument \"nodes\" to have data type %s. But got %s." % (g.idtype, nodes.dtype))
    dev, idt = g.device, g.idtype
    # only the relations the metapath uses enter the table (their formats and CDFs are built on first use)
    used = sorted(set(metapath)) or [0]
    table = []
    for etid in used:
        rel = g._graph.relations[etid]
        fmt = rel.csr()
        csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], rel.num_dst)    # (refuses a CPU graph: no CPU fallback)
        cdf = None
        if prob is not None and prob in g._edge_frames[etid]:
            w = g._edge_frames[etid][prob]
            if w.dim() == 0 or w.shape[0] != rel.num_edges or w.numel() != rel.num_edges:
                raise _DGLError("random_walk: prob must hold one value per edge of the relation (%d), got shape %s"
                                % (rel.num_edges, tuple(w.shape)))
            cdf = _walk_cdf(rel, csr, w.to(dev))
        table.append((csr, cdf))
    nodes = _node_ids(nodes, dev, idt)
    if restart_steps is not None:
        restart_steps = restart_steps.to(dev)
        if restart_steps.dtype not in (torch.float32, torch.float64):
            restart_steps = restart_steps.float()
        restart_steps = restart_steps.contiguous()
    seed = _call_seed(seed)
    traces, eids = _capi.random_walk(table, [used.index(m) for m in metapath], nodes, restart_scalar, restart_steps,
                                     int(seed), return_eids)
    types = torch.tensor(types, dtype=idt, device=dev)
    return (traces, eids, types) if return_eids else (traces, types)


def _walk_members(rel, fmt, csr):
    """The membership list of relation ``rel`` (every row's column ids ascending, what the node2vec step bisects): one
    :func:`_relation_slot`, keyed by the CSR's arrays.  It costs ``nnz`` ids of device memory."""
    return _relation_slot(rel, "_walk_members", fmt[:2], lambda: _capi.csr_sorted_columns(csr))


def node2vec_random_walk(g, nodes, p, q, walk_length, prob=None, return_eids=False, seed=None):
    """``dgl.sampling.node2vec_random_walk`` (python/dgl/sampling/node2vec_randomwalk.py): one node2vec walk of
    ``walk_length`` steps per entry of ``nodes`` on a homogeneous graph.  ``p`` steers the return to the node the walk
    came from (weight ``1/p``), ``q`` the move away from it (weight ``1/q`` for a successor that has no edge to the
    previous node, 1 for one that has); both must be finite and > 0.  ``prob`` names an edge feature of unnormalised
    weights (zero, negative and NaN weights are never taken).  Returns ``traces`` ``(len(nodes), walk_length + 1)`` with -1
    after a walk halted, or ``(traces, eids)``.  The walks run on the device (csrc/node2vec.hip): a step makes a bounded
    number of rejection attempts and then scans the row exactly, so the law is the reference's whatever ``p`` and ``q``
    (the step rule: include/dgl_amd.h).  ``seed`` as in :func:`random_walk`; with ``p == q == 1`` the walks are those of
    :func:`random_walk` under the same seed."""
    if len(g.canonical_etypes) != 1 or len(g.ntypes) != 1:
        raise _DGLError("node2vec_random_walk: Node2vec only support homogeneous graph.")
    if torch.is_tensor(nodes) and nodes.dtype != g.idtype:
        raise _DGLError("Expect argument \"nodes\" to have data type %s. But got %s." % (g.idtype, nodes.dtype))
    p, q, walk_length = float(p), float(q), int(walk_length)
    if not (math.isfinite(p) and math.isfinite(q) and p > 0 and q > 0):
        raise _DGLError("node2vec_random_walk: p and q must be finite and > 0, got p = %r, q = %r" % (p, q))
    if walk_length < 0:
        raise _DGLError("node2vec_random_walk: walk_length must not be negative")
    rel = g._graph.relations[0]
    w = None
    if prob is not None:
        w = g.edata[prob] if isinstance(prob, str) else prob
        if w.dim() == 0 or w.shape[0] != rel.num_edges or w.numel() != rel.num_edges:
            raise _DGLError("node2vec_random_walk: prob must hold one value per edge of the graph (%d), got shape %s"
                            % (rel.num_edges, tuple(w.shape)))
    dev, idt = g.device, g.idtype
    fmt = rel.csr()
    csr = _capi.make_csr(fmt[0], fmt[1], fmt[2], rel.num_dst)    # (refuses a CPU graph: no CPU fallback)
    cdf = None if w is None else _walk_cdf(rel, csr, w.to(dev))   # the slot random_walk uses
    member = _walk_members(rel, fmt, csr)
    nodes = _node_ids(nodes, dev, idt)
    seed = _call_seed(seed)
    traces, eids = _capi.node2vec_walk(csr, cdf, member, nodes, walk_length, p, q, int(seed), return_eids)
    return (traces, eids) if return_eids else traces


# ---- negative sampling ---------------------------------------------------------------------------
NEGATIVE_SAMPLING_TRIALS = 3     # trials per slot, as in the reference (python/dgl/sampling/negative.py)


def _negative_redundancy(k_hat, num_edges, num_pairs, r=3):
    """How many more slots than samples to draw: the reference's ``_calc_redundancy`` in closed form.  With
    ``p_m = num_edges / num_pairs`` and ``p_k = 1 - p_m`` the chance that a pair is no edge, it solves
    ``k_hat = N p_k - r sqrt(N p_k p_m)`` for N, the larger root ``(-b + sqrt(b^2 - 4ac)) / 2a`` of ``a N^2 + b N + c``
    with ``a = p_k^2``, ``b = -p_k (2 k_hat + r^2 p_m)``, ``c = k_hat^2``, and returns ``N / k_hat - 1``.  The
    discriminant is taken in its factored form ``p_k^2 r^2 p_m (4 k_hat + r^2 p_m)``: the subtraction ``b^2 - 4ac`` loses
    ten digits on a sparse graph."""
    p_m = num_edges / num_pairs
    p_k = 1 - p_m
    n = (2 * k_hat + r ** 2 * p_m + r * math.sqrt(p_m * (4 * k_hat + r ** 2 * p_m))) / (2 * p_k)
    return n / k_hat - 1.0


def _relation_lookup(rel):
    """``(dgla_csr, membership list)`` of relation ``rel``: the list is the slot :func:`node2vec_random_walk` uses; the
    struct is kept next to it under the same key, so a small lookup does not pay for building it on every call."""
    fmt = rel.csr()
    csr = _relation_slot(rel, "_walk_csr", fmt[:2],
                         lambda: _capi.make_csr(fmt[0], fmt[1], fmt[2], rel.num_dst))    # (refuses a CPU graph)
    return csr, _walk_members(rel, fmt, csr)


def _has_edges(rel, u, v):
    """``DGLGraph.has_edges_between`` on a GPU graph: ``u``, ``v`` 1-D id tensors of the graph's id type."""
    if u.numel() != v.numel():
        u, v = torch.broadcast_tensors(u, v)
    csr, member = _relation_lookup(rel)
    return _capi.csr_has_edges(csr, member, u.contiguous(), v.contiguous())


def global_uniform_negative_sampling(g, num_samples, exclude_self_loops=True, replace=False, etype=None, redundancy=None,
                                     seed=None, padded=False):
    """``dgl.sampling.global_uniform_negative_sampling`` (python/dgl/sampling/negative.py): up to ``num_samples``
    pairs ``(src, dst)``, ``src`` uniform over the source nodes and ``dst`` over the destination nodes of edge type
    ``etype``, such that no edge ``src -> dst`` of that type exists.  ``exclude_self_loops`` also drops ``src == dst``
    (only when the source and destination node types are equal); without ``replace`` the pairs are distinct.  Fewer than
    ``num_samples`` pairs may come back when the graph is small or dense.

    The pairs are drawn on the device (csrc/negative_sampling.hip; the rule: include/dgl_amd.h):
    ``n_slots = int(num_samples * (1 + redundancy))`` slots make up to three uniform draws each and keep the first that
    is no edge, by a bisection of the relation's membership list (built once per relation, shared with
    :func:`node2vec_random_walk` and ``has_edges_between``).  ``redundancy=None`` takes the reference's estimate from the
    density of the graph; a value the caller gives is honoured (the reference overwrites it).

    **Order of the result.**  The reference sorts the pairs it drew and, without ``replace``, returns the
    lexicographically smallest ``num_samples`` of the distinct ones, a sample biased toward small source ids.  Here the
    accepted slots stay in slot order and the first occurrence of every pair is kept, so cutting the list at
    ``num_samples`` is an unbiased sample without replacement, and the result for a smaller ``num_samples`` is a prefix
    of the result for a larger one at the same number of slots.

    Returns ``(src, dst)`` cut to the number of pairs found, which costs one read of that number by the host.
    ``padded=True`` returns ``(src, dst, count)`` instead: both tensors of length ``num_samples`` with -1 from ``count``
    (a 1-element int64 device tensor) on, nothing read back, usable inside a graph capture once the relation's
    membership list exists.  ``seed`` as in :func:`random_walk`."""
    num_samples = int(num_samples)
    if num_samples < 0:
        raise _DGLError("global_uniform_negative_sampling: num_samples must not be negative")
    if etype is None:
        etype = g.canonical_etypes[0]
    utype, _, vtype = g.to_canonical_etype(etype)
    exclude_self_loops = bool(exclude_self_loops) and utype == vtype
    rel = g._graph.relations[g.get_etype_id(etype)]
    dev, idt = g.device, g.idtype
    if dev.type != "cuda":
        raise _DGLError("global_uniform_negative_sampling runs on a ROCm GPU; the graph is on %s (no CPU fallback)" % dev)
    num_pairs, num_edges = rel.num_src * rel.num_dst, rel.num_edges
    n_slots = 0
    if num_samples > 0 and num_pairs > num_edges:     # (a relation in which every pair is an edge has no negatives)
        if redundancy is None:
            redundancy = _negative_redundancy(num_samples, num_edges, num_pairs)
        redundancy = float(redundancy)
        if not (math.isfinite(redundancy) and redundancy >= 0):
            raise _DGLError("global_uniform_negative_sampling: redundancy must be finite and >= 0, got %r" % redundancy)
        n_slots = int(num_samples * (1 + redundancy))
    if n_slots == 0:
        src = torch.full((num_samples if padded else 0,), -1, dtype=idt, device=dev)
        return (src, src.clone(), torch.zeros(1, dtype=torch.int64, device=dev)) if padded else (src, src.clone())
    csr, member = _relation_lookup(rel)
    seed = _call_seed(seed)
    src, dst, count = _capi.negative_sample(csr, member, n_slots, num_samples, NEGATIVE_SAMPLING_TRIALS,
                                            exclude_self_loops, replace, int(seed))
    if padded:
        return src, dst, count
    k = int(count.item())
    return src[:k], dst[:k]


DGLGraph.global_uniform_negative_sampling = global_uniform_negative_sampling


def pack_traces(traces, types):
    """``dgl.sampling.pack_traces`` (python/dgl/sampling/randomwalks.py:229-310): the -1 padding of ``traces`` removed
    and the rest concatenated.  Returns ``(concat_vids, concat_types, lengths, offsets)``: node ids, their node types,
    the length of every trace and where it starts in ``concat_vids``.  Plain torch, on the inputs' device (the
    reference takes CPU tensors only)."""
    if traces.dim() != 2 or types.dim() != 1 or types.shape[0] != traces.shape[1]:
        raise _DGLError("pack_traces: traces must be (num_traces, len) and types (len,)")
    keep = traces != -1
    lengths = keep.sum(1).to(traces.dtype)
    offsets = torch.cumsum(lengths, 0).to(traces.dtype) - lengths
    return traces[keep], types.to(traces.device).expand_as(traces)[keep], lengths, offsets


# ---- subgraph samplers ---------------------------------------------------------------------------
def _induced_on(g, ids_per_type):
    """The node-induced subgraph of ``g`` on ``ids_per_type`` in list order: the kernels of csrc/subgraph.hip on a GPU
    graph (work proportional to the selected nodes' degrees), ``node_subgraph`` on a CPU graph."""
    from . import transforms

    if g.device.type == "cuda":
        return transforms._induced_rows(g, ids_per_type, True, True)
    return transforms.node_subgraph(g, ids_per_type if len(g.ntypes) > 1 else ids_per_type[g.ntypes[0]])


class ShaDowKHopSampler:
    """``dgl.dataloading.ShaDowKHopSampler`` (python/dgl/dataloading/shadow.py): the subgraph induced on a sampled
    k-hop in-neighbourhood of the seeds (Zeng et al., arXiv:2012.01380).  For each fanout in reverse it runs
    ``sample_neighbors`` + ``to_block`` and takes the block's source nodes as the next seeds; the subgraph is then cut
    on that node list, so the seeds come first and ``subg.ndata[dgl.NID] == input_nodes``.  Fanouts may be dicts keyed
    by edge type; ``seed_nodes`` is a dict per node type on a heterograph.  ``seed`` pins the picks as in
    :class:`NeighborSampler`.  A CPU graph takes all neighbours only (every fanout -1): sampled fanouts run on the
    device.  ``exclude_eids`` and the prefetch arguments are refused."""

    def __init__(self, fanouts, replace=False, prob=None, seed=0, prefetch_node_feats=None, prefetch_edge_feats=None):
        if prefetch_node_feats is not None:
            raise _DGLError("ShaDowKHopSampler: prefetch_node_feats is not supported (features follow the subgraph eagerly)")
        if prefetch_edge_feats is not None:
            raise _DGLError("ShaDowKHopSampler: prefetch_edge_feats is not supported (features follow the subgraph eagerly)")
        self.fanouts = [f if isinstance(f, dict) else int(f) for f in fanouts]
        self.replace = bool(replace)
        self.prob = prob
        self.seed = int(seed)
        self._calls = 0

    def sample(self, g, seed_nodes, exclude_eids=None):
        """``(input_nodes, output_nodes, subg)``: the node ids inducing the subgraph, the seeds, the subgraph."""
        from . import transforms

        if exclude_eids is not None:
            raise _DGLError("ShaDowKHopSampler: exclude_eids is not supported")
        if g.is_block:
            raise _DGLError("ShaDowKHopSampler: the graph must not be a block")
        is_mapping = isinstance(seed_nodes, dict)
        if not is_mapping:
            if len(g.ntypes) != 1:
                raise _DGLError("seed_nodes must be a dict of node type -> ids on a graph with several node types")
            seed_nodes = {g.ntypes[0]: seed_nodes}
        seeds = {}
        for n, v in seed_nodes.items():
            t = _node_ids(v, g.device, g.idtype)
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= g.num_nodes(n)):
                raise _DGLError("ShaDowKHopSampler: node id out of range for node type %s" % n)
            seeds[n] = t
        output_nodes = dict(seeds)
        on_gpu = g.device.type == "cuda"
        for layer, fanout in enumerate(reversed(self.fanouts)):
            if on_gpu:
                rng = (self.seed * 1000003 + self._calls) * 64 + layer
                frontier = sample_neighbors(g, seeds, fanout, prob=self.prob, replace=self.replace, seed=rng)
            else:
                if any(int(f) != -1 for f in (fanout.values() if isinstance(fanout, dict) else [fanout])):
                    raise _DGLError("ShaDowKHopSampler: a sampled fanout needs a graph on the GPU (no CPU fallback); "
                                    "a CPU graph takes fanout -1 only")
                frontier = transforms.in_subgraph(g, seeds)
            blk = to_block(frontier, seeds)
            seeds = {n: blk.srcnodes[n].data[NID] for n in g.ntypes}
        self._calls += 1
        subg = _induced_on(g, seeds)
        if is_mapping:
            return seeds, output_nodes, subg
        return seeds[g.ntypes[0]], output_nodes[g.ntypes[0]], subg


class SAINTSampler:
    """``dgl.dataloading.SAINTSampler`` (python/dgl/dataloading/graphsaint.py; Zeng et al., arXiv:1907.04931): the
    subgraph induced on a random node set of a homogeneous graph.  ``mode='node'`` draws ``budget`` nodes with
    probability proportional to ``max(out-degree, 1)``; ``'edge'`` draws ``budget`` edges with probability proportional
    to ``1 / in_deg(dst) + 1 / out_deg(src)`` and keeps their end points; ``'walk'`` takes ``budget = (num_roots,
    walk_length)`` uniform roots and keeps every node their walks visit (this package's :func:`random_walk`, so the
    graph is on the GPU).  The draws come from torch's generators, like the reference's; ``cache`` keeps the
    probabilities between calls.  The result lists the distinct node ids in ascending order."""

    def __init__(self, mode, budget, cache=True):
        if mode not in ("node", "edge", "walk"):
            raise _DGLError("Expect mode to be 'node', 'edge' or 'walk', got {}.".format(mode))
        self.mode = mode
        self.budget = budget
        self.cache = cache
        self.prob = None

    def _cached(self, build):
        if self.cache and self.prob is not None:
            return self.prob
        prob = build()
        if self.cache:
            self.prob = prob
        return prob

    def node_sampler(self, g):
        prob = self._cached(lambda: g.out_degrees().float().clamp(min=1))
        return torch.multinomial(prob, num_samples=self.budget, replacement=True).unique().to(g.idtype)

    def edge_sampler(self, g):
        src, dst = g.edges()

        def build():
            p = 1.0 / g.in_degrees().float().clamp(min=1)[dst.long()] + 1.0 / g.out_degrees().float().clamp(min=1)[src.long()]
            return p / p.sum()
        picked = torch.multinomial(self._cached(build), num_samples=self.budget, replacement=True).unique()
        return torch.cat([src[picked], dst[picked]]).unique().to(g.idtype)

    def walk_sampler(self, g):
        num_roots, walk_length = self.budget
        roots = torch.randint(0, g.num_nodes(), (num_roots,)).to(device=g.device, dtype=g.idtype)
        traces, types = random_walk(g, roots, length=walk_length)
        return pack_traces(traces, types)[0].unique().to(g.idtype)

    def sample(self, g, indices=None):  # noqa: ARG002  (a placeholder in the reference too)
        """The sampled subgraph; ``subg.ndata[dgl.NID]`` are the drawn nodes."""
        if len(g.ntypes) != 1 or len(g.canonical_etypes) != 1:
            raise _DGLError("SAINTSampler only supports homogeneous graphs")
        node_ids = getattr(self, self.mode + "_sampler")(g)
        return _induced_on(g, {g.ntypes[0]: node_ids})


# ---- PinSAGE neighbourhoods ----------------------------------------------------------------------
class RandomWalkNeighborSampler:
    """``dgl.sampling.RandomWalkNeighborSampler`` (python/dgl/sampling/pinsage.py:27-163): the neighbours of a seed are
    the nodes of its own type that ``num_random_walks`` walks from it visit most often.  A walk is up to
    ``num_traversals`` passes over ``metapath`` (which must end in the node type it starts from) and halts with
    ``termination_prob`` in front of every pass but the first.  Calling the sampler returns a graph over ALL nodes of that
    type with one edge ``neighbour -> seed`` per kept neighbour, at most ``num_neighbors`` per seed, ranked by
    (visits, id) descending, and the visit counts in ``edata[weight_column]``.  Walks and selection run on the device
    (csrc/random_walk.hip, csrc/pinsage.hip); ``seed`` pins the walks as in :func:`random_walk`."""

    def __init__(self, G, num_traversals, termination_prob, num_random_walks, num_neighbors, metapath=None,
                 weight_column="weights"):
        self.G = G
        self.weight_column = weight_column
        self.num_random_walks = int(num_random_walks)
        self.num_neighbors = int(num_neighbors)
        self.num_traversals = int(num_traversals)
        if metapath is None:
            if len(G.ntypes) > 1 or len(G.etypes) > 1:
                raise ValueError("Metapath must be specified if the graph is homogeneous.")   # (the reference's wording)
            metapath = [G.canonical_etypes[0]]
        metapath = list(metapath)
        start_ntype = G.to_canonical_etype(metapath[0])[0]
        end_ntype = G.to_canonical_etype(metapath[-1])[-1]
        if start_ntype != end_ntype:
            raise ValueError("The metapath must start and end at the same node type.")
        self.ntype = start_ntype
        self.metapath_hops = len(metapath)
        self.metapath = metapath
        self.full_metapath = metapath * self.num_traversals
        # halting is tested in front of the first step of every pass but the first
        restart_prob = torch.zeros(self.metapath_hops * self.num_traversals, dtype=torch.float32)
        restart_prob[self.metapath_hops::self.metapath_hops] = termination_prob
        self.restart_prob = restart_prob.to(G.device)

    def __call__(self, seed_nodes, seed=None):
        G = self.G
        if not torch.is_tensor(seed_nodes):
            seed_nodes = torch.as_tensor(seed_nodes, dtype=G.idtype)
        if seed_nodes.dtype != G.idtype:
            raise _DGLError("Expect argument \"seed_nodes\" to have data type %s. But got %s." % (G.idtype, seed_nodes.dtype))
        seed_nodes = seed_nodes.reshape(-1).to(G.device)
        walks = seed_nodes.repeat_interleave(self.num_random_walks)
        paths, _ = random_walk(G, walks, metapath=self.full_metapath, restart_prob=self.restart_prob, seed=seed)
        src = paths[:, self.metapath_hops::self.metapath_hops].reshape(-1).contiguous()   # (one column stays a strided view)
        dst = paths[:, 0].repeat_interleave(self.num_traversals)
        if src.numel():
            src, dst, counts = _capi.select_pinsage_neighbors(src, dst, self.num_random_walks * self.num_traversals,
                                                              self.num_neighbors)
        else:
            counts = src
        g = _heterograph({(self.ntype, "_E", self.ntype): (src, dst)}, {self.ntype: G.num_nodes(self.ntype)},
                         idtype=G.idtype, device=G.device)
        g.edata[self.weight_column] = counts
        return g


class PinSAGESampler(RandomWalkNeighborSampler):
    """``dgl.sampling.PinSAGESampler`` (python/dgl/sampling/pinsage.py:166-272): :class:`RandomWalkNeighborSampler` on a
    bidirectional bipartite graph, along the metapath ``ntype -> other_type -> ntype`` (the first edge type of each
    direction)."""

    def __init__(self, G, ntype, other_type, num_traversals, termination_prob, num_random_walks, num_neighbors,
                 weight_column="weights"):
        def etype_between(a, b):
            for c in G.canonical_etypes:
                if c[0] == a and c[2] == b:
                    return c
            raise _DGLError("PinSAGESampler: no edge type goes from '%s' to '%s'" % (a, b))

        super().__init__(G, num_traversals, termination_prob, num_random_walks, num_neighbors,
                         metapath=[etype_between(ntype, other_type), etype_between(other_type, ntype)],
                         weight_column=weight_column)
