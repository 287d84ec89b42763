"""Operator API of the hot path: the ``dgl.ops`` surface for g-SpMM / g-SDDMM / edge softmax.

Same names, argument meaning and semantics as python/dgl/ops/spmm.py (``gspmm`` :39-116 and
the generated ``u_mul_e_sum`` ... ``copy_e_mean`` aliases :224-241), python/dgl/ops/sddmm.py
(``gsddmm`` :40-98, ``u_add_v`` ... ``copy_e`` :146-207) and python/dgl/ops/edge_softmax.py
(:12).  ``g`` is a :class:`dgl_amd.heterograph.DGLGraph`.
"""
import sys

import torch

from . import autograd as _F
from . import _capi
from ._lib import DGLAMDError

__all__ = ["gspmm", "gsddmm", "edge_softmax", "copy_u", "copy_v", "copy_e", "gat_attention", "gat_attention_applies",
           "graphormer_bias", "graphormer_bias_gather", "biased_attention", "biased_attention_applies",
           "spatial_encoder_3d", "spatial_encoder_3d_applies"]


def _reshape_for_broadcast(op, lhs, rhs):
    """Pad the shorter feature shape with 1s right after the node/edge axis so both operands
    have the same rank (ops/spmm.py:13-36); `dot` keeps the last (reduced) axis aligned."""
    ls, rs = lhs.shape, rhs.shape
    if len(ls) == len(rs):
        return lhs, rhs
    if len(ls) < len(rs):
        lhs = lhs.reshape((ls[0],) + (1,) * (len(rs) - len(ls)) + tuple(ls[1:]))
    else:
        rhs = rhs.reshape((rs[0],) + (1,) * (len(ls) - len(rs)) + tuple(rs[1:]))
    return lhs, rhs


def gspmm(g, op, reduce_op, lhs_data, rhs_data):
    r"""Generalized SpMM: messages ``op(lhs[src], rhs[edge])`` reduced into destination nodes.

    op in {add, sub, mul, div, copy_lhs, copy_rhs}; reduce_op in {sum, max, min, mean}.
    For graphs with several relations pass tuples/dicts as the reference does (lhs indexed by
    source node type, rhs by edge type)."""
    if op not in ("add", "sub", "mul", "div", "copy_lhs", "copy_rhs"):
        raise DGLAMDError("Unsupported SpMM binary operator: {}".format(op))
    if reduce_op not in ("sum", "max", "min", "mean"):
        raise DGLAMDError("Unsupported SpMM reducer: {}".format(reduce_op))
    gidx = g._graph
    if gidx.number_of_etypes() == 1:
        if op not in ("copy_lhs", "copy_rhs"):
            lhs_data, rhs_data = _reshape_for_broadcast(op, lhs_data, rhs_data)
        if reduce_op == "mean" and gidx.relations[0].allowed("csc"):
            # the division by clamp(in_degree, 1) happens inside the kernel (DGLA_MEAN)
            return _F.gspmm_mean(gidx, op, lhs_data, rhs_data, g.in_degrees())
        ret = _F.gspmm(gidx, op, "sum" if reduce_op == "mean" else reduce_op, lhs_data, rhs_data)
    else:
        lhs_t = _to_type_tuple(g, lhs_data, "ntype") if op != "copy_rhs" else ()
        rhs_t = _to_type_tuple(g, rhs_data, "etype") if op != "copy_lhs" else ()
        if op not in ("copy_lhs", "copy_rhs"):
            lhs_t, rhs_t = list(lhs_t), list(rhs_t)
            for et in range(gidx.number_of_etypes()):
                s, _ = gidx.metagraph.find_edge(et)
                if lhs_t[s] is not None and rhs_t[et] is not None:
                    lhs_t[s], rhs_t[et] = _reshape_for_broadcast(op, lhs_t[s], rhs_t[et])
        ret = _F.gspmm_hetero(gidx, op, "sum" if reduce_op == "mean" else reduce_op,
                              len(lhs_t), *(tuple(lhs_t) + tuple(rhs_t)))
    if reduce_op == "mean":
        # mean = sum / clamp(in_degree, 1)  (ops/spmm.py:109-114)
        def div(x, deg):
            shp = (x.shape[0],) + (1,) * (x.dim() - 1)
            return x / deg.to(x.dtype).clamp(min=1).reshape(shp)

        if gidx.number_of_etypes() == 1:
            ret = div(ret, g.in_degrees())
        else:
            raise DGLAMDError("Reduce op 'mean' is not supported on graphs with several relations "
                              "(python/dgl/heterograph.py:5133-5138).")
    return ret


def gsddmm(g, op, lhs_data, rhs_data, lhs_target="u", rhs_target="v"):
    r"""Generalized SDDMM: ``out[e] = op(lhs[target_l(e)], rhs[target_r(e)])``.

    op in {add, sub, mul, div, dot, copy_lhs, copy_rhs}; targets in {u, v, e}."""
    if op not in ("add", "sub", "mul", "div", "dot", "copy_lhs", "copy_rhs"):
        raise DGLAMDError("Unsupported SDDMM binary operator: {}".format(op))
    if lhs_target not in "uve" or rhs_target not in "uve":
        raise DGLAMDError("targets must be one of 'u', 'v', 'e'")
    gidx = g._graph
    if gidx.number_of_etypes() == 1:
        if op not in ("copy_lhs", "copy_rhs"):
            lhs_data, rhs_data = _reshape_for_broadcast(op, lhs_data, rhs_data)
        return _F.gsddmm(gidx, op, lhs_data, rhs_data, lhs_target, rhs_target)
    kind = lambda t: "etype" if t == "e" else "ntype"
    lhs_t = _to_type_tuple(g, lhs_data, kind(lhs_target)) if op != "copy_rhs" else ()
    rhs_t = _to_type_tuple(g, rhs_data, kind(rhs_target)) if op != "copy_lhs" else ()
    return _F.gsddmm_hetero(gidx, op, len(lhs_t), lhs_target, rhs_target,
                            *(tuple(lhs_t) + tuple(rhs_t)))


def _to_type_tuple(g, data, kind):
    """dict keyed by type name (or tuple/list already in type-id order) -> tuple in id order."""
    if isinstance(data, (tuple, list)):
        return tuple(data)
    n = len(g.ntypes) if kind == "ntype" else len(g.canonical_etypes)
    out = [None] * n
    for k, v in data.items():
        idx = g.get_ntype_id(k) if kind == "ntype" else g.get_etype_id(k)
        out[idx] = v
    return tuple(out)


def edge_softmax(graph, logits, eids=None, norm_by="dst"):
    r"""Softmax of edge scores over the edges that share a destination (or source) node
    (python/dgl/ops/edge_softmax.py:12-140)."""
    if norm_by not in ("dst", "src"):
        raise DGLAMDError("norm_by must be 'dst' or 'src'")
    gidx = graph._graph
    if gidx.number_of_etypes() == 1:
        if eids is not None and not isinstance(eids, torch.Tensor):
            eids = torch.as_tensor(eids)
        return _F.edge_softmax(gidx, logits, eids, norm_by)
    # several relations: the normaliser runs over ALL incoming edges of a node regardless of
    # relation (EdgeSoftmax_hetero, sparse.py:750-850): concatenate per destination type
    scores = _to_type_tuple(graph, logits, "etype")
    if eids is not None:
        # the reference hands ``eids`` to ``gidx.edge_subgraph([eids], True)`` (sparse.py:771-772), i.e. ONE id array
        # per relation: here a dict {etype: ids} / a sequence in edge-type order (None = all edges of that type); a
        # single tensor is accepted when exactly one relation carries a score.  The softmax then runs on the
        # edge-induced subgraph (same nodes), scores listed in the order of the ids.
        if isinstance(eids, torch.Tensor):
            with_score = [et for et, sc in enumerate(scores) if sc is not None]
            if len(with_score) != 1:
                raise DGLAMDError("edge_softmax on a graph with several relations: give eids as a dict "
                                  "{edge type: ids} (a single id tensor is ambiguous)")
            per = [None] * len(scores)
            per[with_score[0]] = eids
        elif isinstance(eids, dict):
            per = [None] * len(scores)
            for k, v in eids.items():
                per[graph.get_etype_id(k)] = v
        else:
            per = list(eids) + [None] * (len(scores) - len(eids))
        full = []
        for et, ids in enumerate(per):
            if ids is None:
                ids = torch.arange(gidx.num_edges(et), dtype=gidx.dtype, device=gidx.ctx)
            elif not isinstance(ids, torch.Tensor):
                ids = torch.as_tensor(ids)
            full.append(ids.to(device=gidx.ctx, dtype=gidx.dtype))
        gidx = gidx.edge_subgraph(full)
    outs = _F.edge_softmax_hetero(gidx, None, norm_by, *scores)
    if isinstance(logits, dict):
        return {graph.canonical_etypes[et]: o for et, o in enumerate(outs) if o is not None}
    return tuple(outs)


# ---- GAT attention block as one operator ------------------------------------------------
def gat_attention_applies(graph, ft, el, er):
    """Whether the one-pass kernel takes this call: one relation with an in-edge CSC (and, when an operand needs a
    gradient, an out-edge CSR, which the backward reads), fp32 / fp16 / bf16 operands of ONE dtype on the GPU of shapes
    (N_src, H, D), (N_src, H, 1), (N_dst, H, 1) with (dtype, H, D) in the set of ``dgla_gat_attention_supported``
    (include/dgl_amd.h): with V = min(16 / itemsize, largest power of two dividing D) elements per lane and
    LPH = next_pow2(ceil(D / V)) lanes per head, H * LPH <= 64.  Anything else runs the composed operators
    (dgl_amd.nn.gat_attention)."""
    gidx = graph._graph
    if gidx.number_of_etypes() != 1 or not gidx.relations[0].allowed("csc"):
        return False
    if "dgl_amd._CAPI_GATAttentionForward" not in _registered():
        return False
    if ft.dim() != 3 or el.dim() != 3 or er.dim() != 3 or el.shape[2] != 1 or er.shape[2] != 1:
        return False
    if not (ft.dtype == el.dtype == er.dtype) or type(ft) is not torch.Tensor:
        return False
    if (torch.is_grad_enabled() and (ft.requires_grad or el.requires_grad or er.requires_grad) and
            not gidx.relations[0].allowed("csr")):
        return False
    h, d = int(ft.shape[1]), int(ft.shape[2])
    return (ft.is_cuda and el.shape[1] == h and er.shape[1] == h and _capi.gat_attention_supported(ft.dtype, h, d) and
            ft.shape[0] == el.shape[0] == graph.num_src_nodes() and er.shape[0] == graph.num_dst_nodes())


_registry_names = []


def _registered():
    if not _registry_names:
        from . import _ffi

        _registry_names.append(frozenset(_ffi.list_global_func_names()))
    return _registry_names[0]


def gat_attention(graph, ft, el, er, negative_slope=0.2, attn_drop=0.0, training=True, seed=None, get_attention=False):
    """``out[v] = sum_{u->v} softmax_v(leaky_relu(el[u] + er[v])) * ft[u]`` per head in ONE pass over the in-edges
    (csrc/gat_attention.hip): no (E, H) tensor is written or read; the backward recomputes the attention weights from
    the per-row (max, sum) the forward saved.  The composition it replaces: gatconv.py:330-347.  Takes fp32 / fp16 /
    bf16 operands of one dtype and every (H, D) of :func:`gat_attention_applies`; output and gradients carry the
    operands' dtype, with fp32 state inside and one rounding at the final stores.

    ``attn_drop`` (in [0, 1)) with ``training=True`` is GATConv's dropout on the attention weights
    (``attn_drop(edge_softmax(graph, e))``, gatconv.py:337), inside the kernel (csrc/gat_attention_train.hip): the keep
    bit is a function of (seed, edge id, head), evaluated in registers by the forward and again by the backward, so no
    mask is stored.  ``seed=None`` draws one 63-bit integer from torch's default CPU generator — ``torch.manual_seed``
    makes a run reproducible —, an explicit ``seed`` is used as given.  A call captured into a graph would replay ONE
    mask, so under stream capture ``attn_drop > 0`` needs an explicit seed.  With ``attn_drop == 0`` or
    ``training=False``, and ``get_attention=False``, this is the call without dropout: same kernels, same bits.
    ``attn_drop`` outside [0, 1) raises ``DGLAMDError`` whatever ``training`` says: a layer configured with an
    impossible rate is wrong in evaluation mode too.

    ``get_attention=True`` returns ``(out, attn)``: ``attn`` is (E, H, 1), in edge-id order, AFTER dropout, as the
    reference's ``get_attention`` returns it.  It is NOT differentiable (``requires_grad`` is False): gradients
    through the attention tensor need the composed route, ``dgl_amd.nn.gat_attention(..., fused=False)``."""
    p = float(attn_drop)
    if not 0.0 <= p < 1.0:
        raise DGLAMDError("gat_attention: attn_drop must lie in [0, 1), got %r" % (attn_drop,))
    if not gat_attention_applies(graph, ft, el, er):
        raise DGLAMDError("gat_attention: the fused kernel does not take these operands (dgl_amd.nn.gat_attention "
                          "falls back to the composed operators)")
    if not training:
        p = 0.0
    if p == 0.0 and not get_attention:
        return _F.gat_attention(graph._graph, ft, el, er, float(negative_slope))
    if p == 0.0:
        seed = 0
    elif seed is None:
        if torch.cuda.is_current_stream_capturing():
            raise DGLAMDError("gat_attention: attn_drop > 0 under stream capture needs an explicit seed — a captured "
                              "call would replay one mask on every launch of the graph")
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    seed = int(seed)
    if not 0 <= seed < 2 ** 63:
        raise DGLAMDError("gat_attention: seed must be an integer in [0, 2**63)")
    return _F.gat_attention(graph._graph, ft, el, er, float(negative_slope), p, seed, bool(get_attention))


# ---- Graphormer attention bias: spatial + path encoding as one operator ------------------------------
_GBIAS_MAX_HEADS, _GBIAS_MAX_LEN = 256, 32


def _gbias_check(dist, paths, floats, heads, max_len, spatial_weight):
    """The refusals of the Graphormer bias, by name, before anything is launched."""
    who = "graphormer_bias: "
    ints = (torch.int32, torch.int64)
    if dist.dtype not in ints or paths.dtype not in ints or dist.dtype != paths.dtype:
        raise DGLAMDError(who + "dist and paths must share one id width (both int64 or both int32), got %s and %s"
                          % (dist.dtype, paths.dtype))
    if paths.dim() != dist.dim() + 1 or paths.shape[:-1] != dist.shape:
        raise DGLAMDError(who + "paths must have the shape of dist plus one axis, got %s for dist %s"
                          % (tuple(paths.shape), tuple(dist.shape)))
    if len({t.dtype for t in floats}) != 1:
        raise DGLAMDError(who + "operand dtypes differ: %s" % ", ".join(str(t.dtype) for t in floats))
    if not 1 <= heads <= _GBIAS_MAX_HEADS:
        raise DGLAMDError(who + "%d heads: the kernels take 1 to %d" % (heads, _GBIAS_MAX_HEADS))
    if not 1 <= max_len <= _GBIAS_MAX_LEN:
        raise DGLAMDError(who + "max_len %d: the kernels take 1 to %d" % (max_len, _GBIAS_MAX_LEN))
    if spatial_weight is not None and (spatial_weight.dim() != 2 or spatial_weight.shape[0] < 2):
        raise DGLAMDError(who + "spatial_weight must be (max_dist + 2, H)")


def _gbias_route(fused, tensors):
    """True: the kernels.  CPU tensors take the torch composition unless the kernels were asked for by name."""
    on_gpu = all(t.is_cuda for t in tensors)
    if fused and not on_gpu:
        raise DGLAMDError("graphormer_bias: dgl_amd kernels run on a ROCm GPU (no CPU fallback); fused=True needs GPU tensors")
    return on_gpu if fused is None else bool(fused)


def _gbias_finish(path_sum, dist, spatial_weight, max_len, padding_idx, dtype):
    """The tail both compositions share: divide by the clamped distance, add the spatial row, round once."""
    out = path_sum / dist.clamp(1, max_len).unsqueeze(-1).to(torch.float32)
    if spatial_weight is not None:
        bins = dist.clamp(-1, spatial_weight.shape[0] - 2).long() + 1
        out = out + torch.nn.functional.embedding(bins, spatial_weight, padding_idx=padding_idx).to(torch.float32)
    return out.to(dtype)


def graphormer_bias_gather(dist, paths, T, spatial_weight=None, *, max_len, padding_idx=None, fused=None):
    """The gather half of :func:`graphormer_bias`: `T` is the projected table ``edge_feat @ path_weight.T``, shape
    (E, max_len * H).  Differentiable in `T` and `spatial_weight`; the gradients are deterministic sums (no atomics).
    An edge id >= E in `paths` is the caller's error in the forward (the pair misses the term) and raises in the
    backward."""
    max_len = int(max_len)
    if T.dim() != 2 or max_len < 1 or T.shape[1] % max_len:
        raise DGLAMDError("graphormer_bias: T must be (E, max_len * H)")
    heads = T.shape[1] // max_len
    floats = (T,) if spatial_weight is None else (T, spatial_weight)
    _gbias_check(dist, paths, floats, heads, max_len, spatial_weight)
    if spatial_weight is not None and spatial_weight.shape[1] != heads:
        raise DGLAMDError("graphormer_bias: spatial_weight has %d heads, T has %d" % (spatial_weight.shape[1], heads))
    if _gbias_route(fused, (dist, paths) + floats):
        out = _F.GraphormerBiasGather.apply(dist.reshape(-1).contiguous(), paths.reshape(-1, paths.shape[-1]).contiguous(),
                                            T, spatial_weight, max_len, heads, padding_idx)
        return out.reshape(tuple(dist.shape) + (heads,))
    lc, num_edges = min(paths.shape[-1], max_len), T.shape[0]
    rows = torch.cat([T.reshape(num_edges, max_len, heads), T.new_zeros(1, max_len, heads)])      # row E: the zero row
    ids = paths[..., :lc].long()
    ids = torch.where(ids < 0, torch.full_like(ids, num_edges), ids)
    acc = torch.zeros(tuple(dist.shape) + (heads,), dtype=torch.float32, device=T.device)
    for l in range(lc):                                                                           # the fixed order of l
        acc = acc + rows[ids[..., l], l].to(torch.float32)
    return _gbias_finish(acc, dist, spatial_weight, max_len, padding_idx, T.dtype)


def graphormer_bias(dist, paths, edge_feat, path_weight, spatial_weight=None, *, max_len=None, padding_idx=None, fused=None):
    """The attention bias of a Graphormer layer, SpatialEncoder + PathEncoder (python/dgl/nn/pytorch/gt) as one operator::

        out[p, h] = S[clamp(dist[p], -1, max_dist) + 1, h]
                  + (sum_{l < Lc, paths[p, l] >= 0} T[paths[p, l], l * H + h]) / clamp(dist[p], 1, max_len)
        T = edge_feat @ path_weight.T,  Lc = min(paths.shape[-1], max_len)

    `dist` (any shape) and `paths` (that shape + (Lp,)) are what ``shortest_dist(g, return_paths=True)`` returns, both
    int64 or both int32; ids index the rows of `edge_feat` (E, d).  `path_weight` is ``PathEncoder.embedding_table.weight``
    (max_len * H, d), `spatial_weight` ``SpatialEncoder.embedding_table.weight`` (max_dist + 2, H) or None.  `max_len`
    defaults to ``path_weight.shape[0] // H`` when a spatial table fixes H and is required otherwise.  ``padding_idx=0``
    zeroes the gradient of that spatial row, as ``nn.Embedding(padding_idx=0)`` does.  Returns ``(*dist.shape, H)``.

    On a GPU (``fused=None`` or True) the projection runs on :func:`segment_mm` with one segment and the gather, its
    backward to T and the backward to S on the kernels of csrc/graphormer_bias.hip: the (pairs, L, d) tensor of the
    reference is never built.  ``fused=False``, and CPU tensors, take the reference's torch composition."""
    if path_weight.dim() != 2 or edge_feat.dim() != 2 or edge_feat.shape[1] != path_weight.shape[1]:
        raise DGLAMDError("graphormer_bias: edge_feat must be (E, d) and path_weight (max_len * H, d)")
    if max_len is None:
        if spatial_weight is None:
            raise DGLAMDError("graphormer_bias: max_len is required when no spatial table fixes the head count")
        max_len = path_weight.shape[0] // max(int(spatial_weight.shape[-1]), 1)
    max_len = int(max_len)
    if max_len < 1 or path_weight.shape[0] % max_len:
        raise DGLAMDError("graphormer_bias: path_weight has %d rows, no multiple of max_len %d" % (path_weight.shape[0], max_len))
    heads = path_weight.shape[0] // max_len
    floats = (edge_feat, path_weight) + (() if spatial_weight is None else (spatial_weight,))
    _gbias_check(dist, paths, floats, heads, max_len, spatial_weight)
    if spatial_weight is not None and spatial_weight.shape[1] != heads:
        raise DGLAMDError("graphormer_bias: spatial_weight has %d heads, path_weight has %d" % (spatial_weight.shape[1], heads))
    if _gbias_route(fused, (dist, paths) + floats):
        seg = torch.tensor([edge_feat.shape[0]], dtype=torch.int64)
        table = segment_mm(edge_feat, path_weight.t().unsqueeze(0), seg)
        return graphormer_bias_gather(dist, paths, table, spatial_weight, max_len=max_len, padding_idx=padding_idx, fused=True)
    lc, num_edges = min(paths.shape[-1], max_len), edge_feat.shape[0]
    ids = paths[..., :lc].long()
    ids = torch.where(ids < 0, torch.full_like(ids, num_edges), ids)
    path_data = torch.cat([edge_feat, edge_feat.new_zeros(1, edge_feat.shape[1])])[ids]           # (..., Lc, d)
    weight = path_weight.reshape(max_len, heads, -1)[:lc]
    acc = torch.einsum("...ld,lhd->...h", path_data, weight).to(torch.float32)
    return _gbias_finish(acc, dist, spatial_weight, max_len, padding_idx, edge_feat.dtype)


# ---- biased multi-head attention: the consumer of the Graphormer bias -------------------------------
_BATTN_MAX_DIM = 128
_BATTN_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _battn_check(q, k, v, attn_bias, attn_mask, attn_drop):
    """The refusals of biased attention, by name, before anything is launched."""
    who = "biased_attention: "
    if q.dim() != 4 or k.shape != q.shape or v.shape != q.shape:
        raise DGLAMDError(who + "q, k, v must share one shape (B, N, H, D), got %s, %s, %s"
                          % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    B, N, H, D = q.shape
    floats = (q, k, v) + (() if attn_bias is None else (attn_bias,))
    if len({t.dtype for t in floats}) != 1:
        raise DGLAMDError(who + "operand dtypes differ: %s" % ", ".join(str(t.dtype) for t in floats))
    if attn_bias is not None and tuple(attn_bias.shape) != (B, N, N, H):
        raise DGLAMDError(who + "attn_bias must be (B, N, N, H) = %s, got %s" % ((B, N, N, H), tuple(attn_bias.shape)))
    if attn_mask is not None and (tuple(attn_mask.shape) != (B, N, N) or attn_mask.dtype not in (torch.bool, torch.uint8)):
        raise DGLAMDError(who + "attn_mask must be a bool or uint8 (B, N, N) = %s, got %s %s"
                          % ((B, N, N), attn_mask.dtype, tuple(attn_mask.shape)))
    if not 0.0 <= float(attn_drop) < 1.0:
        raise DGLAMDError(who + "attn_drop must lie in [0, 1), got %r" % (attn_drop,))
    tensors = floats + (() if attn_mask is None else (attn_mask,))
    if len({t.device for t in tensors}) != 1:
        raise DGLAMDError(who + "operands lie on different devices: %s" % ", ".join(str(t.device) for t in tensors))


def biased_attention_applies(q, k, v, attn_bias=None, attn_mask=None):
    """Whether the kernels of csrc/biased_attention.hip take this call: fp32 / fp16 / bf16 operands of one dtype on one
    GPU, q, k, v (B, N, H, D) with 1 <= D <= 128 and N, H >= 1, the bias (B, N, N, H), the mask a bool / uint8 (B, N, N)."""
    try:
        _battn_check(q, k, v, attn_bias, attn_mask, 0.0)
    except DGLAMDError:
        return False
    return (q.is_cuda and q.dtype in _BATTN_DTYPES and 1 <= q.shape[3] <= _BATTN_MAX_DIM and q.shape[1] >= 1 and q.shape[2] >= 1
            and all(type(t) is torch.Tensor for t in (q, k, v)))


def biased_attention(q, k, v, attn_bias=None, attn_mask=None, *, scale=None, attn_drop=0.0, training=True, seed=None, fused=None):
    """Dense multi-head attention with a graph attention bias, what BiasedMHA (python/dgl/nn/pytorch/gt/biased_mha.py)
    computes between its projections::

        s[b, i, j, h] = scale * <q[b, i, h], k[b, j, h]> + attn_bias[b, i, j, h];   -inf where attn_mask[b, i, j]
        out[b, i, h]  = sum_j dropout(softmax_j(s))[b, i, j, h] * v[b, j, h]

    `q`, `k`, `v` are (B, N, H, D), views of the (B, N, H * D) projections; `attn_bias` is (B, N, N, H), as
    :func:`graphormer_bias` lays it out; `attn_mask` (B, N, N), bool or uint8, True = masked, shared by the heads; `scale`
    defaults to ``D ** -0.5``.  Returns (B, N, H, D).  Differentiable in q, k, v and attn_bias.

    ``fused=None`` takes the kernels except for fp32 operands with N > 128 (slower than the composition at N = 512).
    On a GPU (``fused=None`` or True) this is ONE kernel forward and three backward (csrc/biased_attention.hip): the
    scores live in registers, the bias is read once in its own layout and its gradient written once in the same, and the
    backward recomputes the weights from the row log-sum-exp, deterministically.  ``fused=False``, and CPU tensors, take
    the reference's sequence in plain torch (bmm, add, masked fill, softmax, dropout, bmm).

    A row whose scores are all -inf (a fully masked row, -inf in the bias) gives a ZERO output row and zero gradients on
    the fused route; the composed route keeps the reference's NaN.  The two routes draw different dropout streams: the
    fused keep bit is a function of (seed, b, h, i, j) (see :func:`dgl_amd._capi.biased_attention_dropout_mask_host`),
    ``seed=None`` draws one from torch's default CPU generator, and under stream capture ``attn_drop > 0`` needs an
    explicit seed."""
    _battn_check(q, k, v, attn_bias, attn_mask, attn_drop)
    p = float(attn_drop) if training else 0.0
    scale = float(q.shape[3]) ** -0.5 if scale is None else float(scale)
    applies = biased_attention_applies(q, k, v, attn_bias, attn_mask)
    if fused and not applies:
        if not q.is_cuda:
            raise DGLAMDError("biased_attention: dgl_amd kernels run on a ROCm GPU (no CPU fallback); fused=True needs GPU tensors")
        if q.shape[3] > _BATTN_MAX_DIM:
            raise DGLAMDError("biased_attention: head width %d: the kernels take 1 to %d" % (q.shape[3], _BATTN_MAX_DIM))
        raise DGLAMDError("biased_attention: the fused kernels take float32, float16 or bfloat16 operands, got %s" % q.dtype)
    # fused=None: the kernels wherever they were measured not slower (profiles/r25): fp32 beyond N = 128 lost at the
    # one larger size measured (N = 512, 0.6-0.9x) and is left to the composition
    auto = applies and not (q.dtype == torch.float32 and q.shape[1] > 128)
    if auto if fused is None else bool(fused):
        if p == 0.0:
            seed = 0
        elif seed is None:
            if torch.cuda.is_current_stream_capturing():
                raise DGLAMDError("biased_attention: attn_drop > 0 under stream capture needs an explicit seed")
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        if not 0 <= int(seed) < 2 ** 63:
            raise DGLAMDError("biased_attention: seed must be an integer in [0, 2**63)")
        mask = None if attn_mask is None else attn_mask.contiguous().view(torch.uint8)
        return _F.BiasedAttention.apply(q, k, v, attn_bias, mask, scale, p, int(seed))
    B, N, H, D = q.shape
    qh = q.permute(0, 2, 1, 3).reshape(B * H, N, D) * scale
    w = torch.bmm(qh, k.permute(0, 2, 3, 1).reshape(B * H, D, N)).reshape(B, H, N, N).permute(0, 2, 3, 1)
    if attn_bias is not None:
        w = w + attn_bias
    if attn_mask is not None:
        w = w.masked_fill(attn_mask.to(torch.bool).unsqueeze(-1), float("-inf"))
    w = torch.softmax(w.permute(0, 3, 1, 2).reshape(B * H, N, N), dim=2)
    w = torch.nn.functional.dropout(w, p=p, training=p > 0.0)
    return torch.bmm(w, v.permute(0, 2, 1, 3).reshape(B * H, N, D)).reshape(B, H, N, D).permute(0, 2, 1, 3)


# ---- 3D spatial encoding: the attention bias of the 3D Graphormer -----------------------------------
_SE3D_MAX_K, _SE3D_MAX_H = 128, 64


def _se3d_check(coord, means, stds, w1, b1, w2, b2, pair):
    """The refusals of the 3D spatial encoding, by name, before anything is launched; returns (B, N, K, H)."""
    who = "spatial_encoder_3d: "
    if coord.dim() != 3 or coord.shape[2] != 3:
        raise DGLAMDError(who + "coord must be (B, N, 3), got %s" % (tuple(coord.shape),))
    B, N = coord.shape[:2]
    K, H = means.shape[0], w2.shape[0]
    shapes = ((means, (K,)), (stds, (K,)), (w1, (K, K)), (b1, (K,)), (w2, (H, K)), (b2, (H,)))
    if means.dim() != 1 or w2.dim() != 2 or any(tuple(t.shape) != s for t, s in shapes):
        raise DGLAMDError(who + "means, stds, b1 must be (K,), w1 (K, K), w2 (H, K), b2 (H,), got %s"
                          % ", ".join(str(tuple(t.shape)) for t, _ in shapes))
    if len({t.dtype for t in (w1, b1, w2, b2)}) != 1:
        raise DGLAMDError(who + "operand dtypes differ: %s" % ", ".join(str(t.dtype) for t in (w1, b1, w2, b2)))
    given = [t for t in pair if t is not None]
    if any(tuple(t.shape) != (B, N) for t in given):
        raise DGLAMDError(who + "gamma_src, gamma_tgt, beta_src, beta_tgt must be (B, N) = %s" % ((B, N),))
    tensors = [coord, means, stds, w1, b1, w2, b2] + given
    if len({t.device for t in tensors}) != 1:
        raise DGLAMDError(who + "operands lie on different devices: %s" % ", ".join(str(t.device) for t in tensors))
    return B, N, K, H


def spatial_encoder_3d_applies(coord, means, stds, w1, b1, w2, b2, gamma_src=None, gamma_tgt=None, beta_src=None, beta_tgt=None):
    """Whether the kernels of csrc/spatial_encoder3d.hip take this call: everything on one GPU, fp32 / fp16 / bf16
    weights of one dtype, 1 <= K <= 128, 1 <= H <= 64, and no gradient asked of `coord`."""
    pair = (gamma_src, gamma_tgt, beta_src, beta_tgt)
    try:
        _, _, K, H = _se3d_check(coord, means, stds, w1, b1, w2, b2, pair)
    except DGLAMDError:
        return False
    return (w1.is_cuda and w1.dtype in _BATTN_DTYPES and 1 <= K <= _SE3D_MAX_K and 1 <= H <= _SE3D_MAX_H
            and not (coord.requires_grad and torch.is_grad_enabled())
            and all(type(t) in (torch.Tensor, torch.nn.Parameter) for t in (coord, means, stds, w1, b1, w2, b2)))


def spatial_encoder_3d(coord, means, stds, w1, b1, w2, b2, gamma_src=None, gamma_tgt=None, beta_src=None, beta_tgt=None, *,
                       fused=None):
    """The 3D spatial encoding of SpatialEncoder3d (python/dgl/nn/pytorch/gt/spatial_encoder.py:136-209), the rule
    "3D spatial encoding" of include/dgl_amd.h::

        d = |coord[b, i] - coord[b, j]|;   x = (gamma_src[b, i] + gamma_tgt[b, j]) * d + (beta_src[b, i] + beta_tgt[b, j])
        g_k = exp(-0.5 * ((x - means[k]) / sd_k) ** 2) / (sqrt(2 * 3.14159) * sd_k),   sd_k = |stds[k]| + 1e-2
        out[b, i, j] = gelu(g @ w1.T + b1) @ w2.T + b2

    `coord` (B, N, 3); `means`, `stds` (K,); `w1` (K, K), `b1` (K,), `w2` (H, K), `b2` (H,) of one dtype, which is the
    result's; the four pair vectors (B, N) are what the reference's gamma / beta embeddings give per source and per
    target node (None: gamma 1 and 0, beta 0 and 0, i.e. x = d).  Returns (B, N, N, H), the layout
    :func:`biased_attention` takes as its bias.  Differentiable in everything but `coord` on the fused route.

    On a GPU (``fused=None`` or True) this is ONE kernel forward and three backward (csrc/spatial_encoder3d.hip): both
    weight matrices stay in registers, the features live in LDS only, and the backward recomputes them; coord, the pair
    vectors, means and stds cross as fp32.  ``fused=False``, CPU tensors, an empty batch and a `coord` that requires
    grad take the reference's sequence in plain torch (cdist without the matmul shortcut, Gaussian, linear, GELU, linear)."""
    pair = (gamma_src, gamma_tgt, beta_src, beta_tgt)
    B, N, K, H = _se3d_check(coord, means, stds, w1, b1, w2, b2, pair)
    applies = spatial_encoder_3d_applies(coord, means, stds, w1, b1, w2, b2, *pair)
    if fused and not applies:
        who = "spatial_encoder_3d: "
        if not 1 <= K <= _SE3D_MAX_K:
            raise DGLAMDError(who + "num_kernels %d: the kernels take 1 to %d" % (K, _SE3D_MAX_K))
        if not 1 <= H <= _SE3D_MAX_H:
            raise DGLAMDError(who + "num_heads %d: the kernels take 1 to %d" % (H, _SE3D_MAX_H))
        if not w1.is_cuda:
            raise DGLAMDError(who + "dgl_amd kernels run on a ROCm GPU (no CPU fallback); fused=True needs GPU tensors")
        if coord.requires_grad:
            raise DGLAMDError(who + "the gradient with respect to coord has no kernel (coord.requires_grad)")
        raise DGLAMDError(who + "the fused kernels take float32, float16 or bfloat16 weights, got %s" % w1.dtype)
    feat = torch.float64 if w1.dtype == torch.float64 else torch.float32
    if pair == (None, None, None, None):
        one, zero = coord.new_ones((B, N), dtype=feat), coord.new_zeros((B, N), dtype=feat)
        pair = (one, zero, zero, zero)
    elif None in pair:
        raise DGLAMDError("spatial_encoder_3d: give all four of gamma_src, gamma_tgt, beta_src, beta_tgt or none")
    coord, means, stds = coord.to(feat), means.to(feat), stds.to(feat)
    gs, gt, bs, bt = (t.to(feat) for t in pair)
    if (applies if fused is None else bool(fused)) and B * N > 0:
        return _F.SpatialEncoder3d.apply(coord, gs, gt, bs, bt, means, stds, w1, b1, w2, b2)
    d = torch.cdist(coord, coord, p=2.0, compute_mode="donot_use_mm_for_euclid_dist")
    x = (gs.unsqueeze(2) + gt.unsqueeze(1)) * d + (bs.unsqueeze(2) + bt.unsqueeze(1))
    sd = stds.abs() + 1e-2
    g = torch.exp(-0.5 * ((x.unsqueeze(-1) - means) / sd) ** 2) / ((2 * 3.14159) ** 0.5 * sd)
    h = torch.nn.functional.gelu(torch.nn.functional.linear(g.to(w1.dtype), w1, b1))
    return torch.nn.functional.linear(h, w2, b2)


# ---- generated aliases -----------------------------------------------------------------
def _make_spmm(binary, reduce_op):
    name = "u_{}_e_{}".format(binary, reduce_op)

    def f(g, x, y):
        return gspmm(g, binary, reduce_op, x, y)

    f.__name__ = name
    f.__doc__ = "Generalized SpMM: message = u {} e, reducer = {} (ops/spmm.py:119-170).".format(
        binary, reduce_op)
    return name, f


def _make_copy_spmm(which, reduce_op):
    name = "copy_{}_{}".format(which, reduce_op)
    op = "copy_lhs" if which == "u" else "copy_rhs"

    def f(g, x):
        return gspmm(g, op, reduce_op, x if which == "u" else None, None if which == "u" else x)

    f.__name__ = name
    f.__doc__ = "Generalized SpMM: message = copy_{}, reducer = {} (ops/spmm.py:173-221).".format(
        which, reduce_op)
    return name, f


def _make_sddmm(lhs, binary, rhs):
    name = "{}_{}_{}".format(lhs, binary, rhs)

    def f(g, x, y):
        return gsddmm(g, binary, x, y, lhs_target=lhs, rhs_target=rhs)

    f.__name__ = name
    f.__doc__ = "Generalized SDDMM: out[e] = {} {} {} (ops/sddmm.py:101-143).".format(lhs, binary, rhs)
    return name, f


_mod = sys.modules[__name__]
for _b in ("add", "sub", "mul", "div"):
    for _r in ("sum", "max", "min", "mean"):
        _n, _f = _make_spmm(_b, _r)
        setattr(_mod, _n, _f)
        __all__.append(_n)
for _w in ("u", "e"):
    for _r in ("sum", "max", "min", "mean"):
        _n, _f = _make_copy_spmm(_w, _r)
        setattr(_mod, _n, _f)
        __all__.append(_n)
for _l in "uve":
    for _r in "uve":
        for _b in ("add", "sub", "mul", "div", "dot"):
            _n, _f = _make_sddmm(_l, _b, _r)
            setattr(_mod, _n, _f)
            __all__.append(_n)


def copy_u(g, x):
    """Edge feature = source node feature (ops/sddmm.py:146-165)."""
    return gsddmm(g, "copy_lhs", x, None)


def copy_v(g, x):
    """Edge feature = destination node feature (ops/sddmm.py:168-187)."""
    return gsddmm(g, "copy_rhs", None, x)


def copy_e(g, x):
    """Identity on edge features (ops/sddmm.py:190-207)."""
    return x


# python/dgl/ops/__init__.py also re-exports the segment and gather / segment matmul operators
# (ops/segment.py:6, ops/gather_mm.py:6): dgl.ops.segment_reduce, segment_softmax, segment_mm, gather_mm
from .mm import gather_mm, segment_mm  # noqa: E402,F401
from .segment import segment_reduce, segment_softmax  # noqa: E402,F401

__all__ += ["segment_reduce", "segment_softmax", "segment_mm", "gather_mm"]
