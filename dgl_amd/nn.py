"""``dgl_amd.nn`` — only what is NEW above the operator API.  The layers themselves (GraphConv, SAGEConv, GATConv,
RelGraphConv, TypedLinear, HeteroGraphConv ...) are the reference's own ``python/dgl/nn/pytorch/*.py``: they stay
untouched above ``update_all`` / ``dgl.ops`` (docs/DESIGN_detail_r1_r5.md §1) and run on this package through the ``dgl`` -> ``dgl_amd``
alias (``tools/ref_suite/run.py --suite nn`` imports them unmodified and runs the reference's layer tests).

``gat_attention`` (and the module ``GATAttention`` around it) is the one addition: GATConv's attention block
(python/dgl/nn/pytorch/conv/gatconv.py:330-347 — ``u_add_v`` -> ``leaky_relu`` -> ``edge_softmax`` -> ``attn_drop`` ->
``u_mul_e_sum``) as ONE operator, so that a layer can hand the whole
block to the fused kernel (csrc/gat_attention.hip) instead of four launches that write and re-read three (E, H) tensors.
"""
import torch
import torch.nn.functional as F

from . import edge_order as _eo
from . import function as fn
from .ops import edge_softmax

__all__ = ["functional", "gat_attention", "GATAttention", "GraphormerBias", "BiasedMHA", "SpatialEncoder3d"]


class functional:  # noqa: N801  (a namespace: python/dgl/nn/functional/__init__.py exports exactly this)
    """``dgl.nn.functional``."""
    edge_softmax = staticmethod(edge_softmax)


def gat_attention(graph, ft, el, er, negative_slope=0.2, fused=None, handoff=False, attn_drop=0.0, training=True,
                  seed=None, get_attention=False):
    """``out[v] = sum_{u->v} softmax_v(leaky_relu(el[u] + er[v])) * ft[u]`` per head.

    ft: (N_src, H, D); el: (N_src, H, 1); er: (N_dst, H, 1) -> (N_dst, H, D).  ``fused=None`` takes the one-pass kernel
    (``dgl_amd.ops.gat_attention``) whenever it applies — fp32 / fp16 / bf16 operands of one dtype and any head width
    with ``H * next_pow2(ceil(D / V)) <= 64``, ``V = min(16 / itemsize, largest power of two dividing D)``
    (``dgl_amd.ops.gat_attention_applies``) — and the composed operators otherwise; ``fused=False`` forces the
    composition (the reference's own sequence, the parity yardstick); ``handoff=True`` runs the composition inside
    ``dgl_amd.edge_order_handoff()`` (opt-in: entering that scope installs edge_order's process-wide shims).

    ``attn_drop`` / ``training`` / ``seed`` / ``get_attention`` as in ``dgl_amd.ops.gat_attention``: dropout on the
    attention weights (gatconv.py:337) and ``(out, attn)`` with ``attn`` (E, H, 1) in edge-id order, after dropout.
    A call that needs the training kernels — ``attn_drop > 0`` with ``training=True``, or ``get_attention=True`` — takes
    them only with ``fused=True``; ``fused=None`` composes such a call, because the training kernels' speed against the
    composition has not been measured yet.  An invalid ``attn_drop`` raises on the fused route only.
    The two routes draw from DIFFERENT random streams: the fused kernel keys a Philox mask by (seed, edge id, head),
    the composition applies ``F.dropout`` (torch's device generator; ``seed`` is not used there), so they agree in
    distribution, not mask for mask.  On the composed route ``attn`` is differentiable; on the fused route it is not."""
    from . import ops

    if fused is None:
        # the training kernels (dropout active, or the weights asked for) are opt-in until their speed is on record
        plain = not get_attention and not (attn_drop and training)
        fused = plain and ops.gat_attention_applies(graph, ft, el, er)
    if fused:
        return ops.gat_attention(graph, ft, el, er, negative_slope, attn_drop, training, seed, get_attention)
    with graph.local_scope():
        graph.srcdata.update({"ft": ft, "el": el})
        graph.dstdata.update({"er": er})
        with _eo.edge_order_handoff(bool(handoff)):
            graph.apply_edges(fn.u_add_v("el", "er", "e"))
            a = edge_softmax(graph, F.leaky_relu(graph.edata.pop("e"), negative_slope))
            graph.edata["a"] = F.dropout(a, attn_drop, training) if attn_drop else a
            graph.update_all(fn.u_mul_e("ft", "a", "m"), fn.sum("m", "ft"))
            if get_attention:
                return graph.dstdata["ft"], graph.edata["a"]
            return graph.dstdata["ft"]


class GATAttention(torch.nn.Module):
    """:func:`gat_attention` as a module: GATConv's attention block with its ``attn_drop``.  ``self.training`` is passed
    through, so ``model.train()`` / ``model.eval()`` switch the dropout mask on and off."""

    def __init__(self, negative_slope=0.2, attn_drop=0.0):
        super().__init__()
        self.negative_slope = float(negative_slope)
        self.attn_drop = float(attn_drop)

    def forward(self, graph, ft, el, er, fused=None, handoff=False, seed=None, get_attention=False):
        return gat_attention(graph, ft, el, er, self.negative_slope, fused=fused, handoff=handoff, attn_drop=self.attn_drop,
                             training=self.training, seed=seed, get_attention=get_attention)

    def extra_repr(self):
        return "negative_slope=%g, attn_drop=%g" % (self.negative_slope, self.attn_drop)


class _EmbeddingTable(torch.nn.Module):
    """One ``embedding_table``, the only parameter of the reference's SpatialEncoder and of its PathEncoder: a state dict
    of either loads into it unchanged."""

    def __init__(self, rows, cols, padding_idx=None):
        super().__init__()
        self.embedding_table = torch.nn.Embedding(rows, cols, padding_idx=padding_idx)


class GraphormerBias(torch.nn.Module):
    """The attention bias of a Graphormer layer: ``SpatialEncoder(max_dist, num_heads)`` plus
    ``PathEncoder(max_len, feat_dim, num_heads)`` (python/dgl/nn/pytorch/gt) as ONE operator,
    :func:`dgl_amd.ops.graphormer_bias`.  The tables sit under the reference's names and shapes,
    ``spatial_encoder.embedding_table.weight`` (max_dist + 2, num_heads; row 0 is the padding row) and
    ``path_encoder.embedding_table.weight`` (max_len * num_heads, feat_dim), so
    ``m.spatial_encoder.load_state_dict(spatial.state_dict())`` and ``m.path_encoder.load_state_dict(path.state_dict())``
    carry trained encoders over.

    ``forward(dist, paths, edge_feat)``: `dist` of any shape and `paths` of that shape plus the path axis, as
    ``shortest_dist(g, return_paths=True)`` returns them (callers slice per-graph blocks out of the batched result with
    torch indexing), `edge_feat` (E, feat_dim) indexed by the ids in `paths`.  Returns ``(*dist.shape, num_heads)``."""

    def __init__(self, max_dist, max_len, feat_dim, num_heads=1):
        super().__init__()
        self.max_dist, self.max_len, self.feat_dim, self.num_heads = int(max_dist), int(max_len), int(feat_dim), int(num_heads)
        self.spatial_encoder = _EmbeddingTable(self.max_dist + 2, self.num_heads, padding_idx=0)
        self.path_encoder = _EmbeddingTable(self.max_len * self.num_heads, self.feat_dim)

    def forward(self, dist, paths, edge_feat, fused=None):
        from . import ops

        return ops.graphormer_bias(dist, paths, edge_feat, self.path_encoder.embedding_table.weight,
                                   self.spatial_encoder.embedding_table.weight, max_len=self.max_len, padding_idx=0, fused=fused)

    def extra_repr(self):
        return "max_dist=%d, max_len=%d, feat_dim=%d, num_heads=%d" % (self.max_dist, self.max_len, self.feat_dim, self.num_heads)


class BiasedMHA(torch.nn.Module):
    """Dense multi-head attention with a graph attention bias, the reference's ``BiasedMHA(feat_size, num_heads,
    bias=True, attn_bias_type="add", attn_drop=0.1)`` (python/dgl/nn/pytorch/gt/biased_mha.py) with its attention on
    :func:`dgl_amd.ops.biased_attention`.  ``q_proj``, ``k_proj``, ``v_proj`` and ``out_proj`` carry the reference's
    names, shapes and initialisation, so its state dict loads unchanged; they stay ``nn.Linear`` and the operator takes
    the (B, N, H, D) views of their outputs without a copy.

    ``forward(ndata, attn_bias=None, attn_mask=None, fused=None, seed=None)``: `ndata` (B, N, feat_size), `attn_bias`
    (B, N, N, num_heads), `attn_mask` (B, N, N) with True = masked.  Returns (B, N, feat_size).  On the fused route a
    fully masked row yields the output bias of ``out_proj`` (a zero attention row) where the reference yields NaN.
    ``attn_bias_type="mul"`` is the torch composition only (absent from the kernels)."""

    def __init__(self, feat_size, num_heads, bias=True, attn_bias_type="add", attn_drop=0.1):
        super().__init__()
        self.feat_size, self.num_heads = int(feat_size), int(num_heads)
        self.head_dim = self.feat_size // self.num_heads
        if self.head_dim * self.num_heads != self.feat_size:
            raise ValueError("feat_size must be divisible by num_heads")
        if attn_bias_type not in ("add", "mul"):
            raise ValueError("attn_bias_type must be 'add' or 'mul'")
        self.scaling = self.head_dim ** -0.5
        self.attn_bias_type, self.attn_drop = attn_bias_type, float(attn_drop)
        self.q_proj = torch.nn.Linear(feat_size, feat_size, bias=bias)
        self.k_proj = torch.nn.Linear(feat_size, feat_size, bias=bias)
        self.v_proj = torch.nn.Linear(feat_size, feat_size, bias=bias)
        self.out_proj = torch.nn.Linear(feat_size, feat_size, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        for proj in (self.q_proj, self.k_proj, self.v_proj):
            torch.nn.init.xavier_uniform_(proj.weight, gain=2 ** -0.5)
        torch.nn.init.xavier_uniform_(self.out_proj.weight)
        if self.out_proj.bias is not None:
            torch.nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, ndata, attn_bias=None, attn_mask=None, fused=None, seed=None):
        from . import ops

        B, N, _ = ndata.shape
        q, k, v = (proj(ndata).view(B, N, self.num_heads, self.head_dim) for proj in (self.q_proj, self.k_proj, self.v_proj))
        if self.attn_bias_type == "mul" and attn_bias is not None:
            if fused:
                raise ops.DGLAMDError("biased_attention: the multiplicative bias has no kernel (attn_bias_type='mul')")
            w = torch.einsum("bihd,bjhd->bijh", q * self.scaling, k) * attn_bias
            if attn_mask is not None:
                w = w.masked_fill(attn_mask.to(torch.bool).unsqueeze(-1), float("-inf"))
            w = torch.nn.functional.dropout(torch.softmax(w, dim=2), p=self.attn_drop, training=self.training)
            attn = torch.einsum("bijh,bjhd->bihd", w, v)
        else:
            attn = ops.biased_attention(q, k, v, attn_bias, attn_mask, scale=self.scaling, attn_drop=self.attn_drop,
                                        training=self.training, seed=seed, fused=fused)
        return self.out_proj(attn.reshape(B, N, self.feat_size))

    def extra_repr(self):
        return "feat_size=%d, num_heads=%d, attn_bias_type=%s, attn_drop=%g" % (self.feat_size, self.num_heads,
                                                                               self.attn_bias_type, self.attn_drop)


class SpatialEncoder3d(torch.nn.Module):
    """The attention bias of the 3D (molecular) Graphormer, the reference's ``SpatialEncoder3d(num_kernels, num_heads=1,
    max_node_type=100)`` (python/dgl/nn/pytorch/gt/spatial_encoder.py) on :func:`dgl_amd.ops.spatial_encoder_3d`.
    ``means``, ``stds``, ``linear_layer_1``, ``linear_layer_2``, ``gamma`` and ``beta`` carry the reference's names,
    shapes and initialisation, so its state dict loads unchanged.

    ``forward(coord, node_type=None, fused=None)``: `coord` (B, N, 3), `node_type` (B, N) integer ids in
    [-1, max_node_type) (-1 = a padded node).  Returns (B, N, N, num_heads).  The module gathers the (B, N) scalars of
    the source rows ``node_type + 2`` and the target rows ``node_type + max_node_type + 3`` of ``gamma`` and ``beta``
    with torch's embedding (row 0, the padding row, for all four when `node_type` is None): the id range check, the
    padding row's zero gradient and the scatter of the gradients into the tables stay torch's, and the kernels never
    index a table by a caller's id."""

    def __init__(self, num_kernels, num_heads=1, max_node_type=100):
        super().__init__()
        self.num_kernels, self.num_heads, self.max_node_type = int(num_kernels), int(num_heads), int(max_node_type)
        self.means = torch.nn.Parameter(torch.empty(self.num_kernels))
        self.stds = torch.nn.Parameter(torch.empty(self.num_kernels))
        self.linear_layer_1 = torch.nn.Linear(self.num_kernels, self.num_kernels)
        self.linear_layer_2 = torch.nn.Linear(self.num_kernels, self.num_heads)
        self.gamma = torch.nn.Embedding(2 * self.max_node_type + 3, 1, padding_idx=0)
        self.beta = torch.nn.Embedding(2 * self.max_node_type + 3, 1, padding_idx=0)
        torch.nn.init.uniform_(self.means, 0, 3)
        torch.nn.init.uniform_(self.stds, 0, 3)
        torch.nn.init.constant_(self.gamma.weight, 1)
        torch.nn.init.constant_(self.beta.weight, 0)

    def forward(self, coord, node_type=None, fused=None):
        from . import ops

        if node_type is None:
            src = tgt = torch.zeros(coord.shape[:2], dtype=torch.long, device=coord.device)
        else:
            src, tgt = node_type.long() + 2, node_type.long() + self.max_node_type + 3
        pair = [table(ids).squeeze(-1) for table in (self.gamma, self.beta) for ids in (src, tgt)]
        return ops.spatial_encoder_3d(coord, self.means, self.stds, self.linear_layer_1.weight, self.linear_layer_1.bias,
                                      self.linear_layer_2.weight, self.linear_layer_2.bias, *pair, fused=fused)

    def extra_repr(self):
        return "num_kernels=%d, num_heads=%d, max_node_type=%d" % (self.num_kernels, self.num_heads, self.max_node_type)
