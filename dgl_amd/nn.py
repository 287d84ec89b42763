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

__all__ = ["functional", "gat_attention", "GATAttention"]


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
