"""``dgl.traversal``: the frontiers of a breadth-first search and of the topological order.

Mirrors python/dgl/traversal.py over csrc/traversal.hip (the rule: include/dgl_amd.h "Graph traversal").  The reference
copies the graph to the CPU on every call and runs a sequential queue; here a GPU graph stays on the GPU: every level is
a mark pass and a select pass over the frontier's rows, the frontiers come out in the queue's order without a sort, and
only sizes come back to the host (24 bytes per level).  A CPU graph runs the same rule compiled for the host.

The depth-first generators are sequential by nature and are not built: they raise by name."""
import torch

from . import _capi
from ._lib import DGLAMDError as _DGLError

__all__ = ["bfs_nodes_generator", "bfs_edges_generator", "topological_nodes_generator", "dfs_edges_generator",
           "dfs_labeled_edges_generator"]


def _relation(graph, who):
    if len(graph.canonical_etypes) != 1 or len(graph.ntypes) != 1 or getattr(graph, "is_block", False):
        raise _DGLError("%s: graph traversal takes a homogeneous graph (one node type, one edge type, no block)" % who)
    return graph._graph.relations[0]


def _csr(rel, fmt, gpu):
    indptr, indices, eids = getattr(rel, fmt)()
    make = _capi.make_csr if gpu else _capi.host_csr
    return make(indptr.contiguous(), indices.contiguous(), None if eids is None else eids.contiguous(), rel.num_dst)


def _sources(graph, source, who):
    if torch.is_tensor(source):
        if source.is_floating_point() or source.dtype == torch.bool:
            raise _DGLError("%s: source must hold node ids, got dtype %s" % (who, source.dtype))
        src = source.reshape(-1)
    else:
        src = torch.as_tensor(source if isinstance(source, (list, tuple)) else [source], dtype=torch.int64).reshape(-1)
    return src.to(device=graph.device, dtype=graph.idtype).contiguous()


def _run(graph, who, mode, source, reverse):
    rel = _relation(graph, who)
    gpu = graph.device.type == "cuda"
    # forward: the out-edge CSR, counts from the in-edge CSR; reverse: the other way round
    walk, other = ("csc", "csr") if reverse else ("csr", "csc")
    csr = _csr(rel, walk, gpu)
    opposite = _csr(rel, other, gpu) if mode == _capi.TRAVERSE_TOPO_NODES else None
    src = None if mode == _capi.TRAVERSE_TOPO_NODES else _sources(graph, source, who)
    try:
        ids, sections = (_capi.traverse if gpu else _capi.traverse_host)(mode, csr, opposite, src)
    except _DGLError as err:
        raise _DGLError("%s: %s" % (who, str(err).split(": ", 1)[-1])) from None
    return tuple(torch.split(ids, sections)) if sections else ()


def bfs_nodes_generator(graph, source, reverse=False):
    """The node frontiers of a breadth-first search from ``source`` (a node id, a list or a tensor of ids): a tuple of
    id tensors in the graph's idtype on its device, the first the sources as given.  Inside a frontier the nodes stand in
    the order a sequential queue discovers them.  ``reverse`` follows the in-edges."""
    return _run(graph, "bfs_nodes_generator", _capi.TRAVERSE_BFS_NODES, source, reverse)


def bfs_edges_generator(graph, source, reverse=False):
    """The edge frontiers of a breadth-first search from ``source``: frontier k holds the ids of the tree edges that
    discover the nodes at distance k + 1, in the order a sequential queue takes them."""
    return _run(graph, "bfs_edges_generator", _capi.TRAVERSE_BFS_EDGES, source, reverse)


def topological_nodes_generator(graph, reverse=False):
    """The node frontiers of the topological order: first the nodes without in-edges (ascending), then every node as
    soon as all its predecessors are in earlier frontiers.  ``reverse`` starts from the nodes without out-edges.  A
    graph with a loop (a self-loop is one) raises ``DGLAMDError`` ("loop detected")."""
    return _run(graph, "topological_nodes_generator", _capi.TRAVERSE_TOPO_NODES, None, reverse)


def dfs_edges_generator(graph, source, reverse=False):  # noqa: ARG001
    """Not built: a depth-first search is sequential by nature and has no device form here."""
    raise _DGLError("dfs_edges_generator is absent: depth-first traversal is sequential and is not built; "
                    "use bfs_edges_generator or topological_nodes_generator")


def dfs_labeled_edges_generator(graph, source, reverse=False, has_reverse_edge=False, has_nontree_edge=False,  # noqa: ARG001
                                return_labels=True):  # noqa: ARG001
    """Not built: a depth-first search is sequential by nature and has no device form here."""
    raise _DGLError("dfs_labeled_edges_generator is absent: depth-first traversal is sequential and is not built; "
                    "use bfs_edges_generator or topological_nodes_generator")
