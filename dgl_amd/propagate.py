"""``dgl.propagate``: message passing frontier by frontier.

Mirrors python/dgl/propagate.py.  The reference moves the whole graph to the CPU to find the frontiers and copies every
frontier back; here the frontiers come from csrc/traversal.hip on the graph's own device (:mod:`dgl_amd.traversal`) and
are handed to ``DGLGraph.pull`` / ``send_and_recv`` where they are."""
from . import traversal as _trv
from ._lib import DGLAMDError as _DGLError

__all__ = ["prop_nodes", "prop_edges", "prop_nodes_bfs", "prop_nodes_topo", "prop_edges_dfs"]


def prop_nodes(graph, nodes_generator, message_func, reduce_func, apply_node_func=None):
    """Functional form of :meth:`dgl_amd.DGLGraph.prop_nodes`."""
    graph.prop_nodes(nodes_generator, message_func, reduce_func, apply_node_func)


def prop_edges(graph, edges_generator, message_func, reduce_func, apply_node_func=None):
    """Functional form of :meth:`dgl_amd.DGLGraph.prop_edges`."""
    graph.prop_edges(edges_generator, message_func, reduce_func, apply_node_func)


def _homogeneous(graph, who):
    if len(graph.canonical_etypes) != 1:
        raise _DGLError("%s only supports a homogeneous graph" % who)


def prop_nodes_bfs(graph, source, message_func, reduce_func, reverse=False, apply_node_func=None):
    """Pull along the node frontiers of a breadth-first search from ``source``
    (:func:`dgl_amd.traversal.bfs_nodes_generator`), the sources' frontier included."""
    _homogeneous(graph, "prop_nodes_bfs")
    prop_nodes(graph, _trv.bfs_nodes_generator(graph, source, reverse), message_func, reduce_func, apply_node_func)


def prop_nodes_topo(graph, message_func, reduce_func, reverse=False, apply_node_func=None):
    """Pull along the frontiers of the topological order (:func:`dgl_amd.traversal.topological_nodes_generator`): the
    sweep of a TreeLSTM or of any computation over a DAG."""
    _homogeneous(graph, "prop_nodes_topo")
    prop_nodes(graph, _trv.topological_nodes_generator(graph, reverse), message_func, reduce_func, apply_node_func)


def prop_edges_dfs(graph, source, message_func, reduce_func, reverse=False, has_reverse_edge=False,  # noqa: ARG001
                   has_nontree_edge=False, apply_node_func=None):  # noqa: ARG001
    """Not built: a depth-first search is sequential by nature and has no device form here."""
    raise _DGLError("prop_edges_dfs is absent: depth-first traversal is sequential and is not built; use prop_nodes_bfs, "
                    "prop_nodes_topo or prop_edges over bfs_edges_generator")
