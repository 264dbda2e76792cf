"""Message propagation along traversal frontiers (python/dgl/propagate.py in
the reference): the functional forms of :meth:`DGLGraph.prop_nodes` and
:meth:`DGLGraph.prop_edges`, and their combinations with dgl.traversal."""
from __future__ import absolute_import

from . import traversal as trv

__all__ = ["prop_nodes", "prop_nodes_bfs", "prop_nodes_topo", "prop_edges", "prop_edges_dfs"]


def prop_nodes(graph, nodes_generator, message_func="default", reduce_func="default",
               apply_node_func="default"):
    """Functional form of :meth:`DGLGraph.prop_nodes`."""
    graph.prop_nodes(nodes_generator, message_func, reduce_func, apply_node_func)


def prop_edges(graph, edges_generator, message_func="default", reduce_func="default",
               apply_node_func="default"):
    """Functional form of :meth:`DGLGraph.prop_edges`."""
    graph.prop_edges(edges_generator, message_func, reduce_func, apply_node_func)


def prop_nodes_bfs(graph, source, reverse=False, message_func="default", reduce_func="default",
                   apply_node_func="default"):
    """``pull`` on every frontier of :func:`dgl.bfs_nodes_generator` from
    ``source`` (a tensor on a ROCm device computes the frontiers there)."""
    prop_nodes(graph, trv.bfs_nodes_generator(graph, source, reverse), message_func,
               reduce_func, apply_node_func)


def prop_nodes_topo(graph, reverse=False, message_func="default", reduce_func="default",
                    apply_node_func="default", ctx=None):
    """``pull`` on every frontier of :func:`dgl.topological_nodes_generator`;
    ``ctx`` a ROCm device computes the frontiers there."""
    prop_nodes(graph, trv.topological_nodes_generator(graph, reverse, ctx=ctx), message_func,
               reduce_func, apply_node_func)


def prop_edges_dfs(graph, source, reverse=False, has_reverse_edge=False, has_nontree_edge=False,
                   message_func="default", reduce_func="default", apply_node_func="default"):
    """``send_and_recv`` on every frontier of
    :func:`dgl.dfs_labeled_edges_generator` (host route)."""
    edges = trv.dfs_labeled_edges_generator(graph, source, reverse, has_reverse_edge,
                                            has_nontree_edge, return_labels=False)
    prop_edges(graph, edges, message_func, reduce_func, apply_node_func)
