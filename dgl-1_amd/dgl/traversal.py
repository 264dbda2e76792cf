"""Graph traversals as frontier generators (python/dgl/traversal.py in the
reference): each function returns a tuple of 1-D int64 tensors, one per
frontier, for :meth:`DGLGraph.prop_nodes` / :meth:`DGLGraph.prop_edges`.

The frontiers come from the native index (``traversal._CAPI_*``,
csrc/graph_traversal.cc). BFS and the topological order also have a device
route (csrc/traversal.hip): on a mutable graph, a ``source`` given as a tensor
on a ROCm device, or ``ctx=`` a ROCm device for the topological order, computes
the frontiers there over the cached adjacency and leaves them there, equal to
the host answer element for element. The device route reads one size per
frontier on the host: a graph of many narrow levels is better served by the
host route, and neither route can run under stream capture on the device.
"""
from __future__ import absolute_import

import torch

__all__ = ["bfs_nodes_generator", "bfs_edges_generator", "topological_nodes_generator",
           "dfs_edges_generator", "dfs_labeled_edges_generator"]


def _frontiers(ids, sections, device=None):
    if device is not None:
        ids = ids.to(device)
    return tuple(torch.split(ids, sections)) if sections else ()


def _is_device_ids(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _bfs(graph, source, reverse, edges):
    gi = graph._graph
    if _is_device_ids(source):
        if not gi.is_readonly():
            run = gi.bfs_edges_device if edges else gi.bfs_nodes_device
            return _frontiers(*run(source, reverse))
        # frontiers live where the source lives
        run = gi.bfs_edges if edges else gi.bfs_nodes
        return _frontiers(*run(source, reverse), device=source.device)
    return _frontiers(*(gi.bfs_edges if edges else gi.bfs_nodes)(source, reverse))


def bfs_nodes_generator(graph, source, reverse=False):
    """Node frontiers of a breadth-first search.

    Parameters
    ----------
    graph : DGLGraph
    source : list, tensor of nodes
        The first frontier, as given. A tensor on a ROCm device selects the
        device route on a mutable graph; on a readonly graph the host result is
        moved to that device.
    reverse : bool
        Follow in-edges.

    Returns
    -------
    tuple of int64 tensors, one per frontier; ``()`` for an empty source.

    >>> g = dgl.DGLGraph([(0, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5)])
    >>> dgl.bfs_nodes_generator(g, 0)
    (tensor([0]), tensor([1]), tensor([2, 3]), tensor([4, 5]))
    """
    return _bfs(graph, source, reverse, False)


def bfs_edges_generator(graph, source, reverse=False):
    """Edge frontiers of a breadth-first search: frontier ``i`` holds the ids of
    the edges that discovered the nodes of :func:`bfs_nodes_generator`'s
    frontier ``i + 1``, in the same order. Arguments as there.

    >>> g = dgl.DGLGraph([(0, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5)])
    >>> dgl.bfs_edges_generator(g, 0)
    (tensor([0]), tensor([1, 2]), tensor([4, 5]))
    """
    return _bfs(graph, source, reverse, True)


def topological_nodes_generator(graph, reverse=False, ctx=None):
    """Node frontiers in topological order (Kahn's algorithm): the nodes
    without in-edges in ascending id, then the nodes all of whose in-edges come
    from earlier frontiers, and so on. A graph with a loop raises DGLError.

    Parameters
    ----------
    graph : DGLGraph
    reverse : bool
        Follow in-edges (start from the nodes without out-edges).
    ctx : device, optional
        A ROCm device computes the frontiers there (mutable graph; a readonly
        graph's host result is moved there). None is the host route.

    >>> g = dgl.DGLGraph([(0, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5)])
    >>> dgl.topological_nodes_generator(g)
    (tensor([0]), tensor([1]), tensor([2]), tensor([3, 4]), tensor([5]))
    """
    gi = graph._graph
    if ctx is not None and torch.device(ctx).type == "cuda":
        if not gi.is_readonly():
            return _frontiers(*gi.topological_nodes_device(ctx, reverse))
        return _frontiers(*gi.topological_nodes(reverse), device=ctx)
    return _frontiers(*gi.topological_nodes(reverse))


def dfs_edges_generator(graph, source, reverse=False):
    """Edge frontiers of a depth-first search: one search per source node, each
    with its own visited set; frontier ``i`` holds the ``i``-th tree edge of
    every search that is that long, in source order. The sources should lie in
    different components.

    Depth-first search is sequential and runs on the host: a ``source`` on a
    ROCm device is copied there and the result is a tuple of host tensors.

    >>> g = dgl.DGLGraph([(0, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5)])
    >>> dgl.dfs_edges_generator(g, 0)
    (tensor([0]), tensor([1]), tensor([3]), tensor([5]), tensor([4]))
    """
    return _frontiers(*graph._graph.dfs_edges(source, reverse))


def dfs_labeled_edges_generator(graph, source, reverse=False, has_reverse_edge=False,
                                has_nontree_edge=False, return_labels=True):
    """Edge frontiers of a depth-first search with a label per edge: FORWARD
    (0) for a tree edge on the way down, REVERSE (1) for the same edge on the
    way back up (listed with ``has_reverse_edge``), NONTREE (2) for an edge to
    a node already visited (listed with ``has_nontree_edge``). Sources and
    merging as in :func:`dfs_edges_generator`; host only, as there.

    Returns the tuple of edge frontiers and, with ``return_labels``, a second
    tuple with the labels in the same layout.

    >>> g = dgl.DGLGraph([(0, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5)])
    >>> dgl.dfs_labeled_edges_generator(g, 0, has_nontree_edge=True)
    ((tensor([0]), tensor([1]), tensor([3]), tensor([5]), tensor([4]), tensor([2])),
     (tensor([0]), tensor([0]), tensor([0]), tensor([0]), tensor([0]), tensor([2])))
    """
    ids, labels, sections = graph._graph.dfs_labeled_edges(
        source, reverse, has_reverse_edge, has_nontree_edge, return_labels)
    if return_labels:
        return _frontiers(ids, sections), _frontiers(labels, sections)
    return _frontiers(ids, sections)
