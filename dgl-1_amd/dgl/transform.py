"""Graph transforms: the line graph and the reverse of a DGLGraph.

The surface of the reference's python/dgl/transform.py. The line graph has a
device route (csrc/line_graph.hip): with ``ctx=`` a ROCm device it is built
there from the graph's cached adjacency and stays there, so message passing
over it on that device never builds a native index. ``reverse`` is host
plumbing only.
"""
from __future__ import absolute_import

import torch

from .base import DGLError
from .batched_graph import BatchedDGLGraph
from .graph import DGLGraph

__all__ = ["line_graph", "reverse"]


def line_graph(g, backtracking=True, shared=False, ctx=None):
    """The line graph L(g) of a mutable graph ``g``.

    L(g) has one node per edge of ``g``: node ``i`` is edge id ``i``. Taking
    the edges ``i = (u, v)`` in id order, L(g) gets an edge from ``i`` to each
    out-edge of ``v``, in edge-id order; the k-th edge made this way is edge
    ``k`` of L(g). Parallel edges of ``g`` are distinct nodes, and a self loop
    ``(v, v)`` links to every out-edge of ``v``, itself included.

    Parameters
    ----------
    g : DGLGraph
        A mutable graph (a batched graph included). A read-only one raises
        DGLError.
    backtracking : bool
        When False, edge ``(u, v)`` is not linked to the edges ``(v, u)``.
    shared : bool
        When True the node frame of L(g) **is** the edge frame of ``g``: a
        write through either graph, or a new column on either, is seen by
        the other.
    ctx : device, optional
        A ROCm device builds L(g) there and leaves its structure there; the
        result equals the host route's, edge for edge. None or a CPU device
        is the host route (the native index).

    Returns
    -------
    DGLGraph
        A mutable graph, never a multigraph.

    >>> g = dgl.DGLGraph()
    >>> g.add_nodes(3)
    >>> g.add_edges([0, 1, 1], [1, 0, 2])
    >>> L = g.line_graph(backtracking=False)
    >>> L.edges()
    (tensor([0]), tensor([2]))
    """
    gi = g._graph
    if ctx is not None and torch.device(ctx).type == "cuda":
        lgi = gi.line_graph_device(ctx, backtracking)
    else:
        lgi = gi.line_graph(backtracking)
    return DGLGraph(lgi, g._edge_frame if shared else None)


def reverse(g, share_ndata=False, share_edata=False):
    """A new mutable graph on the nodes of ``g`` whose edge ``i`` is edge ``i``
    of ``g`` turned round: ``(dst[i], src[i])``. It is a multigraph when ``g``
    is one.

    Parameters
    ----------
    g : DGLGraph
        Not a BatchedDGLGraph: that raises DGLError.
    share_ndata, share_edata : bool
        When True the new graph's node (edge) frame **is** that of ``g``;
        otherwise it starts without features. The structures are independent:
        a later mutation of either graph is not followed by the other, which
        leaves a shared frame with the wrong number of rows for one of them.

    >>> g = dgl.DGLGraph()
    >>> g.add_nodes(3)
    >>> g.add_edges([0, 1, 2], [1, 2, 0])
    >>> rg = g.reverse()
    >>> rg.edges()
    (tensor([1, 2, 0]), tensor([0, 1, 2]))
    """
    if isinstance(g, BatchedDGLGraph):
        raise DGLError("reverse is not supported for a BatchedDGLGraph")
    rg = DGLGraph(multigraph=g.is_multigraph)
    rg.add_nodes(g.number_of_nodes())
    src, dst, _ = g._graph.edges("eid")
    rg.add_edges(dst, src)
    if share_ndata:
        rg._node_frame = g._node_frame
    if share_edata:
        rg._edge_frame = g._edge_frame
    return rg
