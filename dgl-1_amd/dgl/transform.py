"""Graph transforms: the line graph and the reverse of a DGLGraph, and the
k-nearest-neighbour graph of a point set.

The surface of the reference's python/dgl/transform.py. The line graph has a
device route (csrc/line_graph.hip): with ``ctx=`` a ROCm device it is built
there from the graph's cached adjacency and stays there, so message passing
over it on that device never builds a native index. ``reverse`` is host
plumbing only. ``knn_graph`` / ``segmented_knn_graph`` (later releases of the
reference) run on the segment kNN (csrc/segment_knn.hip) where the points are;
on a ROCm device the edge list stays there like the line graph's.
``radius_graph`` / ``segmented_radius_graph`` do the same on the segment
fixed-radius search (csrc/segment_radius.hip).
"""
from __future__ import absolute_import

import torch

from . import kernel
from .base import DGLError
from .batched_graph import BatchedDGLGraph
from .graph import DGLGraph
from .graph_index import _DeviceLineGraphIndex

__all__ = ["line_graph", "reverse", "knn_graph", "segmented_knn_graph", "radius_graph",
           "segmented_radius_graph"]


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


def segmented_knn_graph(x, k, segs, exclude_self=False):
    """The k-nearest-neighbour graph of the points ``x (N, D)`` float32 taken
    as consecutive clouds of ``segs`` (a list of sizes summing to ``N``)
    points: a node per point, and edge ``i * k + j`` runs **from** the j-th
    nearest point of node ``i``'s cloud **to** node ``i``, so every node's
    predecessors are its neighbours, nearest first, and ``update_all`` pulls
    from them. Distances, order and ties are kernel.segment_knn's; without
    ``exclude_self`` a point is its own first neighbour. Every cloud must hold
    ``k`` candidates (``k + 1`` points with ``exclude_self``), else DGLError.

    For ``x`` on a ROCm device the graph is built and left there (the f32
    MFMA kernel, no distance matrix): message passing over it on that device
    never builds a native index. The graph is mutable and never a multigraph;
    it is not differentiable in ``x``.

    >>> x = torch.tensor([[0.], [1.], [3.], [10.], [12.]])
    >>> dgl.segmented_knn_graph(x, 2, [3, 2]).edges()
    (tensor([0, 1, 1, 0, 2, 1, 3, 4, 4, 3]), tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 4]))
    """
    sizes = [int(n) for n in segs]
    need = int(k) + (1 if exclude_self else 0)
    if sizes and min(sizes) < need:
        raise DGLError("every segment needs at least %d points for k = %d%s, got one of %d"
                       % (need, int(k), " without self" if exclude_self else "", min(sizes)))
    nbr, _ = kernel.segment_knn(x, sizes, k, exclude_self)
    N = x.shape[0]
    src = nbr.reshape(-1)
    dst = torch.arange(N, dtype=torch.int64, device=x.device).repeat_interleave(nbr.shape[1])
    if x.is_cuda:
        return DGLGraph(_DeviceLineGraphIndex(N, src, dst))
    g = DGLGraph()
    g.add_nodes(N)
    g.add_edges(src, dst)
    return g


def knn_graph(x, k, exclude_self=False):
    """:func:`segmented_knn_graph` of one cloud ``x (N, D)``, or of ``B``
    clouds of ``N`` points ``x (B, N, D)`` (a graph on ``B * N`` nodes, node
    ``b * N + i`` being point ``i`` of cloud ``b``)."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise DGLError("knn_graph expects (N, D) or (B, N, D) points")
    if x.dim() == 2:
        return segmented_knn_graph(x, k, [x.shape[0]], exclude_self)
    B, N, D = x.shape
    return segmented_knn_graph(x.reshape(B * N, D), k, [N] * B, exclude_self)


def segmented_radius_graph(x, r, segs, max_num_neighbors=32, self_loop=False):
    """The cutoff graph of the points ``x (N, D)`` float32 taken as
    consecutive clouds of ``segs`` (a list of sizes summing to ``N``) points:
    a node per point and an edge **from** every point ``j`` of node ``i``'s
    cloud closer than ``r`` **to** node ``i``. Node ``i``'s edges are
    consecutive and ascending in ``j``; a node with more than
    ``max_num_neighbors`` points inside keeps the first that many in point
    order (not the nearest). ``self_loop`` keeps the edge ``(i, i)``.
    Distances and membership are kernel.segment_radius's.

    For ``x`` on a ROCm device the graph is built and left there (the ball
    query in HIP, then a boolean index over its slots): message passing over
    it on that device never builds a native index. The graph is mutable and
    never a multigraph; it is not differentiable in ``x``.

    >>> x = torch.tensor([[0.], [1.], [3.], [10.], [12.]])
    >>> dgl.segmented_radius_graph(x, 2.5, [3, 2]).edges()
    (tensor([1, 0, 2, 1, 4, 3]), tensor([0, 1, 1, 2, 3, 4]))
    """
    nbr, cnt, _ = kernel.segment_radius(x, [int(n) for n in segs], r, max_num_neighbors,
                                        exclude_self=not self_loop)
    N, k = nbr.shape
    valid = torch.arange(k, device=x.device)[None, :] < cnt[:, None]
    src = nbr[valid]
    dst = torch.arange(N, dtype=torch.int64, device=x.device)[:, None].expand(N, k)[valid]
    if x.is_cuda:
        return DGLGraph(_DeviceLineGraphIndex(N, src, dst))
    g = DGLGraph()
    g.add_nodes(N)
    g.add_edges(src, dst)
    return g


def radius_graph(x, r, max_num_neighbors=32, self_loop=False):
    """:func:`segmented_radius_graph` of one cloud ``x (N, D)``, or of ``B``
    clouds of ``N`` points ``x (B, N, D)`` (a graph on ``B * N`` nodes, node
    ``b * N + i`` being point ``i`` of cloud ``b``)."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise DGLError("radius_graph expects (N, D) or (B, N, D) points")
    if x.dim() == 2:
        return segmented_radius_graph(x, r, [x.shape[0]], max_num_neighbors, self_loop)
    B, N, D = x.shape
    return segmented_radius_graph(x.reshape(B * N, D), r, [N] * B, max_num_neighbors, self_loop)
