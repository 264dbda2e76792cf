"""Softmax over the edges of each node (the ``edge_softmax`` later releases of
the reference added to ``dgl.nn.pytorch``): one HIP kernel forward and one
backward (``kernel.edge_softmax``, csrc/edge_softmax.hip)."""
from __future__ import absolute_import

from ... import kernel

__all__ = ["edge_softmax"]


def edge_softmax(graph, logits, norm_by="dst"):
    """Normalise the edge scores ``logits`` over the in-edges of every node
    (``norm_by="dst"``) or over its out-edges (``"src"``).

    ``graph`` is a DGLGraph, a BatchedDGLGraph or a DGLSubGraph, mutable or
    readonly; ``logits`` is ``(E,)`` or ``(E, ...)`` float32 indexed by edge
    id, every trailing position (an attention head) normalised on its own.
    Returns a tensor of ``logits``' shape, differentiable in it:

    >>> e = kernel.gsddmm_dot(adj, q, k)            # scores per edge and head
    >>> g.edata["a"] = edge_softmax(g, e)
    >>> g.update_all(fn.src_mul_edge("v", "a", "m"), fn.sum("m", "o"))
    """
    return kernel.edge_softmax(graph.sparse_adjacency(logits.device), logits, norm_by)
