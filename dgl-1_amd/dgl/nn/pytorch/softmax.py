"""Softmax over the edges of each node (the ``edge_softmax`` later releases of
the reference added to ``dgl.nn.pytorch``): one HIP kernel forward and one
backward (``kernel.edge_softmax``, csrc/edge_softmax.hip), and the fused
attentions over them: scaled dot-product (``kernel.dot_attention``) and GATv2
(``kernel.gatv2_attention``)."""
from __future__ import absolute_import

from ... import kernel

__all__ = ["edge_softmax", "dot_attention", "gatv2_attention"]


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


def dot_attention(graph, q, k, v, scale=None, clamp=None):
    """Scaled dot-product attention over the edges of ``graph``: every node
    attends over its in-edges, ``out[n, h] = sum_j softmax_j(<q[n, h], k[u_j,
    h]> * scale) v[u_j, h]`` (``scale`` None: ``D ** -0.5``; ``clamp=(lo, hi)``
    bounds the scaled scores first, the transformer example's
    ``clamp(-10, 10)``). ``q``, ``k``, ``v`` are ``(N, H, D)`` float32 node
    tensors; returns ``(N, H, D)``, differentiable in all three, a node
    without in-edges gets zeros. One fused HIP kernel forward and two backward
    (``kernel.dot_attention``, csrc/dot_attention.hip): no per-edge tensor is
    made.

    >>> out = dot_attention(g, q, k, v)             # instead of gsddmm_dot,
    ...                                             # edge_softmax, update_all
    """
    return kernel.dot_attention(graph.sparse_adjacency(q.device), q, k, v, scale, clamp)


def gatv2_attention(graph, fs, fd, attn, negative_slope=0.2):
    """GATv2 attention over the edges of ``graph``: every node attends over
    its in-edges, ``out[n, h] = sum_j softmax_j(<attn[h], leaky_relu(fs[u_j, h]
    + fd[n, h])>) fs[u_j, h]``. ``fs`` and ``fd`` are ``(N, H, D)`` float32
    node tensors (the source and destination projections), ``attn`` is ``(H,
    D)`` or ``(1, H, D)``; returns ``(N, H, D)``, differentiable in all three,
    a node without in-edges gets zeros. One fused HIP kernel forward with one
    gathered row per edge, two walks backward (``kernel.gatv2_attention``,
    csrc/gatv2_attention.hip): no per-edge tensor is made.

    >>> out = gatv2_attention(g, fc_src(x).view(-1, H, D), fc_dst(x).view(-1, H, D), attn)
    """
    return kernel.gatv2_attention(graph.sparse_adjacency(fd.device), fs, fd, attn, negative_slope)
