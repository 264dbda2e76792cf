"""Geometry operators on point clouds (the ``dgl.geometry`` module of later
releases of the reference): farthest point sampling, the step that picks the
centroids of every set abstraction of PointNet++. Both functions run on the
segment sampler (csrc/segment_fps.hip) where the points are: on a ROCm device
one workgroup keeps a cloud on chip for all the picks. The ball query that
groups points round those centroids runs on the segment fixed-radius search
(csrc/segment_radius.hip): no distance matrix is written.
"""
from __future__ import absolute_import

import torch

from . import kernel
from .base import DGLError

__all__ = ["farthest_point_sampler", "segmented_farthest_point_sampler", "ball_query",
           "segmented_ball_query"]


def _starts(start_idx, sizes, device):
    """start_idx (None, an int or a (B,) tensor) as kernel.segment_fps's start."""
    if start_idx is None or isinstance(start_idx, torch.Tensor):
        return start_idx
    v = int(start_idx)
    if sizes and not 0 <= v < min(sizes):
        raise DGLError("start_idx = %d is no point of a cloud of %d" % (v, min(sizes)))
    return torch.full((len(sizes),), v, dtype=torch.int64, device=device)


def segmented_farthest_point_sampler(x, npoints, segs, start_idx=None):
    """``npoints`` points of each of the consecutive clouds of ``segs`` (a
    list of sizes summing to ``N``) points of ``x (N, D)`` float32, each the
    point of its cloud farthest from those picked before it: ``(B, npoints)``
    int64 **global** row ids in pick order, ``-1`` past the end of a cloud of
    fewer than ``npoints`` points. The first pick of every cloud is its point
    ``start_idx`` (None: point 0; an int; or a ``(B,)`` int64 tensor). Distances,
    order and ties are kernel.segment_fps's; not differentiable.

    >>> x = torch.tensor([[0.], [1.], [3.], [10.], [12.]])
    >>> dgl.geometry.segmented_farthest_point_sampler(x, 2, [3, 2])
    tensor([[0, 2], [3, 4]])
    """
    sizes = [int(n) for n in segs]
    idx, _ = kernel.segment_fps(x, sizes, npoints, _starts(start_idx, sizes, x.device))
    return idx


def farthest_point_sampler(pos, npoints, start_idx=None):
    """``npoints`` points of each of the ``B`` clouds ``pos (B, N, D)``
    float32 by farthest point sampling: ``(B, npoints)`` int64 indices **within
    each cloud**, in pick order. ``npoints > N`` is a DGLError.

    ``start_idx`` is the first pick of every cloud: None, an int, or a ``(B,)``
    int64 tensor. None means point 0: the reference draws a random start
    there, this project does not, so that a call has one answer; pass
    ``torch.randint(N, (B,))`` for the reference's behaviour."""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3:
        raise DGLError("farthest_point_sampler expects (B, N, D) points")
    B, N, D = pos.shape
    if int(npoints) > N:
        raise DGLError("cannot sample %d points of clouds of %d" % (int(npoints), N))
    idx = segmented_farthest_point_sampler(pos.reshape(B * N, D), npoints, [N] * B, start_idx)
    return idx - torch.arange(B, dtype=torch.int64, device=pos.device)[:, None] * N


def segmented_ball_query(x, segs, q, q_segs, radius, n_neighbor):
    """For every query ``q[i]`` of the consecutive query sets of ``q_segs``
    (sizes summing to ``M``) the first ``n_neighbor`` points, in row order, of
    the matching cloud of ``segs`` (sizes summing to ``N``) of ``x (N, D)``
    float32 closer than ``radius``: ``(M, n_neighbor)`` int64 **global** row
    ids of ``x``. A query with fewer members repeats its first one
    (PointNet++'s grouping); one with none holds ``-1``. Distances and
    membership are kernel.segment_radius's; not differentiable.

    >>> x = torch.tensor([[0.], [1.], [3.], [10.], [12.]])
    >>> q = torch.tensor([[2.], [11.]])
    >>> dgl.geometry.segmented_ball_query(x, [3, 2], q, [1, 1], 1.5, 3)
    tensor([[1, 2, 1], [3, 4, 3]])
    """
    nbr, _, _ = kernel.segment_radius(x, [int(n) for n in segs], radius, n_neighbor, q,
                                      [int(n) for n in q_segs], pad_first=True)
    return nbr


def ball_query(pos, centroids, radius, n_neighbor):
    """The grouping of a PointNet++ set abstraction: for each centroid of each
    of the ``B`` clouds ``pos (B, N, D)`` float32 the first ``n_neighbor``
    points of its cloud, in point order, closer than ``radius``. ``centroids``
    is ``(B, M)`` int64 indices into each cloud (what
    :func:`farthest_point_sampler` returns) or ``(B, M, D)`` points. Returns
    ``(B, M, n_neighbor)`` int64 indices **within each cloud**, padded with the
    first member (``-1`` where no point is inside, which an index centroid
    never sees: it is its own member)."""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3:
        raise DGLError("ball_query expects (B, N, D) points")
    B, N, D = pos.shape
    if not isinstance(centroids, torch.Tensor) or centroids.shape[0] != B:
        raise DGLError("ball_query expects the centroids of the %d clouds" % B)
    if centroids.dim() == 2 and centroids.dtype == torch.int64:
        q = torch.gather(pos, 1, centroids.to(pos.device)[:, :, None].expand(-1, -1, D))
    elif centroids.dim() == 3 and centroids.shape[2] == D:
        q = centroids
    else:
        raise DGLError("centroids must be (B, M) int64 indices or (B, M, D) points")
    M = q.shape[1]
    nbr = segmented_ball_query(pos.reshape(B * N, D), [N] * B, q.reshape(B * M, D), [M] * B,
                               radius, n_neighbor).view(B, M, -1)
    first = torch.arange(B, dtype=torch.int64, device=pos.device)[:, None, None] * N
    return torch.where(nbr < 0, nbr, nbr - first)
