"""Geometry operators on point clouds (the ``dgl.geometry`` module of later
releases of the reference): farthest point sampling, the step that picks the
centroids of every set abstraction of PointNet++. Both functions run on the
segment sampler (csrc/segment_fps.hip) where the points are: on a ROCm device
one workgroup keeps a cloud on chip for all the picks.
"""
from __future__ import absolute_import

import torch

from . import kernel
from .base import DGLError

__all__ = ["farthest_point_sampler", "segmented_farthest_point_sampler"]


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
