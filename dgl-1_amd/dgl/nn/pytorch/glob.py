"""Global pooling over the graphs of a batch (the ``glob`` module later
releases of the reference added to ``dgl.nn.pytorch``), and the layers that
make a graph from points (its ``factory`` module)."""
from __future__ import absolute_import

import torch
from torch import nn

from ... import kernel
from ...batched_graph import _topk_segments
from ...geometry import farthest_point_sampler
from ...transform import knn_graph, segmented_knn_graph

__all__ = ["SortPooling", "KNNGraph", "SegmentedKNNGraph", "FarthestPointSampler"]


class SortPooling(nn.Module):
    """The sort pooling of DGCNN (Zhang et al., "An End-to-End Deep Learning
    Architecture for Graph Classification", AAAI 2018): every node's channels
    are sorted ascending, then each graph keeps its ``k`` nodes with the
    largest last channel, in that order, zero-padded when it has fewer.

    ``forward(feat, graph)`` takes ``feat (N, F)`` float32 and returns
    ``(batch_size, k * F)`` (``(1, k * F)`` for a plain graph),
    differentiable in ``feat``. The selection and the row copy are one HIP
    segment top-k (``kernel.segment_topk`` with ``sortby=-1``). The sort of
    the ``F`` channels inside each node's row stays ``torch.sort(dim=-1)``: it
    orders values within a row, not rows within a graph, so it is no segment
    operation."""

    def __init__(self, k):
        super(SortPooling, self).__init__()
        self.k = k

    def forward(self, feat, graph):
        feat, _ = torch.sort(feat, dim=-1)
        segs = _topk_segments(graph, "nodes", feat.shape[0])
        values, _ = kernel.segment_topk(feat, segs, self.k, sortby=-1)
        return values.reshape(values.shape[0], -1)


class KNNGraph(nn.Module):
    """Points to their k-nearest-neighbour graph (``dgl.knn_graph``), the
    graph layer of DGCNN / EdgeConv models, which rebuild it in feature space
    at every layer: ``forward(x)`` with ``x (N, D)`` or ``(B, N, D)``."""

    def __init__(self, k):
        super(KNNGraph, self).__init__()
        self.k = k

    def forward(self, x, exclude_self=False):
        return knn_graph(x, self.k, exclude_self)


class SegmentedKNNGraph(nn.Module):
    """:class:`KNNGraph` over clouds of unequal sizes
    (``dgl.segmented_knn_graph``): ``forward(x, segs)`` with ``x (N, D)`` and
    the list of sizes ``segs``."""

    def __init__(self, k):
        super(SegmentedKNNGraph, self).__init__()
        self.k = k

    def forward(self, x, segs, exclude_self=False):
        return segmented_knn_graph(x, self.k, segs, exclude_self)


class FarthestPointSampler(nn.Module):
    """The centroids of a PointNet++ set abstraction
    (``dgl.geometry.farthest_point_sampler``): ``forward(pos)`` with ``pos (B,
    N, D)`` returns the ``(B, npoints)`` indices within each cloud, the first
    being point 0 (or ``start_idx``)."""

    def __init__(self, npoints):
        super(FarthestPointSampler, self).__init__()
        self.npoints = npoints

    def forward(self, pos, start_idx=None):
        return farthest_point_sampler(pos, self.npoints, start_idx)
