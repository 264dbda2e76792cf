"""Global pooling over the graphs of a batch (the ``glob`` module later
releases of the reference added to ``dgl.nn.pytorch``), and the layers that
make a graph from points (its ``factory`` module)."""
from __future__ import absolute_import

import torch
from torch import nn

from ... import kernel
from ...batched_graph import _topk_segments
from ...geometry import ball_query, farthest_point_sampler
from ...transform import knn_graph, radius_graph, segmented_knn_graph

__all__ = ["SortPooling", "KNNGraph", "SegmentedKNNGraph", "RadiusGraph", "FarthestPointSampler",
           "FixedRadiusNearNeighbors"]


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


class RadiusGraph(nn.Module):
    """Points to their cutoff graph (``dgl.radius_graph``), the graph layer of
    the molecular and mesh models built on a distance cutoff: ``forward(x)``
    with ``x (N, D)`` or ``(B, N, D)``."""

    def __init__(self, r, max_num_neighbors=32, self_loop=False):
        super(RadiusGraph, self).__init__()
        self.r = r
        self.max_num_neighbors = max_num_neighbors
        self.self_loop = self_loop

    def forward(self, x):
        return radius_graph(x, self.r, self.max_num_neighbors, self.self_loop)


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


class FixedRadiusNearNeighbors(nn.Module):
    """The grouping of a PointNet++ set abstraction
    (``dgl.geometry.ball_query``): ``forward(pos, centroids)`` with ``pos (B, N,
    D)`` and the ``(B, M)`` indices a :class:`FarthestPointSampler` returns (or
    ``(B, M, D)`` points) gives the ``(B, M, n_neighbor)`` indices within each
    cloud of the first ``n_neighbor`` points closer than ``radius``, padded
    with the first."""

    def __init__(self, radius, n_neighbor):
        super(FixedRadiusNearNeighbors, self).__init__()
        self.radius = radius
        self.n_neighbor = n_neighbor

    def forward(self, pos, centroids):
        return ball_query(pos, centroids, self.radius, self.n_neighbor)
