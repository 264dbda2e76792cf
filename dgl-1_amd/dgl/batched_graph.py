"""Batched graphs and per-graph readout.

The surface of the reference's python/dgl/batched_graph.py: ``batch`` merges
graphs into one ``BatchedDGLGraph`` (a DGLGraph on the disjoint union of their
indices, so message passing needs nothing new), ``unbatch`` splits it back, and
``sum_nodes`` / ``mean_nodes`` / ``max_nodes`` and their ``_edges`` twins
reduce a feature over each member graph.

Where the reference delegates readout to ``scatter_add_`` and a Python loop of
``torch.max`` per graph (batched_graph.py:362-399,542-588,730-766), every
readout here is one call of ``kernel.segment_reduce``: a batch's nodes (and
edges) of one graph are consecutive rows, so the graphs are the segments.
``softmax_nodes`` / ``softmax_edges`` normalise a feature over each member
graph the same way, on the edge-softmax kernel (``kernel.segment_softmax``).
"""
from __future__ import absolute_import

from collections.abc import Iterable

import torch

from . import graph_index as gi
from . import kernel
from .base import ALL, DGLError, is_all
from .frame import Frame
from .graph import DGLGraph

__all__ = ["BatchedDGLGraph", "batch", "unbatch", "split", "sum_nodes", "sum_edges",
           "mean_nodes", "mean_edges", "max_nodes", "max_edges", "softmax_nodes", "softmax_edges"]


def _items_and_fields(g, mode):
    if mode == "node":
        return g.number_of_nodes(), set(g.node_attr_schemes().keys())
    return g.number_of_edges(), set(g.edge_attr_schemes().keys())


def _select_attrs(graphs, attrs, mode):
    """The field names to batch: ``None`` none, ``ALL`` the fields shared by
    every graph that has items (they must agree), a name, or an iterable."""
    if attrs is None:
        return []
    if is_all(attrs):
        ref, ref_i = None, -1
        for i, g in enumerate(graphs):
            num, fields = _items_and_fields(g, mode)
            if num > 0 and fields:
                ref, ref_i = fields, i
                break
        if ref is None:
            return []
        for i, g in enumerate(graphs):
            num, fields = _items_and_fields(g, mode)
            if num > 0 and fields != ref:
                raise ValueError("Expect graph %d and %d to have the same %s attributes when "
                                 "%s_attrs=ALL, got %s and %s." % (ref_i, i, mode, mode, ref, fields))
        return sorted(ref)
    if isinstance(attrs, str):
        return [attrs]
    if isinstance(attrs, Iterable):
        return list(attrs)
    raise ValueError("Expected %s attrs to be of type None, str or Iterable, got type %s"
                     % (mode, type(attrs)))


def _cat_frame(graphs, keys, mode, num_rows):
    frame = Frame(num_rows)
    for key in keys:
        cols = []
        for g in graphs:
            num, _ = _items_and_fields(g, mode)
            if num > 0:
                cols.append((g._node_frame if mode == "node" else g._edge_frame)[key])
        if cols:
            frame[key] = torch.cat(cols, 0)
    return frame


class BatchedDGLGraph(DGLGraph):
    """A list of graphs merged into one read-only graph: graph ``k``'s nodes
    (edges) take the ids after those of graphs ``0..k-1``, in their own order.

    Parameters
    ----------
    graph_list : iterable of DGLGraph (batched graphs are flattened)
    node_attrs, edge_attrs : ``ALL``, None, str or iterable
        The feature fields to concatenate. Under ``ALL`` the graphs that have
        nodes (edges) must carry the same fields. The batch owns its columns:
        writing to them leaves the member graphs unchanged.
    """

    def __init__(self, graph_list, node_attrs=ALL, edge_attrs=ALL):
        graphs = list(graph_list)
        node_keys = _select_attrs(graphs, node_attrs, "node")
        edge_keys = _select_attrs(graphs, edge_attrs, "edge")
        index = gi.disjoint_union([g._graph for g in graphs])
        super(BatchedDGLGraph, self).__init__(
            graph_data=index,
            node_frame=_cat_frame(graphs, node_keys, "node", index.number_of_nodes()),
            edge_frame=_cat_frame(graphs, edge_keys, "edge", index.number_of_edges()))
        self._batch_size = 0
        self._batch_num_nodes = []
        self._batch_num_edges = []
        for g in graphs:
            if isinstance(g, BatchedDGLGraph):
                self._batch_size += g._batch_size
                self._batch_num_nodes += g._batch_num_nodes
                self._batch_num_edges += g._batch_num_edges
            else:
                self._batch_size += 1
                self._batch_num_nodes.append(g.number_of_nodes())
                self._batch_num_edges.append(g.number_of_edges())
        self._segments = {}

    @property
    def batch_size(self):
        """Number of graphs in the batch."""
        return self._batch_size

    @property
    def batch_num_nodes(self):
        """Number of nodes of each graph of the batch (list)."""
        return self._batch_num_nodes

    @property
    def batch_num_edges(self):
        """Number of edges of each graph of the batch (list)."""
        return self._batch_num_edges

    def _readout_segments(self, typestr):
        # the graphs as row ranges, with their per-device copies: every
        # readout of this batch shares one upload
        seg = self._segments.get(typestr)
        if seg is None:
            sizes = self._batch_num_nodes if typestr == "nodes" else self._batch_num_edges
            seg = self._segments[typestr] = kernel.SegmentOffsets(sizes=sizes)
        return seg

    def add_nodes(self, num, data=None):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def add_edge(self, u, v, data=None):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def add_edges(self, u, v, data=None):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def __getitem__(self, idx):
        raise NotImplementedError

    def __setitem__(self, idx, val):
        raise NotImplementedError


def split(graph_batch, num_or_size_splits):  # pylint: disable=unused-argument
    """Split the batch (not implemented, as in the reference)."""
    raise NotImplementedError


def batch(graph_list, node_attrs=ALL, edge_attrs=ALL):
    """Merge ``graph_list`` into one :class:`BatchedDGLGraph` that is
    independent of its members."""
    return BatchedDGLGraph(graph_list, node_attrs, edge_attrs)


def unbatch(graph):
    """The member graphs of a batch: its index partitioned by the node counts,
    and every node / edge column split by the node / edge counts."""
    if not isinstance(graph, BatchedDGLGraph):
        raise DGLError("unbatch expects a BatchedDGLGraph, got %s" % type(graph))
    nn, ne = graph.batch_num_nodes, graph.batch_num_edges
    parts = gi.disjoint_partition(graph._graph, nn)
    node_frames = [Frame(n) for n in nn]
    edge_frames = [Frame(m) for m in ne]
    for frames, sizes, src in ((node_frames, nn, graph._node_frame),
                               (edge_frames, ne, graph._edge_frame)):
        for key, col in src.items():
            for frame, piece in zip(frames, torch.split(col, sizes, 0)):
                frame[key] = piece
    return [DGLGraph(graph_data=p, node_frame=nf, edge_frame=ef)
            for p, nf, ef in zip(parts, node_frames, edge_frames)]


def _readout(graph, typestr, feat, weight, reduce):
    data = graph.ndata if typestr == "nodes" else graph.edata
    x = data[feat]
    w = None if weight is None else data[weight]
    if isinstance(graph, BatchedDGLGraph):
        return kernel.segment_reduce(x, graph._readout_segments(typestr), reduce, w)
    # a plain graph is one segment; the result drops the batch dimension
    return kernel.segment_reduce(x, [x.shape[0]], reduce, w)[0]


def sum_nodes(graph, feat, weight=None):
    """Per graph, the sum of node field ``feat`` (each row first multiplied by
    the scalar node field ``weight`` if given): ``(batch_size, *fshape)`` for a
    batch, ``fshape`` for a plain graph."""
    return _readout(graph, "nodes", feat, weight, "sum")


def sum_edges(graph, feat, weight=None):
    """:func:`sum_nodes` over edge fields."""
    return _readout(graph, "edges", feat, weight, "sum")


def mean_nodes(graph, feat, weight=None):
    """Per graph, the mean of node field ``feat``; with ``weight`` the weighted
    sum over the sum of the weights. A graph without nodes gives zeros (NaN
    with a weight, as 0 / 0)."""
    return _readout(graph, "nodes", feat, weight, "mean")


def mean_edges(graph, feat, weight=None):
    """:func:`mean_nodes` over edge fields."""
    return _readout(graph, "edges", feat, weight, "mean")


def max_nodes(graph, feat):
    """Per graph, the elementwise maximum of node field ``feat`` (zeros for a
    graph without nodes)."""
    return _readout(graph, "nodes", feat, None, "max")


def max_edges(graph, feat):
    """:func:`max_nodes` over edge fields."""
    return _readout(graph, "edges", feat, None, "max")


def _softmax_readout(graph, typestr, feat):
    x = (graph.ndata if typestr == "nodes" else graph.edata)[feat]
    if isinstance(graph, BatchedDGLGraph):
        return kernel.segment_softmax(x, graph._readout_segments(typestr))
    # a plain graph is one segment
    return kernel.segment_softmax(x, kernel.SegmentOffsets(sizes=[x.shape[0]]))


def softmax_nodes(graph, feat):
    """Node field ``feat`` normalised by a softmax over the nodes of each
    graph of the batch (of the whole graph for a plain one), every feature
    position on its own: a tensor of the field's shape, differentiable in it.
    A graph without nodes contributes nothing."""
    return _softmax_readout(graph, "nodes", feat)


def softmax_edges(graph, feat):
    """:func:`softmax_nodes` over edge fields."""
    return _softmax_readout(graph, "edges", feat)
