"""DGLSubGraph: a graph induced from a parent graph's nodes or edges.

The surface of the reference's python/dgl/subgraph.py. A subgraph is a
DGLGraph of its own, read-only in structure, that remembers the parent ids of
its nodes and edges. Features are not shared: ``copy_from_parent`` gathers the
parent's rows (differentiably), ``copy_to_parent`` writes the subgraph's rows
back. A subgraph made from node ids on a ROCm device (DGLGraph.subgraph) keeps
its ids and its structure there: the gathers and whole-graph message passing
need no copy through the host.
"""
from __future__ import absolute_import

from . import graph_index as gi
from . import utils
from .base import DGLError
from .frame import Frame
from .graph import DGLGraph

__all__ = ["DGLSubGraph"]


class DGLSubGraph(DGLGraph):
    """The subgraph class.

    Parameters
    ----------
    parent : DGLGraph
    parent_nid, parent_eid : int64 tensors
        The parent id of every node / edge of this subgraph.
    graph_idx : SubgraphIndex
    shared : bool
        Sharing features with the parent is not supported.
    """

    def __init__(self, parent, parent_nid, parent_eid, graph_idx, shared=False):
        super(DGLSubGraph, self).__init__(graph_data=graph_idx, readonly=graph_idx.is_readonly())
        if shared:
            raise DGLError("Shared mode is not yet supported.")
        self._parent = parent
        self._parent_nid = parent_nid
        self._parent_eid = parent_eid

    def add_nodes(self, num, data=None):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def add_edge(self, u, v, data=None):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def add_edges(self, u, v, data=None):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    @property
    def parent_nid(self):
        """Parent node id of every node: a map from this subgraph's node ids
        to the parent's."""
        return self._parent_nid

    @property
    def parent_eid(self):
        """Parent edge id of every edge."""
        return self._parent_eid

    def copy_from_parent(self):
        """Replace this subgraph's features by the parent's rows at
        ``parent_nid`` / ``parent_eid``. The rows are gathered, so gradients
        flow back to the parent's columns. A frame the parent has no rows in
        is left as it is."""
        pairs = (("_node_frame", self._parent_nid), ("_edge_frame", self._parent_eid))
        for name, ids in pairs:
            src = getattr(self._parent, name)
            if src.num_rows == 0:
                continue
            frame = Frame(ids.numel())
            for key, col in src.select_rows(ids).items():
                frame[key] = col
            setattr(self, name, frame)

    def copy_to_parent(self, inplace=False):
        """Write this subgraph's features to the parent's rows; ``inplace``
        writes into the parent's columns' storage (no gradient)."""
        self._parent._node_frame.update_rows(self._parent_nid, dict(self._node_frame.items()),
                                             inplace=inplace)
        if self._parent._edge_frame.num_rows != 0:
            self._parent._edge_frame.update_rows(self._parent_eid,
                                                 dict(self._edge_frame.items()), inplace=inplace)

    def map_to_subgraph_nid(self, parent_vids):
        """Ids in this subgraph of the parent node ids ``parent_vids``."""
        return gi.map_to_subgraph_nid(self._graph, utils.toindex(parent_vids))
