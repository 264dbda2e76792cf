"""DGLGraph: the user-facing graph + message-passing API.

Same public surface and semantics as python/dgl/graph.py (DGLGraph, 2939
lines in the reference) for graph construction, feature storage and the
message-passing entry points the hot path starts from:
update_all (graph.py:2398-2441), send_and_recv (2089-2196), pull (2198-2299),
push (2301-2396), send / recv (1926-2087), apply_nodes / apply_edges
(1800-1924), adjacency_matrix (2721-2742).

Each message-passing call is lowered by runtime.scheduler onto the g-SpMM
kernels of libdgl_hip.so; see that module for the lowering rules.
"""
from __future__ import absolute_import

import torch

from . import kernel, utils
from .base import ALL, DGLError, is_all
from .frame import Frame
from .graph_index import create_graph_index
from .runtime import scheduler
from .udf import EdgeBatch, LazyDict, NodeBatch
from .view import EdgeView, NodeView

__all__ = ["DGLGraph"]


class DGLGraph(object):
    """Directed graph with node/edge features and message passing.

    Parameters
    ----------
    graph_data : None, networkx graph, scipy sparse matrix, edge list, (u, v)
    node_frame, edge_frame : Frame, optional
    multigraph : bool
    readonly : bool
    """

    def __init__(self, graph_data=None, node_frame=None, edge_frame=None,
                 multigraph=False, readonly=False):
        self._graph = create_graph_index(graph_data, multigraph, readonly)
        n, m = self._graph.number_of_nodes(), self._graph.number_of_edges()
        self._node_frame = node_frame if node_frame is not None else Frame(n)
        self._edge_frame = edge_frame if edge_frame is not None else Frame(m)
        self._msg_frame = Frame(m)
        self._msg_pending = torch.zeros(m, dtype=torch.bool)
        self._message_func = None
        self._reduce_func = None
        self._apply_node_func = None
        self._apply_edge_func = None

    # -- structure -------------------------------------------------------------
    def add_nodes(self, num, data=None):
        """Add ``num`` isolated nodes (optionally with features)."""
        self._graph.add_nodes(num)
        if data is None:
            self._node_frame.add_rows(num)
        else:
            lo = self._node_frame.num_rows
            self._node_frame.add_rows(num)
            self._node_frame.update_rows(torch.arange(lo, lo + num), data)

    def add_edge(self, u, v, data=None):
        """Add one edge u -> v."""
        self.add_edges([u], [v], data)

    def add_edges(self, u, v, data=None):
        """Add edges u[i] -> v[i] (a scalar end broadcasts)."""
        before = self._graph.number_of_edges()
        self._graph.add_edges(u, v)
        num = self._graph.number_of_edges() - before
        self._edge_frame.add_rows(num)
        self._msg_frame.add_rows(num)
        self._msg_pending = torch.cat([self._msg_pending, torch.zeros(num, dtype=torch.bool)])
        if data is not None:
            self._edge_frame.update_rows(torch.arange(before, before + num), data)

    def clear(self):
        """Remove all nodes, edges and features."""
        self._graph.clear()
        self._node_frame = Frame(0)
        self._edge_frame = Frame(0)
        self._msg_frame = Frame(0)
        self._msg_pending = torch.zeros(0, dtype=torch.bool)

    def clear_cache(self):
        """Drop cached adjacencies (rebuilt on next use)."""
        self._graph._invalidate()

    def number_of_nodes(self):
        return self._graph.number_of_nodes()

    def __len__(self):
        return self.number_of_nodes()

    def number_of_edges(self):
        return self._graph.number_of_edges()

    @property
    def is_multigraph(self):
        return self._graph.is_multigraph()

    @property
    def is_readonly(self):
        return self._graph.is_readonly()

    def has_node(self, vid):
        return 0 <= int(vid) < self.number_of_nodes()

    def __contains__(self, vid):
        return self.has_node(vid)

    def has_nodes(self, vids):
        return self._graph.has_nodes(vids)

    def has_edge_between(self, u, v):
        return bool(self._graph.has_edges_between([u], [v])[0])

    def has_edges_between(self, u, v):
        return self._graph.has_edges_between(u, v)

    def predecessors(self, v):
        return self._graph.predecessors(v)

    def successors(self, v):
        return self._graph.successors(v)

    def edge_id(self, u, v, force_multi=False):
        _, _, eid = self._graph.edge_ids([u], [v])
        return eid if (force_multi or self.is_multigraph) else int(eid[0])

    def edge_ids(self, u, v, force_multi=False):
        src, dst, eid = self._graph.edge_ids(u, v)
        return (src, dst, eid) if (force_multi or self.is_multigraph) else eid

    def find_edges(self, eid):
        src, dst, _ = self._graph.find_edges(eid)
        return src, dst

    def in_edges(self, v, form="uv"):
        return self._form(self._graph.in_edges(v), form)

    def out_edges(self, v, form="uv"):
        return self._form(self._graph.out_edges(v), form)

    def all_edges(self, form="uv", order=None):
        return self._form(self._graph.edges(order), form)

    @staticmethod
    def _form(edges, form):
        src, dst, eid = edges
        if form == "all":
            return src, dst, eid
        if form == "uv":
            return src, dst
        if form == "eid":
            return eid
        raise DGLError("Invalid form: %s" % form)

    def in_degree(self, v):
        return int(self._graph.in_degrees([v])[0])

    def in_degrees(self, v=ALL):
        return self._graph.in_degrees(None if is_all(v) else v)

    def out_degree(self, v):
        return int(self._graph.out_degrees([v])[0])

    def out_degrees(self, v=ALL):
        return self._graph.out_degrees(None if is_all(v) else v)

    def to_networkx(self, node_attrs=None, edge_attrs=None):
        """networkx (Multi)DiGraph of the structure (graph.py:1094-1135): every
        edge carries its id as the 'id' attribute; node_attrs / edge_attrs
        name feature columns copied as per-node / per-edge tensor rows."""
        import networkx as nx
        nxg = nx.MultiDiGraph() if self.is_multigraph else nx.DiGraph()
        n = self.number_of_nodes()
        nxg.add_nodes_from(range(n))
        src, dst = self._graph.src().tolist(), self._graph.dst().tolist()
        for e, (u, v) in enumerate(zip(src, dst)):
            nxg.add_edge(u, v, id=e)
        for attr in node_attrs or ():
            col = self._node_frame[attr]
            for i in range(n):
                nxg.nodes[i][attr] = col[i]
        if edge_attrs:
            cols = {attr: self._edge_frame[attr] for attr in edge_attrs}
            for _, _, d in nxg.edges(data=True):
                for attr, col in cols.items():
                    d[attr] = col[d["id"]]
        return nxg

    def from_networkx(self, nx_graph, node_attrs=None, edge_attrs=None):
        """Replace the structure by a networkx graph (graph.py:1136-1232)."""
        self.clear()
        self._graph = create_graph_index(nx_graph, self._graph.is_multigraph(), False)
        self._reset_frames()
        import networkx as nx
        nxg = nx.convert_node_labels_to_integers(nx_graph, ordering="sorted")
        if not nxg.is_directed():
            nxg = nxg.to_directed()
        if node_attrs:
            for attr in node_attrs:
                vals = [nxg.nodes[i][attr] for i in range(nxg.number_of_nodes())]
                self._node_frame[attr] = _batch(vals)
        if edge_attrs:
            elist = list(nxg.edges(data=True))
            if elist and "id" in elist[0][2]:
                elist.sort(key=lambda e: e[2]["id"])
            for attr in edge_attrs:
                self._edge_frame[attr] = _batch([e[2][attr] for e in elist])

    def from_scipy_sparse_matrix(self, spmat):
        """Replace the structure by a scipy sparse matrix: u = row, v = col."""
        self.clear()
        self._graph = create_graph_index(spmat, self._graph.is_multigraph(), False)
        self._reset_frames()

    def _reset_frames(self):
        n, m = self.number_of_nodes(), self.number_of_edges()
        self._node_frame = Frame(n)
        self._edge_frame = Frame(m)
        self._msg_frame = Frame(m)
        self._msg_pending = torch.zeros(m, dtype=torch.bool)

    # -- features --------------------------------------------------------------
    def node_attr_schemes(self):
        return self._node_frame.schemes()

    def edge_attr_schemes(self):
        return self._edge_frame.schemes()

    def set_n_initializer(self, initializer, field=None):
        self._node_frame.set_initializer(initializer, field)

    def set_e_initializer(self, initializer, field=None):
        self._edge_frame.set_initializer(initializer, field)

    @property
    def nodes(self):
        return NodeView(self)

    @property
    def ndata(self):
        return self.nodes[:].data

    @property
    def edges(self):
        return EdgeView(self)

    @property
    def edata(self):
        return self.edges[:].data

    def set_n_repr(self, data, u=ALL, inplace=False):
        if not isinstance(data, dict):
            raise DGLError("Expect dictionary type for feature data. Got %s" % type(data))
        if is_all(u):
            for k, val in data.items():
                self._node_frame[k] = val
        else:
            u = utils.toindex(u)
            for k, val in data.items():
                if val.shape[0] != len(u):
                    raise DGLError("Expect number of features to match number of nodes "
                                   "(len(u)). Got %d and %d instead." % (val.shape[0], len(u)))
            self._node_frame.update_rows(u, data, inplace)

    def get_n_repr(self, u=ALL):
        if len(self._node_frame) == 0:
            return {}
        if is_all(u):
            return dict(self._node_frame.items())
        return self._node_frame.select_rows(utils.toindex(u))

    def pop_n_repr(self, key):
        return self._node_frame.pop(key)

    def set_e_repr(self, data, edges=ALL, inplace=False):
        if not isinstance(data, dict):
            raise DGLError("Expect dictionary type for feature data. Got %s" % type(data))
        if is_all(edges):
            for k, val in data.items():
                self._edge_frame[k] = val
            return
        eid = self._resolve_edges(edges)
        self._edge_frame.update_rows(eid, data, inplace)

    def get_e_repr(self, edges=ALL):
        if len(self._edge_frame) == 0:
            return {}
        if is_all(edges):
            return dict(self._edge_frame.items())
        return self._edge_frame.select_rows(self._resolve_edges(edges))

    def pop_e_repr(self, key):
        return self._edge_frame.pop(key)

    def _resolve_edges(self, edges):
        if isinstance(edges, tuple):
            _, _, eid = self._graph.edge_ids(edges[0], edges[1])
            return eid
        return utils.toindex(edges)

    def _edge_triplet(self, edges):
        if is_all(edges):
            return self._graph.edges()
        if isinstance(edges, tuple):
            return self._graph.edge_ids(edges[0], edges[1])
        return self._graph.find_edges(utils.toindex(edges))

    # -- registered functions --------------------------------------------------
    def register_message_func(self, func):
        self._message_func = func

    def register_reduce_func(self, func):
        self._reduce_func = func

    def register_apply_node_func(self, func):
        self._apply_node_func = func

    def register_apply_edge_func(self, func):
        self._apply_edge_func = func

    def _defaults(self, message_func=None, reduce_func=None, apply_node_func=None):
        mf = self._message_func if message_func == "default" else message_func
        rf = self._reduce_func if reduce_func == "default" else reduce_func
        af = self._apply_node_func if apply_node_func == "default" else apply_node_func
        return mf, rf, af

    # -- computation -----------------------------------------------------------
    def apply_nodes(self, func="default", v=ALL, inplace=False):
        """Update node features with a node UDF."""
        if func == "default":
            func = self._apply_node_func
        if func is None:
            return
        v = None if is_all(v) else utils.toindex(v)
        scheduler.schedule_apply_nodes(self, v, func, inplace)

    def apply_edges(self, func="default", edges=ALL, inplace=False):
        """Update edge features with an edge UDF."""
        if func == "default":
            func = self._apply_edge_func
        assert func is not None
        if is_all(edges):
            scheduler.schedule_apply_edges(self, None, None, None, func, inplace)
        else:
            u, v, eid = self._edge_triplet(edges)
            scheduler.schedule_apply_edges(self, u, v, eid, func, inplace)

    def send(self, edges=ALL, message_func="default"):
        """Compute messages on ``edges`` and store them for a later recv."""
        if message_func == "default":
            message_func = self._message_func
        u, v, eid = self._edge_triplet(edges)
        if len(eid) == 0:
            return
        scheduler.schedule_send(self, u, v, eid, message_func)

    def recv(self, v=ALL, reduce_func="default", apply_node_func="default", inplace=False):
        """Reduce pending messages at ``v``."""
        _, reduce_func, apply_node_func = self._defaults(None, reduce_func, apply_node_func)
        assert reduce_func is not None
        v = torch.arange(self.number_of_nodes()) if is_all(v) else utils.toindex(v)
        if len(v) == 0:
            return
        scheduler.schedule_recv(self, v, reduce_func, apply_node_func, inplace)

    def send_and_recv(self, edges, message_func="default", reduce_func="default",
                      apply_node_func="default", inplace=False):
        """Send along ``edges`` and reduce at their destinations."""
        mf, rf, af = self._defaults(message_func, reduce_func, apply_node_func)
        assert mf is not None
        assert rf is not None
        u, v, eid = self._edge_triplet(edges)
        if len(u) == 0:
            return
        scheduler.schedule_snr(self, u, v, eid, mf, rf, af, inplace)

    def pull(self, v, message_func="default", reduce_func="default",
             apply_node_func="default", inplace=False):
        """Pull messages from the predecessors of ``v``."""
        mf, rf, af = self._defaults(message_func, reduce_func, apply_node_func)
        assert mf is not None
        assert rf is not None
        v = utils.toindex(v)
        if len(v) == 0:
            return
        scheduler.schedule_pull(self, v, mf, rf, af, inplace)

    def push(self, u, message_func="default", reduce_func="default",
             apply_node_func="default", inplace=False):
        """Push messages from ``u`` to its successors."""
        mf, rf, af = self._defaults(message_func, reduce_func, apply_node_func)
        assert mf is not None
        assert rf is not None
        u = utils.toindex(u)
        if len(u) == 0:
            return
        scheduler.schedule_push(self, u, mf, rf, af, inplace)

    def update_all(self, message_func="default", reduce_func="default",
                   apply_node_func="default"):
        """Send along every edge and reduce at every node."""
        mf, rf, af = self._defaults(message_func, reduce_func, apply_node_func)
        assert mf is not None
        assert rf is not None
        scheduler.schedule_update_all(self, mf, rf, af)

    def prop_nodes(self, nodes_generator, message_func="default", reduce_func="default",
                   apply_node_func="default"):
        """:meth:`pull` on each node frontier of ``nodes_generator`` in turn
        (graph.py:2443-2517): an iterable of lists or tensors of node ids, such
        as :func:`dgl.bfs_nodes_generator` or
        :func:`dgl.topological_nodes_generator` return.

        >>> g = dgl.DGLGraph(); g.add_nodes(4)
        >>> g.ndata['x'] = torch.tensor([[1.], [2.], [3.], [4.]])
        >>> g.add_edges([0, 1, 1, 2], [1, 2, 3, 3])
        >>> g.register_message_func(lambda edges: {'m': edges.src['x']})
        >>> g.register_reduce_func(lambda nodes: {'x': nodes.mailbox['m'].sum(1)})
        >>> g.prop_nodes([[1, 2], [3]])
        >>> g.ndata['x'].flatten()
        tensor([1., 1., 2., 3.])
        """
        for frontier in nodes_generator:
            self.pull(frontier, message_func, reduce_func, apply_node_func)

    def prop_edges(self, edges_generator, message_func="default", reduce_func="default",
                   apply_node_func="default"):
        """:meth:`send_and_recv` on each edge frontier of ``edges_generator``
        in turn (graph.py:2519-2593): an iterable of edge specifications (edge
        ids, or ``(u, v)`` pairs), such as :func:`dgl.bfs_edges_generator` or
        :func:`dgl.dfs_labeled_edges_generator` return.

        With the graph of :meth:`prop_nodes`:

        >>> g.prop_edges([([0, 1], [1, 3]), ([1, 2], [2, 3])])
        >>> g.ndata['x'].flatten()
        tensor([1., 1., 1., 3.])
        """
        for frontier in edges_generator:
            self.send_and_recv(frontier, message_func, reduce_func, apply_node_func)

    # -- sparse views ----------------------------------------------------------
    def _cached_view(self, key, build):
        # per (view, arguments, ctx); cleared by mutation and clear_cache(),
        # as the reference's adjacency / incidence caches (graph_index.py:537-662)
        cache = self._graph._cache
        if key not in cache:
            cache[key] = build()
        return cache[key]

    def adjacency_matrix(self, transpose=False, ctx=torch.device("cpu")):
        """Adjacency as a torch sparse COO tensor (rows = dst unless transpose)
        in the reference's nnz order (graph.py:2721-2742); cached per
        (transpose, ctx) until the graph changes."""
        ctx = torch.device(ctx)
        return self._cached_view(("adjmat", bool(transpose), str(ctx)),
                                 lambda: self._adjacency_matrix(transpose, ctx))

    def _adjacency_matrix(self, transpose, ctx):
        # the index's COO (graph_index.py:565-583 -> _CAPI_DGLGraphGetAdj):
        # edge-id order for a mutable graph, in-CSR order for an immutable one
        idx = self._graph.get_adj(transpose, "coo")[0]
        n, m = self.number_of_nodes(), self.number_of_edges()
        return torch.sparse_coo_tensor(idx.reshape(2, m), torch.ones(m), (n, n)).to(ctx)

    def incidence_matrix(self, typestr, ctx=torch.device("cpu")):
        """'in' / 'out' / 'both' incidence matrix (graph_index.py:587-662);
        cached per (type, ctx) until the graph changes."""
        if typestr not in ("in", "out", "both"):
            raise DGLError("Invalid incidence matrix type: %s" % typestr)
        ctx = torch.device(ctx)
        return self._cached_view(("incmat", typestr, str(ctx)),
                                 lambda: self._incidence_matrix(typestr, ctx))

    def _incidence_matrix(self, typestr, ctx):
        src, dst, eid = self._graph.edges()
        n, m = self.number_of_nodes(), self.number_of_edges()
        if typestr == "in":
            idx, val = torch.stack([dst, eid]), torch.ones(m)
        elif typestr == "out":
            idx, val = torch.stack([src, eid]), torch.ones(m)
        elif typestr == "both":
            keep = src != dst
            idx = torch.cat([torch.stack([src[keep], eid[keep]]),
                             torch.stack([dst[keep], eid[keep]])], 1)
            val = torch.cat([-torch.ones(int(keep.sum())), torch.ones(int(keep.sum()))])
        else:
            raise DGLError("Invalid incidence matrix type: %s" % typestr)
        return torch.sparse_coo_tensor(idx, val, (n, m)).to(ctx)

    def sparse_adjacency(self, ctx):
        """The engine's cached g-SpMM adjacency (kernel.SparseAdj) on ``ctx``."""
        return self._graph.adjacency(ctx)

    # -- subgraphs and filters (graph.py:2600-2719, 2800-2931) ------------------
    def subgraph(self, nodes):
        """The subgraph induced by ``nodes``: subgraph node ``i`` is
        ``nodes[i]`` and the edges are those of the parent with both ends in
        the set (``parent_nid`` / ``parent_eid`` map back). Features are not
        copied; see :meth:`DGLSubGraph.copy_from_parent`.

        Ids given as a tensor on a ROCm device, on a mutable parent, are
        induced there by a HIP kernel over the cached source-major adjacency:
        the ids, the structure and the parent ids stay on the device, the
        result equals the host answer element for element, and ids that are
        out of range or repeated raise DGLError. Lists, arrays and host
        tensors, and every readonly parent (sorted ids), go through the native
        index.

        >>> g = dgl.DGLGraph(); g.add_nodes(5)
        >>> g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 0])
        >>> sg = g.subgraph([0, 1, 4])
        >>> sg.edges(), sg.parent_nid, sg.parent_eid
        ((tensor([0, 2]), tensor([1, 0])), tensor([0, 1, 4]), tensor([0, 4]))
        """
        from .subgraph import DGLSubGraph
        if isinstance(nodes, torch.Tensor) and nodes.is_cuda and not self.is_readonly:
            sgi = self._graph.node_subgraph_device(nodes)
        else:
            sgi = self._graph.node_subgraph(utils.toindex(nodes))
        return DGLSubGraph(self, sgi.induced_nodes, sgi.induced_edges, sgi)

    def subgraphs(self, nodes):
        """One :meth:`subgraph` per node set of the list ``nodes``."""
        return [self.subgraph(v) for v in nodes]

    def edge_subgraph(self, edges):
        """The subgraph of the given edge ids: subgraph edge ``i`` is
        ``edges[i]``; its nodes are the edges' end points, numbered by first
        appearance."""
        from .subgraph import DGLSubGraph
        sgi = self._graph.edge_subgraph(utils.toindex(edges))
        return DGLSubGraph(self, sgi.induced_nodes, sgi.induced_edges, sgi)

    # -- transforms (graph.py:2786-2798) ------------------------------------------
    def line_graph(self, backtracking=True, shared=False, ctx=None):
        """The line graph of this graph: see :func:`dgl.transform.line_graph`."""
        from .transform import line_graph
        return line_graph(self, backtracking, shared, ctx)

    def reverse(self, share_ndata=False, share_edata=False):
        """This graph with every edge turned round: see
        :func:`dgl.transform.reverse`."""
        from .transform import reverse
        return reverse(self, share_ndata, share_edata)

    def filter_nodes(self, predicate, nodes=ALL):
        """Ids of the nodes that satisfy ``predicate``, a function of a
        :class:`~dgl.udf.NodeBatch` returning a 1-D boolean mask. The ids are
        on the mask's device, so ``g.subgraph(g.filter_nodes(pred))`` over
        device features stays there."""
        if is_all(nodes):
            v = torch.arange(self.number_of_nodes(), dtype=torch.int64)
            mask = predicate(NodeBatch(self, v, self.get_n_repr()))
            return torch.nonzero(mask).reshape(-1)
        v = utils.toindex(nodes)
        mask = predicate(NodeBatch(self, v, self.get_n_repr(v)))
        return v.to(mask.device)[mask]

    def filter_edges(self, predicate, edges=ALL):
        """Ids of the edges that satisfy ``predicate``, a function of an
        :class:`~dgl.udf.EdgeBatch` returning a 1-D boolean mask (``edges``
        as for :meth:`send`); on the mask's device."""
        u, v, eid = self._edge_triplet(edges)
        nf = self._node_frame
        src = LazyDict(lambda k: nf[k].index_select(0, u.to(nf[k].device)), nf.keys())
        dst = LazyDict(lambda k: nf[k].index_select(0, v.to(nf[k].device)), nf.keys())
        edata = self.get_e_repr() if is_all(edges) else self.get_e_repr(eid)
        mask = predicate(EdgeBatch(self, (u, v, eid), src, edata, dst))
        if is_all(edges):
            return torch.nonzero(mask).reshape(-1)
        return eid.to(mask.device)[mask]

    def __repr__(self):
        return ("DGLGraph(num_nodes={n}, num_edges={m},\n         ndata_schemes={ns}\n"
                "         edata_schemes={es})").format(
                    n=self.number_of_nodes(), m=self.number_of_edges(),
                    ns=self.node_attr_schemes(), es=self.edge_attr_schemes())


def _batch(vals):
    if isinstance(vals[0], torch.Tensor):
        return torch.stack(vals, 0)
    return torch.tensor(vals)



