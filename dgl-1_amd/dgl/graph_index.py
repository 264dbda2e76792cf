"""Graph structure index: the native graph of libdgl_hip.so behind a handle.

Same shape as the reference's python/dgl/graph_index.py (GraphIndex, 1027
lines): the structure lives in the library (src/graph/graph.cc mutable
adjacency, immutable_graph.cc sorted CSRs there; csrc/graph_index.cc here) and
every structural query is one ``graph_index._CAPI_*`` call through the
PackedFunc registry, with the reference's names, arguments and returns
(graph_apis.cc). So the engine's DGLGraph and the reference's own Python layer
bound to this library read the same index.

What this class adds on the Python side are caches, as the reference's
GraphIndex caches its adjacency matrices (graph_index.py:537 cached_member):
the edge list in id order as torch tensors (fetched once from the index with
``_CAPI_DGLGraphEdges``, zero-copy through DLPack) and the engine's g-SpMM CSRs
built from it per device (kernel.from_coo); all are dropped on mutation.
"""
from __future__ import absolute_import

import ctypes
import os

import numpy as np
import torch

from . import _ffi, kernel
from .base import DGLError

__all__ = ["GraphIndex", "SubgraphIndex", "NodeProb", "create_graph_index", "disjoint_union",
           "disjoint_partition", "map_to_subgraph_nid"]

_CAPI = _ffi.CAPINamespace("graph_index")


class NodeProb(object):
    """The ``node_prob`` of weighted neighbour sampling, checked once: one
    finite entry >= 0 per node (else DGLError), kept as float32 where it was
    given and copied to a device the first time seeds on it are sampled."""

    def __init__(self, node_prob, num_nodes):
        if isinstance(node_prob, NodeProb):
            node_prob = node_prob._on[0]
        if not isinstance(node_prob, torch.Tensor):
            try:
                node_prob = torch.as_tensor(np.asarray(node_prob))
            except (TypeError, ValueError, RuntimeError):
                raise DGLError("node_prob must be a tensor of numbers")
        if node_prob.dim() != 1 or node_prob.numel() != num_nodes:
            raise DGLError("node_prob needs one sampling probability per node (%d), got shape %s"
                           % (num_nodes, tuple(node_prob.shape)))
        if node_prob.dtype == torch.bool or node_prob.is_complex():
            raise DGLError("node_prob must hold real numbers, got %s" % node_prob.dtype)
        w = node_prob.detach().to(torch.float32).contiguous()
        # (after the conversion: a float64 beyond float32's range is refused too)
        if num_nodes and not bool((torch.isfinite(w) & (w >= 0)).all()):
            raise DGLError("node_prob must be finite and >= 0 in float32")
        self._on = [w]

    def on(self, device):
        """The float32 weights on ``device``."""
        device = torch.device(device)
        for w in self._on:
            if w.device == device:
                return w
        self._on.append(self._on[0].to(device))
        return self._on[-1]


def _as_i64(x):
    if isinstance(x, torch.Tensor):
        if x.numel() == 0:  # (an empty view may carry any stride)
            return torch.zeros(0, dtype=torch.int64)
        return x.detach().to(dtype=torch.int64, device="cpu").reshape(-1).contiguous()
    if isinstance(x, slice):
        return torch.arange(x.start or 0, x.stop, x.step or 1, dtype=torch.int64)
    if isinstance(x, (int, np.integer)):
        return torch.tensor([int(x)], dtype=torch.int64)
    arr = np.asarray(x, dtype=np.int64)
    if arr.size == 0:
        return torch.zeros(0, dtype=torch.int64)
    return torch.as_tensor(arr).reshape(-1).contiguous()


def _triple(f):
    """(src, dst, eid) of an EdgeArray packed function (graph_apis.cc:21-36)."""
    return f(0), f(1), f(2)


def _call(api, *args):
    """A graph_index._CAPI_* call whose library error surfaces as DGLError."""
    return getattr(_CAPI, api)(*args)


_TRAVERSAL_CAPI = _ffi.CAPINamespace("traversal")


def _call_trv(api, *args):
    """A traversal._CAPI_* call."""
    return getattr(_TRAVERSAL_CAPI, api)(*args)


class GraphIndex(object):
    """Directed (multi)graph with integer node ids 0..N-1 and edge ids 0..E-1,
    stored in the library's native index (mutable, or immutable when
    ``readonly``)."""

    def __init__(self, multigraph=False, readonly=False, handle=None):
        # a readonly index is created with its edges (create_graph_index)
        if handle is None:
            if readonly:
                handle = _call("_CAPI_DGLGraphCreate", torch.zeros(0, dtype=torch.int64),
                               torch.zeros(0, dtype=torch.int64),
                               torch.zeros(0, dtype=torch.int64), int(multigraph), 0, 1)
            else:
                handle = _call("_CAPI_DGLGraphCreateMutable", int(multigraph))
        self._handle = handle
        self._multigraph = bool(multigraph)
        self._readonly = bool(readonly)
        self._cache = {}
        self._sync_sizes()

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                _call("_CAPI_DGLGraphFree", ("handle", h))
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass
            self._handle = None

    def _h(self):
        return ("handle", self._handle)

    def _sync_sizes(self):
        # sizes mirrored on the Python side: they are read on every
        # message-passing call, the index is only asked after a mutation
        self._n = _call("_CAPI_DGLGraphNumVertices", self._h())
        self._m = _call("_CAPI_DGLGraphNumEdges", self._h())

    # -- mutation ----------------------------------------------------------
    def _invalidate(self):
        self._cache = {}

    def add_nodes(self, num):
        if self._readonly:
            raise DGLError("readonly graph cannot be mutated")
        _call("_CAPI_DGLGraphAddVertices", self._h(), int(num))
        self._sync_sizes()
        self._invalidate()

    def add_edges(self, u, v):
        if self._readonly:
            raise DGLError("readonly graph cannot be mutated")
        u = _as_i64(u)
        v = _as_i64(v)
        if u.numel() == 1 and v.numel() > 1:
            u = u.expand(v.numel()).contiguous()
        elif v.numel() == 1 and u.numel() > 1:
            v = v.expand(u.numel()).contiguous()
        if u.numel() != v.numel():
            raise DGLError("Invalid edges: %d sources vs %d destinations" % (u.numel(), v.numel()))
        if u.numel() == 0:
            return
        hi = max(int(u.max()), int(v.max()))
        if int(min(u.min(), v.min())) < 0 or hi >= self._n:
            raise DGLError("Invalid node id in edges (graph has %d nodes)" % self._n)
        _call("_CAPI_DGLGraphAddEdges", self._h(), u, v)
        self._sync_sizes()
        self._invalidate()

    def clear(self):
        if self._readonly:
            raise DGLError("readonly graph cannot be mutated")
        _call("_CAPI_DGLGraphClear", self._h())
        self._sync_sizes()
        self._invalidate()

    def is_multigraph(self):
        return self._multigraph

    def is_readonly(self):
        return self._readonly

    # -- sizes / raw arrays ------------------------------------------------
    def number_of_nodes(self):
        return self._n

    def number_of_edges(self):
        return self._m

    def _id_order(self):
        key = ("edges_id_order",)
        if key not in self._cache:
            src, dst, eid = _triple(_call("_CAPI_DGLGraphEdges", self._h(), "eid"))
            if not self._readonly:
                eid = None  # a mutable graph's ids are its positions
            self._cache[key] = (src, dst, eid)
        return self._cache[key]

    def src(self):
        """Source of every edge, in edge-id order (int64, host)."""
        return self._id_order()[0]

    def dst(self):
        """Destination of every edge, in edge-id order (int64, host)."""
        return self._id_order()[1]

    def edges(self, order=None):
        """(src, dst, eid) of all edges (graph_index.py:409-431): ``order`` None
        is the index's own order (edge ids for a mutable graph, the out-CSR for
        an immutable one), 'eid' sorts by edge id, 'srcdst' by (src, dst)."""
        if order == "eid" or (order is None and not self._readonly):
            src, dst, _ = self._id_order()
            return src, dst, torch.arange(self._m, dtype=torch.int64)
        return _triple(_call("_CAPI_DGLGraphEdges", self._h(), order or ""))

    # -- cached CSRs --------------------------------------------------------
    def _slot_order(self):
        # ImmutableGraph keeps CSR sorted by (dst, src) (immutable_graph.cc:206-237);
        # the mutable graph's COO is in edge-id order (graph.cc:509-524).
        return kernel.ORDER_COL if self._readonly else kernel.ORDER_EID

    def adjacency(self, ctx):
        """The engine's g-SpMM adjacency (kernel.SparseAdj) of the whole graph
        on ``ctx``: rows = dst, cols = src, slots in the index's adjacency
        order (the reference's adjacency_matrix(transpose=False),
        graph_index.py:537-585); built from the id-order edge list by the
        library's CSR builder and cached per device until the next mutation."""
        ctx = torch.device(ctx)
        if ctx.type == "cuda" and ctx.index is None:
            ctx = torch.device("cuda", torch.cuda.current_device())
        key = ("adj", str(ctx))
        if key not in self._cache:
            src, dst, _ = self._id_order()
            # the native index validated every edge when it was added
            self._cache[key] = kernel.from_coo(self._n, self._n, dst, src, self._slot_order(), ctx,
                                               validate=False)
        return self._cache[key]

    def incidence_in(self, ctx):
        """Destination incidence (rows = dst, cols = eid) — the e2v reduction
        matrix of graph_index.py:629-635, as a CSR over edge ids."""
        ctx = torch.device(ctx)
        key = ("inc_in", str(ctx))
        if key not in self._cache:
            n, m = self._n, self._m
            eids = torch.arange(m, dtype=torch.int64)
            self._cache[key] = kernel.from_coo(n, m, self.dst(), eids, kernel.ORDER_EID, ctx)
        return self._cache[key]

    def get_adj(self, transpose, fmt):
        """``_CAPI_DGLGraphGetAdj``: [idx(2E), eid] for 'coo', [indptr, indices,
        eid] for 'csr' (graph.cc:506-554, immutable_graph.cc:553-575)."""
        f = _call("_CAPI_DGLGraphGetAdj", self._h(), int(bool(transpose)), fmt)
        return [f(i) for i in range(2 if fmt == "coo" else 3)]

    # -- queries ------------------------------------------------------------
    def has_nodes(self, vids):
        return _call("_CAPI_DGLGraphHasVertices", self._h(), _as_i64(vids))

    def in_degrees(self, v=None):
        v = torch.arange(self._n, dtype=torch.int64) if v is None else _as_i64(v)
        return _call("_CAPI_DGLGraphInDegrees", self._h(), v)

    def out_degrees(self, v=None):
        v = torch.arange(self._n, dtype=torch.int64) if v is None else _as_i64(v)
        return _call("_CAPI_DGLGraphOutDegrees", self._h(), v)

    def in_edges(self, v):
        """(src, dst, eid) of the in-edges of ``v`` (query order; each node's
        edges in the index's adjacency order)."""
        return _triple(_call("_CAPI_DGLGraphInEdges_2", self._h(), _as_i64(v)))

    def out_edges(self, u):
        """(src, dst, eid) of the out-edges of ``u``."""
        return _triple(_call("_CAPI_DGLGraphOutEdges_2", self._h(), _as_i64(u)))

    def predecessors(self, v, radius=1):
        """Distinct predecessors of node ``v`` (graph.cc:148-162)."""
        return _call("_CAPI_DGLGraphPredecessors", self._h(), int(v), int(radius))

    def successors(self, u, radius=1):
        """Distinct successors of node ``u`` (graph.cc:164-178)."""
        return _call("_CAPI_DGLGraphSuccessors", self._h(), int(u), int(radius))

    def find_edges(self, eid):
        eid = _as_i64(eid)
        if self._readonly:  # the immutable index has no FindEdges (graph_apis.cc)
            if eid.numel() and (int(eid.min()) < 0 or int(eid.max()) >= self._m):
                raise DGLError("Invalid edge id")
            src, dst, _ = self._id_order()
            return src[eid], dst[eid], eid
        return _triple(_call("_CAPI_DGLGraphFindEdges", self._h(), eid))

    def edge_ids(self, u, v):
        """All edges between each (u, v) pair, with broadcasting of a scalar
        end (graph.cc:205-249 EdgeIds); returns (src, dst, eid)."""
        u = _as_i64(u)
        v = _as_i64(v)
        if u.numel() != v.numel() and u.numel() != 1 and v.numel() != 1:
            raise DGLError("Invalid edges: %d vs %d" % (u.numel(), v.numel()))
        if u.numel() == 0 or v.numel() == 0:
            e = torch.zeros(0, dtype=torch.int64)
            return e, e, e
        hit = self.has_edges_between(u, v)
        if not bool(hit.all()):
            bad = int((hit == 0).nonzero()[0])
            raise DGLError("Edge (%d, %d) does not exist"
                           % (int(u[bad if u.numel() > 1 else 0]),
                              int(v[bad if v.numel() > 1 else 0])))
        return _triple(_call("_CAPI_DGLGraphEdgeIds", self._h(), u, v))

    def has_edges_between(self, u, v):
        return _call("_CAPI_DGLGraphHasEdgesBetween", self._h(), _as_i64(u), _as_i64(v))

    # -- subgraphs (graph_index.py:483-535) ------------------------------------
    def node_subgraph(self, v):
        """The subgraph induced by the nodes ``v`` (``_CAPI_DGLGraphVertexSubgraph``):
        subgraph node ``i`` is ``v[i]``. A mutable index lists the out-edges of
        ``v[0]``, ``v[1]``, ... in edge-id order that end inside the set; an
        immutable one takes a sorted ``v`` and numbers the edges by CSR slot."""
        f = _call("_CAPI_DGLGraphVertexSubgraph", self._h(), _as_i64(v))
        return SubgraphIndex(self, f(1), f(2), handle=f(0))

    def node_subgraphs(self, vs):
        """One :meth:`node_subgraph` per node set of the list ``vs``."""
        return [self.node_subgraph(v) for v in vs]

    def edge_subgraph(self, e):
        """The subgraph of the edges ``e`` (``_CAPI_DGLGraphEdgeSubgraph``):
        subgraph edge ``i`` is ``e[i]``, nodes are numbered by first appearance."""
        f = _call("_CAPI_DGLGraphEdgeSubgraph", self._h(), _as_i64(e))
        return SubgraphIndex(self, f(1), f(2), handle=f(0))

    def node_subgraph_device(self, v):
        """:meth:`node_subgraph` of a mutable index for ids ``v`` on a ROCm
        device, extracted there from the source-major CSR of the cached
        adjacency (kernel.induced_subgraph); the same nodes, edges and order as
        the native index gives. Ids outside the graph or listed twice raise."""
        if self._readonly:
            raise DGLError("the device route needs a mutable parent index")
        if torch.cuda.is_current_stream_capturing():  # before anything is launched
            raise DGLError("subgraph() of device ids reads the subgraph's size on the host: "
                           "it cannot run while a stream is being captured")
        adj = self.adjacency(v.device)
        src, dst, eid = kernel.induced_subgraph(adj.bwd, v)
        nid = v.detach().to(torch.int64).reshape(-1)
        return SubgraphIndex(self, nid, eid, device_coo=(nid.numel(), src, dst))

    # -- line graph (graph_index.py:793-808) -------------------------------------
    def line_graph(self, backtracking=True):
        """The line graph of a mutable index (``_CAPI_DGLGraphLineGraph``): one
        node per edge; edge ``i = (u, v)`` links to the out-edges of ``v`` in
        edge-id order, without those back to ``u`` unless ``backtracking``. A
        plain mutable, non-multigraph index."""
        if self._readonly:
            raise DGLError("line_graph isn't implemented in immutable graph")
        h = _call("_CAPI_DGLGraphLineGraph", self._h(), int(bool(backtracking)))
        return GraphIndex(False, False, handle=h)

    def line_graph_device(self, ctx, backtracking=True):
        """:meth:`line_graph` built on the ROCm device ``ctx`` from the
        source-major CSR of the cached adjacency (kernel.line_graph): the same
        edges in the same order, left on the device. The returned index builds
        its native graph only when a query or a mutation needs it."""
        if self._readonly:
            raise DGLError("line_graph isn't implemented in immutable graph")
        if torch.cuda.is_current_stream_capturing():  # before anything is launched
            raise DGLError("line_graph() on a device reads the line graph's size on the host: "
                           "it cannot run while a stream is being captured")
        ctx = torch.device(ctx)
        if ctx.type != "cuda":
            raise DGLError("line_graph_device needs a ROCm device, got %s" % (ctx,))
        if ctx.index is None:
            ctx = torch.device("cuda", torch.cuda.current_device())
        adj = self.adjacency(ctx)
        coo = getattr(self, "_dev_coo", None)
        if coo is not None and coo[0].device == ctx:
            src, dst = coo  # this index already lives there
        else:
            src, dst, _ = self._id_order()
            both = torch.stack([src, dst]).to(ctx)  # one upload
            src, dst = both[0], both[1]
        lsrc, ldst = kernel.line_graph(adj.bwd, src, dst, backtracking)
        return _DeviceLineGraphIndex(self._m, lsrc, ldst)

    # -- neighbour sampling (graph_index.py:664-678, 1018-1027) ------------------
    def neighbor_sampling(self, seed_ids, expand_factor, num_hops, neighbor_type, node_prob,
                          seed=None):
        """One sampled ``num_hops``-hop subgraph per seed set of the list
        ``seed_ids``: each expanded vertex keeps at most ``expand_factor`` of
        its 'in' or 'out' neighbours, drawn uniformly, or with ``node_prob``
        (one finite entry >= 0 per node, or a :class:`NodeProb`; else
        DGLError) without replacement with each draw proportional to the
        neighbour's entry.

        Seed sets on the host with ``seed`` None go to the native sampler
        (``_CAPI_DGLGraphUniformSampling*``), which draws afresh on every call.
        Seed sets on a ROCm device, or any with a ``seed``, take the stateless
        rule of kernel.neighbor_sample over the cached adjacency on the seeds'
        device; subgraph ``i`` of the call is drawn under ``mix(seed + i)``,
        and a device call without a ``seed`` draws a fresh one. That route
        leaves a subgraph's ids and edge list where the seeds are. Every
        returned index carries the layer of its nodes as ``induced_layers``.

        The native sampler has no weighted draw: ``node_prob`` with host seeds
        and no ``seed`` raises NotImplementedError. With device seeds or a
        ``seed`` the weights are checked once per call, converted to float32
        and moved to the seeds' device (kernel.neighbor_sample's
        ``node_weight``)."""
        if not self._readonly:
            raise NotImplementedError("neighbor sampling only supports read-only graphs.")
        if node_prob is not None and not isinstance(node_prob, NodeProb):
            node_prob = NodeProb(node_prob, self.number_of_nodes())
        if neighbor_type not in ("in", "out"):
            raise DGLError("neighbor_type must be 'in' or 'out', got %r" % (neighbor_type,))
        if isinstance(expand_factor, bool) or not isinstance(expand_factor, (int, np.integer)):
            raise DGLError("expand_factor must be an integer, got %r" % (expand_factor,))
        expand_factor, num_hops = int(expand_factor), int(num_hops)
        if expand_factor < 0 or num_hops < 0:
            raise DGLError("invalid sampling parameters: fan-out %d, %d hops"
                           % (expand_factor, num_hops))
        seed_ids = list(seed_ids)
        if len(seed_ids) == 0:
            return []
        on_device = [isinstance(s, torch.Tensor) and s.is_cuda for s in seed_ids]
        if seed is None and not any(on_device) and node_prob is not None:
            raise NotImplementedError("the native sampler has no non-uniform draw: pass seed= "
                                      "or give the seeds as a tensor on a ROCm device.")
        if seed is None and not any(on_device):
            return self._native_sampling([_as_i64(s) for s in seed_ids], expand_factor, num_hops,
                                         neighbor_type)
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        out = []
        for i, ids in enumerate(seed_ids):
            ctx = ids.device if on_device[i] else torch.device("cpu")
            if not on_device[i]:
                ids = _as_i64(ids)
            adj = self.adjacency(ctx)
            in_dir = neighbor_type == "in"
            vertices, layers, src, dst, eid = kernel.neighbor_sample(
                adj.fwd if in_dir else adj.bwd, ids, num_hops, expand_factor,
                kernel.sample_mix(int(seed) + i), in_dir=in_dir,
                node_weight=None if node_prob is None else node_prob.on(ctx))
            sgi = SubgraphIndex(self, vertices, eid, device_coo=(vertices.numel(), src, dst))
            sgi.induced_layers = layers
            out.append(sgi)
        return out

    def _native_sampling(self, seed_ids, expand_factor, num_hops, neighbor_type):
        n = len(seed_ids)
        # the registry holds the sampler at 1, 2, 4, ..., 128 seed arrays: pad
        # with empty ones up to the next width and say how many are real
        out = []
        for b in range(0, n, 128):
            part = seed_ids[b:b + 128]
            width = 1
            while width < len(part):
                width *= 2
            pad = [torch.zeros(0, dtype=torch.int64) for _ in range(width - len(part))]
            api = "_CAPI_DGLGraphUniformSampling" + ("" if width == 1 else str(width))
            f = _call(api, self._h(), *(part + pad + [neighbor_type, num_hops, expand_factor,
                                                      len(part)]))
            for i in range(len(part)):
                sgi = SubgraphIndex(self, f(width + i), f(2 * width + i), handle=f(i))
                sgi.induced_layers = f(3 * width + i)
                out.append(sgi)
        return out

    # -- traversals (python/dgl/traversal.py -> traversal._CAPI_*) --------------
    # Each returns (ids, sections): the frontiers are consecutive runs of the
    # int64 tensor ``ids`` whose lengths are the Python list ``sections``.
    def bfs_nodes(self, source, reverse=False):
        """Node frontiers of a breadth-first search from ``source``
        (``_CAPI_DGLBFSNodes``); the first frontier is ``source`` as given."""
        f = _call_trv("_CAPI_DGLBFSNodes", self._h(), _as_i64(source), int(bool(reverse)))
        return f(0), f(1).tolist()

    def bfs_edges(self, source, reverse=False):
        """The ids of the edges that discovered each node of
        :meth:`bfs_nodes`' frontiers after the first (``_CAPI_DGLBFSEdges``)."""
        f = _call_trv("_CAPI_DGLBFSEdges", self._h(), _as_i64(source), int(bool(reverse)))
        return f(0), f(1).tolist()

    def topological_nodes(self, reverse=False):
        """Node frontiers in topological order (``_CAPI_DGLTopologicalNodes``);
        a graph with a loop raises."""
        f = _call_trv("_CAPI_DGLTopologicalNodes", self._h(), int(bool(reverse)))
        return f(0), f(1).tolist()

    def dfs_labeled_edges(self, source, reverse=False, has_reverse_edge=False,
                          has_nontree_edge=False, return_labels=True):
        """Edge frontiers of one depth-first search per source, merged
        position-wise (``_CAPI_DGLDFSLabeledEdges``): (ids, labels, sections),
        with ``labels`` None unless asked for."""
        f = _call_trv("_CAPI_DGLDFSLabeledEdges", self._h(), _as_i64(source), int(bool(reverse)),
                      int(bool(has_reverse_edge)), int(bool(has_nontree_edge)),
                      int(bool(return_labels)))
        if return_labels:
            return f(0), f(1), f(2).tolist()
        return f(0), None, f(1).tolist()

    def dfs_edges(self, source, reverse=False):
        """FORWARD edges of :meth:`dfs_labeled_edges` (``_CAPI_DGLDFSEdges``)."""
        f = _call_trv("_CAPI_DGLDFSEdges", self._h(), _as_i64(source), int(bool(reverse)))
        return f(0), f(1).tolist()

    def _walk_csrs(self, ctx, reverse):
        """(the CSR a device traversal walks, the opposite one) of a mutable
        index: slots in edge-id order, which is the native index's slot order."""
        if self._readonly:
            raise DGLError("the device route needs a mutable index")
        if torch.cuda.is_current_stream_capturing():  # before anything is launched
            raise DGLError("a traversal reads every frontier's size on the host: it cannot "
                           "run while a stream is being captured")
        adj = self.adjacency(ctx)
        return (adj.fwd, adj.bwd) if reverse else (adj.bwd, adj.fwd)

    def bfs_nodes_device(self, source, reverse=False):
        """:meth:`bfs_nodes` of a mutable index for ``source`` on a ROCm device,
        computed there over the cached adjacency (kernel.bfs_frontiers): the
        same frontiers in the same order, ``ids`` on the device."""
        return kernel.bfs_frontiers(self._walk_csrs(source.device, reverse)[0], source)

    def bfs_edges_device(self, source, reverse=False):
        """:meth:`bfs_edges` on the device of ``source``."""
        return kernel.bfs_frontiers(self._walk_csrs(source.device, reverse)[0], source,
                                    edges=True)

    def topological_nodes_device(self, ctx, reverse=False):
        """:meth:`topological_nodes` computed on the ROCm device ``ctx``."""
        return kernel.topological_frontiers(*self._walk_csrs(ctx, reverse))

    # -- pickling (graph_index.py:35-59): rebuildable from (n, multigraph, readonly, src, dst)
    def __getstate__(self):
        return (self._n, self._multigraph, self._readonly, self.src().numpy().copy(),
                self.dst().numpy().copy())

    def __setstate__(self, state):
        n, multi, ro, src, dst = state
        g = _from_edges(n, torch.as_tensor(src), torch.as_tensor(dst), multi, ro)
        self.__dict__.update(g.__dict__)
        g._handle = None  # ownership moved to self


class _DeviceCOOIndex(GraphIndex):
    """An index whose edge list a device kernel left on the GPU as
    ``_dev_coo = (src, dst)`` in edge-id order, with the sizes known from the
    construction: the g-SpMM CSRs on that device come straight from the device
    arrays, and the native index is only built, from one download of the edge
    list, when a query needs it (:attr:`has_native_index`). With ``_dev_coo``
    None it behaves as the plain index around ``_handle``."""

    _dev_coo = None

    def _h(self):
        if self._handle is None:
            # the extraction validated the endpoints: straight into a new index
            src, dst = (t.cpu() for t in self._dev_coo)
            if self._readonly:
                # a sampled subgraph of a read-only parent: an immutable index
                # whose edge ids are the positions in the edge list
                self._handle = _call("_CAPI_DGLGraphCreate", src, dst,
                                     torch.arange(self._m, dtype=torch.int64),
                                     int(self._multigraph), self._n, 1)
                return ("handle", self._handle)
            h = _call("_CAPI_DGLGraphCreateMutable", int(self._multigraph))
            self._handle = h
            _call("_CAPI_DGLGraphAddVertices", ("handle", h), self._n)
            if self._m:
                _call("_CAPI_DGLGraphAddEdges", ("handle", h), src, dst)
        return ("handle", self._handle)

    @property
    def has_native_index(self):
        """Whether the library's graph object exists yet. False for an index
        made on the device until a structural query (``edges()``, degrees,
        ``in_edges`` ...) asks for it; message passing over the whole graph
        on that device never does. Read-only."""
        return self._handle is not None

    def _on_coo_device(self, ctx):
        if self._dev_coo is None or ctx.type != "cuda":
            return False
        idx = ctx.index if ctx.index is not None else torch.cuda.current_device()
        return self._dev_coo[0].device == torch.device("cuda", idx)

    def adjacency(self, ctx):
        ctx = torch.device(ctx)
        if not self._on_coo_device(ctx):
            return super(_DeviceCOOIndex, self).adjacency(ctx)
        ctx = self._dev_coo[0].device
        key = ("adj", str(ctx))
        if key not in self._cache:
            src, dst = self._dev_coo
            # (slots in the order the index itself would give: edge ids under a
            # mutable parent, (dst, src) under a read-only one)
            self._cache[key] = kernel.from_coo(self._n, self._n, dst, src, self._slot_order(),
                                               ctx, validate=False)
        return self._cache[key]

    def incidence_in(self, ctx):
        ctx = torch.device(ctx)
        if not self._on_coo_device(ctx):
            return super(_DeviceCOOIndex, self).incidence_in(ctx)
        key = ("inc_in", str(ctx))
        if key not in self._cache:
            dst = self._dev_coo[1]
            eids = torch.arange(self._m, dtype=torch.int64, device=dst.device)
            self._cache[key] = kernel.from_coo(self._n, self._m, dst, eids, kernel.ORDER_EID,
                                               dst.device, validate=False)
        return self._cache[key]


class SubgraphIndex(_DeviceCOOIndex):
    """The index of a subgraph (graph_index.py:810-890): a read-only structure
    that remembers which parent nodes and edges it was induced from.

    Made either from the handle the native index returned, or from the edge
    list ``device_coo = (n, src, dst)`` a device extraction left on the GPU
    (GraphIndex.node_subgraph_device under a mutable parent, the seeded route
    of GraphIndex.neighbor_sampling under a read-only one; the native index
    built on demand is mutable or immutable to match). In the second form the
    sizes and the g-SpMM CSRs on that device come straight from the device
    arrays, and the native index is only built, from one download of the edge
    list, when a query needs it (:attr:`has_native_index`)."""

    def __init__(self, parent, induced_nodes, induced_edges, handle=None, device_coo=None):
        # not GraphIndex.__init__: that creates a native index at once
        self._handle = handle
        self._multigraph = parent.is_multigraph()
        self._readonly = parent.is_readonly()
        self._cache = {}
        self._parent = parent
        self._induced_nodes = induced_nodes
        self._induced_edges = induced_edges
        self._dev_coo = None
        self.induced_layers = None  # the hop of every node of a sampled subgraph
        if handle is not None:
            self._sync_sizes()
        else:
            n, src, dst = device_coo
            self._n, self._m = int(n), int(src.numel())
            self._dev_coo = (src, dst)

    @property
    def induced_nodes(self):
        """int64 parent id of every subgraph node (on the device for a device
        extraction)."""
        return self._induced_nodes

    @property
    def induced_edges(self):
        """int64 parent id of every subgraph edge."""
        return self._induced_edges

    def add_nodes(self, num):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def add_edges(self, u, v):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def clear(self):
        raise DGLError("Readonly graph. Mutation is not allowed.")

    def __getstate__(self):
        raise NotImplementedError("SubgraphIndex pickling is not supported yet.")

    def __setstate__(self, state):
        raise NotImplementedError("SubgraphIndex unpickling is not supported yet.")


class _DeviceLineGraphIndex(_DeviceCOOIndex):
    """The mutable, non-multigraph index of a line graph whose edge list
    GraphIndex.line_graph_device left on the GPU. The first mutation builds
    the native index, drops the device edge list and the caches, and goes on
    as any index does."""

    def __init__(self, n, src, dst):
        # not GraphIndex.__init__: that creates a native index at once
        self._handle = None
        self._multigraph = False
        self._readonly = False
        self._cache = {}
        self._n, self._m = int(n), int(src.numel())
        self._dev_coo = (src, dst)

    def _leave_device(self):
        self._h()
        self._dev_coo = None
        self._invalidate()

    def add_nodes(self, num):
        self._leave_device()
        super(_DeviceLineGraphIndex, self).add_nodes(num)

    def add_edges(self, u, v):
        self._leave_device()
        super(_DeviceLineGraphIndex, self).add_edges(u, v)

    def clear(self):
        self._leave_device()
        super(_DeviceLineGraphIndex, self).clear()


def map_to_subgraph_nid(subgraph_index, parent_nids):
    """Subgraph ids of the parent node ids ``parent_nids`` (graph_index.py:
    871-890, ``_CAPI_DGLMapSubgraphNID``); every id must be in the subgraph.
    int64, host."""
    return _call("_CAPI_DGLMapSubgraphNID", _as_i64(subgraph_index.induced_nodes),
                 _as_i64(parent_nids))


def _from_edges(n, src, dst, multigraph, readonly):
    src, dst = _as_i64(src), _as_i64(dst)
    if readonly:
        # immutable index: in/out CSRs sorted per row (immutable_graph.cc:260-281)
        if src.numel() and (int(min(src.min(), dst.min())) < 0
                            or int(max(src.max(), dst.max())) >= n):
            raise DGLError("Invalid node id in edges (graph has %d nodes)" % n)
        h = _call("_CAPI_DGLGraphCreate", src, dst, torch.arange(src.numel(), dtype=torch.int64),
                  int(multigraph), int(n), 1)
        return GraphIndex(multigraph, True, handle=h)
    gi = GraphIndex(multigraph, False)
    gi.add_nodes(n)
    gi.add_edges(src, dst)
    return gi


def disjoint_union(graphs):
    """One index holding the given indices side by side, node and edge ids
    offset by the running sizes (graph_index.py:895-917): one
    ``_CAPI_DGLDisjointUnion`` call over the list of handles."""
    graphs = list(graphs)
    handles = (ctypes.c_void_p * max(len(graphs), 1))(*[g._h()[1] for g in graphs])
    h = _call("_CAPI_DGLDisjointUnion", ("handle", ctypes.addressof(handles)), len(graphs))
    return GraphIndex(any(g.is_multigraph() for g in graphs), False, handle=h)


def disjoint_partition(graph, num_or_size_splits):
    """The inverse of :func:`disjoint_union` (graph_index.py:919-947): the
    parts of ``graph`` with the given node counts (a list / tensor of sizes),
    or an int number of equal parts; edges may not cross parts."""
    if isinstance(num_or_size_splits, (int, np.integer)):
        hs = _call("_CAPI_DGLDisjointPartitionByNum", graph._h(), int(num_or_size_splits))
    else:
        hs = _call("_CAPI_DGLDisjointPartitionBySizes", graph._h(), _as_i64(num_or_size_splits))
    return [GraphIndex(graph.is_multigraph(), False, handle=int(h)) for h in hs.tolist()]


def create_graph_index(graph_data=None, multigraph=False, readonly=False):
    """Build a GraphIndex from None, (src, dst), an edge list, a scipy sparse
    matrix, a networkx graph, or another GraphIndex (graph_index.py:950-998)."""
    if isinstance(graph_data, GraphIndex):
        return graph_data
    if graph_data is None:
        return GraphIndex(multigraph=multigraph, readonly=readonly)
    if isinstance(graph_data, tuple) and len(graph_data) == 2:
        src, dst = _as_i64(graph_data[0]), _as_i64(graph_data[1])
        n = 0 if src.numel() == 0 else int(max(src.max(), dst.max())) + 1
    elif isinstance(graph_data, (list,)):
        arr = np.asarray(graph_data, dtype=np.int64).reshape(-1, 2)
        n = 0 if arr.size == 0 else int(arr.max()) + 1
        src, dst = arr[:, 0], arr[:, 1]
    elif hasattr(graph_data, "tocoo"):
        coo = graph_data.tocoo()
        n = coo.shape[0]
        src, dst = coo.row.astype(np.int64), coo.col.astype(np.int64)
    elif hasattr(graph_data, "is_directed") and hasattr(graph_data, "edges"):
        import networkx as nx
        nxg = nx.convert_node_labels_to_integers(graph_data, ordering="sorted")
        if not nxg.is_directed():
            nxg = nxg.to_directed()
        n = nxg.number_of_nodes()
        elist = list(nxg.edges(data=True))
        if elist and "id" in elist[0][2]:
            elist.sort(key=lambda e: e[2]["id"])
        src = [e[0] for e in elist]
        dst = [e[1] for e in elist]
    else:
        raise DGLError("Unsupported graph data type: %s" % type(graph_data))
    return _from_edges(n, src, dst, multigraph, readonly)
