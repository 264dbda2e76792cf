"""Subgraph samplers: the surface of the reference's dgl.contrib.sampling.

``NeighborSampler`` walks the seed nodes in batches and yields, per batch, the
sampled multi-hop neighbourhood as a :class:`~dgl.subgraph.DGLSubGraph` plus a
dict of auxiliary data. Seeds on the host go to the native sampler, as in the
reference. Seeds given as a tensor on a ROCm device are sampled there by the
HIP kernels of csrc/neighbor_sample.hip, uniformly or by ``node_prob``: the
subgraph's ids and structure stay on the device, ``copy_from_parent`` gathers
there and message passing over the subgraph needs no native index. A ``seed``
makes every batch reproducible on either route (the stateless rules of
csrc/sample_key.h).
"""
from __future__ import absolute_import

import queue
import threading

import torch

from ... import utils
from ...graph_index import NodeProb
from ...subgraph import DGLSubGraph

__all__ = ["NeighborSampler"]


class NSSubgraphLoader(object):
    """Iterator over ``(subgraph, aux)`` of consecutive seed batches. When it
    runs dry it samples the next ``num_workers`` batches in one call to the
    graph index."""

    def __init__(self, g, batch_size, expand_factor, num_hops=1, neighbor_type="in",
                 node_prob=None, seed_nodes=None, shuffle=False, num_workers=1,
                 return_seed_id=False, seed=None):
        if not g._graph.is_readonly():
            raise NotImplementedError("subgraph loader only support read-only graphs.")
        if node_prob is not None:
            # checked and converted once, not per batch; uploaded once per device
            node_prob = NodeProb(node_prob, g.number_of_nodes())
        self._g = g
        self._args = (expand_factor, num_hops, neighbor_type, node_prob)
        self._batch_size = int(batch_size)
        self._num_workers = max(int(num_workers), 1)
        self._return_seed_id = bool(return_seed_id)
        self._seed = None if seed is None else int(seed)
        if seed_nodes is None:
            seeds = torch.arange(g.number_of_nodes(), dtype=torch.int64)
        elif isinstance(seed_nodes, torch.Tensor) and seed_nodes.is_cuda:
            # ids on a device stay there and select the device route
            seeds = seed_nodes.detach().to(torch.int64).reshape(-1)
        else:
            seeds = utils.toindex(seed_nodes)
        if shuffle:
            gen = None
            if self._seed is not None:
                gen = torch.Generator().manual_seed(self._seed & 0x7FFFFFFFFFFFFFFF)
            seeds = seeds[torch.randperm(seeds.numel(), generator=gen).to(seeds.device)]
        self._seeds = seeds
        self._next_batch = 0
        self._ready = []  # (subgraph, seed ids) sampled and not yet handed out

    def _sample_ahead(self):
        n, bs = self._seeds.numel(), self._batch_size
        first = self._next_batch
        batches = []
        while len(batches) < self._num_workers and self._next_batch * bs < n:
            lo = self._next_batch * bs
            batches.append(self._seeds[lo:min(lo + bs, n)])
            self._next_batch += 1
        # batch j of the whole walk is drawn under mix(seed + j)
        seed = None if self._seed is None else self._seed + first
        indices = self._g._graph.neighbor_sampling(batches, *self._args, seed=seed)
        for sgi, ids in zip(indices, batches):
            sg = DGLSubGraph(self._g, sgi.induced_nodes, sgi.induced_edges, sgi)
            self._ready.append((sg, ids))

    def __iter__(self):
        return self

    def __next__(self):
        if not self._ready:
            self._sample_ahead()
        if not self._ready:  # every seed has been walked
            raise StopIteration
        sg, ids = self._ready.pop(0)
        return sg, ({"seeds": ids} if self._return_seed_id else {})

    next = __next__


class _ThreadPrefetcher(object):
    """Iterator that runs ``loader`` in a daemon thread, at most ``depth``
    elements ahead of the consumer. An exception in the thread is raised by the
    ``next()`` that reaches it."""

    _ITEM, _END, _ERROR = 0, 1, 2

    def __init__(self, loader, depth):
        self._q = queue.Queue(depth)
        self._closed = threading.Event()
        self._done = False
        self._thread = threading.Thread(target=self._work, args=(loader,))
        self._thread.daemon = True
        self._thread.start()

    def _put(self, kind, value=None):
        # a put that gives up once the consumer is gone: a thread blocked on a
        # full queue for ever would keep its prefetched subgraphs alive
        while not self._closed.is_set():
            try:
                self._q.put((kind, value), timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def _work(self, loader):
        try:
            for item in loader:
                if not self._put(self._ITEM, item):
                    return
            self._put(self._END)
        except BaseException as err:  # noqa: BLE001 - handed to the consumer
            self._put(self._ERROR, err)

    def __iter__(self):
        return self

    def __next__(self):
        if self._done:
            raise StopIteration
        kind, value = self._q.get()
        if kind == self._ITEM:
            return value
        self._done = True
        self._closed.set()
        if kind == self._ERROR:
            raise value
        raise StopIteration

    next = __next__

    def __del__(self):
        self._closed.set()


class _PrefetchingLoader(object):
    """An iterable whose every ``iter()`` starts a thread running ``loader``
    ``num_prefetch`` (>= 1) elements ahead."""

    def __init__(self, loader, num_prefetch=1):
        if num_prefetch < 1:
            raise ValueError("num_prefetch must be greater 0.")
        self._loader = loader
        self._num_prefetch = num_prefetch

    def __iter__(self):
        return _ThreadPrefetcher(self._loader, self._num_prefetch)


def NeighborSampler(g, batch_size, expand_factor, num_hops=1, neighbor_type="in",
                    node_prob=None, seed_nodes=None, shuffle=False, num_workers=1,
                    return_seed_id=False, prefetch=False, seed=None):
    """An iterator over neighbour-sampled subgraphs of the read-only graph ``g``.

    The seeds are cut into batches of ``batch_size`` and every batch grows one
    subgraph: its seeds, at most ``expand_factor`` uniformly drawn neighbours
    of each (all of them when there are no more), theirs in turn up to
    ``num_hops`` hops, and the edges from each expanded vertex to the
    neighbours drawn for it. Each step yields ``(subgraph, aux)``; the hop that
    reached every node is ``subgraph._graph.induced_layers`` (seeds: 0).

    Parameters
    ----------
    g : DGLGraph
        Read-only; a mutable graph raises NotImplementedError.
    batch_size : int
    expand_factor : int
    num_hops : int
    neighbor_type : 'in' or 'out'
        Follow in-edges (towards predecessors) or out-edges.
    node_prob : tensor, optional
        One finite sampling weight >= 0 per node of ``g`` (any real dtype, on
        the host or a device; anything else raises DGLError). A vertex with
        more than ``expand_factor`` neighbours keeps ``expand_factor`` of
        them drawn without replacement, each draw proportional to the
        neighbour's weight; shorter neighbour lists are kept whole whatever
        the weights. The weights are converted to float32 once and moved to
        the seeds' device once. A neighbour of weight zero (or below
        float32's normal range) is taken only when fewer than
        ``expand_factor`` neighbours carry weight. Needs ``seed`` or seeds on
        a device: the native sampler has no weighted draw
        (NotImplementedError). All-ones weights are uniform in law but do not
        reproduce the batches of ``node_prob=None``: the keys differ.
    seed_nodes : ids, optional
        All nodes when None. A tensor on a ROCm device selects the device
        route: sampling runs there and the subgraph's ids, its structure and
        ``aux['seeds']`` stay there.
    shuffle : bool
        Walk the seeds in random order (reproducible with ``seed``).
    num_workers : int
        Batches sampled per call to the index; the native sampler draws them
        in parallel.
    return_seed_id : bool
        Put the batch's seeds (parent ids) into ``aux['seeds']``.
    prefetch : bool
        Sample ``2 * num_workers`` batches ahead in a background thread.
    seed : int, optional
        Batch ``j`` is drawn by the stateless rule under ``mix(seed + j)``,
        the same on the host and on a device. None draws afresh (host seeds:
        the native sampler).
    """
    loader = NSSubgraphLoader(g, batch_size, expand_factor, num_hops, neighbor_type, node_prob,
                              seed_nodes, shuffle, num_workers, return_seed_id, seed)
    if not prefetch:
        return loader
    return _PrefetchingLoader(loader, num_prefetch=2 * max(int(num_workers), 1))
