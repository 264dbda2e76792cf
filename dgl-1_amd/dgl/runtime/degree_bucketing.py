"""Degree bucketing for user-defined reduce functions.

Counterpart of python/dgl/runtime/degree_bucketing.py:13-190 and the native
``sched::DegreeBucketing`` (src/scheduler/scheduler.cc:13-93): receiving
nodes are grouped by in-degree so each bucket's mailbox is a dense
(n_bucket, degree, *feat) tensor the UDF can reduce over dim 1. A node's
messages appear in the order of the triggered edge list (scheduler.cc:22-33
appends message ids per destination in edge order). Buckets are processed in
ascending degree and the results are merged back in receiving-node order
(MERGE_ROW, executor.py:600-663); receiving nodes without messages get the
frame initializer's value (degree_bucketing.py:72-78).

Builtin reducers never come here: they run as g-SpMM kernels. The bucket
schedule itself is computed natively, on one of two routes with the same
arrays: on the host (dglhip_degree_bucketing_host) for messages in host
memory, and on the device (csrc/degree_buckets.hip, kernel.degree_buckets)
when every message tensor is on one ROCm device. The device route takes the
schedule from a receiver-major CSR, keeps it on the index's cached CSR for a
whole-graph call, and neither uploads nor waits inside the bucket loop.
"""
from __future__ import absolute_import

import ctypes

import torch

from .. import kernel
from .._ffi import LIB, check_call, ptr
from ..udf import NodeBatch

__all__ = ["bucket_reduce", "route_counts"]

_ROUTES = {"host": 0, "device": 0, "device_builds": 0}
_PLAN_KEY = "degree_buckets"


def route_counts():
    """Calls of :func:`bucket_reduce` since import by the route they took,
    and the schedules the device route built (a whole-graph call whose
    schedule was cached builds none): ``{"host", "device", "device_builds"}``."""
    return dict(_ROUTES)


def _message_device(msgs):
    """The ROCm device every message tensor is on, or None."""
    devs = set(t.device for _, t in msgs.items())
    if len(devs) != 1:
        return None
    dev = devs.pop()
    if dev.type != "cuda" or torch.cuda.is_current_stream_capturing():
        return None
    return dev


def _whole_graph_csr(index, dev):
    """A destination-major CSR of the whole graph in edge-id order that the
    index caches on ``dev``: the incidence matrix's or the adjacency's (the
    same rows and edge ids), the adjacency built when neither is there."""
    for key in (("inc_in", str(dev)), ("adj", str(dev))):
        hit = index._cache.get(key)
        if hit is not None:
            return hit.fwd
    return index.adjacency(dev).fwd


def _device_schedule(g, recv_nodes, msg_dst, n_msgs, dev):
    """(schedule, receiver ids on the device or None for row = node id)."""
    index = g._graph
    if recv_nodes is None and not index.is_readonly():
        # message i is edge i: the schedule of the index's own CSR, kept on it
        # (a mutation drops the index's CSRs and the schedule with them)
        csr = _whole_graph_csr(index, dev)
        if csr.nnz == n_msgs:
            sched = csr._plans.get(_PLAN_KEY)
            if sched is None:
                sched = csr._plans[_PLAN_KEY] = kernel.degree_buckets(csr, csr.eid)
                _ROUTES["device_builds"] += 1
            return sched, None
    dst = kernel._upload(msg_dst, dev)
    if recv_nodes is None:
        recv, pos, n_recv = None, dst, g.number_of_nodes()
    else:
        recv = kernel._upload(recv_nodes, dev)
        pos, n_recv = torch.searchsorted(recv, dst), recv.numel()
    # (its range check stands for the host function's "receiver out of range")
    csr = kernel.build_csr(n_recv, n_msgs, pos, torch.arange(n_msgs, device=dev),
                           kernel.ORDER_EID, device=dev, schedule=False)
    _ROUTES["device_builds"] += 1
    return kernel.degree_buckets(csr, csr.eid), recv


def _bucket_reduce_device(g, reduce_udf, recv_nodes, msg_dst, msgs, node_frame, dev):
    n_msgs = next(t.shape[0] for _, t in msgs.items())
    sched, recv = _device_schedule(g, recv_nodes, msg_dst, n_msgs, dev)
    ids = sched.nodes if recv is None else recv.index_select(0, sched.nodes)
    outs = []
    moff = 0
    for b in range(sched.num_buckets):
        d = sched.host_deg[b]
        lo, hi = sched.host_node_ptr[b], sched.host_node_ptr[b + 1]
        n = hi - lo
        mids = sched.msg_ids[moff:moff + n * d]
        moff += n * d
        nodes = ids[lo:hi]
        mailbox = {}
        for k, t in msgs.items():
            mailbox[k] = t.index_select(0, mids).reshape((n, d) + tuple(t.shape[1:]))
        data = node_frame.select_rows(nodes)
        outs.append(reduce_udf(NodeBatch(g, nodes.cpu, data, mailbox, batch_size=n)))
    results = {}
    if not outs:
        return results
    zeros = sched.R - sched.listed
    for key in outs[0].keys():
        parts = [o[key] for o in outs]
        ref = parts[0]
        if zeros:
            init = node_frame.get_initializer(key)
            fill = init((zeros,) + tuple(ref.shape[1:]), ref.dtype, ref.device, slice(0, zeros))
            parts.append(fill.to(ref.device))
        cat = torch.cat(parts, 0)
        results[key] = cat.index_select(0, sched.merge_inv.to(cat.device))
    return results


def bucket_reduce(g, reduce_udf, recv_nodes, msg_dst, msgs, node_frame):
    """Run ``reduce_udf`` over degree buckets.

    recv_nodes : sorted unique node ids (CPU int64) receiving the reduction;
                 None stands for every node (update_all)
    msg_dst    : destination node of every message (CPU int64, message order)
    msgs       : dict of message tensors, first dim = len(msg_dst)
    returns    : dict of reduced features, first dim = len(recv_nodes)
    """
    dev = _message_device(msgs)
    if dev is not None:
        _ROUTES["device"] += 1
        return _bucket_reduce_device(g, reduce_udf, recv_nodes, msg_dst, msgs, node_frame, dev)
    _ROUTES["host"] += 1
    return _bucket_reduce_host(g, reduce_udf, recv_nodes, msg_dst, msgs, node_frame)


def _bucket_reduce_host(g, reduce_udf, recv_nodes, msg_dst, msgs, node_frame):
    """The host route: the schedule of dglhip_degree_bucketing_host, each
    bucket's message ids brought to the messages' device as they are used."""
    if recv_nodes is None:
        recv_nodes = torch.arange(g.number_of_nodes(), dtype=torch.int64)
    n_recv = len(recv_nodes)
    pos = torch.searchsorted(recv_nodes, msg_dst).contiguous()
    n_msgs = pos.numel()
    nb = ctypes.c_int64()
    bdeg = torch.empty(max(n_recv, 1), dtype=torch.int64)
    bptr = torch.empty(n_recv + 1, dtype=torch.int64)
    bnodes = torch.empty(max(n_recv, 1), dtype=torch.int64)
    mids_all = torch.empty(max(n_msgs, 1), dtype=torch.int64)
    check_call(LIB.dglhip_degree_bucketing_host(n_msgs, ptr(pos), n_recv, ctypes.byref(nb),
                                                ptr(bdeg), ptr(bptr), ptr(bnodes),
                                                ptr(mids_all)))
    results = {}
    positions = []
    outs = []
    moff = 0
    for b in range(nb.value):
        d = int(bdeg[b])
        members = bnodes[int(bptr[b]):int(bptr[b + 1])]
        mids = mids_all[moff:moff + d * len(members)]
        moff += d * len(members)
        nodes = recv_nodes[members]
        mailbox = {}
        for k, t in msgs.items():
            sel = t.index_select(0, mids.to(t.device))
            mailbox[k] = sel.reshape((len(members), d) + tuple(t.shape[1:]))
        data = node_frame.select_rows(nodes)
        out = reduce_udf(NodeBatch(g, nodes, data, mailbox))
        positions.append(members)
        outs.append(out)
    if not outs:
        return results
    has_msg = torch.zeros(n_recv, dtype=torch.bool)
    has_msg[bnodes[:int(bptr[nb.value])]] = True
    zero_deg = (~has_msg).nonzero(as_tuple=True)[0]
    allpos = torch.cat(positions + [zero_deg])
    inv = torch.empty_like(allpos)
    inv[allpos] = torch.arange(len(allpos))
    for key in outs[0].keys():
        parts = [o[key] for o in outs]
        ref = parts[0]
        if len(zero_deg):
            init = node_frame.get_initializer(key)
            fill = init((len(zero_deg),) + tuple(ref.shape[1:]), ref.dtype, ref.device,
                        slice(0, len(zero_deg)))
            parts.append(fill.to(ref.device))
        cat = torch.cat(parts, 0)
        results[key] = cat.index_select(0, inv.to(cat.device))
    return results
