"""The device route of degree bucketing (csrc/degree_buckets.hip,
kernel.degree_buckets, runtime/degree_bucketing.py) against the host route.

The kernel's arrays are compared with dglhip_degree_bucketing_host and the
numpy restatement of test_degree_buckets.py on that file's case list, each
case built through kernel.build_csr(..., ORDER_EID) on the device. Through the
public interface a graph with features on the device is compared with its twin
on the host (which takes the host route). Features are small integers held as
float32, so every sum a reducer forms is exact and every comparison here is
integer equality or torch.equal. No case feeds an out-of-range receiver to the
kernel: build_csr refuses those before anything is launched."""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import kernel
from dgl.runtime import degree_bucketing
from test_degree_buckets import CHUNK, cases, host_schedule, restate

pytestmark = pytest.mark.gpu

ARRAYS = ("bucket_deg", "bucket_node_ptr", "nodes", "zero_nodes", "msg_ids", "merge_inv")


def device_csr(recv, R):
    recv = torch.from_numpy(recv)
    M = recv.numel()
    return kernel.build_csr(R, M, recv, torch.arange(M), kernel.ORDER_EID,
                            device=torch.device("cuda", 0), schedule=False)


def arrays_of(sched):
    return {k: getattr(sched, k).cpu().numpy() for k in ARRAYS}


@pytest.mark.parametrize("name", sorted(cases()))
def test_kernel_equals_host_function(name):
    recv, R = cases()[name]
    csr = device_csr(recv, R)
    if name not in ("known", "no_rows", "no_messages", "one_bucket"):
        assert not torch.equal(csr.eid.cpu(), torch.arange(recv.size))  # a real permutation
    want, full = host_schedule(recv, R), restate(recv, R)
    deg = np.bincount(recv, minlength=R)
    _, counts = kernel.degree_buckets_count(csr)
    assert counts == [want["bucket_deg"].size, int((deg > 0).sum()),
                      int(deg.max()) if R else 0, int(((deg + CHUNK - 1) // CHUNK).sum())]
    sched = kernel.degree_buckets(csr, csr.eid)
    got = arrays_of(sched)
    assert sched.num_buckets == want["bucket_deg"].size
    for key in ("bucket_deg", "bucket_node_ptr", "nodes", "msg_ids"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("zero_nodes", "merge_inv"):
        assert np.array_equal(got[key], full[key]), key
    assert sched.R == R and sched.listed == want["nodes"].size
    assert sched.host_deg == want["bucket_deg"].tolist()
    assert sched.host_node_ptr == want["bucket_node_ptr"].tolist()


def test_null_slot_msg_is_the_identity():
    recv, R = cases()["skewed"]
    csr = device_csr(recv, R)
    null = arrays_of(kernel.degree_buckets(csr))
    ident = arrays_of(kernel.degree_buckets(csr, torch.arange(recv.size).cuda()))
    for key in ARRAYS:
        assert np.array_equal(null[key], ident[key]), key
    # slot k of the CSR is message k of the receivers in slot order
    assert np.array_equal(null["msg_ids"], restate(np.sort(recv), R)["msg_ids"])


# ---- through the public interface -----------------------------------------
N, E, HUB, HUB_DEG, F = 300, 3000, 7, 600, 4
NO_IN = np.arange(N - 20, N)  # 20 nodes without in-edges


def _seven(shape, dtype, ctx, id_range):
    return torch.full(shape, 7, dtype=dtype, device=ctx)


def message(edges):
    return {"m": edges.src["h"]}


def r_position(nodes):
    m = nodes.mailbox["m"]
    w = torch.arange(m.shape[1], dtype=m.dtype, device=m.device)
    return {"o": (m * w[None, :, None]).sum(1)}


def r_max(nodes):
    return {"o": nodes.mailbox["m"].max(1)[0]}


def r_two_fields(nodes):
    m = nodes.mailbox["m"]
    return {"o": m.sum(1) + nodes.data["h"], "first": 2 * m[:, 0]}


class Recorder(object):
    def __init__(self):
        self.seen = []

    def __call__(self, nodes):
        assert nodes.batch_size() == nodes.mailbox["m"].shape[0]
        self.seen.append(nodes.nodes())
        return {"o": nodes.mailbox["m"].sum(1)}


class Pair(object):
    """The same graph twice: features on the device and on the host."""

    def __init__(self):
        rng = np.random.default_rng(31)
        others = np.setdiff1d(np.arange(N - 20), [HUB])
        src = rng.integers(0, N, E)
        dst = np.concatenate([np.full(HUB_DEG, HUB), rng.choice(others, E - HUB_DEG)])
        src[HUB_DEG + 50:HUB_DEG + 100] = src[HUB_DEG:HUB_DEG + 50]  # multi-edges
        dst[HUB_DEG + 50:HUB_DEG + 100] = dst[HUB_DEG:HUB_DEG + 50]
        order = rng.permutation(E)
        self.src, self.dst = src[order], dst[order]
        deg = np.bincount(self.dst, minlength=N)
        assert deg[HUB] == HUB_DEG and (deg[NO_IN] == 0).all()
        self.zero_in = np.flatnonzero(deg == 0)
        self.h = torch.from_numpy(rng.integers(-4, 5, (N, F)).astype(np.float32))
        self.k = torch.from_numpy(rng.integers(-4, 5, (N, F)))
        self.up = torch.from_numpy(rng.integers(-3, 4, (N, F)).astype(np.float32))
        self.eids = torch.from_numpy(rng.choice(E, 700, replace=False))
        has_in = np.setdiff1d(np.arange(N), self.zero_in)
        self.pulled = torch.from_numpy(rng.permutation(
            np.concatenate([rng.choice(has_in, 40, replace=False), NO_IN[:10]])))
        self.extra = (rng.integers(0, N, 40), rng.integers(0, N, 40))

    def graph(self, dev):
        g = dgl.DGLGraph(multigraph=True)
        g.add_nodes(N)
        g.add_edges(self.src, self.dst)
        g.set_n_initializer(_seven)
        g.ndata["h"] = self.h.clone().to(dev)
        g.ndata["k"] = self.k.clone().to(dev)
        return g

    def both(self):
        return self.graph(torch.device("cuda", 0)), self.graph(torch.device("cpu"))


@pytest.fixture(scope="module")
def pair():
    return Pair()


def run_both(pair, call, fields=("o",)):
    """``call(g)`` on the device graph and on the host graph; the routes each
    took, then the fields compared."""
    gd, gh = pair.both()
    c0 = degree_bucketing.route_counts()
    call(gd)
    c1 = degree_bucketing.route_counts()
    call(gh)
    c2 = degree_bucketing.route_counts()
    assert c1["device"] > c0["device"] and c1["host"] == c0["host"]
    assert c2["host"] > c1["host"] and c2["device"] == c1["device"]
    assert c2["device_builds"] == c1["device_builds"]
    for f in fields:
        assert gd.ndata[f].device.type == "cuda"
        assert torch.equal(gd.ndata[f].cpu(), gh.ndata[f]), f
    return gd, gh


@pytest.mark.parametrize("reducer,fields", [(r_position, ("o",)), (r_max, ("o",)),
                                            (r_two_fields, ("o", "first"))])
def test_update_all(pair, reducer, fields):
    gd, _ = run_both(pair, lambda g: g.update_all(message, reducer), fields)
    for f in fields:  # rows without messages hold the initializer's value
        assert bool((gd.ndata[f][torch.from_numpy(pair.zero_in).cuda()] == 7).all())
    assert len(pair.zero_in) >= 20


def test_recorded_node_ids_are_host_tensors(pair):
    rd, rh = Recorder(), Recorder()
    gd, gh = pair.both()
    gd.update_all(message, rd)
    gh.update_all(message, rh)
    assert len(rd.seen) == len(rh.seen) > 3
    for a, b in zip(rd.seen, rh.seen):
        assert a.device.type == "cpu" and a.dtype == torch.int64 and torch.equal(a, b)
    assert torch.equal(gd.ndata["o"].cpu(), gh.ndata["o"])
    # and of a partial call: parent node ids, not receiver positions
    rd, rh = Recorder(), Recorder()
    gd.pull(pair.pulled, message, rd)
    gh.pull(pair.pulled, message, rh)
    assert len(rd.seen) == len(rh.seen) > 1
    for a, b in zip(rd.seen, rh.seen):
        assert a.device.type == "cpu" and torch.equal(a, b)


@pytest.mark.parametrize("reducer", [r_position, r_two_fields])
def test_send_and_recv(pair, reducer):
    def call(g):
        g.ndata["o"] = torch.zeros(N, F, device=g.ndata["h"].device)
        g.send_and_recv(pair.eids, message, reducer)
    run_both(pair, call)


def test_pull_with_nodes_without_in_edges(pair):
    def call(g):
        g.ndata["o"] = torch.zeros(N, F, device=g.ndata["h"].device)
        g.pull(pair.pulled, message, r_position)
    gd, _ = run_both(pair, call)
    assert bool((gd.ndata["o"][torch.from_numpy(NO_IN[:10]).cuda()] == 7).all())


def test_send_then_recv(pair):
    def call(g):
        g.ndata["o"] = torch.zeros(N, F, device=g.ndata["h"].device)
        g.send(pair.eids, message)
        g.recv(pair.pulled, r_position)
    run_both(pair, call)


def test_builtin_sum_over_int64_messages(pair):
    def call(g):
        g.update_all(lambda e: {"m": e.src["k"]}, fn.sum("m", "o"))
    gd, _ = run_both(pair, call)
    assert gd.ndata["o"].dtype == torch.int64


def test_backward(pair):
    gd, gh = pair.both()
    grads = []
    for g in (gd, gh):
        h = pair.h.clone().to(g.ndata["h"].device).requires_grad_(True)
        g.ndata["h"] = h
        g.update_all(message, r_position)
        out = g.ndata["o"]
        (out * pair.up.to(out.device)).sum().backward()
        grads.append(h.grad.cpu())
    assert torch.equal(gd.ndata["o"].detach().cpu(), gh.ndata["o"].detach())
    assert torch.equal(grads[0], grads[1]) and bool(grads[0].abs().sum() > 0)


def test_schedule_is_cached_until_a_mutation(pair):
    gd, gh = pair.both()
    c0 = degree_bucketing.route_counts()
    gd.update_all(message, r_position)
    c1 = degree_bucketing.route_counts()
    assert c1["device_builds"] == c0["device_builds"] + 1
    gd.update_all(message, r_max)
    c2 = degree_bucketing.route_counts()
    assert c2["device_builds"] == c1["device_builds"] and c2["device"] == c0["device"] + 2
    for g in (gd, gh):
        g.add_edges(*pair.extra)
        g.update_all(message, r_position)
    c3 = degree_bucketing.route_counts()
    assert c3["device_builds"] == c2["device_builds"] + 1
    assert torch.equal(gd.ndata["o"].cpu(), gh.ndata["o"])


def test_strided_and_offset_message_tensors(pair):
    gd, _ = pair.both()
    dev = gd.ndata["h"].device
    dst = torch.from_numpy(pair.dst)
    m = gd.ndata["h"][torch.from_numpy(pair.src).to(dev)].contiguous()
    wide = torch.zeros(E, 2 * F, device=dev)
    wide[:, ::2] = m
    strided = wide[:, ::2]
    buf = torch.zeros(E * F + 1, device=dev)
    buf[1:] = m.reshape(-1)
    offset = buf[1:].view(E, F)
    assert not strided.is_contiguous() and offset.storage_offset() == 1
    want = degree_bucketing.bucket_reduce(gd, r_position, None, dst, {"m": m},
                                          gd._node_frame)["o"]
    for view in (strided, offset):
        got = degree_bucketing.bucket_reduce(gd, r_position, None, dst, {"m": view},
                                             gd._node_frame)["o"]
        assert torch.equal(got, want)
    # a partial call over a slice of the views: still strided, still offset
    cut = slice(100, 800)
    recv = torch.unique(dst[cut], sorted=True)
    want = degree_bucketing.bucket_reduce(gd, r_position, recv, dst[cut],
                                          {"m": m[cut].contiguous()}, gd._node_frame)["o"]
    for view in (strided[cut], offset[cut]):
        assert not (view.is_contiguous() and view.storage_offset() % 2 == 0)
        got = degree_bucketing.bucket_reduce(gd, r_position, recv, dst[cut], {"m": view},
                                             gd._node_frame)["o"]
        assert torch.equal(got, want)
