"""Degree bucketing on two routes (runtime/degree_bucketing.py): what can be
checked without a device. The contract of the device builder
(csrc/degree_buckets.hip, include/dgl_hip.h) is restated in numpy and pinned
to dglhip_degree_bucketing_host on the case list that test_degree_buckets_gpu.py
runs on the device; the host route of bucket_reduce is pinned to a per-node
restatement; NodeBatch takes its ids lazily. Every comparison is integer
equality or torch.equal."""
import ctypes
import functools
import os

import numpy as np
import torch

import dgl
from dgl import kernel
from dgl._ffi import LIB, check_call, ptr
from dgl.runtime import degree_bucketing
from dgl.udf import NodeBatch

CHUNK = 512  # DGLHIP_BUCKET_CHUNK
KNOWN = ([3, 1, 3, 0, 3, 1, 4], 6)  # test_degree_bucketing_schedule_native's case


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (message -> receiver, int64; R). Seeded; built once."""
    rng = np.random.default_rng(97)
    out = {"known": (np.array(KNOWN[0], dtype=np.int64), KNOWN[1]),
           "no_rows": (np.zeros(0, dtype=np.int64), 0),
           "no_messages": (np.zeros(0, dtype=np.int64), 5),
           "one_bucket": (np.arange(3 * 65, dtype=np.int64) % 65, 65)}
    stairs = np.repeat(np.arange(130, dtype=np.int64), np.arange(130))
    out["staircase"] = (rng.permutation(stairs), 130)
    for R in (63, 64, 65):
        for d in (63, 64, 65):
            out["wave_%d_%d" % (R, d)] = (rng.permutation(np.tile(np.arange(R, dtype=np.int64), d)),
                                          R)
    deg = rng.integers(0, 4, 70)
    deg[[5, 17, 40, 69]] = [CHUNK, CHUNK + 1, 2 * CHUNK, 1500]
    out["chunk_edges"] = (rng.permutation(np.repeat(np.arange(70, dtype=np.int64), deg)), 70)
    out["skewed"] = (np.floor(2000 * rng.random(20000) ** 3).astype(np.int64), 2000)
    return out


def restate(recv, R):
    """The contract in numpy: rows by (degree, id) through a stable argsort,
    then every listed row's messages in message order."""
    recv = np.asarray(recv, dtype=np.int64)
    deg = np.bincount(recv, minlength=R)[:R] if R else np.zeros(0, dtype=np.int64)
    order = np.argsort(deg, kind="stable")
    zero_nodes = order[deg[order] == 0]
    nodes = order[deg[order] > 0]
    bucket_deg = np.unique(deg[nodes])
    node_ptr = np.append(np.searchsorted(deg[nodes], bucket_deg), nodes.size)
    by_row = np.argsort(recv, kind="stable")
    start = np.concatenate([[0], np.cumsum(deg)])
    lists = [by_row[start[v]:start[v + 1]] for v in nodes]
    merge_inv = np.empty(R, dtype=np.int64)
    merge_inv[np.concatenate([nodes, zero_nodes]).astype(np.int64)] = np.arange(R)
    return {"bucket_deg": bucket_deg.astype(np.int64), "bucket_node_ptr": node_ptr.astype(np.int64),
            "nodes": nodes.astype(np.int64), "zero_nodes": zero_nodes.astype(np.int64),
            "msg_ids": (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int64),
            "merge_inv": merge_inv}


def host_schedule(recv, R):
    """dglhip_degree_bucketing_host's arrays, cut to their true sizes."""
    recv = torch.as_tensor(np.asarray(recv, dtype=np.int64))
    M = recv.numel()
    nb = ctypes.c_int64()
    bdeg = torch.empty(max(R, 1), dtype=torch.int64)
    bptr = torch.empty(R + 1, dtype=torch.int64)
    nodes = torch.empty(max(R, 1), dtype=torch.int64)
    mids = torch.empty(max(M, 1), dtype=torch.int64)
    check_call(LIB.dglhip_degree_bucketing_host(M, ptr(recv), R, ctypes.byref(nb), ptr(bdeg),
                                                ptr(bptr), ptr(nodes), ptr(mids)))
    n = nb.value
    listed = int(bptr[n])
    return {"bucket_deg": bdeg[:n].numpy(), "bucket_node_ptr": bptr[:n + 1].numpy(),
            "nodes": nodes[:listed].numpy(), "msg_ids": mids[:M].numpy()}


def test_symbols_declared_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dgl_hip.h")) as f:
        header = f.read()
    for name in ("dglhip_degree_buckets_workspace_bytes", "dglhip_degree_buckets_count_device",
                 "dglhip_degree_buckets_fill_device"):
        assert name + "(" in header
        assert getattr(LIB, name).argtypes is not None
    assert "#define DGLHIP_BUCKET_CHUNK %d" % CHUNK in header
    assert kernel.BUCKET_CHUNK == CHUNK
    assert callable(kernel.degree_buckets) and callable(kernel.degree_buckets_count)
    assert callable(kernel.degree_buckets_fill)
    assert set(degree_bucketing.route_counts()) == {"host", "device", "device_builds"}


def test_argument_checks_need_no_device():
    assert LIB.dglhip_degree_buckets_workspace_bytes(-1, 0) == -1
    assert LIB.dglhip_degree_buckets_workspace_bytes(3, -2) == -1
    assert "negative size" in LIB.DGLGetLastError().decode()
    assert LIB.dglhip_degree_buckets_workspace_bytes(1 << 31, 0) == -1


def test_restatement_reproduces_the_known_answer():
    r = restate(*KNOWN)
    assert r["bucket_deg"].tolist() == [1, 2, 3]
    assert r["bucket_node_ptr"].tolist() == [0, 2, 3, 4]
    assert r["nodes"].tolist() == [0, 4, 1, 3]
    assert r["msg_ids"].tolist() == [3, 6, 1, 5, 0, 2, 4]
    assert r["zero_nodes"].tolist() == [2, 5]
    assert r["merge_inv"].tolist() == [0, 2, 4, 3, 1, 5]


def test_case_list_is_what_it_says():
    c = cases()
    assert len(c) == 16
    deg = {k: np.bincount(v[0], minlength=v[1]) for k, v in c.items()}
    assert sorted(deg["staircase"].tolist()) == list(range(130))
    assert not np.array_equal(c["staircase"][0], np.sort(c["staircase"][0]))
    assert set(deg["one_bucket"].tolist()) == {3}
    for R in (63, 64, 65):
        for d in (63, 64, 65):
            assert deg["wave_%d_%d" % (R, d)].tolist() == [d] * R
    ce = deg["chunk_edges"]
    assert {CHUNK, CHUNK + 1, 2 * CHUNK, 1500} <= set(ce.tolist()) and (ce == 0).any()
    assert int((ce > 3).sum()) == 4
    sk = deg["skewed"]
    assert c["skewed"][0].size == 20000 and sk.max() > CHUNK and (sk == 0).any()
    assert len(set(sk.tolist())) > 30  # many buckets


def test_restatement_equals_host_function_on_every_case():
    for name, (recv, R) in cases().items():
        want, got = host_schedule(recv, R), restate(recv, R)
        for key, val in want.items():
            assert np.array_equal(got[key], val), (name, key)
        both = np.concatenate([got["nodes"], got["zero_nodes"]])
        assert np.array_equal(np.sort(both), np.arange(R)), name
        assert np.array_equal(got["merge_inv"][both], np.arange(R)), name


def _graph(n, src, dst, h):
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src, dst)
    g.ndata["h"] = h
    return g


def _seven(shape, dtype, ctx, id_range):
    return torch.full(shape, 7, dtype=dtype, device=ctx)


def _position_weighted(nodes):
    m = nodes.mailbox["m"]
    w = torch.arange(m.shape[1], dtype=m.dtype, device=m.device)
    return {"o": (m * w[None, :, None]).sum(1)}


def test_cpu_messages_take_the_host_route_with_the_same_results():
    rng = np.random.default_rng(5)
    n, m, F = 200, 1500, 3
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n - 15, m)  # 15 nodes without in-edges
    dst[:300] = 11  # a hub
    h = torch.from_numpy(rng.integers(-4, 5, (n, F)).astype(np.float32))
    g = _graph(n, src, dst, h)
    g.set_n_initializer(_seven)
    before = degree_bucketing.route_counts()
    g.update_all(lambda e: {"m": e.src["h"]}, _position_weighted)
    after = degree_bucketing.route_counts()
    assert after["host"] == before["host"] + 1
    assert after["device"] == before["device"]
    assert after["device_builds"] == before["device_builds"]
    # per node: its in-edges in edge-id order, weighted by their position
    want = torch.full((n, F), 7, dtype=torch.float32)
    for v in range(n):
        mail = h[src[dst == v]]
        if len(mail):
            want[v] = (mail * torch.arange(len(mail), dtype=torch.float32)[:, None]).sum(0)
    assert torch.equal(g.ndata["o"], want)
    # a partial call: the rows of the receivers alone
    eids = torch.from_numpy(rng.choice(m, 400, replace=False))
    g.ndata["o"] = torch.zeros(n, F)
    g.send_and_recv(eids, lambda e: {"m": e.src["h"]}, _position_weighted)
    want = torch.zeros(n, F)
    e = eids.numpy()
    for v in np.unique(dst[e]):
        mail = h[src[e[dst[e] == v]]]
        want[v] = (mail * torch.arange(len(mail), dtype=torch.float32)[:, None]).sum(0)
    assert torch.equal(g.ndata["o"], want)
    assert degree_bucketing.route_counts()["host"] == before["host"] + 2


def test_node_batch_takes_its_ids_lazily():
    ids = torch.tensor([4, 9, 2])
    calls = []

    def give():
        calls.append(1)
        return ids.clone()

    eager = NodeBatch(None, ids, {})
    lazy = NodeBatch(None, give, {}, batch_size=3)
    assert lazy.batch_size() == 3 and len(lazy) == 3 and not calls
    assert eager.batch_size() == 3 and len(eager) == 3
    assert torch.equal(lazy.nodes(), eager.nodes()) and len(calls) == 1
    assert torch.equal(lazy.nodes(), ids) and len(calls) == 1
    assert lazy.nodes() is lazy.nodes()
