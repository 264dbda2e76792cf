"""The device route of DGLGraph.subgraph (node ids given as a cuda tensor,
csrc/induced_subgraph.hip) pinned against the host route (the native index):
the same edges in the same order with the same ids, exactly.

Every error case here is rejected by the kernels' validation before any
dependent access: an invalid id is counted, never used as an index."""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import _ffi, kernel
from dgl.base import DGLError
from dgl.kernel import SUBGRAPH_CHUNK

pytestmark = pytest.mark.gpu

N = 300
HUB = 7
HUB_DEG = 4 * SUBGRAPH_CHUNK + 37  # more than four items, the last one partial
NO_OUT = list(range(N - 25, N))    # 25 nodes without out-edges
F = 8


class Case(object):
    """The parent graph (built once) and the selections."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        others = max(4000 - HUB_DEG, 1500)  # about 4,000 edges at a chunk of 512 slots
        srcs = np.setdiff1d(np.arange(N - 25), [HUB])
        src = rng.choice(srcs, others)
        dst = rng.integers(0, N, others)
        # duplicate edges and self loops, on purpose
        src[:40] = src[40:80]
        dst[:40] = dst[40:80]
        dst[100:130] = src[100:130]
        src = np.concatenate([src, np.full(HUB_DEG, HUB)])
        dst = np.concatenate([dst, rng.integers(0, N, HUB_DEG)])
        # edges are added source-major, so the identity selection gives the
        # parent's own edge order back
        order = np.argsort(src, kind="stable")
        self.src, self.dst = src[order], dst[order]
        self.E = self.src.size
        g = dgl.DGLGraph(multigraph=True)
        g.add_nodes(N)
        g.add_edges(self.src, self.dst)
        self.g = g
        deg = np.bincount(self.src, minlength=N)
        assert deg[HUB] > 4 * SUBGRAPH_CHUNK and int((deg == 0).sum()) >= 20
        assert int((self.src == self.dst).sum()) >= 30
        rest = np.setdiff1d(np.arange(N), [HUB])
        with_hub = np.concatenate([[HUB], rng.choice(rest, 119, replace=False)])
        rng.shuffle(with_hub)
        no_hub = with_hub[with_hub != HUB]
        hub_targets = np.unique(self.dst[self.src == HUB])
        assert np.isin(no_hub, hub_targets).sum() > 60
        self.sels = {
            "with_hub": with_hub,
            "without_hub": no_hub,
            "single": self.src[self.src == self.dst][:1].copy(),  # a node with a self loop
            "empty": np.zeros(0, dtype=np.int64),
            "no_internal_edges": np.array(NO_OUT[::-1]),
            "permutation": rng.permutation(N),
            "identity": np.arange(N),
        }
        self._host = {}

    def host(self, name):
        """The host-route subgraph of a selection (computed once, left as it is)."""
        if name not in self._host:
            self._host[name] = self.g.subgraph(self.sels[name].tolist())
        return self._host[name]

    def device(self, name):
        return self.g.subgraph(torch.from_numpy(self.sels[name]).cuda())


@pytest.fixture(scope="module")
def case():
    return Case()


def same_subgraph(a, b):
    for x, y in zip(a.edges(), b.edges()):
        assert torch.equal(x.cpu(), y.cpu())
    assert torch.equal(a.parent_nid.cpu(), b.parent_nid.cpu())
    assert torch.equal(a.parent_eid.cpu(), b.parent_eid.cpu())
    assert a.number_of_nodes() == b.number_of_nodes()
    assert a.number_of_edges() == b.number_of_edges()


SELECTIONS = ["with_hub", "without_hub", "single", "empty", "no_internal_edges", "permutation",
              "identity"]


@pytest.mark.parametrize("name", SELECTIONS)
def test_device_route_equals_host_route(case, name):
    dev, host = case.device(name), case.host(name)
    assert dev.parent_nid.is_cuda and dev.parent_eid.is_cuda
    assert not dev._graph.has_native_index
    assert dev.number_of_edges() == host.number_of_edges()  # known before any download
    same_subgraph(dev, host)
    assert dev._graph.has_native_index  # edges() asked for it
    if name == "identity":
        assert torch.equal(dev.parent_eid.cpu(), torch.arange(case.E))
        assert torch.equal(dev.edges()[0], torch.from_numpy(case.src))
        assert torch.equal(dev.edges()[1], torch.from_numpy(case.dst))
    if name in ("empty", "no_internal_edges"):
        assert dev.number_of_edges() == 0
    if name == "with_hub":
        assert dev.number_of_edges() > SUBGRAPH_CHUNK


def test_device_route_is_deterministic(case):
    a, b = case.device("permutation"), case.device("permutation")
    assert torch.equal(a.parent_eid, b.parent_eid)
    assert torch.equal(a._graph._dev_coo[0], b._graph._dev_coo[0])
    assert torch.equal(a._graph._dev_coo[1], b._graph._dev_coo[1])


def _message_passing(sg, h0, w0, grad, mfunc):
    h = h0.clone().requires_grad_()
    w = w0.clone().requires_grad_()
    sg.ndata["h"] = h
    sg.edata["w"] = w
    sg.update_all(mfunc, fn.sum("m", "o"))
    out = sg.ndata["o"]
    out.backward(grad)
    return out.detach(), h.grad, w.grad


@pytest.mark.parametrize("msg", ["copy_src", "src_mul_edge"])
def test_message_passing_matches_the_host_route_bit_for_bit(case, msg):
    dev, host = case.device("with_hub"), case.g.subgraph(case.sels["with_hub"].tolist())
    n, m = host.number_of_nodes(), host.number_of_edges()
    gen = torch.Generator().manual_seed(5)
    h0 = torch.randn(n, F, generator=gen).cuda()
    w0 = torch.randn(m, F, generator=gen).cuda()
    grad = torch.randn(n, F, generator=gen).cuda()
    mfunc = fn.copy_src("h", "m") if msg == "copy_src" else fn.src_mul_edge("h", "w", "m")
    got = _message_passing(dev, h0, w0, grad, mfunc)
    want = _message_passing(host, h0, w0, grad, mfunc)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if msg == "src_mul_edge":
        assert torch.equal(got[2], want[2])
    else:
        assert got[2] is None and want[2] is None
    assert got[0].abs().sum() > 0
    # whole-graph message passing on the device never asked for the native index
    assert not dev._graph.has_native_index
    deg = dev.in_degrees()
    assert dev._graph.has_native_index
    assert torch.equal(deg, host.in_degrees())
    assert torch.equal(dev.out_degrees(), host.out_degrees())


def test_copy_from_parent_gathers_on_the_device(case):
    g = case.g
    g.ndata["x"] = torch.arange(N * 2, dtype=torch.float32).reshape(N, 2).cuda()
    g.edata["y"] = torch.arange(case.E, dtype=torch.float32).reshape(case.E, 1).cuda()
    try:
        dev, host = case.device("without_hub"), case.host("without_hub")
        dev.copy_from_parent()
        assert dev.ndata["x"].is_cuda and dev.edata["y"].is_cuda
        assert not dev._graph.has_native_index
        assert torch.equal(dev.ndata["x"].cpu(), g.ndata["x"].cpu()[host.parent_nid])
        assert torch.equal(dev.edata["y"].cpu(), g.edata["y"].cpu()[host.parent_eid])
        assert dev.map_to_subgraph_nid(host.parent_nid[:5]).tolist() == [0, 1, 2, 3, 4]
    finally:
        g.pop_n_repr("x")
        g.pop_e_repr("y")


@pytest.mark.parametrize("bad", ["too_large", "negative", "duplicate"])
def test_invalid_ids_raise_and_leave_no_trace(case, bad):
    sel = case.sels["without_hub"].copy()
    if bad == "too_large":
        sel[17] = N
    elif bad == "negative":
        sel[3] = -1
    else:
        sel[50] = sel[2]
    with pytest.raises(DGLError, match="%d nodes" % N if bad != "duplicate" else "distinct"):
        case.g.subgraph(torch.from_numpy(sel).cuda())
    # the next valid call on the same parent is still right (a membership map
    # left dirty would show here)
    same_subgraph(case.device("with_hub"), case.host("with_hub"))
    same_subgraph(case.device("without_hub"), case.host("without_hub"))


def test_capture_is_refused_before_anything_is_launched(case):
    sel = torch.from_numpy(case.sels["single"]).cuda()
    case.g.subgraph(sel)  # warm: the parent's adjacency is cached
    x = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x.add_(1.0)
            with pytest.raises(DGLError, match="captured"):
                case.g.subgraph(sel)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 4  # the capture holds the one add, nothing else
    same_subgraph(case.device("single"), case.host("single"))


def test_filter_nodes_then_subgraph_stays_on_the_device(case):
    g = case.g
    rng = np.random.default_rng(77)
    mask = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    g.ndata["m"] = mask.cuda()
    try:
        ids = g.filter_nodes(lambda nodes: nodes.data["m"] > 0)
        assert ids.is_cuda
        dev = g.subgraph(ids)
        assert dev.parent_nid.is_cuda and not dev._graph.has_native_index
        g.ndata["m"] = mask
        host_ids = g.filter_nodes(lambda nodes: nodes.data["m"] > 0)
        assert not host_ids.is_cuda and torch.equal(ids.cpu(), host_ids)
        same_subgraph(dev, g.subgraph(host_ids))
    finally:
        g.pop_n_repr("m")


def test_readonly_parent_takes_the_native_index(case):
    g = dgl.DGLGraph((case.src, case.dst), multigraph=True, readonly=True)
    sel = np.sort(case.sels["with_hub"])
    dev = g.subgraph(torch.from_numpy(sel).cuda())
    host = g.subgraph(sel.tolist())
    assert dev._graph.has_native_index and dev.is_readonly and not dev.parent_nid.is_cuda
    same_subgraph(dev, host)
    with pytest.raises(DGLError, match="has to be sorted"):
        g.subgraph(torch.from_numpy(case.sels["with_hub"]).cuda())


def test_c_abi_entry_points(case):
    """dglhip_induced_subgraph_* called directly: the status and the three
    arrays on the hub selection; the counters on a selection with bad ids."""
    LIB, ptr = _ffi.LIB, _ffi.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    csr = case.g._graph.adjacency(dev).bwd
    assert csr.num_rows == N and csr.nnz == case.E
    stream = torch.cuda.current_stream(dev).cuda_stream

    def count(sel):
        nbytes = LIB.dglhip_induced_subgraph_workspace_bytes(N, sel.numel(), csr.nnz)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        status = torch.full((4,), -1, dtype=torch.int64, device=dev)
        _ffi.check_call(LIB.dglhip_induced_subgraph_count_device(
            N, sel.numel(), csr.nnz, ptr(csr.indptr), ptr(csr.indices), ptr(sel), ptr(ws), nbytes,
            ptr(status), stream))
        return ws, nbytes, status.tolist()

    sel = torch.from_numpy(case.sels["with_hub"]).to(dev)
    host = case.host("with_hub")
    ws, nbytes, (m, invalid, dup, items) = count(sel)
    assert (m, invalid, dup) == (host.number_of_edges(), 0, 0)
    deg = np.bincount(case.src, minlength=N)[case.sels["with_hub"]]
    assert items == int(((deg + SUBGRAPH_CHUNK - 1) // SUBGRAPH_CHUNK).sum())
    out = torch.full((3, m), -1, dtype=torch.int64, device=dev)
    _ffi.check_call(LIB.dglhip_induced_subgraph_fill_device(
        N, sel.numel(), csr.nnz, ptr(csr.indptr), ptr(csr.indices), ptr(csr.eid), ptr(sel),
        ptr(ws), nbytes, items, m, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream))
    u, v = host.edges()
    assert torch.equal(out[0].cpu(), u) and torch.equal(out[1].cpu(), v)
    assert torch.equal(out[2].cpu(), host.parent_eid)

    bad = sel.clone()
    bad[0], bad[1], bad[9] = N + 5, -3, bad[8]
    _, _, (_, invalid, dup, _) = count(bad)
    assert (invalid, dup) == (2, 1)
    # a workspace that is too small is refused, not overrun
    assert LIB.dglhip_induced_subgraph_count_device(
        N, sel.numel(), csr.nnz, ptr(csr.indptr), ptr(csr.indices), ptr(sel), ptr(ws), 16,
        ptr(out), stream) == -1
    assert b"workspace" in LIB.DGLGetLastError()
    assert kernel.SUBGRAPH_CHUNK == SUBGRAPH_CHUNK


def test_rows_at_exact_multiples_of_the_chunk():
    """Rows of out-degree 0, 1, K - 1, K, K + 1 and 2K: a row of exactly
    deg / K whole items and no partial one, followed by rows without items.
    Isolated nodes lie between the rows and at both ends of the id range, so
    the item search skips empty positions everywhere."""
    K = SUBGRAPH_CHUNK
    degs = [0, 1, K - 1, K, K + 1, 2 * K]
    rows = 1 + 2 * np.arange(len(degs))  # odd ids; the even ids between them are isolated
    first = 2 * len(degs) + 1            # the targets are first .. first + 2K - 1
    n = first + 2 * K + 1                # node 0 and node n - 1 are isolated
    src = np.concatenate([np.full(d, r) for r, d in zip(rows, degs)])
    dst = np.concatenate([first + np.arange(d) for d in degs])
    assert n == 2 * K + 14 and src.size == 5 * K + 1
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src, dst)
    # without the row of K + 1 slots and every third target
    fewer = np.setdiff1d(np.arange(n), np.concatenate([rows[4:5], first + np.arange(0, 2 * K, 3)]))
    for sel in (np.arange(n), fewer, fewer[::-1].copy()):
        dev = g.subgraph(torch.from_numpy(sel).cuda())
        same_subgraph(dev, g.subgraph(sel.tolist()))
    assert dev.number_of_edges() > K
    csr = g._graph.adjacency(torch.device("cuda", torch.cuda.current_device())).bwd
    _, (m, invalid, dup, items) = kernel.induced_subgraph_count(csr, torch.arange(n).cuda())
    assert (m, invalid, dup, items) == (src.size, 0, 0, 0 + 1 + 1 + 1 + 2 + 2)
