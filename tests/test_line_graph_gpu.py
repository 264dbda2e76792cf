"""The device route of DGLGraph.line_graph (ctx = a ROCm device,
csrc/line_graph.hip) pinned three ways: device == host route == the plain
Python checker of test_transform.py, the edges exactly and in order.

Every bad value given to the C-ABI here is bounded by the kernels before any
dependent access: an invalid endpoint is counted, never used as an index."""
import os
import re

import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import _ffi, kernel
from dgl.base import DGLError
from test_transform import N, build, check_line_graph, random_multigraph

pytestmark = pytest.mark.gpu

TILE = kernel.LINE_GRAPH_TILE
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "include", "dgl_hip.h")


def edges_of(L):
    u, v = L.edges()
    return u.cpu(), v.cpu()


def three_way(n, src, dst, backtracking):
    """Device == host == checker on the graph (src, dst); returns the device
    line graph and the number of its edges."""
    g = build(n, src, dst)
    dev = g.line_graph(backtracking=backtracking, ctx="cuda")
    host = g.line_graph(backtracking=backtracking)
    ws, wd = check_line_graph(list(map(int, src)), list(map(int, dst)), backtracking)
    want = (torch.tensor(ws, dtype=torch.int64), torch.tensor(wd, dtype=torch.int64))
    assert dev.number_of_nodes() == host.number_of_nodes() == len(src)
    assert dev.number_of_edges() == host.number_of_edges() == len(ws)
    assert not dev.is_multigraph and not dev.is_readonly
    du, dv = edges_of(dev)
    hu, hv = edges_of(host)
    assert torch.equal(du, hu) and torch.equal(dv, hv)
    assert torch.equal(hu, want[0]) and torch.equal(hv, want[1])
    return dev, len(ws)


def boundary_graph(d):
    """Edge 0 -> 1, then d out-edges of node 1: every third goes back to node
    0, the others to sinks of their own."""
    src, dst = [0], [1]
    back = 0
    for j in range(d):
        src.append(1)
        if j % 3 == 0:
            dst.append(0)
            back += 1
        else:
            dst.append(2 + j)
    return d + 2, src, dst, back


def test_tile_matches_the_header():
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+DGLHIP_LINE_GRAPH_TILE\s+(\d+)", text).group(1)) == TILE
    assert TILE % 64 == 0


@pytest.mark.parametrize("d", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_boundary_family(d):
    n, src, dst, back = boundary_graph(d)
    # candidates: the d slots of row 1 after edge 0, one slot of row 0 after
    # every back edge
    _, m = three_way(n, src, dst, True)
    assert m == d + back
    # without backtracking exactly the pairs through 0->1->0 and 1->0->1 go
    _, m_nb = three_way(n, src, dst, False)
    assert m_nb == d + back - 2 * back


@pytest.fixture(scope="module")
def multigraph():
    src, dst = random_multigraph(TILE)
    return src, dst


def test_random_multigraph(multigraph):
    src, dst = multigraph
    outdeg, indeg = np.bincount(src, minlength=N), np.bincount(dst, minlength=N)
    _, m = three_way(N, src, dst, True)
    assert m == int((indeg * outdeg).sum()) and m > 16 * TILE
    _, m_nb = three_way(N, src, dst, False)
    assert m - m_nb > 0  # pairs removed


@pytest.mark.parametrize("backtracking", [True, False])
def test_degenerate_graphs(backtracking):
    dev, m = three_way(5, [], [], backtracking)  # no edges
    assert m == 0 and dev.number_of_nodes() == 0
    _, m = three_way(6, [0, 1, 2, 0], [3, 4, 5, 5], backtracking)  # every edge into a sink
    assert m == 0
    _, m = three_way(1, [0], [0], backtracking)  # one self loop
    assert m == (1 if backtracking else 0)


def test_line_graph_stays_on_the_device(multigraph):
    src, dst = multigraph
    g = build(N, src, dst)
    rng = np.random.default_rng(3)
    h = torch.from_numpy(rng.standard_normal((src.size, 8)).astype(np.float32)).cuda()
    g.edata["h"] = h
    L = g.line_graph(backtracking=False, shared=True, ctx="cuda")
    assert L._node_frame is g._edge_frame
    assert not L._graph.has_native_index
    host = g.line_graph(backtracking=False)
    assert L.number_of_nodes() == src.size
    assert L.number_of_edges() == host.number_of_edges()
    L.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
    host.ndata["h"] = h
    host.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
    assert L.ndata["o"].is_cuda and host.ndata["o"].is_cuda
    # the same ORDER_EID adjacency, so the same summation order: bit for bit
    assert torch.equal(L.ndata["o"].view(torch.int32), host.ndata["o"].view(torch.int32))
    assert torch.equal(g.edata["o"], L.ndata["o"])  # the shared frame
    assert not L._graph.has_native_index
    u, v = L.edges()
    assert L._graph.has_native_index
    hu, hv = host.edges()
    assert torch.equal(u.cpu(), hu.cpu()) and torch.equal(v.cpu(), hv.cpu())
    g.pop_e_repr("o")


def test_device_line_graph_can_be_mutated():
    g = build(3, [0, 1, 1], [1, 2, 0])
    L = g.line_graph(ctx="cuda")
    assert not L._graph.has_native_index
    L.add_nodes(1)
    assert L._graph.has_native_index and L._graph._dev_coo is None
    L.add_edge(3, 0)
    u, v = edges_of(L)
    assert (u.tolist(), v.tolist()) == ([0, 0, 2, 3], [1, 2, 0, 0])
    adj = L.sparse_adjacency("cuda")
    assert adj.fwd.nnz == 4 and adj.shape == (4, 4)


@pytest.mark.parametrize("backtracking", [True, False])
def test_two_constructions_are_identical(multigraph, backtracking):
    src, dst = multigraph
    g = build(N, src, dst)
    a = g._graph.line_graph_device("cuda", backtracking)
    b = g._graph.line_graph_device("cuda", backtracking)
    assert a._dev_coo[0].is_cuda and a._dev_coo[0].data_ptr() != b._dev_coo[0].data_ptr()
    assert torch.equal(a._dev_coo[0], b._dev_coo[0]) and torch.equal(a._dev_coo[1], b._dev_coo[1])


def test_line_graph_of_a_device_line_graph():
    rng = np.random.default_rng(11)
    src, dst = rng.integers(0, 40, 160), rng.integers(0, 40, 160)
    g = build(40, src, dst)
    L1 = g.line_graph(backtracking=False, ctx="cuda")
    L2 = L1.line_graph(backtracking=False, ctx="cuda")  # from L1's device edge list
    assert not L1._graph.has_native_index and not L2._graph.has_native_index
    H2 = g.line_graph(backtracking=False).line_graph(backtracking=False)
    assert L2.number_of_nodes() == H2.number_of_nodes() == L1.number_of_edges()
    assert L2.number_of_edges() > TILE
    du, dv = edges_of(L2)
    hu, hv = edges_of(H2)
    assert torch.equal(du, hu) and torch.equal(dv, hv)


def test_readonly_parent_raises_on_the_device_route():
    g = dgl.DGLGraph(([0, 1], [1, 0]), readonly=True)
    with pytest.raises(DGLError, match="immutable"):
        g.line_graph(ctx="cuda")


def test_c_abi_entry_points(multigraph):
    """dglhip_line_graph_* called directly: the status and both arrays; the
    invalid counter on a `dst` with two bad entries; a short workspace."""
    src, dst = multigraph
    LIB, ptr = _ffi.LIB, _ffi.ptr
    dev = torch.device("cuda", torch.cuda.current_device())
    g = build(N, src, dst)
    csr = g._graph.adjacency(dev).bwd
    E = src.size
    assert csr.num_rows == N and csr.nnz == E
    stream = torch.cuda.current_stream(dev).cuda_stream
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    nbytes = LIB.dglhip_line_graph_workspace_bytes(N, E)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def count(t, backtracking):
        status = torch.full((4,), -1, dtype=torch.int64, device=dev)
        _ffi.check_call(LIB.dglhip_line_graph_count_device(
            N, E, ptr(s), ptr(t), ptr(csr.indptr), ptr(csr.indices), backtracking, ptr(ws), nbytes,
            ptr(status), stream))
        return status.tolist()

    outdeg, indeg = np.bincount(src, minlength=N), np.bincount(dst, minlength=N)
    K = int((indeg * outdeg).sum())
    for backtracking in (1, 0):
        want = check_line_graph(src.tolist(), dst.tolist(), bool(backtracking))
        m, k, invalid, units = count(t, backtracking)
        assert (m, k, invalid, units) == (len(want[0]), K, 0, (K + TILE - 1) // TILE)
        out = torch.full((2, m), -1, dtype=torch.int64, device=dev)
        _ffi.check_call(LIB.dglhip_line_graph_fill_device(
            N, E, ptr(s), ptr(t), ptr(csr.indptr), ptr(csr.indices), ptr(csr.eid), backtracking,
            ptr(ws), nbytes, units, m, ptr(out[0]), ptr(out[1]), stream))
        assert out[0].tolist() == want[0] and out[1].tolist() == want[1]

    # a destination of N and one of -1 are counted and never followed: the
    # call returns normally and the rest of the graph is still counted
    bad = t.clone()
    first_live = int(np.flatnonzero(outdeg[dst] > 0)[0])
    bad[first_live], bad[E - 1] = N, -1
    m, k, invalid, _ = count(bad, 1)
    assert invalid == 2
    assert m == k == K - int(outdeg[dst[first_live]]) - int(outdeg[dst[E - 1]])
    with pytest.raises(DGLError, match="Invalid vertex"):
        kernel.line_graph(csr, s, bad, True)
    # a workspace that is too small is refused, not overrun
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    assert LIB.dglhip_line_graph_count_device(
        N, E, ptr(s), ptr(t), ptr(csr.indptr), ptr(csr.indices), 1, ptr(ws), 16, ptr(status),
        stream) == -1
    assert b"workspace" in LIB.DGLGetLastError()
    # sizes past 32 bits are refused with a message
    assert LIB.dglhip_line_graph_workspace_bytes(1 << 31, 8) == -1
    assert b"2^31" in LIB.DGLGetLastError()


def test_capture_is_refused_before_anything_is_launched():
    g = build(3, [0, 1, 1], [1, 2, 0])
    g.line_graph(ctx="cuda")  # warm: the parent's adjacency is cached
    x = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x.add_(1.0)
            with pytest.raises(DGLError, match="captured"):
                g.line_graph(ctx="cuda")
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 4  # the capture holds the one add, nothing else
    u, v = edges_of(g.line_graph(ctx="cuda"))
    assert (u.tolist(), v.tolist()) == ([0, 0, 2], [1, 2, 0])


def test_memory_guard_names_the_size(monkeypatch, multigraph):
    src, dst = multigraph
    g = build(N, src, dst)
    m = g.line_graph().number_of_edges()
    g._graph.adjacency("cuda").bwd  # built before free memory is misreported
    monkeypatch.setattr(kernel.torch.cuda, "mem_get_info",
                        lambda device=None: (1024, 1 << 30))
    with pytest.raises(DGLError) as err:
        g.line_graph(ctx="cuda")
    assert "M = %d" % m in str(err.value) and "%d bytes" % (16 * m) in str(err.value)
