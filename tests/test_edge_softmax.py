"""kernel.edge_softmax and dgl.nn.pytorch.edge_softmax: the softmax of edge
scores over the in-edges (norm_by="dst") or out-edges ("src") of every node.

The reference is float64, computed here from the same float32 inputs with
plain torch indexing (one torch.softmax per node's edge list), its gradient by
float64 autograd. Inputs are standard_normal * exp(standard_normal) clipped to
[-8, 8], so |x - max| <= 16: the rounding of x - m alone puts |x - m| * 2^-24
into each exponential, and the clip is part of what the bounds mean.

  forward   |y - y64| <= 1e-5 * y64 per element (the project's fp32 bound; a
            float32 model of one sequential chain per row stays at 3.2e-6)
  backward  |dx - dx64| <= 1e-5 * (|y64 dy| + y64 sum_j |y64_j dy_j|), the
            sum-of-|terms| form of the segment-reduce and GAT tests

The graph has about 40 destinations whose in-degrees sit on every path of the
kernel: 0, 1, 2, 3, 63, 64, 65, 257 and C - 1, C, C + 1, 2 C + 3 around
kernel.EDGE_SOFTMAX_CHUNK, with duplicate edges and self-loops, in three edge
numberings (destination-major: the kernel's form without edge ids;
source-major; shuffled)."""
import functools

import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import kernel
from dgl.base import DGLError
from dgl.nn.pytorch import edge_softmax

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
C = kernel.EDGE_SOFTMAX_CHUNK
SHORT_DEGREES = (0, 1, 2, 3, 63, 64, 65, 257)
LONG_DEGREES = (C - 1, C, C + 1, 2 * C + 3)
NUMBERINGS = ("dst_major", "src_major", "shuffled")
FULL_H = (1, 3, 8, 65)
SHORT_H = (2, 16, 17, 64)
N = 40


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


@functools.lru_cache(maxsize=None)
def _edges(full, numbering):
    """(src, dst) int64 arrays over N nodes, in the numbering's edge-id order.
    The listed in-degrees, the other nodes with 0 to 5 in-edges; node 4 has a
    self-loop and its first edge twice."""
    rng = np.random.default_rng(7)
    degs = list(SHORT_DEGREES) + (list(LONG_DEGREES) if full else [])
    degs += [int(d) for d in rng.integers(0, 6, N - len(degs))]
    order = rng.permutation(N)  # which node gets which degree
    dst = np.concatenate([np.full(d, order[i], dtype=np.int64) for i, d in enumerate(degs)])
    src = rng.integers(0, N, dst.size).astype(np.int64)
    v = int(order[4])  # in-degree 63
    at = np.flatnonzero(dst == v)
    src[at[0]] = v  # a self-loop
    src[at[2]] = src[at[1]]  # a duplicate edge
    if numbering == "dst_major":
        key = np.argsort(dst, kind="stable")
    elif numbering == "src_major":
        key = np.argsort(src, kind="stable")
    else:
        key = rng.permutation(dst.size)
    src, dst = src[key], dst[key]
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


@functools.lru_cache(maxsize=None)
def _adj(full, numbering):
    src, dst = _edges(full, numbering)
    return kernel.from_coo(N, N, torch.from_numpy(dst.copy()), torch.from_numpy(src.copy()))


@functools.lru_cache(maxsize=None)
def _inputs(E, H, seed=0):
    rng = np.random.default_rng(seed)
    x = np.clip(rng.standard_normal((E, H)) * np.exp(rng.standard_normal((E, H))), -8, 8)
    dy = rng.standard_normal((E, H)) * np.exp(rng.standard_normal((E, H)))
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(dy.astype(np.float32))


def _groups(ids, n):
    """The positions of each group 0..n-1 in ``ids`` (plain indexing)."""
    ids = torch.as_tensor(np.array(ids))
    return [torch.nonzero(ids == v).flatten() for v in range(n)]


def _softmax64(x, groups):
    """(y64, differentiable x64): one float64 torch.softmax per group."""
    x64 = x.detach().cpu().double().requires_grad_(True)
    y = torch.zeros_like(x64)
    for idx in groups:
        if idx.numel():
            y = y.index_put((idx,), torch.softmax(x64[idx], 0))
    return y, x64


@functools.lru_cache(maxsize=None)
def _reference(full, numbering, H, norm_by="dst"):
    """(x, dy, y64, dx64, bound of the backward) on the host, read only."""
    src, dst = _edges(full, numbering)
    x, dy = _inputs(dst.size, H)
    groups = _groups(dst if norm_by == "dst" else src, N)
    y64, x64 = _softmax64(x, groups)
    y64.backward(dy.double())
    yd = y64.detach()
    terms = (yd * dy.double()).abs()
    tot = torch.zeros_like(yd)
    for idx in groups:
        if idx.numel():
            tot[idx] = terms[idx].sum(0, keepdim=True)
    return x, dy, yd, x64.grad, terms + yd * tot


def _check_fwd(y, y64, what=""):
    err = (y.detach().cpu().double() - y64).abs()
    bad = err > 1e-5 * y64
    worst = float((err / y64.clamp(min=1e-300)).max()) if y64.numel() else 0.0
    print("%s forward: worst |y - y64| / y64 = %.3g" % (what, worst))
    assert not bool(bad.any()), "%s: %d elements beyond 1e-5 * y64, worst %.3g" % (
        what, int(bad.sum()), worst)


def _check_bwd(dx, dx64, bound, what=""):
    err = (dx.detach().cpu().double() - dx64).abs()
    worst = float((err / bound.clamp(min=1e-300)).max()) if bound.numel() else 0.0
    print("%s backward: worst error / sum|terms| = %.3g" % (what, worst))
    assert bool((err <= 1e-5 * bound).all()), "%s: worst %.3g of the terms" % (what, worst)


def _leaf(t, dev):
    """A leaf of its own on ``dev`` (the inputs are shared between tests)."""
    return t.to(dev).clone().requires_grad_(True)


def _run(adj, x, dy, dev, **kw):
    xd = _leaf(x, dev)
    y = kernel.edge_softmax(adj, xd, **kw)
    y.backward(dy.to(dev))
    return y.detach(), xd.grad


CASES = [(True, H) for H in FULL_H] + [(False, H) for H in SHORT_H]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("full,H", CASES, ids=["H%d" % h for _, h in CASES])
def test_forward_backward_against_float64(device, numbering, full, H):
    dev = _dev(device)
    adj = _adj(full, numbering)
    assert (adj.fwd.slot_eid is None) == (numbering == "dst_major")
    x, dy, y64, dx64, bound = _reference(full, numbering, H)
    y, dx = _run(adj, x, dy, dev)
    assert y.shape == x.shape and dx.shape == x.shape
    _check_fwd(y, y64, "%s H=%d" % (numbering, H))
    _check_bwd(dx, dx64, bound, "%s H=%d" % (numbering, H))
    # degree-1 groups are exactly 1.0, every group sums to 1, the same bits again
    src, dst = _edges(full, numbering)
    deg = np.bincount(dst, minlength=N)
    single = torch.from_numpy(np.flatnonzero(deg[dst] == 1))
    assert single.numel() and bool((y.cpu()[single] == 1.0).all())
    sums = torch.zeros(N, H, dtype=torch.float64).index_add_(0, torch.from_numpy(dst.copy()),
                                                            y.cpu().double())
    assert float((sums[torch.from_numpy(deg > 0)] - 1).abs().max()) <= 1e-5
    y2, dx2 = _run(adj, x, dy, dev)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))
    assert torch.equal(dx.view(torch.int32), dx2.view(torch.int32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("H", [1, 8])
def test_norm_by_src(device, numbering, H):
    dev = _dev(device)
    x, dy, y64, dx64, bound = _reference(True, numbering, H, "src")
    y, dx = _run(_adj(True, numbering), x, dy, dev, norm_by="src")
    _check_fwd(y, y64, "src %s H=%d" % (numbering, H))
    _check_bwd(dx, dx64, bound, "src %s H=%d" % (numbering, H))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H", [1, 3, 8])
def test_slot_order(device, H):
    """edge_order="slot": values in and out in forward-CSR slot order."""
    dev = _dev(device)
    adj = _adj(True, "shuffled")
    x, dy, y64, dx64, bound = _reference(True, "shuffled", H)
    perm = kernel.slot_permutation(adj).cpu()
    y, dx = _run(adj, x[perm], dy[perm], dev, edge_order="slot")
    _check_fwd(y, y64[perm], "slot H=%d" % H)
    _check_bwd(dx, dx64[perm], bound[perm], "slot H=%d" % H)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("numbering", ["dst_major", "shuffled"])
def test_offset_and_transposed_views(device, numbering):
    """The vector-width gate: 8 columns from a storage that starts one float
    late (the scalar kernels), and a transposed input (copied, then aligned)."""
    dev = _dev(device)
    adj = _adj(True, numbering)
    x, dy, y64, dx64, bound = _reference(True, numbering, 8)
    E = x.shape[0]
    store = torch.zeros(E * 8 + 1, device=dev)
    store[1:] = x.to(dev).reshape(-1)
    view = store[1:].view(E, 8)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    gstore = torch.zeros(E * 8 + 1, device=dev)
    gstore[1:] = dy.to(dev).reshape(-1)
    xo = view.requires_grad_(True)
    y = kernel.edge_softmax(adj, xo)
    y.backward(gstore[1:].view(E, 8))
    _check_fwd(y, y64, "offset view")
    _check_bwd(xo.grad, dx64, bound, "offset view")
    xt = x.to(dev).t().contiguous().t()
    assert not xt.is_contiguous()
    xt.requires_grad_(True)
    yt = kernel.edge_softmax(adj, xt)
    yt.backward(dy.to(dev).t().contiguous().t())
    _check_fwd(yt, y64, "transposed")
    _check_bwd(xt.grad, dx64, bound, "transposed")


@pytest.mark.parametrize("device", DEVICES)
def test_trailing_shapes(device):
    dev = _dev(device)
    adj = _adj(False, "shuffled")
    x, dy, y64, _, _ = _reference(False, "shuffled", 16)
    E = x.shape[0]
    y = kernel.edge_softmax(adj, x.to(dev).view(E, 2, 8))
    assert y.shape == (E, 2, 8)
    _check_fwd(y.reshape(E, 16), y64, "(E, 2, 8)")
    x1, _, y1, _, _ = _reference(False, "shuffled", 1)
    y = kernel.edge_softmax(adj, x1.to(dev).view(E))
    assert y.shape == (E,)
    _check_fwd(y.view(E, 1), y1, "(E,)")


def _special_graph():
    """Six destinations, one group each of: a NaN, a +inf, a -inf beside finite
    values, only -inf, a -0.0, finite values."""
    sizes = [5, 4, 6, 3, 4, 7]
    dst = np.concatenate([np.full(s, i, dtype=np.int64) for i, s in enumerate(sizes)])
    rng = np.random.default_rng(3)
    src = rng.integers(0, 6, dst.size).astype(np.int64)
    x = rng.standard_normal((dst.size, 3)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    x[off[0] + 2, :] = np.nan
    x[off[1] + 1, :] = np.inf
    x[off[2] + 3, :] = -np.inf
    x[off[2] + 5, 1] = -np.inf
    x[off[3]:off[4], :] = -np.inf
    x[off[4] + 1, :] = -0.0
    return src, dst, off, torch.from_numpy(x)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shuffle", [False, True])
def test_special_values(device, shuffle):
    dev = _dev(device)
    src, dst, off, x = _special_graph()
    if shuffle:
        key = np.random.default_rng(5).permutation(dst.size)
        src, dst, x = src[key], dst[key], x[torch.from_numpy(key)]
    adj = kernel.from_coo(6, 6, torch.from_numpy(dst), torch.from_numpy(src))
    y = kernel.edge_softmax(adj, x.to(dev)).cpu()
    want = torch.zeros_like(x)
    for idx in _groups(dst, 6):
        want[idx] = torch.softmax(x[idx], 0)
    assert torch.equal(torch.isnan(y), torch.isnan(want))
    assert torch.equal(y == 0, want == 0)
    d = torch.from_numpy(dst)
    assert bool(torch.isnan(y[(d == 0) | (d == 1) | (d == 3)]).all())
    assert bool((y[d == 2][torch.isinf(x[d == 2])] == 0).all())
    fin = y[(d == 2) | (d == 4) | (d == 5)]
    assert bool(torch.isfinite(fin).all())
    ok = ~torch.isnan(want)
    assert bool(((y[ok] - want[ok]).abs() <= 1e-5 * want[ok]).all())


@pytest.mark.parametrize("device", DEVICES)
def test_special_values_in_a_long_row(device):
    """A row cut into pieces: a piece of only -inf beside finite pieces adds
    nothing, a NaN in one piece reaches the others' columns, a row of only
    -inf is NaN."""
    dev = _dev(device)
    L = 2 * C + 3
    dst = np.concatenate([np.zeros(L, np.int64), np.ones(L, np.int64), np.full(L, 2, np.int64)])
    src = np.zeros_like(dst)
    x = np.random.default_rng(4).standard_normal((3 * L, 2)).astype(np.float32)
    x[:C + 7, 0] = -np.inf  # the first piece of row 0 and a little more, column 0
    x[L + C + 5, 1] = np.nan  # the second piece of row 1, column 1
    x[2 * L:, 0] = -np.inf  # all of row 2, column 0
    x = torch.from_numpy(x)
    adj = kernel.from_coo(3, 1, torch.from_numpy(dst), torch.from_numpy(src))
    y = kernel.edge_softmax(adj, x.to(dev)).cpu()
    want = torch.cat([torch.softmax(x[i * L:(i + 1) * L].double(), 0) for i in range(3)])
    assert torch.equal(torch.isnan(y), torch.isnan(want))
    assert torch.equal(y == 0, want == 0)
    ok = ~torch.isnan(want)
    assert bool(((y[ok].double() - want[ok]).abs() <= 1e-5 * want[ok]).all())


@pytest.mark.parametrize("device", DEVICES)
def test_errors_and_empty(device):
    dev = _dev(device)
    adj = _adj(False, "shuffled")
    E = adj.fwd.nnz
    x = torch.zeros(E, 2, device=dev)
    with pytest.raises(DGLError):
        kernel.edge_softmax(adj, x[:-1])
    with pytest.raises(DGLError):
        kernel.edge_softmax(adj, x, norm_by="both")
    with pytest.raises(DGLError):
        kernel.edge_softmax(adj, x, edge_order="row")
    with pytest.raises(DGLError):
        kernel.edge_softmax(adj, x, norm_by="src", edge_order="slot")
    with pytest.raises(DGLError):
        kernel.edge_softmax(adj, x.double())
    empty = kernel.from_coo(3, 3, torch.zeros(0, dtype=torch.int64),
                            torch.zeros(0, dtype=torch.int64))
    y = kernel.edge_softmax(empty, torch.zeros(0, 4, device=dev))
    assert y.shape == (0, 4) and y.device.type == dev.type


@pytest.mark.gpu
def test_no_host_synchronise():
    """With the adjacency and its longest row cached by a first call, the
    forward and the backward wait for nothing on the host."""
    dev = _dev("cuda")
    for numbering, kw in (("dst_major", {}), ("shuffled", {}), ("shuffled", {"norm_by": "src"})):
        adj = _adj(True, numbering)
        x, dy, _, _, _ = _reference(True, numbering, 8)
        xd, dyd = _leaf(x, dev), dy.to(dev)
        kernel.edge_softmax(adj, xd, **kw).backward(dyd)
        torch.cuda.synchronize()
        old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            kernel.edge_softmax(adj, xd, **kw).backward(dyd)
        finally:
            torch.cuda.set_sync_debug_mode(old)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# The public layer: dgl.nn.pytorch.edge_softmax
# ---------------------------------------------------------------------------
def _graph(numbering="shuffled", readonly=False):
    src, dst = _edges(False, numbering)
    if readonly:
        return dgl.DGLGraph((src.copy(), dst.copy()), multigraph=True, readonly=True)
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(N)
    g.add_edges(src.copy(), dst.copy())
    return g


def _graph_reference(g, x, norm_by="dst"):
    u, v = g.edges(order="eid")
    ids = (v if norm_by == "dst" else u).cpu().numpy()
    y64, _ = _softmax64(x, _groups(ids, g.number_of_nodes()))
    return y64.detach()


@pytest.mark.parametrize("device", DEVICES)
def test_graph_entry_equals_the_operator(device):
    dev = _dev(device)
    g = _graph()
    x, _ = _inputs(g.number_of_edges(), 4)
    xd = x.to(dev)
    for norm_by in ("dst", "src"):
        y = edge_softmax(g, xd, norm_by)
        want = kernel.edge_softmax(g.sparse_adjacency(dev), xd, norm_by)
        assert torch.equal(y.view(torch.int32), want.view(torch.int32))
        _check_fwd(y, _graph_reference(g, x, norm_by), "graph " + norm_by)


@pytest.mark.parametrize("device", DEVICES)
def test_attention_from_builtins(device):
    """Dot-product attention written from builtins: gsddmm_dot scores (no
    autograd of its own), edge_softmax, update_all(src_mul_edge, sum), against
    the float64 layer on the same float32 scores, with the gradients to the
    node features and to the scores. Every bound is 1e-5 of the float64
    formula's terms with each factor replaced by its magnitude."""
    dev = _dev(device)
    g = _graph()
    E = g.number_of_edges()
    heads, D = 2, 4
    rng = np.random.default_rng(11)
    q, k, val, gout = (torch.from_numpy(rng.standard_normal((N, heads, D)).astype(np.float32))
                       for _ in range(4))
    adj = g.sparse_adjacency(dev)
    # e[edge u -> v, h] = <q[v, h], k[u, h]>
    e = kernel.gsddmm_dot(adj, q.to(dev), k.to(dev), E, heads).requires_grad_(True)
    assert e.shape == (E, heads)
    vd = _leaf(val, dev)
    a = edge_softmax(g, e)
    g.ndata["v"] = vd
    g.edata["a"] = a.view(E, heads, 1)
    g.update_all(fn.src_mul_edge("v", "a", "m"), fn.sum("m", "o"))
    out = g.ndata["o"]
    out.backward(gout.to(dev))
    # the scores themselves: float32 dots of four products
    u, v = (t.cpu() for t in g.edges(order="eid"))
    dots = (q.double()[v] * k.double()[u])
    assert bool(((e.detach().cpu().double() - dots.sum(-1)).abs()
                 <= 1e-5 * dots.abs().sum(-1)).all())
    # float64 from those scores, plain indexing
    e64 = e.detach().cpu().double().requires_grad_(True)
    v64 = val.double().requires_grad_(True)
    groups = _groups(v.numpy(), N)
    a64 = torch.zeros_like(e64)
    for idx in groups:
        if idx.numel():
            a64 = a64.index_put((idx,), torch.softmax(e64[idx], 0))
    msg = a64.unsqueeze(-1) * v64[u]
    out64 = torch.zeros(N, heads, D, dtype=torch.float64).index_add_(0, v, msg)
    out64.backward(gout.double())
    ad = a64.detach()
    _check_fwd(a, ad, "attention")
    mag = torch.zeros(N, heads, D, dtype=torch.float64).index_add_(0, v, msg.detach().abs())
    assert bool(((out.detach().cpu().double() - out64.detach()).abs() <= 1e-5 * mag).all())
    gmag = torch.zeros(N, heads, D, dtype=torch.float64).index_add_(
        0, u, ad.unsqueeze(-1) * gout.double()[v].abs())
    assert bool(((vd.grad.cpu().double() - v64.grad).abs() <= 1e-5 * gmag).all())
    # d e = a (d a - sum a d a) with d a = <gout[v], val[u]>, magnitudes throughout
    da = (gout.double()[v] * val.double()[u]).abs().sum(-1)
    tot = torch.zeros_like(da)
    for idx in groups:
        if idx.numel():
            tot[idx] = (ad[idx] * da[idx]).sum(0, keepdim=True)
    _check_bwd(e.grad, e64.grad, ad * da + ad * tot, "attention")


@pytest.mark.parametrize("device", DEVICES)
def test_readonly_graph(device):
    dev = _dev(device)
    g = _graph("src_major", readonly=True)
    x, _ = _inputs(g.number_of_edges(), 3)
    _check_fwd(edge_softmax(g, x.to(dev)), _graph_reference(g, x), "readonly")


@pytest.mark.parametrize("device", DEVICES)
def test_subgraph(device):
    dev = _dev(device)
    g = _graph()
    sg = g.subgraph(list(range(0, N, 2)) + [1, 3])
    assert isinstance(sg, dgl.DGLSubGraph) and sg.number_of_edges() > 0
    x, _ = _inputs(sg.number_of_edges(), 2)
    xd = _leaf(x, dev)
    y = edge_softmax(sg, xd)
    _check_fwd(y, _graph_reference(sg, x), "subgraph")
    y.sum().backward()  # every group sums to one: no gradient
    assert float(xd.grad.abs().max()) <= 1e-6


@pytest.mark.parametrize("device", DEVICES)
def test_graph_entry_errors(device):
    dev = _dev(device)
    g = _graph()
    x = torch.zeros(g.number_of_edges(), 2, device=dev)
    with pytest.raises(DGLError):
        edge_softmax(g, x[1:])
    with pytest.raises(DGLError):
        edge_softmax(g, x, norm_by="node")
