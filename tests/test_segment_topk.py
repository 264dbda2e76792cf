"""kernel.segment_topk: per segment, the first k rows in the order of a stable
sort, and what is built on it (topk_nodes / topk_edges, SortPooling).

The reference is torch.sort(x.double(), dim=0, stable=True) per segment on the
CPU (widening is exact, so the order is float32's), its first k rows, padded
with 0 / -1. Values are compared as bits (int32 views), indices and gradients
with torch.equal: no tolerance. Inputs come from a small integer set, so most
columns are full of ties, with +0.0 / -0.0, NaN and infinities mixed in and one
segment of a single value."""
import functools
import itertools

import numpy as np
import pytest
import torch

import dgl
from dgl import _ffi, kernel
from dgl.base import DGLError
from dgl.nn.pytorch import SortPooling

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
C = kernel.TOPK_CHUNK
SIZES = (0, 1, 3, 63, 64, 65, 0, 257, 0)
SMALL_SIZES = (5, 0, 17, 32, 30, 1, 9)  # several segments share a workgroup
LONG_SIZES = (C - 1, C, C + 1, 2 * C + 3)
MODES = list(itertools.product((True, False), (None, 0, -1)))  # descending x sortby


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


@functools.lru_cache(maxsize=None)
def _inputs(sizes, F, seed=0):
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    x = rng.integers(-3, 4, (N, F)).astype(np.float32)
    u = rng.random((N, F))
    x[(u < 0.05) & (x == 0)] = -0.0
    x[u > 0.98] = np.nan
    x[(u > 0.96) & (u <= 0.97)] = np.inf
    x[(u > 0.97) & (u <= 0.98)] = -np.inf
    x.view(np.uint32)[(u > 0.99)] |= 0x80000001  # negative NaNs with a payload
    if len(sizes) > 3:
        b = int(sum(sizes[:3]))
        x[b:b + sizes[3]] = 2.0  # a segment that is all one value
    return torch.from_numpy(x)


def _reference(x, sizes, k, descending, sortby):
    """(values, indices) from torch.sort per segment; differentiable in x."""
    F = x.shape[1]
    vals, idxs, b = [], [], 0
    for n in sizes:
        xs = x[b:b + n]
        b += n
        key = xs.detach().double() if sortby is None else xs.detach().double()[:, sortby]
        order = torch.sort(key, dim=0, stable=True, descending=descending).indices[:k]
        v = torch.gather(xs, 0, order) if sortby is None else xs[order]
        m = k - order.shape[0]
        vals.append(torch.cat([v, x.new_zeros(m, F)]))
        idxs.append(torch.cat([order, order.new_full((m,) + order.shape[1:], -1)]))
    return torch.stack(vals), torch.stack(idxs)


@functools.lru_cache(maxsize=None)
def _expected(sizes, F, k, descending, sortby):
    return _reference(_inputs(sizes, F), sizes, k, descending, sortby)


def _check(values, indices, want):
    assert values.dtype == torch.float32 and indices.dtype == torch.int64
    assert torch.equal(indices.cpu(), want[1])
    assert torch.equal(values.cpu().view(torch.int32), want[0].view(torch.int32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("k", [1, 5, 64, 65])
@pytest.mark.parametrize("F", [1, 3, 64, 130])
def test_forward_short(F, k, device):
    dev = _dev(device)
    for sizes in (SIZES, SMALL_SIZES):
        x = _inputs(sizes, F).to(dev)
        for descending, sortby in MODES:
            got = kernel.segment_topk(x, list(sizes), k, descending, sortby)
            _check(*got, _expected(sizes, F, k, descending, sortby))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F,k", [(3, 5), (3, C), (64, 65), (130, C)])
def test_forward_long(F, k, device):
    """Segments around one and two chunks: the chunk lists and their merge."""
    dev = _dev(device)
    x = _inputs(LONG_SIZES, F).to(dev)
    for descending, sortby in MODES:
        got = kernel.segment_topk(x, list(LONG_SIZES), k, descending, sortby)
        _check(*got, _expected(LONG_SIZES, F, k, descending, sortby))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [3, 64])
def test_forward_offsets_on_the_device(F, device):
    """Offsets given as a tensor on x's device: the longest segment is not
    known, so short segments run beside the chunk items (more than C rows)."""
    dev = _dev(device)
    sizes = SIZES * 5
    x = _inputs(sizes, F).to(dev)
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    for descending, sortby in MODES:
        got = kernel.segment_topk(x, off, 65, descending, sortby)
        _check(*got, _expected(sizes, F, 65, descending, sortby))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("sizes", [SIZES, LONG_SIZES], ids=["short", "long"])
def test_strided_view(sizes, device):
    """The leading F columns of wider rows at a one-element storage offset,
    read in place."""
    dev = _dev(device)
    F, N = 64, sum(sizes)
    flat = torch.zeros(N * (F + 3) + 1)
    x = flat[1:].view(N, F + 3)[:, :F]
    x.copy_(_inputs(sizes, F))
    x = flat.to(dev)[1:].view(N, F + 3)[:, :F]
    for descending, sortby in MODES:
        got = kernel.segment_topk(x, list(sizes), 5, descending, sortby)
        _check(*got, _expected(sizes, F, 5, descending, sortby))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("sortby", [None, -1])
@pytest.mark.parametrize("sizes,F,k", [(SIZES, 3, 5), (SIZES, 130, 65), (LONG_SIZES, 64, 65)])
def test_backward(sizes, F, k, sortby, device):
    """dx is dy scattered to the selected elements (rows), zero elsewhere;
    the padding slots of segments shorter than k contribute nothing."""
    dev = _dev(device)
    xr = _inputs(sizes, F).clone().requires_grad_(True)
    dy = torch.from_numpy(np.random.default_rng(1).standard_normal((len(sizes), k, F))
                          .astype(np.float32))
    _reference(xr, sizes, k, True, sortby)[0].backward(dy)
    x = _inputs(sizes, F).clone().to(dev).requires_grad_(True)
    values, indices = kernel.segment_topk(x, list(sizes), k, True, sortby)
    assert values.requires_grad and not indices.requires_grad
    values.backward(dy.to(dev))
    assert torch.equal(x.grad.cpu(), xr.grad)


def test_empty_and_errors():
    x = _inputs(SIZES, 3)
    v, i = kernel.segment_topk(x[:0], [0, 0], 4)
    assert v.shape == (2, 4, 3) and not v.any() and i.shape == (2, 4, 3) and (i == -1).all()
    v, i = kernel.segment_topk(x[:0], [], 4, sortby=0)
    assert v.shape == (0, 4, 3) and i.shape == (0, 4)
    v, i = kernel.segment_topk(x[:, :0], list(SIZES), 4)
    assert v.shape == (len(SIZES), 4, 0) and i.shape == (len(SIZES), 4, 0)
    for k in (0, C + 1):
        with pytest.raises(DGLError, match=str(C)):
            kernel.segment_topk(x, list(SIZES), k)
    for c in (3, -4):
        with pytest.raises(DGLError):
            kernel.segment_topk(x, list(SIZES), 2, sortby=c)
    # the C entry point refuses a k past the chunk itself: -1 and a message
    assert _ffi.LIB.dglhip_segment_topk_host(1, 1, 1, C + 1, 1, -1, *[None] * 2, 1, *[None] * 2,
                                             0) == -1
    assert b"DGLHIP_TOPK_CHUNK" in _ffi.LIB.DGLGetLastError()


@pytest.mark.parametrize("device", DEVICES)
def test_topk_nodes_edges_and_sort_pooling(device):
    dev = _dev(device)
    sizes, graphs = (4, 7, 2), []
    for n in sizes:
        g = dgl.DGLGraph()
        g.add_nodes(n)
        g.add_edges(list(range(n)), [(i + 1) % n for i in range(n)])  # n edges
        graphs.append(g)
    bg = dgl.batch(graphs)
    h = _inputs(sizes, 6)
    bg.ndata["h"] = h.view(-1, 2, 3).to(dev)  # idx counts in the flattened row
    bg.edata["w"] = h.to(dev)
    for fn, field, x in ((dgl.topk_nodes, "h", h), (dgl.topk_edges, "w", h)):
        for idx in (None, 4):
            v, i = fn(bg, field, 3, descending=False, idx=idx)
            want = _reference(x, sizes, 3, False, idx)
            _check(v.reshape(3, 3, 6), i.reshape(want[1].shape), want)
            assert v.shape == ((3, 3, 2, 3) if field == "h" else (3, 3, 6))
    g = graphs[1]
    g.ndata["h"] = h[:7].to(dev)
    _check(*dgl.topk_nodes(g, "h", 3, idx=-1), _reference(h[:7], (7,), 3, True, -1))
    for k in (0, C + 1):
        with pytest.raises(DGLError):
            dgl.topk_nodes(g, "h", k)

    xr = torch.from_numpy(np.random.default_rng(2).standard_normal((13, 6)).astype(np.float32))
    xr.requires_grad_(True)
    x = xr.detach().to(dev).requires_grad_(True)
    out = SortPooling(5)(x, bg)
    want = _reference(torch.sort(xr, dim=-1)[0], sizes, 5, True, -1)[0].reshape(3, 30)
    assert torch.equal(out.cpu(), want)
    dy = torch.from_numpy(np.random.default_rng(3).standard_normal((3, 30)).astype(np.float32))
    want.backward(dy)
    out.backward(dy.to(dev))
    assert torch.equal(x.grad.cpu(), xr.grad)
