"""dgl.softmax_nodes / dgl.softmax_edges: the softmax of a feature over the
nodes (edges) of each graph of a batch, on the edge-softmax kernel with the
batch's offsets as its row pointer.

Checked against one float64 torch.softmax per graph under the bounds of
test_edge_softmax.py (inputs clipped to [-8, 8]):
  forward   |y - y64| <= 1e-5 * y64
  backward  |dx - dx64| <= 1e-5 * (|y64 dy| + y64 sum_j |y64_j dy_j|)
The batch sizes put graphs on every path of the kernel, empty graphs among
them, and one graph longer than kernel.EDGE_SOFTMAX_CHUNK."""
import functools

import numpy as np
import pytest
import torch

import dgl
from dgl import kernel

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
C = kernel.EDGE_SOFTMAX_CHUNK
SIZES = (0, 1, 3, 64, 65, 257, 0, C + 1)
WIDTHS = (1, 5, 128)


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


@functools.lru_cache(maxsize=None)
def _batch():
    """A batch whose graph i has SIZES[i] nodes and as many edges (a ring)."""
    graphs = []
    for n in SIZES:
        g = dgl.DGLGraph(multigraph=True)
        g.add_nodes(n)
        if n:
            g.add_edges(np.arange(n), (np.arange(n) + 1) % n)
        graphs.append(g)
    return dgl.batch(graphs, node_attrs=None, edge_attrs=None)


@functools.lru_cache(maxsize=None)
def _reference(F):
    """(x, dy, y64, dx64, bound) over sum(SIZES) rows, on the host, read only."""
    rng = np.random.default_rng(F)
    n = sum(SIZES)
    x = np.clip(rng.standard_normal((n, F)) * np.exp(rng.standard_normal((n, F))), -8, 8)
    dy = rng.standard_normal((n, F)) * np.exp(rng.standard_normal((n, F)))
    x, dy = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(dy.astype(np.float32))
    x64 = x.double().requires_grad_(True)
    y64 = torch.cat([torch.softmax(p, 0) for p in torch.split(x64, list(SIZES), 0)])
    y64.backward(dy.double())
    yd = y64.detach()
    terms = (yd * dy.double()).abs()
    tot = torch.cat([p.sum(0, keepdim=True).expand_as(p)
                     for p in torch.split(terms, list(SIZES), 0)])
    return x, dy, yd, x64.grad, terms + yd * tot


def _check(y, dx, F):
    _, _, y64, dx64, bound = _reference(F)
    err = (y.detach().cpu().double() - y64).abs()
    print("F=%d forward: worst |y - y64| / y64 = %.3g" % (F, float((err / y64).max())))
    assert bool((err <= 1e-5 * y64).all())
    gerr = (dx.cpu().double() - dx64).abs()
    print("F=%d backward: worst error / sum|terms| = %.3g"
          % (F, float((gerr / bound.clamp(min=1e-300)).max())))
    assert bool((gerr <= 1e-5 * bound).all())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("typestr", ["nodes", "edges"])
@pytest.mark.parametrize("F", WIDTHS)
def test_softmax_readout(device, typestr, F):
    dev = _dev(device)
    bg = _batch()
    assert bg.batch_num_nodes == list(SIZES) and bg.batch_num_edges == list(SIZES)
    x, dy, _, _, _ = _reference(F)
    xd = x.to(dev).clone().requires_grad_(True)
    if typestr == "nodes":
        bg.ndata["h"] = xd
        y = dgl.softmax_nodes(bg, "h")
    else:
        bg.edata["h"] = xd
        y = dgl.softmax_edges(bg, "h")
    assert y.shape == x.shape and y.device.type == dev.type
    y.backward(dy.to(dev))
    _check(y, xd.grad, F)
    # every graph with rows sums to one per column
    sums = torch.stack([p.sum(0) for p in torch.split(y.detach().cpu().double(), list(SIZES), 0)])
    live = torch.tensor([s > 0 for s in SIZES])
    assert float((sums[live] - 1).abs().max()) <= 1e-5
    assert float(sums[~live].abs().max()) == 0.0  # an empty graph contributes nothing


@pytest.mark.parametrize("device", DEVICES)
def test_feature_shape_is_kept(device):
    dev = _dev(device)
    bg = _batch()
    x, _, y64, _, _ = _reference(128)
    bg.ndata["h3"] = x.to(dev).view(-1, 2, 64)
    y = dgl.softmax_nodes(bg, "h3")
    assert y.shape == (sum(SIZES), 2, 64)
    assert bool(((y.cpu().double().view(-1, 128) - y64).abs() <= 1e-5 * y64).all())


@pytest.mark.parametrize("device", DEVICES)
def test_unbatched_graph_is_one_segment(device):
    dev = _dev(device)
    n = C + 70
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(np.arange(n - 1), np.arange(1, n))
    rng = np.random.default_rng(2)
    x = torch.from_numpy(np.clip(rng.standard_normal((n, 5)) * np.exp(rng.standard_normal((n, 5))),
                                 -8, 8).astype(np.float32))
    xd = x.to(dev).clone().requires_grad_(True)
    g.ndata["h"] = xd
    y = dgl.softmax_nodes(g, "h")
    y64 = torch.softmax(x.double(), 0)
    assert y.shape == x.shape
    assert bool(((y.detach().cpu().double() - y64).abs() <= 1e-5 * y64).all())
    (y * y).sum().backward()
    x64 = x.double().requires_grad_(True)
    y64g = torch.softmax(x64, 0)
    (y64g * y64g).sum().backward()
    dy = 2 * y64
    bound = (y64 * dy).abs() + y64 * (y64 * dy).abs().sum(0, keepdim=True)
    assert bool(((xd.grad.cpu().double() - x64.grad).abs() <= 1e-5 * bound).all())
    g.edata["w"] = x[:n - 1].to(dev)
    ye = dgl.softmax_edges(g, "w")
    ye64 = torch.softmax(x[:n - 1].double(), 0)
    assert bool(((ye.cpu().double() - ye64).abs() <= 1e-5 * ye64).all())
