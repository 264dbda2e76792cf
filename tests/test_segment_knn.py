"""kernel.segment_knn (csrc/segment_knn.hip and its host twin) and what is
built on it: dgl.knn_graph / segmented_knn_graph, KNNGraph, EdgeConv.

The reference is float64 per segment: squared distances, the diagonal 0 (or
removed with exclude_self), a stable ascending sort, the first k, padded with
-1 / +inf. With integer coordinates in [-4, 4] every product, norm and sum is
an integer below 2^24, exact in float32 in any order, so device, host and
float64 agree index for index and bit for bit, and the many ties are settled
by the (d, j) rule alone."""
import functools

import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import kernel
from dgl.base import DGLError
from dgl.nn.pytorch import EdgeConv, KNNGraph, SegmentedKNNGraph

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 0, 129)


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


@functools.lru_cache(maxsize=None)
def _points(sizes, D, gaussian=False):
    rng = np.random.default_rng(D)
    N = int(sum(sizes))
    x = rng.standard_normal((N, D)) if gaussian else rng.integers(-4, 5, (N, D))
    return torch.from_numpy(x.astype(np.float32))


def _d64(xs):
    d = (xs.double()[:, None, :] - xs.double()[None, :, :]).pow(2).sum(-1)
    return d.fill_diagonal_(0.0)


@functools.lru_cache(maxsize=None)
def _ranked(sizes, D, exclude_self):
    """Per segment (first row, float64 distances, every row's candidates in order)."""
    x, out, b = _points(sizes, D), [], 0
    for n in sizes:
        d = _d64(x[b:b + n])
        order = torch.sort(d, dim=1, stable=True).indices
        if exclude_self:
            order = order[order != torch.arange(n)[:, None]].view(n, max(n - 1, 0))
        out.append((b, d, order))
        b += n
    return out


def _expected(sizes, D, k, exclude_self):
    nbr, dist = [], []
    for b, d, order in _ranked(sizes, D, exclude_self):
        o = order[:, :k]
        pad = k - o.shape[1]
        nbr.append(torch.cat([o + b, o.new_full((o.shape[0], pad), -1)], 1))
        dist.append(torch.cat([d.gather(1, o), d.new_full((o.shape[0], pad), float("inf"))], 1))
    return torch.cat(nbr), torch.cat(dist).float()


def _check_exact(got, want):
    nbr, dist = got
    assert nbr.dtype == torch.int64 and dist.dtype == torch.float32
    assert not nbr.requires_grad and not dist.requires_grad
    assert torch.equal(nbr.cpu(), want[0])
    assert torch.equal(dist.cpu().view(torch.int32), want[1].view(torch.int32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("k", [1, 5, 20, 64])
@pytest.mark.parametrize("D", [1, 3, 4, 5, 33, 256])
def test_exact_on_integer_points(D, k, exclude_self, device):
    dev = _dev(device)
    x = _points(SIZES, D).to(dev)
    _check_exact(kernel.segment_knn(x, list(SIZES), k, exclude_self),
                 _expected(SIZES, D, k, exclude_self))


@pytest.mark.parametrize("device", DEVICES)
def test_offsets_on_the_device_and_strided_rows(device):
    """Offsets as a tensor on x's device (no size is known on the host), and x
    as the leading D columns of wider rows at a one-element storage offset."""
    dev = _dev(device)
    D, k, N = 33, 20, sum(SIZES)
    off = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int64, device=dev)
    want = _expected(SIZES, D, k, False)
    _check_exact(kernel.segment_knn(_points(SIZES, D).to(dev), off, k), want)
    flat = torch.zeros(N * (D + 3) + 1)
    flat[1:].view(N, D + 3)[:, :D].copy_(_points(SIZES, D))
    _check_exact(kernel.segment_knn(flat.to(dev)[1:].view(N, D + 3)[:, :D], list(SIZES), k), want)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("D", [3, 64])
def test_random_points_within_the_float32_bound(D, exclude_self, device):
    """Gaussian points: a float32 dot product of length D in any order errs by
    at most gamma_D |x||y| (gamma_n = n u / (1 - n u), u = 2^-24); two norms
    and three adds give |d_hat - d| <= gamma_{D+3} (|x_i| + |x_j|)^2 <= tol_i =
    gamma_{D+3} (|x_i| + max_j |x_j|)^2. Derived, not measured."""
    dev = _dev(device)
    sizes, k = (200, 70), 20
    x = _points(sizes, D, gaussian=True)
    nbr, dist = (t.cpu() for t in kernel.segment_knn(x.to(dev), list(sizes), k, exclude_self))
    u = 2.0 ** -24
    gamma = (D + 3) * u / (1 - (D + 3) * u)
    b = 0
    for n in sizes:
        xs, ids, dh = x[b:b + n], nbr[b:b + n] - b, dist[b:b + n].double()
        rows = torch.arange(n)[:, None]
        norm = xs.double().norm(dim=1)
        tol = (gamma * (norm + norm.max()) ** 2)[:, None]
        d = _d64(xs)
        assert bool(((ids >= 0) & (ids < n)).all())  # every row, every slot, its own segment
        assert bool((ids.sort(1).values.diff(dim=1) > 0).all())  # distinct
        if exclude_self:
            assert bool((ids != rows).all())
            d[rows[:, 0], rows[:, 0]] = float("inf")
        else:
            assert torch.equal(ids[:, :1], rows) and bool((dh[:, 0] == 0).all())
        dsel = d.gather(1, ids)
        kth = d.sort(1).values[:, k - 1:k]
        assert bool((dsel <= kth + 2 * tol).all())
        later = dsel.flip(1).cummin(1).values.flip(1)  # the smallest from each slot on
        assert bool((dsel[:, :-1] <= later[:, 1:] + 2 * tol).all())
        assert bool(((dh - dsel).abs() <= tol).all())
        b += n


def _ref_ids(pts, segs, k, exclude_self=False):
    """(n, k) neighbour ids of clouds that all hold more than k points."""
    out, b = [], 0
    for n in segs:
        d = _d64(pts[b:b + n])
        if exclude_self:
            d.fill_diagonal_(float("inf"))
        out.append(torch.sort(d, dim=1, stable=True).indices[:, :k] + b)
        b += n
    return torch.cat(out)


def _lattice_points(n, seed):
    """n distinct integer points of [-4, 4]^3."""
    cells = np.random.default_rng(seed).permutation(729)[:n]
    return torch.from_numpy(np.stack([cells // 81, cells // 9 % 9, cells % 9], 1) - 4).float()


@pytest.mark.parametrize("device", DEVICES)
def test_knn_graphs(device):
    dev = _dev(device)
    sizes, D, k = (17, 30, 9), 5, 4
    x = _points(sizes, D)
    x3 = x[:2 * 28].view(2, 28, D)
    cases = [(dgl.knn_graph(x[:30].to(dev), k, True), x[:30], (30,), True),
             (KNNGraph(k)(x3.to(dev)), x3.reshape(-1, D), (28, 28), False),
             (SegmentedKNNGraph(k)(x.to(dev), list(sizes)), x, sizes, False)]
    for g, pts, segs, exclude_self in cases:
        n = pts.shape[0]
        ids = _ref_ids(pts, segs, k, exclude_self)
        assert g.number_of_nodes() == n and g.number_of_edges() == n * k
        g.ndata["h"] = pts.to(dev)
        g.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))  # integers: exact in any order
        assert torch.equal(g.ndata["o"].cpu(), pts[ids].sum(1))
        if device == "cuda":
            assert not g._graph.has_native_index
        u, v = g.edges()
        assert torch.equal(u.cpu(), ids.reshape(-1))
        assert torch.equal(v.cpu(), torch.arange(n).repeat_interleave(k))
    for bad in (lambda: dgl.segmented_knn_graph(x.to(dev), 10, list(sizes)),
                lambda: dgl.segmented_knn_graph(x.to(dev), 9, list(sizes), exclude_self=True),
                lambda: dgl.knn_graph(torch.zeros(70, 2, device=dev), kernel.KNN_MAX_K + 1),
                lambda: dgl.knn_graph(torch.zeros(9, kernel.KNN_MAX_DIM + 1, device=dev), 2),
                lambda: dgl.knn_graph(x.double().to(dev), 2)):
        with pytest.raises(DGLError):
            bad()


@pytest.mark.parametrize("device", DEVICES)
def test_edge_conv_on_a_knn_graph(device):
    """Forward and the gradients of x, Theta and Phi against the per-edge
    float64 formulation max over edges of Theta (x_u - x_v) + Phi x_v; every
    element within 1e-5 of the sum of the magnitudes of its terms. Distinct
    integer points and a random Theta: the arg-max is unique."""
    dev = _dev(device)
    n, k, out = 60, 6, 8
    pts = _lattice_points(n, 1)
    torch.manual_seed(0)
    conv = EdgeConv(3, out).to(dev)
    x = pts.clone().to(dev).requires_grad_(True)
    g = dgl.knn_graph(pts.to(dev), k)
    h = conv(g, x)
    dy = torch.from_numpy(np.random.default_rng(2).standard_normal((n, out))).float()
    h.backward(dy.to(dev))

    src = _ref_ids(pts, (n,), k)  # (n, k): u of v's in-edges
    th, ph, bias = (p.detach().cpu().double() for p in
                    (conv.theta.weight, conv.phi.weight, conv.phi.bias))
    x64 = pts.double()
    e = ((x64[src] - x64[:, None, :]) @ th.t() + (x64 @ ph.t() + bias)[:, None, :])  # (n, k, out)
    top = e.topk(2, dim=1).values
    assert bool((top[:, 0] > top[:, 1]).all()), "the reference's arg-max is not unique"
    arg = src.gather(1, e.argmax(1))  # (n, out): the source node of each maximum

    def chain(xv, tv, pv, bv, sign):
        """The maximal edge's chain; sign -1: its value, +1 over magnitudes: its bound."""
        return (tv[None] * xv[arg]).sum(-1) + sign * (xv @ tv.t()) + xv @ pv.t() + bv

    def grads(leaves, sign, dyv):
        leaves = [t.clone().requires_grad_(True) for t in leaves]
        val = chain(*leaves, sign)
        val.backward(dyv)
        return [val.detach()] + [t.grad for t in leaves[:3]]

    want = grads([x64, th, ph, bias], -1.0, dy.double())
    bound = grads([x64.abs(), th.abs(), ph.abs(), bias.abs()], 1.0, dy.double().abs())
    assert torch.equal(want[0], e.max(1).values) or bool(
        ((want[0] - e.max(1).values).abs() <= 1e-12 * bound[0]).all())
    got = [h.detach(), x.grad, conv.theta.weight.grad, conv.phi.weight.grad]
    for name, a, w, bd in zip(("h", "dx", "dTheta", "dPhi"), got, want, bound):
        err = (a.double().cpu() - w).abs()
        assert bool((err <= 1e-5 * bd + 1e-30).all()), \
            "%s: max err / bound %.3g" % (name, float((err / (bd + 1e-30)).max()))
