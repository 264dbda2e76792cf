"""kernel.segment_radius (csrc/segment_radius.hip and its host twin) and what
is built on it: dgl.geometry's ball queries, FixedRadiusNearNeighbors,
dgl.radius_graph / segmented_radius_graph and RadiusGraph.

The reference is the plain loop in float64: squared differences, d < r2, the
members in row order, the first k of them, the padding. With integer
coordinates in [-4, 4] every distance is an integer, exact in float32, and with
an integer r2 many pairs sit exactly on d == r2, which pins the strict <."""
import functools

import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import kernel
from dgl.base import DGLError
from dgl.nn.pytorch import FarthestPointSampler, FixedRadiusNearNeighbors, RadiusGraph

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
INF = float("inf")
# candidate segments on the edges of the 256-row tile, query segments on the
# edges of a wave's 16 queries and a workgroup's 64, paired segment by segment
X_SIZES = (513, 0, 1, 255, 256, 257, 513, 1, 257)
Q_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 129)
# an integer r per D whose square is a sum of D squares of differences (9; 9 +
# 16; 16 + 16 + 4; 16 + 16 + 16 + 1; ...): pairs lie exactly on the sphere, and
# a tenth to a quarter of a cloud lies inside, so that some queries fill up
# early and some never do
RADIUS = {1: 3.0, 3: 5.0, 4: 6.0, 5: 7.0, 16: 12.0}


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


@functools.lru_cache(maxsize=None)
def _points(n, D, seed, gaussian=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D)) if gaussian else rng.integers(-4, 5, (n, D))
    return torch.from_numpy(x.astype(np.float32))


def _members(x, sizes, q, qsizes, r2, exclude_self=False):
    """Per query, every member in row order: (global rows, float64 distances)."""
    out, xb, qb = [], 0, 0
    for n, m in zip(sizes, qsizes):
        d = (q[qb:qb + m].double()[:, None] - x[xb:xb + n].double()[None]).pow(2).sum(-1)
        for i in range(m):
            inside = d[i] < r2
            if exclude_self and xb <= qb + i < xb + n:
                inside[qb + i - xb] = False
            j = inside.nonzero()[:, 0]
            out.append((j + xb, d[i, j]))
        xb, qb = xb + n, qb + m
    return out


def _expected(members, k, pad_first=False):
    M = len(members)
    nbr = torch.full((M, k), -1, dtype=torch.int64)
    cnt = torch.zeros(M, dtype=torch.int32)
    dist = torch.full((M, k), INF, dtype=torch.float64)
    for i, (j, d) in enumerate(members):
        c = cnt[i] = min(len(j), k)
        nbr[i, :c], dist[i, :c] = j[:c], d[:c]
        if pad_first and c:
            nbr[i, c:], dist[i, c:] = j[0], d[0]
    return nbr, cnt, dist


def _check(got, want, dist_bits=True):
    nbr, cnt, dist = (t.cpu() for t in got)
    assert (nbr.dtype, cnt.dtype, dist.dtype) == (torch.int64, torch.int32, torch.float32)
    assert torch.equal(nbr, want[0]) and torch.equal(cnt, want[1])
    if dist_bits:
        assert torch.equal(dist.view(torch.int32), want[2].float().view(torch.int32))


def _offsets(sizes, dev):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)


def _wide(t, dev):
    """t as the leading columns of wider rows at a one-element storage offset."""
    n, D = t.shape
    flat = torch.zeros(n * (D + 3) + 1)
    flat[1:].view(n, D + 3)[:, :D].copy_(t)
    return flat.to(dev)[1:].view(n, D + 3)[:, :D]


@functools.lru_cache(maxsize=None)
def _integer_case(D, self_query):
    x = _points(sum(X_SIZES), D, D)
    q, qsizes = (x, X_SIZES) if self_query else (_points(sum(Q_SIZES), D, 100 + D), Q_SIZES)
    return x, q, qsizes, _members(x, X_SIZES, q, qsizes, RADIUS[D] ** 2, self_query)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("pad_first", [False, True], ids=["inf", "pad"])
@pytest.mark.parametrize("self_query", [False, True], ids=["q", "self"])
@pytest.mark.parametrize("k", [1, 5, 32, 64])
@pytest.mark.parametrize("D", [1, 3, 4, 5, 16])
def test_exact_on_integer_points(D, k, self_query, pad_first, device):
    dev = _dev(device)
    x, q, qsizes, members = _integer_case(D, self_query)
    r, want = RADIUS[D], _expected(members, k, pad_first)
    xd = x.to(dev)
    if self_query:
        got = kernel.segment_radius(xd, list(X_SIZES), r, k, exclude_self=True,
                                    pad_first=pad_first)
    else:
        got = kernel.segment_radius(xd, list(X_SIZES), r, k, q.to(dev), list(qsizes),
                                    pad_first=pad_first)
    _check(got, want)
    # offsets known only where the points are, rows read through a stride
    _check(kernel.segment_radius(_wide(x, dev), _offsets(X_SIZES, dev), r, k, _wide(q, dev),
                                 _offsets(qsizes, dev), exclude_self=self_query,
                                 pad_first=pad_first), want)


@pytest.mark.parametrize("device", DEVICES)
def test_first_k_not_nearest_and_the_walk_goes_on_for_one_query(device):
    dev = _dev(device)
    k, far = 4, torch.tensor([50., 50., 50.])
    # cloud 0: every query holds k members after rows 0 .. 9 of the first tile;
    # the points at distance 0 lie in later tiles and must not be taken
    x0 = far.repeat(600, 1)
    x0[:10] = torch.tensor([1., 1., 1.])
    x0[300:310] = x0[590:] = 0.0
    q0 = torch.zeros(64, 3)
    # cloud 1: the same, but query 37 finds its k-th member in the last row of
    # the third tile (767), and more members in the fourth
    x1 = far.repeat(1000, 1)
    x1[:10] = torch.tensor([1., 1., 1.])
    x1[[20, 300, 600, 767]] = x1[800:810] = torch.tensor([100., 1., 0.])
    q1 = torch.zeros(64, 3)
    q1[37] = torch.tensor([100., 0., 0.])
    x, q, sizes, qsizes = torch.cat([x0, x1]), torch.cat([q0, q1]), [600, 1000], [64, 64]
    want = _expected(_members(x, sizes, q, qsizes, 4.0), k)
    by_hand = torch.cat([torch.arange(4).repeat(64, 1), torch.arange(600, 604).repeat(64, 1)])
    by_hand[64 + 37] = torch.tensor([620, 900, 1200, 1367])
    assert torch.equal(want[0], by_hand) and bool((want[1] == k).all())
    for offsets, q_offsets in ((sizes, qsizes), (_offsets(sizes, dev), _offsets(qsizes, dev))):
        _check(kernel.segment_radius(x.to(dev), offsets, 2.0, k, q.to(dev), q_offsets), want)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D,r", [(3, 1.5), (16, 5.0)])
def test_gaussian_points(D, r, device):
    """The chain errs by at most gamma_{D+2} d (test_segment_fps.py derives
    it), so where no float64 distance lies within gamma_{D+2} r2 of r2 the
    float32 membership is the float64 one: exact in nbr and cnt. The device
    promises the host's bits on all three outputs."""
    dev = _dev(device)
    sizes, qsizes, k, r2 = (300, 170), (70, 40), 64, r * r
    x, q = _points(470, D, 7, True), _points(110, D, 8, True)
    u = 2.0 ** -24
    gamma = (D + 2) * u / (1 - (D + 2) * u)
    d = (q.double()[:, None] - x.double()[None]).pow(2).sum(-1)
    assert not bool(((d - r2).abs() <= gamma * r2).any())
    host = kernel.segment_radius(x, list(sizes), r, k, q, list(qsizes))
    want = _expected(_members(x, sizes, q, qsizes, r2), k)
    _check(host, want, dist_bits=False)
    real = want[0] >= 0
    assert bool(((host[2].double() - want[2])[real].abs() <= gamma * want[2][real]).all())
    assert 0 < int((want[1] == k).sum()) < 110  # full and partial lists both occur
    if device == "cuda":
        got = kernel.segment_radius(x.to(dev), _offsets(sizes, dev), r, k, q.to(dev),
                                    _offsets(qsizes, dev))
        _check(got, (host[0], host[1], host[2].double()))


@pytest.mark.parametrize("device", DEVICES)
def test_ball_query_and_grouping(device):
    dev = _dev(device)
    B, n, D, m, k = 3, 40, 3, 8, 6
    pos = _points(B * n, D, 1).view(B, n, D)
    cent = FarthestPointSampler(m)(pos.to(dev))
    q = torch.gather(pos, 1, cent.cpu()[:, :, None].expand(-1, -1, D))
    nbr = _expected(_members(pos.reshape(-1, D), [n] * B, q.reshape(-1, D), [m] * B, 9.0), k,
                    True)[0]
    want = (nbr - (torch.arange(B) * n).repeat_interleave(m)[:, None]).view(B, m, k)
    for centroids in (cent, q.to(dev)):
        got = dgl.geometry.ball_query(pos.to(dev), centroids, 3.0, k)
        assert got.device.type == dev.type and torch.equal(got.cpu(), want)
    assert torch.equal(FixedRadiusNearNeighbors(3.0, k)(pos.to(dev), cent).cpu(), want)
    got = dgl.geometry.segmented_ball_query(pos.reshape(-1, D).to(dev), [50, 70],
                                            q.reshape(-1, D).to(dev), [10, 14], 3.0, k)
    assert torch.equal(got.cpu(), _expected(_members(pos.reshape(-1, D), [50, 70],
                                                     q.reshape(-1, D), [10, 14], 9.0), k, True)[0])
    # no coordinates: every distance is +0.0, inside any r > 0
    nbr, cnt, dist = kernel.segment_radius(torch.zeros(5, 0, device=dev), [3, 2], 1.0, 2)
    assert nbr.tolist() == [[0, 1]] * 3 + [[3, 4]] * 2 and cnt.tolist() == [2] * 5
    assert kernel.segment_radius(torch.zeros(0, 3, device=dev), [0], 1.0, 2)[0].shape == (0, 2)


@pytest.mark.parametrize("device", DEVICES)
def test_radius_graphs(device):
    dev = _dev(device)
    sizes, D, k = (17, 30, 9), 3, 5
    x = _points(56, D, 2)
    x3 = x[:54].view(2, 27, D)
    cases = [(dgl.radius_graph(x[:30].to(dev), 3.0, k), x[:30], (30,), False, k),
             (RadiusGraph(3.0, k, self_loop=True)(x3.to(dev)), x3.reshape(-1, D), (27, 27), True,
              k),
             (dgl.segmented_radius_graph(x.to(dev), 3.0, list(sizes)), x, sizes, False, 32)]
    for g, pts, segs, self_loop, kk in cases:
        n = pts.shape[0]
        members = _members(pts, segs, pts, segs, 9.0, not self_loop)
        src = torch.cat([j[:kk] for j, _ in members])
        dst = torch.cat([torch.full((min(len(j), kk),), i) for i, (j, _) in enumerate(members)])
        assert g.number_of_nodes() == n and g.number_of_edges() == src.numel() > 0
        g.ndata["h"] = pts.to(dev)
        g.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))  # integers: exact in any order
        want = torch.stack([pts[j[:kk]].double().sum(0) for j, _ in members])
        assert torch.equal(g.ndata["o"].cpu().double(), want)
        if device == "cuda":
            assert not g._graph.has_native_index
        u, v = g.edges()
        assert torch.equal(u.cpu(), src) and torch.equal(v.cpu(), dst)


@pytest.mark.parametrize("device", DEVICES)
def test_errors(device):
    dev = _dev(device)
    x = _points(30, 3, 3).to(dev)
    wide = torch.zeros(9, kernel.RADIUS_MAX_DIM + 1, device=dev)
    for bad in (lambda: kernel.segment_radius(x, [30], 1.0, 0),
                lambda: kernel.segment_radius(x, [30], 1.0, kernel.RADIUS_MAX_K + 1),
                lambda: kernel.segment_radius(wide, [9], 1.0, 2),
                lambda: kernel.segment_radius(x.double(), [30], 1.0, 2),
                lambda: kernel.segment_radius(x, [30], 1.0, 2, x.double(), [30]),
                lambda: kernel.segment_radius(x[:, 0], [30], 1.0, 2),
                lambda: kernel.segment_radius(x, [10, 19], 1.0, 2),
                lambda: kernel.segment_radius(x, [10, 20], 1.0, 2, x[:5], [2, 2]),
                lambda: kernel.segment_radius(x, [10, 20], 1.0, 2, x[:5], [5]),
                lambda: kernel.segment_radius(x, [10, 20], 1.0, 2, x[:5]),
                lambda: dgl.geometry.ball_query(x.view(3, 10, 3), torch.zeros(3, 2, 2), 1.0, 2),
                lambda: dgl.radius_graph(x[:, 0], 1.0)):
        with pytest.raises(DGLError):
            bad()
