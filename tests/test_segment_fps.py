"""kernel.segment_fps (csrc/segment_fps.hip and its host twin) and what is
built on it: dgl.geometry's samplers and FarthestPointSampler.

The reference is the greedy loop in float64 per segment: squared differences,
a running minimum that only a smaller distance lowers, a taken mask, argmax
(first occurrence: the lowest row). With integer coordinates in [-4, 4] every
distance is an integer below 2^24, exact in float32, so device, host and
float64 agree index for index and bit for bit, and the many ties are settled
by the lowest-row rule alone."""
import functools

import numpy as np
import pytest
import torch

import dgl
from dgl import kernel
from dgl.base import DGLError
from dgl.nn.pytorch import FarthestPointSampler

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
INF = float("inf")
# The longest segment of a batch picks the kernel: (waves x rows per lane) hold
# 64, 256, 1024, 4096 and 8192 rows, longer ones take the general kernel; for
# D > 4 the staged segment must fit 32768 floats of LDS at a row stride of
# D | 1: 6553 rows at D = 5, 992 at D = 33.
BATCHES = [(0, 1, 2, 63, 64), (65, 0, 255, 256), (257, 1023, 1024), (1025, 4095, 4096),
           (4097, 8191, 8192), (8193, 3), (992,), (993,), (6553,), (6554,)]


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


def _greedy(xs, m, start=0):
    """(rows, distances) of one segment's picks, in float64."""
    x64, n = xs.double(), xs.shape[0]
    mind, taken = torch.full((n,), INF, dtype=torch.float64), torch.zeros(n, dtype=torch.bool)
    rows, dists, p, dp = [], [], start, INF
    for _ in range(min(m, n)):
        rows.append(p)
        dists.append(dp)
        taken[p] = True
        d = (x64 - x64[p]).pow(2).sum(-1)
        mind = torch.where(d < mind, d, mind)
        score = torch.where(taken, -1.0, mind)
        p = int(score.argmax())
        dp = float(score[p])
    return rows, dists


def _expected(x, sizes, m, start=None):
    idx = torch.full((len(sizes), m), -1, dtype=torch.int64)
    dist = torch.zeros(len(sizes), m, dtype=torch.float32)
    b = 0
    for s, n in enumerate(sizes):
        rows, dists = _greedy(x[b:b + n], m, 0 if start is None else int(start[s]))
        idx[s, :len(rows)] = torch.tensor(rows, dtype=torch.int64) + b
        dist[s, :len(rows)] = torch.tensor(dists, dtype=torch.float32)
        b += n
    return idx, dist


@functools.lru_cache(maxsize=None)
def _expected_int(sizes, D):
    return _expected(_points(sizes, D), sizes, 70)


def _check_exact(got, want, m=None):
    idx, dist = got
    m = idx.shape[1] if m is None else m
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32
    assert not idx.requires_grad and not dist.requires_grad
    # the first m picks of a longer run are the run of m picks: its padding too
    wi, wd = want[0][:, :m], want[1][:, :m]
    assert torch.equal(idx.cpu(), wi)
    assert torch.equal(dist.cpu().view(torch.int32), wd.contiguous().view(torch.int32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [1, 3, 4, 5, 33])
@pytest.mark.parametrize("sizes", BATCHES, ids=lambda b: "n%d" % max(b))
def test_exact_on_integer_points(sizes, D, device):
    dev = _dev(device)
    x, want = _points(sizes, D).to(dev), _expected_int(sizes, D)
    for m in (1, 7, 70):
        _check_exact(kernel.segment_fps(x, list(sizes), m), want, m)
    # no size known on the host: the general kernel
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    _check_exact(kernel.segment_fps(x, off, 7), want, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 64])
def test_host_and_device_agree_bit_for_bit(D):
    dev = _dev("cuda")
    sizes, m = (200, 70), 66
    x = _points(sizes, D, gaussian=True)
    for offsets in (list(sizes), torch.tensor([0, 200, 270], device=dev)):
        hi, hd = kernel.segment_fps(x, list(sizes), m)
        di, dd = kernel.segment_fps(x.to(dev), offsets, m)
        assert torch.equal(di.cpu(), hi)
        assert torch.equal(dd.cpu().view(torch.int32), hd.view(torch.int32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [3, 64])
def test_random_points_within_the_float32_bound(D, device):
    """Gaussian points, step by step along the path's own prefix (the greedy
    choice diverges for good after one near-tie). The difference t rounds once
    and enters the fma squared, exactly: a factor (1 + e)^2. Every fma then
    rounds the running sum once, and the first term passes through all D of
    them: (1 + e)^(D + 2) at most on any term, all terms non-negative. So a
    computed distance errs by at most gamma_{D+2} d <= tol = gamma_{D+2} max d
    (gamma_n = n u / (1 - n u), u = 2^-24), and so does a minimum of them. The
    pick maximises minima that are each within tol: its true minimum is within
    2 tol of the true maximum. Derived, not measured."""
    dev = _dev(device)
    sizes, m = (200, 70), 66
    x = _points(sizes, D, gaussian=True)
    idx, dist = (t.cpu() for t in kernel.segment_fps(x.to(dev), list(sizes), m))
    u = 2.0 ** -24
    gamma = (D + 2) * u / (1 - (D + 2) * u)
    b = 0
    for s, n in enumerate(sizes):
        d = (x[b:b + n].double()[:, None, :] - x[b:b + n].double()[None, :, :]).pow(2).sum(-1)
        tol = gamma * float(d.max())
        rows = idx[s] - b
        assert bool(((rows >= 0) & (rows < n)).all()) and rows.unique().numel() == m
        assert rows[0] == 0 and dist[s, 0] == INF
        mind = d[rows].cummin(0).values  # row i: the true minima after picks 0 .. i
        for i in range(1, m):
            open_ = torch.ones(n, dtype=torch.bool)
            open_[rows[:i]] = False
            true = mind[i - 1, rows[i]]
            assert true >= mind[i - 1][open_].max() - 2 * tol
            assert abs(float(dist[s, i]) - true) <= tol
        b += n


@pytest.mark.parametrize("device", DEVICES)
def test_start_strided_rows_and_nan(device):
    dev = _dev(device)
    sizes, D, m = (70, 5, 300, 0), 3, 9
    N = sum(sizes)
    x = _points(sizes, D)
    start = torch.tensor([69, 2, 150, 0])
    want = _expected(x, sizes, m, start)
    assert not torch.equal(want[0], _expected(x, sizes, m)[0])
    _check_exact(kernel.segment_fps(x.to(dev), list(sizes), m, start.to(dev)), want)
    _check_exact(kernel.segment_fps(x.to(dev), list(sizes), m, start), want)
    # the leading D columns of wider rows at a one-element storage offset
    flat = torch.zeros(N * (D + 3) + 1)
    flat[1:].view(N, D + 3)[:, :D].copy_(x)
    _check_exact(kernel.segment_fps(flat.to(dev)[1:].view(N, D + 3)[:, :D], list(sizes), m,
                                    start.to(dev)), want)
    # a row with a NaN coordinate keeps its minimum at +inf: picked next, lowest row first
    xn = x.clone()
    xn[10, 1] = xn[3, 0] = xn[72, 2] = float("nan")
    for offsets in (list(sizes), torch.tensor([0, 70, 75, 375, 375], device=dev)):
        idx, dist = kernel.segment_fps(xn.to(dev), offsets, m)
        _check_exact((idx, dist), _expected(xn, sizes, m))
        assert idx[0, :3].tolist() == [0, 3, 10] and idx[1, :2].tolist() == [70, 72]
        assert dist[0, :3].tolist() == [INF, INF, INF]


@pytest.mark.parametrize("device", DEVICES)
def test_geometry_samplers(device):
    dev = _dev(device)
    B, n, D, m = 3, 40, 3, 12
    pos = _points((B * n,), D).view(B, n, D)
    for start_idx, start in ((None, None), (7, [7] * B), (torch.tensor([1, 0, 39]), [1, 0, 39])):
        want = _expected(pos.reshape(-1, D), (n,) * B, m, start)[0] - torch.arange(B)[:, None] * n
        got = dgl.geometry.farthest_point_sampler(pos.to(dev), m, start_idx)
        assert got.device.type == dev.type and torch.equal(got.cpu(), want)
        assert torch.equal(FarthestPointSampler(m)(pos.to(dev), start_idx).cpu(), want)
    sizes = (5, 40, 75)
    got = dgl.geometry.segmented_farthest_point_sampler(pos.reshape(-1, D).to(dev), m, sizes)
    assert torch.equal(got.cpu(), _expected(pos.reshape(-1, D), sizes, m)[0])
    # no coordinates: every distance is +0.0, the rows follow the first pick in order
    idx, dist = kernel.segment_fps(torch.zeros(7, 0, device=dev), [4, 0, 3], 3,
                                   torch.tensor([2, 0, 0], device=dev))
    assert idx.tolist() == [[2, 0, 1], [-1, -1, -1], [4, 5, 6]]
    assert dist.tolist() == [[INF, 0, 0], [0, 0, 0], [INF, 0, 0]]


@pytest.mark.parametrize("device", DEVICES)
def test_errors(device):
    dev = _dev(device)
    x = _points((30,), 3).to(dev)
    for bad in (lambda: kernel.segment_fps(x.double(), [30], 4),
                lambda: kernel.segment_fps(x[:, 0], [30], 4),
                lambda: kernel.segment_fps(torch.zeros(9, kernel.FPS_MAX_DIM + 1, device=dev), [9], 2),
                lambda: kernel.segment_fps(x, [30], 0),
                lambda: kernel.segment_fps(x, [10, 19], 4),
                lambda: kernel.segment_fps(x, [10, 20], 4, torch.tensor([0])),
                lambda: kernel.segment_fps(x, [10, 20], 4, torch.tensor([0, 20])),
                lambda: kernel.segment_fps(x, [10, 20], 4, torch.tensor([-1, 0])),
                lambda: dgl.geometry.farthest_point_sampler(x.view(3, 10, 3), 11),
                lambda: dgl.geometry.farthest_point_sampler(x.view(3, 10, 3), 4, 10)):
        with pytest.raises(DGLError):
            bad()
