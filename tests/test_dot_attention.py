"""kernel.dot_attention, dgl.nn.pytorch.dot_attention and DotGatConv: scaled
dot-product attention over each destination's in-edges, fused.

The reference is float64, computed here from the same float32 inputs with
plain torch indexing (one torch.softmax per destination's edge list), its
gradients by float64 autograd; it never calls the library. The bounds are per
element, 1e-5 x the sum of |terms| taken from the float64 values (a the
attention, dp_j = <dout[r], v[u_j]>):

  out[r]  1e-5 * sum_j a_j |v_j|
  dv[u]   1e-5 * sum over u's out-edges of a |dout[r]|
  dq[r]   1e-5 * scale * sum_j a_j (|dp_j| + sum_i a_i |dp_i|) |k_j|
  dk[u]   the same sum over u's out-edges with |q[r]|

q, k, v and dout are standard normal and scale = D ** -0.5. A plain float32
torch composition on the CPU (index, sum, one softmax and one sum per
destination, autograd) measured against these bounds, worst over the shapes
below: out 0.24, dq 0.28, dk 0.20, dv 0.18 of the bound; in the clamp case
(q * 12) 0.40, 0.10, 0.21, 0.26. All within half of each bound. On an MI355X
the kernels' worst figures were out 0.29, dq 0.25, dk 0.22, dv 0.50 (clamp:
0.39, 0.07, 0.16, 0.28); the tests print each before they assert.

Copies of one edge are what the bounds are sensitive to: a float32 chain that
adds the same term m times in a row's binade rounds the same way every time,
an error of up to m ulp / 2. With 600 copies of a (destination, source) pair
the float32 torch composition itself left the forward bound by 2.5 x, so the
graph keeps them to 30 to 60 a pair.

The graph has 40 destinations and 37 sources (a rectangular CSR) with
in-degrees 0, 1, 2, 3, B - 1, B, B + 1 around kernel.DOT_ATTENTION_BATCH, 63,
64, 65 around the 64 column ids a wave takes per trip, 257, and C - 1, C,
C + 1, 2 C + 3 around kernel.DOT_ATTENTION_CHUNK; the other destinations have 150 in-edges. Every
destination of 150 or more sends 30 (45 when it has more) edges to each of the
sources 0 and 1, whose out-degrees so cross the chunk too (the transposed
kernel's pieces); the other sources are drawn uniformly, so every longer row
has duplicate edges, and one row a self-loop. Two edge
numberings."""
import functools

import numpy as np
import pytest
import torch

import dgl
from dgl import kernel
from dgl.base import DGLError
from dgl.nn.pytorch import DotGatConv, dot_attention

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
B, C = kernel.DOT_ATTENTION_BATCH, kernel.DOT_ATTENTION_CHUNK
SHORT_DEGREES = (0, 1, 2, 3, B - 1, B, B + 1, 63, 64, 65, 257)
LONG_DEGREES = (C - 1, C, C + 1, 2 * C + 3)
NR, NC = 40, 37
MID_DEGREE = 150  # the destinations the lists leave over
# (H, D, the long degrees too)
SHAPES = [(1, 1, False), (3, 5, True), (5, 24, False), (8, 16, True), (8, 64, False),
          (1, 256, False), (1, 65, False)]


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


@functools.lru_cache(maxsize=None)
def _edges(full, numbering):
    """(src, dst) int64 tensors in the numbering's edge-id order."""
    rng = np.random.default_rng(11)
    degs = list(SHORT_DEGREES) + (list(LONG_DEGREES) if full else [])
    degs += [MID_DEGREE] * (NR - len(degs))
    order = rng.permutation(NR)  # which destination gets which degree
    dst = np.concatenate([np.full(d, order[i], dtype=np.int64) for i, d in enumerate(degs)])
    src = rng.integers(0, NC, dst.size).astype(np.int64)
    for i, d in enumerate(degs):
        if d >= MID_DEGREE:  # 30 (45 from the rows past MID_DEGREE) edges to each hub
            at = rng.permutation(np.flatnonzero(dst == order[i]))
            n = 30 if d == MID_DEGREE else 45
            src[at[:n]], src[at[n:2 * n]] = 0, 1
    at = np.flatnonzero(dst == order[7])  # in-degree 63
    src[at[0]] = min(int(order[7]), NC - 1)  # a self-loop (where the id is a source's)
    src[at[2]] = src[at[1]]  # a duplicate edge
    key = np.argsort(dst, kind="stable") if numbering == "dst_major" else \
        rng.permutation(dst.size)
    return torch.from_numpy(src[key].copy()), torch.from_numpy(dst[key].copy())


@functools.lru_cache(maxsize=None)
def _adj(full, numbering):
    src, dst = _edges(full, numbering)
    return kernel.from_coo(NR, NC, dst, src)


@functools.lru_cache(maxsize=None)
def _inputs(H, D, nr=NR, nc=NC):
    gen = torch.Generator().manual_seed(100 * H + D)
    return tuple(torch.randn(n, H, D, generator=gen) for n in (nr, nc, nc, nr))


def _reference(src, dst, q, k, v, dout, scale, clamp=None):
    """float64: out, (dq, dk, dv) and the bounds' sums of |terms|, in that order."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    dout = dout.double()
    s = (q[dst] * k[src]).sum(-1) * scale
    s = s if clamp is None else s.clamp(*clamp)
    a = torch.zeros_like(s)
    for r in range(q.shape[0]):
        at = torch.nonzero(dst == r).flatten()
        if at.numel():
            a = a.index_put((at,), torch.softmax(s[at], 0))
    out = torch.zeros_like(q).index_add(0, dst, a.unsqueeze(-1) * v[src])
    grads = torch.autograd.grad(out, (q, k, v), dout)
    with torch.no_grad():
        a1 = a.unsqueeze(-1)
        dp = (dout[dst] * v[src]).sum(-1).abs()
        w = (a * (dp + torch.zeros_like(out[..., 0]).index_add(0, dst, a * dp)[dst])).unsqueeze(-1)
        sums = (torch.zeros_like(q).index_add(0, dst, a1 * v[src].abs()),
                scale * torch.zeros_like(q).index_add(0, dst, w * k[src].abs()),
                scale * torch.zeros_like(k).index_add(0, src, w * q[dst].abs()),
                torch.zeros_like(v).index_add(0, src, a1 * dout[dst].abs()))
    return (out.detach(),) + grads, sums


@functools.lru_cache(maxsize=None)
def _case(full, numbering, H, D, qscale=1.0, clamp=None):
    q, k, v, dout = _inputs(H, D)
    q = q * qscale
    return (q, k, v, dout) + _reference(*_edges(full, numbering), q, k, v, dout, D ** -0.5, clamp)


def _run(adj, q, k, v, dout, dev, **kw):
    """(out, dq, dk, dv) of kernel.dot_attention on leaves of their own on ``dev``."""
    q, k, v = (t.to(dev).clone().requires_grad_(True) for t in (q, k, v))
    out = kernel.dot_attention(adj, q, k, v, **kw)
    return (out,) + torch.autograd.grad(out, (q, k, v), dout.to(dev))


def _check(got, want, sums, what, names=("out", "dq", "dk", "dv")):
    for name, g, w, s in zip(names, got, want, sums):
        err = (g.detach().cpu().double() - w).abs()
        worst = float((err / s.clamp(min=1e-300)).max())
        print("%s %s: worst error / sum|terms| = %.3g" % (what, name, worst))
        assert bool((err <= 1e-5 * s).all()), "%s %s: worst %.3g of the terms" % (what, name, worst)


@pytest.mark.parametrize("numbering", ["dst_major", "shuffled"])
@pytest.mark.parametrize("H,D,full", SHAPES)
@pytest.mark.parametrize("device", DEVICES)
def test_against_float64(device, H, D, full, numbering):
    """Forward and the three gradients at every lane map ((1, 65): the
    composed fallback); a destination without in-edges gets exact zeros."""
    dev = _dev(device)
    q, k, v, dout, want, sums = _case(full, numbering, H, D)
    got = _run(_adj(full, numbering), q, k, v, dout, dev)
    _check(got, want, sums, "%dx%d %s" % (H, D, numbering))


@pytest.mark.parametrize("device", DEVICES)
def test_clamp(device):
    """clamp=(-10, 10) with q * 12: 18.6 % of the scores are clamped at the
    lower bound and 18.0 % at the upper one; their gradient is 0."""
    dev = _dev(device)
    q, k, v, dout, want, sums = _case(True, "shuffled", 8, 16, 12.0, (-10.0, 10.0))
    got = _run(_adj(True, "shuffled"), q, k, v, dout, dev, clamp=(-10.0, 10.0))
    _check(got, want, sums, "clamp")


@pytest.mark.parametrize("device", DEVICES)
def test_views(device):
    """q, k, v as views offset by one float (the narrower accesses: 5 x 24
    runs on single floats, 32 lanes a head), and a non-contiguous v."""
    dev = _dev(device)
    q, k, v, dout, want, sums = _case(False, "shuffled", 5, 24)
    adj = _adj(False, "shuffled")

    def offset(t):
        buf = torch.empty(t.numel() + 1, device=dev)
        buf[1:] = t.to(dev).flatten()
        return buf[1:].view(t.shape).requires_grad_(True)

    qo, ko, vo = offset(q), offset(k), offset(v)
    out = kernel.dot_attention(adj, qo, ko, vo)
    _check((out,) + torch.autograd.grad(out, (qo, ko, vo), dout.to(dev)), want, sums, "offset")
    wide = torch.stack([v, -v], -1).to(dev).requires_grad_(True)  # v at a stride of two floats
    assert not wide[..., 0].is_contiguous()
    out = kernel.dot_attention(adj, q.to(dev), k.to(dev), wide[..., 0])
    dv = torch.autograd.grad(out, wide, dout.to(dev))[0]
    assert float(dv[..., 1].abs().max()) == 0.0
    _check((out, dv[..., 0]), (want[0], want[3]), (sums[0], sums[3]), "strided v",
           ("out", "dv"))


@pytest.mark.parametrize("device", DEVICES)
def test_same_bits_every_call(device):
    dev = _dev(device)
    q, k, v, dout = _case(True, "shuffled", 8, 16)[:4]
    first = _run(_adj(True, "shuffled"), q, k, v, dout, dev)
    again = _run(_adj(True, "shuffled"), q, k, v, dout, dev)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("device", DEVICES)
def test_public_path(device):
    """dgl.nn.pytorch.dot_attention on a DGLGraph, and DotGatConv forward and
    backward against its float64 restatement: the projection is the module's
    own (float32), so out keeps its bound; the weight gradient is x^T (dq + dk
    + dv), so it gets the three bounds summed over the nodes with |x| plus
    1e-5 of the float32 product's own sum of |terms|."""
    dev = _dev(device)
    n, H, D, F = 12, 2, 6, 5
    rng = np.random.default_rng(3)
    src, dst = (torch.from_numpy(rng.integers(0, n, 50)) for _ in range(2))
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src, dst)
    q, k, v, dout = _inputs(H, D, n, n)
    want, sums = _reference(src, dst, q, k, v, dout, 0.3, (-1.0, 1.0))
    ql, kl, vl = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    out = dot_attention(g, ql, kl, vl, scale=0.3, clamp=(-1.0, 1.0))
    _check((out,) + torch.autograd.grad(out, (ql, kl, vl), dout.to(dev)), want, sums, "graph")
    torch.manual_seed(0)
    conv = DotGatConv(F, D, H).to(dev)
    x = torch.randn(n, F, device=dev)
    out = conv(g, x)
    assert out.shape == (n, H, D)
    out.backward(dout.to(dev))
    ft = conv.fc(x).detach().cpu().view(n, H, D)
    want, sums = _reference(src, dst, ft, ft, ft, dout, D ** -0.5)
    _check((out,), want, sums, "DotGatConv")
    x64 = x.cpu().double()
    dft = sum(want[1:]).reshape(n, H * D)
    bound = (sum(sums[1:]).reshape(n, H * D) + dft.abs()).t() @ x64.abs()
    err = (conv.fc.weight.grad.cpu().double() - dft.t() @ x64).abs()
    assert bool((err <= 1e-5 * bound).all()), float((err / bound).max())


def test_errors_and_empty():
    adj = _adj(False, "dst_major")
    q, k, v, _ = _inputs(3, 5)
    for bad in ((q[0], k, v), (q, k[:, :2], v[:, :2]), (q, k, v[:, :, :4]), (q[:-1], k, v),
                (q, k[:-1], v[:-1]), (k, q, q)):
        with pytest.raises(DGLError):
            kernel.dot_attention(adj, *bad)
    with pytest.raises(DGLError):
        kernel.dot_attention(adj, q, k, v, clamp=(1.0, -1.0))
    with pytest.raises(DGLError):
        kernel.dot_attention(adj, q.double(), k.double(), v.double())
    none = torch.zeros(0, dtype=torch.int64)
    out = kernel.dot_attention(kernel.from_coo(NR, NC, none, none), q, k, v)
    assert out.shape == q.shape and float(out.abs().max()) == 0.0
    assert kernel.dot_attention(adj, q[:, :0], k[:, :0], v[:, :0]).shape == (NR, 0, 5)
