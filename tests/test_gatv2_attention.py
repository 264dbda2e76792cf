"""kernel.gatv2_attention, dgl.nn.pytorch.gatv2_attention and GATv2Conv: GATv2
attention over each destination's in-edges, fused.

The reference is float64, computed here from the same float32 inputs with
plain torch indexing (one torch.softmax per destination's edge list), its
gradients by float64 autograd; it never calls the library. The bounds are per
element, 1e-5 x the sum of |terms| taken from the float64 values (a the
attention, z_j = fs[u_j] + fd[r], dp_j = <dout[r], fs[u_j]>, g' the leaky
relu's slope at z_j, w_j = a_j (|dp_j| + sum_i a_i |dp_i|)):

  out[r]  1e-5 * sum_j a_j |fs_j|
  dfs[u]  1e-5 * sum over u's out-edges of (a_j |dout[r]| + w_j |attn| g'(z_j))
  dfd[r]  1e-5 * sum_j w_j |attn| g'(z_j)
  dattn   1e-5 * sum over all edges of w_j |lrelu(z_j)|

fs, fd and dout are standard normal, attn standard normal times D ** -0.5, the
slope 0.2. A plain float32 torch composition on the CPU (index, leaky_relu,
sum, one softmax and one sum per destination, autograd) measured against
these bounds, worst over the shapes and this graph below: out 0.40, dfs 0.12,
dfd 0.26, dattn 0.016 of the bound (on the graph of the issue that asked for
this test: 0.29, 0.32, 0.41, 0.013). The host kernels' worst figures were out
0.03, dfs 0.37, dfd 0.38, dattn 0.16 (dattn is one float32 chain over a range
of 256 rows); on an MI355X the device kernels' were out 0.31, dfs 0.38, dfd
0.14, dattn 0.011; the tests print each (as error / sum|terms|, 1e-5 being the
bound) before they assert.

The graph is tests/test_dot_attention.py's (see its docstring for why a pair
has at most 30 to 45 copies of an edge): 40 destinations and 37 sources with
in-degrees 0, 1, 2, 3, B - 1, B, B + 1 around each of the batch constants
kernel.GATV2_BATCH, _BATCH_DFD and _BATCH_DFS, 63, 64, 65 around the 64 column
ids a wave takes per trip, 257, and C - 1, C, C + 1, 2 C + 3 around
kernel.GATV2_CHUNK; the other destinations have 150 in-edges. Every destination
of 150 or more sends 30 (45 when it has more) edges to each of the sources 0
and 1, whose out-degrees so cross the chunk too (the transposed walk's
pieces). Two edge numberings."""
import functools

import numpy as np
import pytest
import torch

import dgl
from dgl import kernel
from dgl.base import DGLError
from dgl.nn.pytorch import GATv2Conv, gatv2_attention

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
C = kernel.GATV2_CHUNK
BATCHES = sorted({kernel.GATV2_BATCH, kernel.GATV2_BATCH_DFD, kernel.GATV2_BATCH_DFS})
SHORT_DEGREES = (0, 1, 2, 3) + tuple(b + i for b in BATCHES for i in (-1, 0, 1)) + \
    (63, 64, 65, 257)
LONG_DEGREES = (C - 1, C, C + 1, 2 * C + 3)
NR, NC = 40, 37
MID_DEGREE = 150  # the destinations the lists leave over
SLOPE = 0.2
# (H, D, the long degrees too); (1, 65) is the composed path
SHAPES = [(1, 1, False), (3, 5, True), (5, 24, False), (8, 16, True), (8, 64, False),
          (1, 256, False), (1, 65, False)]
NAMES = ("out", "dfs", "dfd", "dattn")


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
    key = np.argsort(dst, kind="stable") if numbering == "dst_major" else \
        rng.permutation(dst.size)
    return torch.from_numpy(src[key].copy()), torch.from_numpy(dst[key].copy())


@functools.lru_cache(maxsize=None)
def _adj(full, numbering):
    src, dst = _edges(full, numbering)
    return kernel.from_coo(NR, NC, dst, src)


@functools.lru_cache(maxsize=None)
def _inputs(H, D, nr=NR, nc=NC):
    """fs, fd, attn, dout"""
    gen = torch.Generator().manual_seed(100 * H + D)
    fs, fd, dout = (torch.randn(n, H, D, generator=gen) for n in (nc, nr, nr))
    return fs, fd, torch.randn(H, D, generator=gen) * D ** -0.5, dout


def _reference(src, dst, fs, fd, attn, dout, slope=SLOPE):
    """float64: (out, dfs, dfd, dattn) and the bounds' sums of |terms|, in that order."""
    fs, fd, attn = (t.detach().double().requires_grad_(True) for t in (fs, fd, attn))
    dout = dout.double()
    z = fs[src] + fd[dst]
    s = (torch.nn.functional.leaky_relu(z, slope) * attn).sum(-1)
    a = torch.zeros_like(s)
    for r in range(fd.shape[0]):
        at = torch.nonzero(dst == r).flatten()
        if at.numel():
            a = a.index_put((at,), torch.softmax(s[at], 0))
    out = torch.zeros_like(fd).index_add(0, dst, a.unsqueeze(-1) * fs[src])
    grads = torch.autograd.grad(out, (fs, fd, attn), dout)
    with torch.no_grad():
        a1 = a.unsqueeze(-1)
        dp = (dout[dst] * fs[src]).sum(-1).abs()
        w = (a * (dp + torch.zeros_like(out[..., 0]).index_add(0, dst, a * dp)[dst])).unsqueeze(-1)
        score = w * attn.abs() * torch.where(z > 0, 1.0, slope)
        sums = (torch.zeros_like(fd).index_add(0, dst, a1 * fs[src].abs()),
                torch.zeros_like(fs).index_add(0, src, a1 * dout[dst].abs() + score),
                torch.zeros_like(fd).index_add(0, dst, score),
                (w * torch.nn.functional.leaky_relu(z, slope).abs()).sum(0))
    return (out.detach(),) + grads, sums


@functools.lru_cache(maxsize=None)
def _case(full, numbering, H, D):
    inputs = _inputs(H, D)
    return inputs + _reference(*_edges(full, numbering), *inputs)


def _run(adj, fs, fd, attn, dout, dev):
    """(out, dfs, dfd, dattn) of kernel.gatv2_attention on leaves of their own on ``dev``."""
    fs, fd, attn = (t.to(dev).clone().requires_grad_(True) for t in (fs, fd, attn))
    out = kernel.gatv2_attention(adj, fs, fd, attn, SLOPE)
    return (out,) + torch.autograd.grad(out, (fs, fd, attn), dout.to(dev))


def _check(got, want, sums, what, names=NAMES):
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
    composed path); a destination without in-edges gets exact zeros."""
    dev = _dev(device)
    fs, fd, attn, dout, want, sums = _case(full, numbering, H, D)
    got = _run(_adj(full, numbering), fs, fd, attn, dout, dev)
    _check(got, want, sums, "%dx%d %s" % (H, D, numbering))


@pytest.mark.parametrize("device", DEVICES)
def test_same_bits_every_call(device):
    """dattn too: its partials are added in a fixed order."""
    dev = _dev(device)
    inputs = _case(True, "shuffled", 8, 16)[:4]
    first = _run(_adj(True, "shuffled"), *inputs, dev)
    again = _run(_adj(True, "shuffled"), *inputs, dev)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("device", DEVICES)
def test_offset_views(device):
    """fs, fd and attn as views offset by one float: 5 x 24 then runs on
    single floats, 32 lanes a head."""
    dev = _dev(device)
    fs, fd, attn, dout, want, sums = _case(False, "shuffled", 5, 24)

    def offset(t):
        buf = torch.empty(t.numel() + 1, device=dev)
        buf[1:] = t.to(dev).flatten()
        return buf[1:].view(t.shape).requires_grad_(True)

    leaves = offset(fs), offset(fd), offset(attn)
    out = kernel.gatv2_attention(_adj(False, "shuffled"), *leaves, SLOPE)
    _check((out,) + torch.autograd.grad(out, leaves, dout.to(dev)), want, sums, "offset")


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("device", DEVICES)
def test_public_path(device, share):
    """dgl.nn.pytorch.gatv2_attention on a DGLGraph, and GATv2Conv forward and
    backward against the float64 formula through its parameters: the
    projections are the module's own (float32), so out keeps its bound; a
    weight gradient is dft^T x (dft = dfs for fc_src, dfd for fc_dst, their sum
    when shared), so it gets dft's bound summed over the nodes with |x| plus
    1e-5 of the float32 product's own sum of |terms|."""
    dev = _dev(device)
    n, H, D, F = 12, 2, 6, 5
    rng = np.random.default_rng(3)
    src, dst = (torch.from_numpy(rng.integers(0, n, 50)) for _ in range(2))
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src, dst)
    fs, fd, attn, dout = _inputs(H, D, n, n)
    want, sums = _reference(src, dst, fs, fd, attn, dout, 0.3)
    leaves = tuple(t.to(dev).requires_grad_(True) for t in (fs, fd, attn))
    out = gatv2_attention(g, *leaves, negative_slope=0.3)
    _check((out,) + torch.autograd.grad(out, leaves, dout.to(dev)), want, sums, "graph")
    torch.manual_seed(0)
    conv = GATv2Conv(F, D, H, share_weights=share).to(dev)
    assert (conv.fc_dst is conv.fc_src) == share and conv.attn.shape == (1, H, D)
    x = torch.randn(n, F, device=dev)
    out = conv(g, x)
    assert out.shape == (n, H, D)
    out.backward(dout.to(dev))
    fs, fd = (fc(x).detach().cpu().view(n, H, D) for fc in (conv.fc_src, conv.fc_dst))
    want, sums = _reference(src, dst, fs, fd, conv.attn.detach().cpu()[0], dout)
    _check((out, conv.attn.grad[0]), want[::3], sums[::3], "GATv2Conv", ("out", "dattn"))
    x64 = x.cpu().double()
    for fc, which in ((conv.fc_src, (1, 2) if share else (1,)), (conv.fc_dst, (2,))):
        dft = sum(want[i] for i in which).reshape(n, H * D)
        bound = (sum(sums[i] for i in which).reshape(n, H * D) + dft.abs()).t() @ x64.abs()
        err = (fc.weight.grad.cpu().double() - dft.t() @ x64).abs()
        assert bool((err <= 1e-5 * bound).all()), float((err / bound).max())
        if share:
            break


@pytest.mark.parametrize("device", DEVICES)
def test_attention_dropout(device):
    """attn_drop > 0: in eval() the fused operator's bits, in train() the
    composition with torch dropout runs and differentiates."""
    dev = _dev(device)
    n, H, D = NR, 3, 5
    src, dst = _edges(False, "shuffled")
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src, dst)
    torch.manual_seed(0)
    conv = GATv2Conv(7, D, H, attn_drop=0.5).to(dev)
    x = torch.randn(n, 7, device=dev)
    fs, fd = (fc(x).view(n, H, D) for fc in (conv.fc_src, conv.fc_dst))
    fused = kernel.gatv2_attention(g.sparse_adjacency(dev), fs, fd, conv.attn)
    assert torch.equal(conv.eval()(g, x), fused)
    out = conv.train()(g, x)
    assert out.shape == (n, H, D) and not torch.equal(out, fused)
    out.sum().backward()
    assert conv.attn.grad.shape == (1, H, D) and bool(torch.isfinite(conv.attn.grad).all())


def test_errors_and_empty():
    adj = _adj(False, "dst_major")
    fs, fd, attn, _ = _inputs(3, 5)
    for bad in ((fs[0], fd, attn), (fs, fd[:, :2], attn), (fs[:, :, :4], fd[:, :, :4], attn),
                (fs, fd, attn[:2]), (fs, fd, attn[0]), (fs[:-1], fd, attn), (fs, fd[:-1], attn),
                (fd, fs, attn), (fs.double(), fd.double(), attn.double())):
        with pytest.raises(DGLError):
            kernel.gatv2_attention(adj, *bad)
    with pytest.raises(DGLError):
        kernel.gatv2_attention(adj, fs, fd, attn, attn_drop=1.0)
    none = torch.zeros(0, dtype=torch.int64)
    out = kernel.gatv2_attention(kernel.from_coo(NR, NC, none, none), fs, fd, attn)
    assert out.shape == fd.shape and float(out.abs().max()) == 0.0
    assert kernel.gatv2_attention(adj, fs[:, :0], fd[:, :0], attn[:0]).shape == (NR, 0, 5)
