"""The typed-block kernels (csrc/typed_block.hip) at every template
instantiation and launcher branch, on a graph whose row and relation lengths
are chosen to sit at the kernels' cuts: the 64-slot chunk (kernel.TYPED_CHUNK),
the 8-position LDS stage of the message and staged-dW kernels, and the 2/4/8
slot batches of the sum kernels. Forward, dH and dW against the float64 bmm
formulation (test_typed_block.reference) and, on a device, bit for bit against
the host kernels; empty graphs; special values through the idle batch slots."""
import numpy as np
import pytest
import torch

import dgl  # noqa: F401
from dgl import kernel
from test_typed_block import _MSG_DEFAULT, reference

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]

ROW_SLOTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 0)
REL_SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 129, 517)
N, M, R = len(ROW_SLOTS), sum(ROW_SLOTS), len(REL_SIZES)


def chosen_graph():
    """(src, dst, etype) by edge id: destination v has ROW_SLOTS[v] in-edges
    (the first and last rows none), relation r holds REL_SIZES[r] edges spread
    over the rows by a seeded permutation, sources uniform over the nodes, and
    the edge ids permuted so that edge id is not slot order."""
    rng = np.random.default_rng(20)
    dst = np.repeat(np.arange(N), ROW_SLOTS)
    etype = rng.permutation(np.repeat(np.arange(R), REL_SIZES))
    src = rng.integers(0, N, M)
    perm = rng.permutation(M)
    return tuple(torch.from_numpy(a[perm].astype(np.int64)) for a in (src, dst, etype))


SRC, DST, ETYPE = chosen_graph()
_ADJ = {}


def _adj(device):
    if device not in _ADJ:
        _ADJ[device] = (kernel.from_coo(N, N, DST, SRC, kernel.ORDER_EID, device),
                        ETYPE.to(device))
    return _ADJ[device]


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


def test_chosen_graph_has_the_intended_lengths():
    """The fixture's edge cases, pinned: a change to the generator must not
    quietly lose one (as test_shaped_launches_have_the_intended_items does for
    the blocked g-SpMM)."""
    assert (N, M, R) == (20, 863, 10)
    assert torch.bincount(DST, minlength=N).tolist() == list(ROW_SLOTS)
    assert torch.bincount(ETYPE, minlength=R).tolist() == list(REL_SIZES)
    assert int(SRC.min()) >= 0 and int(SRC.max()) < N
    adj, et = _adj("cpu")
    fwd = adj.fwd
    assert (fwd.indptr[1:] - fwd.indptr[:-1]).tolist() == list(ROW_SLOTS)
    assert not torch.equal(fwd.eid, torch.arange(M))  # edge id is not slot order
    # relation ids are spread over the rows, not blocked: the long rows hold
    # several relations each, and the big relation reaches most rows
    rel_of_slot = et[fwd.eid]
    assert len(set(rel_of_slot[fwd.indptr[18]:fwd.indptr[19]].tolist())) >= 5
    assert len(set(DST[ETYPE == 9].tolist())) >= 10
    want = {0: 1, 1: 1, 63: 1, 64: 1, 65: 2, 127: 2, 128: 2, 129: 3, 200: 4, 517: 9}
    item_ptr, item_row = kernel._typed_items(fwd.indptr, M)
    nit = (item_ptr[1:] - item_ptr[:-1]).tolist()
    assert nit == [want.get(d, 1) for d in ROW_SLOTS]
    assert item_row.numel() == N + -(-M // kernel.TYPED_CHUNK)
    assert item_row[:sum(nit)].tolist() == [r for r, c in enumerate(nit) for _ in range(c)]
    assert (item_row[sum(nit):] == N).all()  # the padding the kernels skip
    g = kernel._RelationGroups(fwd, et, R)
    assert (g.ptr[1:] - g.ptr[:-1]).tolist() == list(REL_SIZES)
    rel_ptr, _ = kernel._typed_items(g.ptr, M)
    assert (rel_ptr[1:] - rel_ptr[:-1]).tolist() == [want.get(d, 1) for d in REL_SIZES]


# (nb, si, so): what each reaches in csrc/typed_block.hip
SHAPES = [
    (1, 1, 1),      # Fi 1 / Fo 1 / wr 1: one output, every lane but one idle
    (16, 4, 5),     # 64 / 80 / 320: staged dW QW = 2
    (10, 8, 8),     # 80 / 80 / 640: staged dW QW = 4
    (50, 8, 8),     # 400 / 400 / 3200: sum kernel T = 4; staged dW QW = 16; one-kernel <8, 4>
    (130, 4, 4),    # 520 / 520 / 2080: message kernel Q = 4; sum in two passes; dW QW = 12, R = 4
    (600, 1, 1),    # 600 / 600 / 600: message kernel <1, 4>; staged dW QW = 4, R = 4
    (128, 8, 2),    # 1024 / 256 / 2048: forward <8, 4>; dH <2, 4> into 1024; dW QW = 8, R = 4
    (256, 4, 4),    # 1024 / 1024 / 4096: the widest staged dW, QW = 16, R = 4, 65,568 B of LDS
    (20, 16, 16),   # 320 / 320 / 5120: message path on, dW unstaged; row_scale not fused
    (8, 16, 40),    # 128 / 320 / 5120: forward by messages, dH runtime-width one-kernel, dW unstaged
    (64, 16, 16),   # 1024 / 1024 / 16384: message kernel <16, 4>; dW unstaged
    (300, 4, 4),    # 1200 / 1200 / 4800: past the message path's 1024: one-kernel forms both ways
]


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


_INPUTS, _F64, _HOST = {}, {}, {}


def _inputs(shape):
    if shape not in _INPUTS:
        nb, si, so = shape
        gen = torch.Generator().manual_seed(1000 * nb + 10 * si + so)
        h = torch.randn(N, nb * si, generator=gen)
        W = torch.randn(R, nb, si, so, generator=gen) * 0.3
        G = torch.randn(N, nb * so, generator=gen)
        norm = torch.rand(M, generator=gen) * 0.9 + 0.1
        _INPUTS[shape] = (h, W, G, norm)
    return _INPUTS[shape]


def _float64(shape, with_norm):
    """(out, dH, dW) of the float64 bmm formulation and each element's
    Σ|terms| (the same formulation over |h|, |W|, |norm|, |G|), computed once."""
    key = (shape, with_norm)
    if key not in _F64:
        h, W, G, norm = _inputs(shape)
        nm = norm.double() if with_norm else None
        res = []
        for f in (lambda t: t, torch.abs):
            h2 = f(h.double()).requires_grad_(True)
            W2 = f(W.double()).requires_grad_(True)
            out = reference(SRC, DST, ETYPE, h2, W2, N, nm)
            out.backward(f(G.double()))
            res.append((out.detach(), h2.grad, W2.grad))
        _F64[key] = res
    return _F64[key]


def _poison(dev, *numels):
    """NaNs into blocks the allocator is about to hand out again: an output
    element the kernels leave unwritten shows as NaN, not as a stale zero."""
    for n in numels:
        t = torch.full((n,), float("nan"), device=dev)
        del t


def _run(shape, with_norm, device, row_scale=None, inputs=None):
    """(out, dH, dW) of kernel.typed_block_spmm on the fixture, computed on
    ``device`` and returned on the host."""
    h, W, G, norm = inputs if inputs is not None else _inputs(shape)
    dev = torch.device(device)
    adj, et = _adj(device)
    h1 = h.to(dev).clone().requires_grad_(True)
    W1 = W.to(dev).clone().requires_grad_(True)
    _poison(dev, G.numel(), h.numel(), W.numel())
    out = kernel.typed_block_spmm(adj, h1, W1, et, norm.to(dev) if with_norm else None,
                                  None if row_scale is None else row_scale.to(dev))
    out.backward(G.to(dev))
    return out.detach().cpu(), h1.grad.cpu(), W1.grad.cpu()


def _host(shape, with_norm):
    key = (shape, with_norm)
    if key not in _HOST:
        _HOST[key] = _run(shape, with_norm, "cpu")
    return _HOST[key]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_every_instantiation_matches_float64(device, shape):
    """Forward, dH and dW on the chosen graph, with and without a per-edge
    norm, against the float64 bmm formulation: every element within
    1e-5 * Σ|terms| (the bound of test_typed_block), and exact zeros where
    that sum is zero (the two empty rows, the empty relation's dW).

    | (nb, si, so)  | Fi / Fo / nb·si·so  | what it reaches                                   |
    |---------------|---------------------|---------------------------------------------------|
    | (1, 1, 1)     | 1 / 1 / 1           | one output, every lane but one idle               |
    | (16, 4, 5)    | 64 / 80 / 320       | staged dW QW = 2                                  |
    | (10, 8, 8)    | 80 / 80 / 640       | staged dW QW = 4                                  |
    | (50, 8, 8)    | 400 / 400 / 3200    | sum kernel T = 4; staged dW QW = 16; the          |
    |               |                     | one-kernel form <8, 4> at widths 4 and 8          |
    | (130, 4, 4)   | 520 / 520 / 2080    | message kernel Q = 4; sum in two passes; staged   |
    |               |                     | dW QW = 12, R = 4                                 |
    | (600, 1, 1)   | 600 / 600 / 600     | message kernel <1, 4>; staged dW QW = 4, R = 4    |
    | (128, 8, 2)   | 1024 / 256 / 2048   | forward <8, 4>; dH <2, 4> into 1024 outputs;      |
    |               |                     | staged dW QW = 8, R = 4                           |
    | (256, 4, 4)   | 1024 / 1024 / 4096  | the widest staged dW: QW = 16, R = 4, 65,568 B    |
    |               |                     | of LDS (test_widest_staged_dw)                    |
    | (20, 16, 16)  | 320 / 320 / 5120    | message path on, dW on the unstaged kernel;       |
    |               |                     | row_scale not fused                               |
    | (8, 16, 40)   | 128 / 320 / 5120    | forward by messages, dH on the runtime-width      |
    |               |                     | one-kernel form, dW unstaged                      |
    | (64, 16, 16)  | 1024 / 1024 / 16384 | message kernel <16, 4>; dW unstaged               |
    | (300, 4, 4)   | 1200 / 1200 / 4800  | past the message path's 1024 limit: one-kernel    |
    |               |                     | forms both ways                                   |
    """
    _dev(device)
    for with_norm in (False, True):
        got = _host(shape, with_norm) if device == "cpu" else _run(shape, with_norm, device)
        want, bound = _float64(shape, with_norm)
        for g, w, b in zip(got, want, bound):
            err = (g.double() - w).abs()
            ratio = float((err / (1e-5 * b + 1e-30)).max())
            print(shape, device, with_norm, "worst err / bound = %.3g" % ratio)
            assert bool((err <= 1e-5 * b + 1e-30).all()), ratio
        out, dh, dw = got
        assert not bound[0][[0, N - 1]].any() and not bound[2][0].any()
        assert not out[[0, N - 1]].any() and not dw[0].any()
        assert out[1:N - 1].abs().sum(1).min() > 0 and dw[1:].abs().sum((1, 2, 3)).min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_every_instantiation_device_bits_equal_host(shape):
    """The shapes of test_every_instantiation_matches_float64 under the
    default settings: the device's out, dH and dW carry the host kernels' bits."""
    _dev("cuda")
    for with_norm in (True, False):
        for a, b in zip(_host(shape, with_norm), _run(shape, with_norm, "cuda")):
            assert _same_bits(a, b)


_WIDTH_SHAPES = [(50, 8, 8), (130, 4, 4), (300, 4, 4), (600, 1, 1), (128, 8, 2), (100, 5, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", _WIDTH_SHAPES, ids=_ids(_WIDTH_SHAPES))
def test_one_kernel_form_at_every_width_bits_equal_host(shape, width):
    """The one-kernel forms (messages off) at 1, 2, 4 and 8 slices of 64
    outputs per wave: typed_block_spmm_kernel<SI, T> with T up to the width,
    in one pass and in several; the host's bits at each. Block widths 8 and 4
    (the last past 1024 features), then 1, 2 (dH of 8 x 2 blocks) and 5."""
    _dev("cuda")
    for with_norm in (True, False):
        kernel.set_typed_block_width(width)
        kernel.set_typed_block_messages(0)
        try:
            got = _run(shape, with_norm, "cuda")
        finally:
            kernel.set_typed_block_width(1)
            kernel.set_typed_block_messages(_MSG_DEFAULT)
        for a, b in zip(_host(shape, with_norm), got):
            assert _same_bits(a, b)


def _stage_bytes(shape):
    nb, si, so = shape
    return 8 * (nb * si + nb * so + 1) * 4  # kMsgRows x (Fi + Fo + 1) floats


def _row_scale_bits(shape):
    h, W, G, norm = _inputs(shape)
    scale = torch.rand(N, generator=torch.Generator().manual_seed(5)) * 0.99 + 0.01
    adj, et = _adj("cpu")
    h1, W1 = h.clone().requires_grad_(True), W.clone().requires_grad_(True)
    out = kernel.typed_block_spmm(adj, h1, W1, et, norm) * scale.unsqueeze(1)
    out.backward(G)
    for a, b in zip((out.detach(), h1.grad, W1.grad),
                    _run(shape, True, "cuda", row_scale=scale)):
        assert _same_bits(a, b)


_SCALE_SHAPES = [((50, 8, 8), True), ((128, 8, 2), True), ((20, 16, 16), False),
                 ((8, 16, 40), False)]


@pytest.mark.parametrize("shape,fused", _SCALE_SHAPES, ids=_ids(s for s, _ in _SCALE_SHAPES))
def test_row_scale_fused_where_the_kernels_take_it(shape, fused):
    """kernel._typed_scale_fused: the scale rides in the kernels where the
    message path runs both ways and dW is staged, else torch's product."""
    assert kernel._typed_scale_fused(torch.device("cuda"), *shape) is fused
    assert not kernel._typed_scale_fused(torch.device("cpu"), *shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,fused", _SCALE_SHAPES, ids=_ids(s for s, _ in _SCALE_SHAPES))
def test_row_scale_bits_on_the_chosen_graph(shape, fused):
    """row_scale, fused into the kernels or not, gives the bits of
    ``typed_block_spmm(...) * scale.unsqueeze(1)`` on the host (out, dH, dW)."""
    _dev("cuda")
    assert kernel._typed_scale_fused(torch.device("cuda"), *shape) is fused
    _row_scale_bits(shape)


def test_widest_staged_dw_agrees_with_scale_fusing():
    """(256, 4, 4): Fi = Fo = 1024 and nb*si*so = 4096, the widest shape the
    staged dW takes; its stage of 8 * (1024 + 1024 + 1) floats is 65,568 B,
    32 B over 64 KiB. The launch is accepted on gfx950 (a workgroup may use up
    to the CU's 160 KiB), so the shape stays on the staged kernel and a
    row_scale stays fused: the two must agree, the unstaged kernel rejecting a
    scaled dout."""
    shape = (256, 4, 4)
    assert _stage_bytes(shape) == 65568
    assert kernel._typed_scale_fused(torch.device("cuda"), *shape)


@pytest.mark.gpu
def test_widest_staged_dw():
    """The 65,568-byte launch itself, unscaled and with a fused row_scale:
    the host's bits (a refused launch would arrive as a DGLError)."""
    _dev("cuda")
    shape = (256, 4, 4)
    for a, b in zip(_host(shape, True), _run(shape, True, "cuda")):
        assert _same_bits(a, b)
    assert kernel._typed_scale_fused(torch.device("cuda"), *shape)
    _row_scale_bits(shape)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape", [(2, 4, 3), (2, 3, 4)], ids=_ids([(2, 4, 3), (2, 3, 4)]))
def test_empty_and_degenerate(device, shape):
    """Graphs with no edges (1 and 5 nodes) and with no nodes, with and
    without enorm and row_scale: out is zeros of (n, Fo), backward gives a dH
    and a dW of zeros (tensors, not None). An empty tensor's data pointer is
    null: the entries accept that where there are no slots (include/dgl_hip.h).
    One node with three self-loops is the control. Block widths on and off the
    message path."""
    dev = _dev(device)
    nb, si, so = shape
    e = torch.empty(0, dtype=torch.int64)
    gen = torch.Generator().manual_seed(9)
    for n in (1, 5, 0):
        adj = kernel.from_coo(n, n, e, e, kernel.ORDER_EID, dev)
        for enorm in (None, torch.empty(0)):
            for rs in (None, torch.full((n,), 0.5)):
                h = torch.randn(n, nb * si, generator=gen).to(dev).requires_grad_(True)
                W = torch.randn(4, nb, si, so, generator=gen).to(dev).requires_grad_(True)
                _poison(dev, n * nb * so, h.numel(), W.numel())
                out = kernel.typed_block_spmm(adj, h, W, e.to(dev),
                                              None if enorm is None else enorm.to(dev),
                                              None if rs is None else rs.to(dev))
                assert out.shape == (n, nb * so) and not out.any()
                dh, dw = torch.autograd.grad(out, (h, W), torch.ones_like(out),
                                             allow_unused=True)
                assert dh is not None and dh.shape == h.shape and not dh.any()
                assert dw is not None and dw.shape == W.shape and not dw.any()
    z = torch.zeros(3, dtype=torch.int64)
    adj = kernel.from_coo(1, 1, z, z, kernel.ORDER_EID, dev)
    h = torch.randn(1, nb * si, generator=gen)
    W = torch.randn(4, nb, si, so, generator=gen)
    et = torch.tensor([2, 0, 2])
    h1, W1 = h.clone().to(dev).requires_grad_(True), W.clone().to(dev).requires_grad_(True)
    out = kernel.typed_block_spmm(adj, h1, W1, et.to(dev))
    out.backward(torch.ones_like(out))
    h2, W2 = h.double().requires_grad_(True), W.double().requires_grad_(True)
    ref = reference(z, z, et, h2, W2, 1)
    ref.backward(torch.ones_like(ref))
    ha, Wa = h.double().abs().requires_grad_(True), W.double().abs().requires_grad_(True)
    mag = reference(z, z, et, ha, Wa, 1)
    mag.backward(torch.ones_like(mag))
    for got, want, bound in ((out, ref, mag), (h1.grad, h2.grad, ha.grad),
                             (W1.grad, W2.grad, Wa.grad)):
        err = (got.detach().double().cpu() - want.detach()).abs()
        assert bool((err <= 1e-5 * bound.detach() + 1e-30).all())
    assert not W1.grad[1].any() and not W1.grad[3].any()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape", [(16, 4, 5), (130, 4, 4)], ids=_ids([(16, 4, 5), (130, 4, 4)]))
def test_special_values_and_idle_slots(device, shape):
    """Source and gradient rows of +inf, -inf, NaN, -0.0 and a denormal, and a
    per-edge norm of 0.0 on a fifth of the edges (0 * inf = NaN in the row
    that owns the edge). The kernels predicate idle batch slots by re-reading
    a valid slot and dropping its product: a dropped product must never reach
    a neighbour's chain. NaN and inf fall exactly where the float64
    formulation puts them, rows no special value reaches are finite, and the
    device has NaN exactly where the host has it and the host's bit pattern
    everywhere else (out, dH, dW)."""
    _dev(device)
    nb, si, so = shape
    h, W, G, norm = (t.clone() for t in _inputs(shape))
    h[2, ::3] = float("inf")
    h[5, 1::4] = float("-inf")
    h[7, 5] = float("nan")
    h[11] = -0.0
    h[13] = 1e-41
    G[1, ::so] = float("inf")    # rows of 1 to 4 slots: few sources see them
    G[2, 1::so] = float("-inf")
    G[3, 2] = float("nan")
    G[4] = -0.0
    norm[::5] = 0.0
    norm[(DST == 1) | (DST == 2)] = 0.5  # their sources' dH keeps the infinities
    zero_inf = (norm == 0) & (SRC == 5)
    assert zero_inf.any()
    host = _run(shape, True, "cpu", inputs=(h, W, G, norm))
    h2, W2 = h.double().requires_grad_(True), W.double().requires_grad_(True)
    ref = reference(SRC, DST, ETYPE, h2, W2, N, norm.double())
    ref.backward(G.double())
    for got, want in zip(host, (ref.detach(), h2.grad, W2.grad)):
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        inf = torch.isinf(want)
        assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf].double(), want[inf])
        assert bool(torch.isnan(got).any()) and bool(inf.any())  # not vacuous
    out, dh, dw = host
    assert torch.isnan(out[DST[zero_inf]]).any(1).all()  # 0 * inf, in the edge's row
    special = (SRC == 2) | (SRC == 5) | (SRC == 7)
    clean = torch.ones(N, dtype=torch.bool)
    clean[DST[special]] = False
    assert int(clean.sum()) >= 3 and torch.isfinite(out[clean]).all()
    clean = torch.ones(N, dtype=torch.bool)
    clean[SRC[(DST >= 1) & (DST <= 3)]] = False
    assert int(clean.sum()) >= 3 and torch.isfinite(dh[clean]).all()
    if device == "cpu":
        return
    for a, b in zip(host, _run(shape, True, device, inputs=(h, W, G, norm))):
        nan = torch.isnan(a)
        assert torch.equal(nan, torch.isnan(b))
        assert torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])
