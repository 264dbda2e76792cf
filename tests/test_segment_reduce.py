"""kernel.segment_reduce: y[s] = REDUCE x[offsets[s]:offsets[s+1]], the
readout of a batched graph.

The forward is compared bit for bit (int32 views) with a numpy float32
restatement of the chain and chunk rule (a chain from +0.0 in row order per
column, products rounded before the add, segments longer than
kernel.SEGMENT_CHUNK rows cut into chunks whose results are combined in order)
and, for segments of at most one chunk, with torch on the CPU running the
reference's readout formulas (zeros.scatter_add_, /= count.clamp(min=1),
weight * feat first, weighted mean y / w, torch.max per segment). The backward
is bit-equal to torch's CPU autograd where an element is a single product or
quotient, and within 1e-5 * sum|terms| of float64 autograd elsewhere.

Weights of the tolerance-checked weighted-mean gradients are positive: every
such gradient carries a factor 1 / W[s] with W the float32 chain of the
weights, whose own relative error is n * eps * sum|w| / |W|, so the 1e-5 bound
is a statement about the gradient only where the weight sum does not cancel
(the |terms| below are the terms of the float64 formulas with every factor
replaced by its magnitude)."""
import functools

import numpy as np
import pytest
import torch

from dgl import _ffi, kernel
from dgl.base import DGLError

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
C = kernel.SEGMENT_CHUNK
SIZES = [0, 1, 3, 63, 64, 65, 0, 257, 0]
LONG_SIZES = [C - 1, C, C + 1, 2 * C + 3]
VARIANTS = [("sum", False), ("sum", True), ("mean", False), ("mean", True), ("max", False)]


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _inputs(sizes, F, seed=0):
    """x with magnitudes over several decades (the order of a sum changes its
    bits), rows of -0.0 inside one segment and a segment of only -0.0."""
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    x = (rng.standard_normal((N, F)) * np.exp(3 * rng.standard_normal((N, 1)))).astype(np.float32)
    w = (rng.standard_normal(N) * np.exp(rng.standard_normal(N))).astype(np.float32)
    off = _offsets(sizes)
    if len(sizes) > 3 and sizes[2] == 3:
        x[off[2]:off[3]] = -0.0  # a segment of only -0.0
        x[off[3] + 2:off[3] + 5] = -0.0  # rows of -0.0 among others
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


def _chunk(x, w, p, q, reduce):
    F = x.shape[1]
    if reduce == "max":
        if p >= q:
            return np.zeros(F, np.float32), np.full(F, -1, np.int64), np.float32(0)
        val, arg = x[p].copy(), np.full(F, p, np.int64)
        for r in range(p + 1, q):
            upd = ~np.isnan(val) & ((x[r] > val) | np.isnan(x[r]))
            val[upd] = x[r][upd]
            arg[upd] = r
        return val, arg, np.float32(0)
    acc, wacc = np.zeros(F, np.float32), np.float32(0)
    for r in range(p, q):
        acc = acc + (x[r] if w is None else w[r] * x[r])
        if w is not None:
            wacc = np.float32(wacc + w[r])
    return acc, None, wacc


def _chain(x, sizes, reduce, w=None):
    """The chain and chunk rule in numpy float32: (y, arg)."""
    off = _offsets(sizes)
    B, F = len(sizes), x.shape[1]
    y = np.zeros((B, F), np.float32)
    arg = np.full((B, F), -1, np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(B):
            beg, end = int(off[s]), int(off[s + 1])
            tot, targ, wtot = _chunk(x, w, beg, min(end, beg + C), reduce)
            for p in range(beg + C, end, C):
                part, parg, wp = _chunk(x, w, p, min(end, p + C), reduce)
                if reduce == "max":
                    upd = ~np.isnan(tot) & ((part > tot) | np.isnan(part))
                    tot[upd] = part[upd]
                    targ[upd] = parg[upd]
                else:
                    tot = tot + part
                    wtot = np.float32(wtot + wp)
            if reduce == "mean":
                tot = tot / (wtot if w is not None else np.float32(max(end - beg, 1)))
            y[s] = tot
            if reduce == "max":
                arg[s] = targ
    return y, arg


@functools.lru_cache(maxsize=None)
def _chain_case(sizes, F, reduce, weighted):
    x, w = _inputs(sizes, F)
    return _chain(x, sizes, reduce, w if weighted else None)


def _torch_formula(x, sizes, reduce, w=None):
    """The reference's readout formulas (python/dgl/batched_graph.py) on the
    tensors given: (y, arg)."""
    B, (N, F) = len(sizes), x.shape
    seg = torch.arange(B).repeat_interleave(torch.tensor(sizes, dtype=torch.int64))
    seg = seg.to(x.device)
    if reduce == "max":
        ys, args, beg = [], [], 0
        for n in sizes:
            if n == 0:
                ys.append(torch.zeros(F, dtype=x.dtype))
                args.append(torch.full((F,), -1, dtype=torch.int64))
            else:
                v, i = torch.max(x[beg:beg + n], 0)
                ys.append(v)
                args.append(i + beg)
            beg += n
        return torch.stack(ys), torch.stack(args)
    feat = x if w is None else w.view(-1, 1) * x
    y = torch.zeros(B, F, dtype=x.dtype).scatter_add_(0, seg[:, None].expand(-1, F), feat)
    if reduce == "mean":
        if w is None:
            cnt = torch.zeros(B, dtype=x.dtype).scatter_add_(0, seg, torch.ones(N, dtype=x.dtype))
            y = y / cnt.clamp(min=1)[:, None]
        else:
            ws = torch.zeros(B, 1, dtype=x.dtype).scatter_add_(0, seg[:, None], w.view(-1, 1))
            y = y / ws
    return y, None


def _same_bits(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    nan = np.isnan(ref)
    return (got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and
            np.array_equal(got.view(np.int32)[~nan], ref.view(np.int32)[~nan]))


def _run(x, sizes, reduce, w, dev, offsets_as="list"):
    xd = torch.from_numpy(np.array(x)).to(dev)
    wd = None if w is None else torch.from_numpy(np.array(w)).to(dev)
    off = list(sizes) if offsets_as == "list" else torch.from_numpy(_offsets(sizes)).to(dev)
    return kernel.segment_reduce(xd, off, reduce, wd)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [1, 4, 5, 41, 128, 130])
def test_forward_bits(device, F):
    dev = _dev(device)
    sizes = tuple(SIZES)
    x, w = _inputs(sizes, F)
    for reduce, weighted in VARIANTS:
        ref, _ = _chain_case(sizes, F, reduce, weighted)
        got = _run(x, sizes, reduce, w if weighted else None, dev).cpu().numpy()
        assert _same_bits(got, ref), (reduce, weighted)
        # every segment is at most one chunk: the reference's formulas on the CPU
        tref, _ = _torch_formula(torch.from_numpy(np.array(x)), sizes, reduce,
                                 torch.from_numpy(np.array(w)) if weighted else None)
        assert _same_bits(got, tref.numpy()), (reduce, weighted)
    # a segment of only -0.0 sums to +0.0 (the chain starts from +0.0)
    y = _run(x, sizes, "sum", None, dev).cpu().numpy()
    assert not np.signbit(y[2]).any() and (y[2] == 0).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("B,F", [(1100, 256), (4200, 64)])
def test_many_segments(device, B, F):
    """Enough segments for a launch of more than 1024 waves, from which the
    device kernel reads 16 bytes per lane (below, one column per lane, which
    the few-segment cases above run): one segment per wave at F = 256, four
    packed into a wave at F = 64."""
    dev = _dev(device)
    sizes = ([0, 1, 2, 3, 17] * (B // 5 + 1))[:B]
    sizes[7] = 2 * C + 3  # and one of several chunks: 16-byte partials
    sizes = tuple(sizes)
    x, w = _inputs(sizes, F)
    for reduce, weighted in (("sum", True), ("mean", False), ("max", False)):
        ref, _ = _chain_case(sizes, F, reduce, weighted)
        got = _run(x, sizes, reduce, w if weighted else None, dev).cpu().numpy()
        assert _same_bits(got, ref), (reduce, weighted)


@pytest.mark.parametrize("device", DEVICES)
def test_long_segments(device):
    dev = _dev(device)
    sizes, F = tuple(LONG_SIZES), 5
    x, w = _inputs(sizes, F)
    for reduce, weighted in VARIANTS:
        ref, rarg = _chain_case(sizes, F, reduce, weighted)
        # offsets as a device tensor: the kernel finds the chunks from the sizes alone
        got = _run(x, sizes, reduce, w if weighted else None, dev, "tensor").cpu().numpy()
        assert _same_bits(got, ref), (reduce, weighted)
        again = _run(x, sizes, reduce, w if weighted else None, dev).cpu().numpy()
        assert _same_bits(again, got), (reduce, weighted)
        tref, _ = _torch_formula(torch.from_numpy(np.array(x)), sizes, reduce,
                                 torch.from_numpy(np.array(w)) if weighted else None)
        short = np.array(sizes) <= C
        assert _same_bits(got[short], tref.numpy()[short]), (reduce, weighted)
        if reduce == "max":  # exact under chunking
            assert np.array_equal(got, tref.numpy())
    # chunked sums against float64, per element
    got = _run(x, sizes, "sum", None, dev).cpu().numpy()
    off = _offsets(sizes)
    x64 = x.astype(np.float64)
    for s in range(len(sizes)):
        exact = x64[off[s]:off[s + 1]].sum(0)
        bound = 1e-5 * np.abs(x64[off[s]:off[s + 1]]).sum(0)
        err = np.abs(got[s] - exact)
        print("segment", s, "max err / bound", float((err / bound).max()))
        assert (err <= bound).all()


@pytest.mark.parametrize("device", DEVICES)
def test_feature_shapes_and_strides(device):
    dev = _dev(device)
    sizes = tuple(SIZES)
    x, w = _inputs(sizes, 12)
    N = x.shape[0]
    for reduce, weighted in VARIANTS:
        ref, _ = _chain_case(sizes, 12, reduce, weighted)
        wd = torch.from_numpy(np.array(w)).to(dev).view(N, 1) if weighted else None
        x3 = torch.from_numpy(np.array(x)).to(dev).view(N, 4, 3)
        y = kernel.segment_reduce(x3, list(sizes), reduce, wd)
        assert tuple(y.shape) == (len(sizes), 4, 3)
        assert _same_bits(y.cpu().numpy().reshape(-1, 12), ref)
    # a column slice of a wider tensor, at an aligned and at an unaligned offset
    for F, lo, width in ((8, 4, 16), (5, 3, 11)):
        xs, _ = _inputs(sizes, width)
        wide = torch.from_numpy(np.array(xs)).to(dev)
        part = wide[:, lo:lo + F]
        assert not part.is_contiguous()
        for reduce in ("sum", "max"):
            ref, _ = _chain(np.ascontiguousarray(xs[:, lo:lo + F]), sizes, reduce)
            got = kernel.segment_reduce(part, list(sizes), reduce)
            assert _same_bits(got.cpu().numpy(), ref), (F, reduce)


def _max_case():
    """Ties inside a segment, ties across a chunk boundary, one NaN, two NaNs,
    rows of -inf."""
    rng = np.random.default_rng(5)
    sizes = [6, 2 * C + 2, 5, 4, 3, 0]
    F = 4
    x = rng.standard_normal((sum(sizes), F)).astype(np.float32)
    off = _offsets(sizes)
    x[off[0] + 1] = x[off[0] + 4] = 9.0  # ties: the first wins
    b = off[1]
    x[b + C - 1, :2] = 50.0  # the maximum at the end of chunk 0 ...
    x[b + C, :2] = 50.0  # ... again at the start of chunk 1
    x[b + 2 * C + 1, 1] = 50.0
    x[b + 5, 2] = 70.0
    x[b + C + 7, 2] = 70.0  # a tie across chunks that are not neighbours in the value
    x[b + 2 * C, 3] = 80.0  # the maximum in the last chunk
    x[off[2] + 3, 0] = np.nan  # one NaN
    x[off[3] + 1, 1] = np.nan  # two NaNs: the first is reported
    x[off[3] + 3, 1] = np.nan
    x[off[4]:off[5]] = -np.inf  # only -inf rows
    x[off[2], 2] = -np.inf
    return x, sizes


def _capi_forward(red, xd, sizes):
    """The C entry point of xd's device: (y, arg)."""
    (N, F), B, dev = xd.shape, len(sizes), xd.device
    off = torch.from_numpy(_offsets(sizes)).to(dev)
    y = torch.empty(B, F, device=dev)
    arg = torch.empty(B, F, dtype=torch.int64, device=dev)
    p = _ffi.ptr
    if dev.type == "cuda":
        nbytes = _ffi.LIB.dglhip_segment_reduce_workspace_bytes(red, B, N, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ffi.check_call(_ffi.LIB.dglhip_segment_reduce_device(
            red, B, N, F, p(off), p(xd), F, None, p(y), None, p(arg), -1, p(ws),
            kernel._stream_of(dev)))
    else:
        _ffi.check_call(_ffi.LIB.dglhip_segment_reduce_host(
            red, B, N, F, p(off), p(xd), F, None, p(y), None, p(arg), 0))
    return y, arg


@pytest.mark.parametrize("device", DEVICES)
def test_max_values_and_arg(device):
    dev = _dev(device)
    x, sizes = _max_case()
    tv, ta = _torch_formula(torch.from_numpy(x), sizes, "max")
    cv, ca = _chain(x, sizes, "max")
    assert _same_bits(cv, tv.numpy()) and np.array_equal(ca, ta.numpy())
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    y = kernel.segment_reduce(xd, sizes, "max")
    assert _same_bits(y.detach().cpu().numpy(), tv.numpy())
    _, arg = _capi_forward(kernel.RED_MAX, xd.detach(), sizes)
    assert np.array_equal(arg.cpu().numpy(), ta.numpy())
    # backward: the gradient goes to the reported row only, bit for bit as
    # torch's CPU autograd of the per-segment torch.max
    dy = torch.from_numpy(np.random.default_rng(6).standard_normal(tuple(y.shape))
                          .astype(np.float32))
    y.backward(dy.to(dev))
    xt = torch.from_numpy(x).requires_grad_(True)
    vals, beg = [], 0
    for n in sizes:
        vals.append(torch.max(xt[beg:beg + n], 0)[0] if n else xt.new_zeros(x.shape[1]))
        beg += n
    torch.stack(vals).backward(dy)
    assert _same_bits(xd.grad.cpu().numpy(), xt.grad.numpy())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_backward_writes_every_element(device, reduce):
    """The backward entry point on a dx buffer pre-filled with NaN: every
    element is written (no memset, nothing accumulated)."""
    dev = _dev(device)
    x, sizes = _max_case()
    N, F = x.shape
    B = len(sizes)
    red = {"sum": kernel.RED_SUM, "mean": kernel.RED_MEAN, "max": kernel.RED_MAX}[reduce]
    xd = torch.from_numpy(x).to(dev)
    off = torch.from_numpy(_offsets(sizes)).to(dev)
    y, arg = _capi_forward(red, xd, sizes)
    dy = torch.ones(B, F, device=dev)
    dx = torch.full((N, F), float("nan"), device=dev)
    p = _ffi.ptr
    if dev.type == "cuda":
        _ffi.check_call(_ffi.LIB.dglhip_segment_reduce_bwd_device(
            red, B, N, F, p(off), p(dy), None, F, None, None, None, p(arg), p(dx), None,
            kernel._stream_of(dev)))
    else:
        _ffi.check_call(_ffi.LIB.dglhip_segment_reduce_bwd_host(
            red, B, N, F, p(off), p(dy), None, F, None, None, None, p(arg), p(dx), None, 0))
    got = dx.cpu().numpy()
    assert not np.isnan(got).any()
    if reduce == "max":  # one row per (segment, column) of a non-empty segment
        assert got.sum() == F * sum(1 for n in sizes if n)
    elif reduce == "sum":
        assert (got == 1).all()


def _grad_inputs(F, seed=11):
    sizes = tuple(SIZES)
    x, _ = _inputs(sizes, F)
    rng = np.random.default_rng(seed)
    w = (0.25 + rng.random(x.shape[0])).astype(np.float32)  # positive: see the module docstring
    dy = rng.standard_normal((len(sizes), F)).astype(np.float32)
    return sizes, np.array(x), w, dy


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [1, 5, 128])
def test_backward_sum_mean(device, F):
    dev = _dev(device)
    sizes, x, w, dy = _grad_inputs(F)
    for reduce, weighted in VARIANTS[:4]:
        xd = torch.from_numpy(x).to(dev).requires_grad_(True)
        wd = torch.from_numpy(w).to(dev).requires_grad_(True) if weighted else None
        kernel.segment_reduce(xd, list(sizes), reduce, wd).backward(torch.from_numpy(dy).to(dev))
        grads = {}
        for dt in (torch.float32, torch.float64):
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            wt = torch.from_numpy(w).to(dt).requires_grad_(True) if weighted else None
            yt, _ = _torch_formula(xt, sizes, reduce, wt)
            yt.backward(torch.from_numpy(dy).to(dt))
            grads[dt] = (xt.grad, wt.grad if weighted else None)
        gx = xd.grad.cpu()
        if not (reduce == "mean" and weighted):
            # a single product or quotient per element: torch's float32 bits
            assert _same_bits(gx.numpy(), grads[torch.float32][0].numpy()), (reduce, weighted)
        if not weighted:
            continue
        # |terms| of the float64 formulas
        seg = torch.arange(len(sizes)).repeat_interleave(torch.tensor(sizes))
        ax, aw = torch.from_numpy(x).double().abs(), torch.from_numpy(w).double()
        ady = torch.from_numpy(dy).double().abs()[seg]  # (N, F)
        if reduce == "sum":
            tx, tw = ady * aw[:, None], (ady * ax).sum(1)
        else:
            W = torch.zeros(len(sizes), dtype=torch.float64).scatter_add_(0, seg, aw)[seg]
            S = torch.zeros(len(sizes), F, dtype=torch.float64).scatter_add_(
                0, seg[:, None].expand(-1, F), aw[:, None] * ax)[seg]
            tx = ady * aw[:, None] / W[:, None]
            tw = (ady * ax).sum(1) / W + (ady * S).sum(1) / W ** 2
        ex = (gx.double() - grads[torch.float64][0]).abs()
        ew = (wd.grad.cpu().double() - grads[torch.float64][1]).abs()
        print(reduce, "F", F, "dx err/bound", float((ex / (1e-5 * tx)).nan_to_num().max()),
              "dw err/bound", float((ew / (1e-5 * tw)).nan_to_num().max()))
        assert (ex <= 1e-5 * tx).all(), (reduce, "dx")
        assert (ew <= 1e-5 * tw).all(), (reduce, "dw")


def test_degenerate_and_errors():
    x = torch.randn(5, 3)
    assert tuple(kernel.segment_reduce(x[:0], [], "sum").shape) == (0, 3)
    assert tuple(kernel.segment_reduce(x[:0].view(0, 3, 1), [], "max").shape) == (0, 3, 1)
    for reduce in ("sum", "mean", "max"):
        y = kernel.segment_reduce(x[:0], [0, 0], reduce)
        assert tuple(y.shape) == (2, 3) and (y == 0).all()
    with pytest.raises(DGLError):
        kernel.segment_reduce(x, [5], "max", torch.ones(5))
    with pytest.raises(DGLError):
        kernel.segment_reduce(x.double(), [5], "sum")
    with pytest.raises(DGLError):
        kernel.segment_reduce(x, [5], "prod")
    with pytest.raises(DGLError):
        kernel.segment_reduce(x, [5], "sum", torch.ones(4))
    with pytest.raises(DGLError):  # offsets not ending at N
        kernel.segment_reduce(x, torch.tensor([0, 2, 4]), "sum")
    with pytest.raises(DGLError):
        kernel.segment_reduce(x, torch.tensor([0, 3, 2, 5]), "sum")
    # the host entry point itself rejects them: -1 and a message
    off = torch.tensor([0, 2, 4])
    y = torch.empty(2, 3)
    rc = _ffi.LIB.dglhip_segment_reduce_host(kernel.RED_SUM, 2, 5, 3, _ffi.ptr(off), _ffi.ptr(x),
                                             3, None, _ffi.ptr(y), None, None, 0)
    assert rc == -1 and b"offsets end at 4" in _ffi.LIB.DGLGetLastError()
    with pytest.raises(DGLError):
        _ffi.check_call(rc)


def test_offsets_upload_is_cached():
    segs = kernel.SegmentOffsets(sizes=[2, 3])
    assert segs.on("cpu") is segs.on("cpu")
    assert segs.num_segments == 2 and segs.num_rows == 5 and segs.max_rows == 3
    x = torch.arange(10, dtype=torch.float32).view(5, 2)
    assert kernel.segment_reduce(x, segs, "sum").tolist() == [[2, 4], [18, 21]]


@pytest.mark.gpu
def test_host_and_device_agree():
    dev = _dev("cuda")
    for sizes, F in ((tuple(SIZES), 41), (tuple(SIZES), 128), (tuple(LONG_SIZES), 5)):
        x, w = _inputs(sizes, F)
        dy = torch.from_numpy(np.random.default_rng(2).standard_normal((len(sizes), F))
                              .astype(np.float32))
        for reduce, weighted in VARIANTS:
            out = []
            for d in (torch.device("cpu"), dev):
                xd = torch.from_numpy(np.array(x)).to(d).requires_grad_(True)
                wd = torch.from_numpy(np.array(w)).to(d) if weighted else None
                y = kernel.segment_reduce(xd, list(sizes), reduce, wd)
                y.backward(dy.to(d))
                out.append((y.detach().cpu().numpy(), xd.grad.cpu().numpy()))
            assert _same_bits(out[1][0], out[0][0]), (reduce, weighted, "y")
            assert _same_bits(out[1][1], out[0][1]), (reduce, weighted, "dx")
