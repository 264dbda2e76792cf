"""The segment reduction: the readout of a batched graph
(csrc/segment_reduce.hip)."""
from __future__ import absolute_import

import numpy as np
import torch

from .._ffi import LIB, check_call, ptr, stream_of as _stream_of
from ..base import DGLError
from .policy import RED_MAX, RED_MEAN, _RED_NAMES
from .spmm import _f32c

# ---------------------------------------------------------------------------
# Segment reduction: the readout of a batched graph (csrc/segment_reduce.hip)
# ---------------------------------------------------------------------------
SEGMENT_CHUNK = 1024  # DGLHIP_SEGMENT_CHUNK: rows per chain of the segment reduction


class SegmentOffsets(object):
    """Row ranges of a segment reduction: segment ``s`` is rows
    ``[offsets[s], offsets[s+1])``. Built from a list of sizes or an int64
    offsets tensor; keeps one copy per device, so repeated readouts of one
    batch upload the offsets once. Host-side offsets are validated here and
    give the longest segment, which lets the device call skip the chunk work
    when no segment exceeds SEGMENT_CHUNK rows."""

    def __init__(self, offsets=None, sizes=None):
        self._dev = {}
        if sizes is not None:
            sz = torch.as_tensor(np.asarray(sizes, dtype=np.int64)).reshape(-1)
            if sz.numel() and int(sz.min()) < 0:
                raise DGLError("negative segment size")
            off = torch.zeros(sz.numel() + 1, dtype=torch.int64)
            torch.cumsum(sz, 0, out=off[1:])
            self.host = off
        else:
            if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
                raise DGLError("offsets must be a 1-D int64 tensor of num_segments + 1 entries")
            off = offsets.detach().contiguous()
            if off.is_cuda:  # no host copy: nothing is read back
                self.host = None
                self._dev[off.device] = off
            else:
                self.host = off
        self.num_segments = (self.host if self.host is not None else off).numel() - 1
        self.num_rows = self.max_rows = -1
        if self.host is not None:
            h = self.host
            d = h[1:] - h[:-1]
            if int(h[0]) != 0 or (d.numel() and int(d.min()) < 0):
                raise DGLError("offsets must start at 0 and not decrease")
            self.num_rows = int(h[-1])
            self.max_rows = int(d.max()) if d.numel() else 0

    def on(self, device):
        t = self._dev.get(device)
        if t is not None:
            return t
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._dev.get(device)
        if t is None:
            src = self.host if self.host is not None else next(iter(self._dev.values()))
            t = self._dev[device] = src if device.type == "cpu" and src.device.type == "cpu" \
                else src.to(device)
        return t


def _segment_offsets(offsets):
    if isinstance(offsets, SegmentOffsets):
        return offsets
    if isinstance(offsets, torch.Tensor):
        return SegmentOffsets(offsets=offsets)
    return SegmentOffsets(sizes=offsets)


def _rows_view(x, F):
    """(tensor, row stride) of a (rows, F) float32 matrix the segment kernels
    read in place: dense rows, or the leading columns of wider rows."""
    if x.stride(1) == 1 and x.stride(0) >= F and x.shape[0] > 0 and F > 0:
        return x, x.stride(0)
    x = x.contiguous()
    return x, F


class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, w, segs, red):
        N, F = x2.shape
        B = segs.num_segments
        dev = x2.device
        off = segs.on(dev)
        xv, ldx = _rows_view(x2.detach(), F)
        wv = None if w is None else w.detach().contiguous()
        y = torch.empty(B, F, dtype=torch.float32, device=dev)
        wsum = torch.empty(B, dtype=torch.float32, device=dev) if w is not None else None
        arg = torch.empty(B, F, dtype=torch.int64, device=dev) if red == RED_MAX else None
        if N == 0:
            # no rows (and no storage to point the library at): every segment
            # is empty, 0 / 0 for the weighted mean
            y.fill_(float("nan") if red == RED_MEAN and w is not None else 0.0)
            if arg is not None:
                arg.fill_(-1)
            if wsum is not None:
                wsum.zero_()
        elif dev.type == "cuda":
            nbytes = 0
            if segs.max_rows < 0 or segs.max_rows > SEGMENT_CHUNK:
                nbytes = LIB.dglhip_segment_reduce_workspace_bytes(red, B, N, F)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
            check_call(LIB.dglhip_segment_reduce_device(
                red, B, N, F, ptr(off), ptr(xv), ldx, ptr(wv), ptr(y), ptr(wsum), ptr(arg),
                segs.max_rows, ptr(ws), _stream_of(dev)))
        else:
            check_call(LIB.dglhip_segment_reduce_host(
                red, B, N, F, ptr(off), ptr(xv), ldx, ptr(wv), ptr(y), ptr(wsum), ptr(arg), 0))
        ctx.segs, ctx.red, ctx.has_w = segs, red, w is not None
        ctx.save_for_backward(x2, w, y if (red == RED_MEAN and w is not None) else None, wsum, arg)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, w, y, wsum, arg = ctx.saved_tensors
        segs, red = ctx.segs, ctx.red
        N, F = x2.shape
        B = segs.num_segments
        dev = x2.device
        dy = _f32c(dy)
        need_dw = ctx.has_w and ctx.needs_input_grad[1]
        dx = torch.empty(N, F, dtype=torch.float32, device=dev)
        dw = torch.empty(N, dtype=torch.float32, device=dev) if need_dw else None
        xv, ldx = (_rows_view(x2.detach(), F) if need_dw else (None, F))
        wv = None if w is None else w.detach().contiguous()
        off = segs.on(dev)
        if dev.type == "cuda":
            check_call(LIB.dglhip_segment_reduce_bwd_device(
                red, B, N, F, ptr(off), ptr(dy), ptr(xv), ldx, ptr(wv), ptr(y), ptr(wsum),
                ptr(arg), ptr(dx), ptr(dw), _stream_of(dev)))
        else:
            check_call(LIB.dglhip_segment_reduce_bwd_host(
                red, B, N, F, ptr(off), ptr(dy), ptr(xv), ldx, ptr(wv), ptr(y), ptr(wsum),
                ptr(arg), ptr(dx), ptr(dw), 0))
        return dx, (dw.view(w.shape) if need_dw else None), None, None


def segment_reduce(x, offsets, reduce, weight=None):
    """``y[s] = REDUCE x[offsets[s] : offsets[s+1]]`` over consecutive row
    ranges, differentiable in ``x`` and ``weight``.

    ``x`` is ``(N, *fshape)`` float32 (any strides), ``offsets`` an int64
    tensor of ``B + 1`` offsets, a list of ``B`` sizes, or a
    :class:`SegmentOffsets` (which a caller keeps to upload the offsets once);
    ``reduce`` is ``"sum"``, ``"mean"`` or ``"max"``; ``weight`` (``(N,)`` or
    ``(N, 1)``, sum and mean only) multiplies each row first. Returns
    ``(B, *fshape)``.

    Every column is one float32 chain in row order from +0.0 (the bits of
    torch's CPU ``scatter_add_``; mean divides once, the weighted mean by the
    chain of the weights); a segment of more than SEGMENT_CHUNK rows is cut
    into chunks of that many rows whose results are combined in order. max
    propagates NaN and takes the first maximal row; an empty segment gives 0.
    Same bits on the host and on the device, no atomics."""
    if reduce not in ("sum", "mean", "max"):
        raise DGLError("unknown segment reducer %r" % (reduce,))
    red = _RED_NAMES[reduce]
    if weight is not None and red == RED_MAX:
        raise DGLError("the max segment reducer takes no weight")
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise DGLError("segment_reduce expects a tensor of rows")
    if x.dtype != torch.float32:
        raise DGLError("segment_reduce computes in float32, got %s" % x.dtype)
    segs = _segment_offsets(offsets)
    N = x.shape[0]
    fshape = tuple(x.shape[1:])
    if segs.num_rows >= 0 and segs.num_rows != N:
        raise DGLError("offsets end at %d, expected the %d rows" % (segs.num_rows, N))
    w = None
    if weight is not None:
        if weight.dtype != torch.float32:
            raise DGLError("segment_reduce computes in float32, got weight %s" % weight.dtype)
        if weight.numel() != N or tuple(weight.shape) not in ((N,), (N, 1)):
            raise DGLError("weight must have shape (%d,) or (%d, 1), got %s"
                           % (N, N, tuple(weight.shape)))
        w = weight.to(x.device)
    B = segs.num_segments
    F = 1
    for d in fshape:
        F *= d
    if B == 0 or F == 0:
        return x.new_zeros((B,) + fshape)
    if x.dim() == 2:
        return _SegmentReduce.apply(x, w, segs, red)
    return _SegmentReduce.apply(x.reshape(N, F), w, segs, red).view((B,) + fshape)
