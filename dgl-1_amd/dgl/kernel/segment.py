"""The segment reduction (csrc/segment_reduce.hip) and the segment top-k
(csrc/segment_topk.hip): the readouts of a batched graph; and the segment
k-nearest neighbours (csrc/segment_knn.hip): the graph of a batch of point
clouds; and the segment farthest point sampling (csrc/segment_fps.hip): the
centroids of a batch of point clouds; and the segment fixed-radius neighbours
(csrc/segment_radius.hip): the ball query round those centroids."""
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
TOPK_CHUNK = 2048  # DGLHIP_TOPK_CHUNK: rows one workgroup ranks in LDS, and the largest k
KNN_MAX_K = 64  # DGLHIP_KNN_MAX_K: the longest neighbour list of the segment kNN
KNN_MAX_DIM = 256  # DGLHIP_KNN_MAX_DIM: the most coordinates of its points
FPS_MAX_DIM = 256  # DGLHIP_FPS_MAX_DIM: the most coordinates of a sampled point
RADIUS_MAX_K = 64  # DGLHIP_RADIUS_MAX_K: the longest member list of the ball query
RADIUS_MAX_DIM = 16  # DGLHIP_RADIUS_MAX_DIM: the most coordinates of its points
_RADIUS_EXCLUDE_SELF, _RADIUS_PAD_FIRST = 1, 2  # DGLHIP_RADIUS_*: the flags


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


# ---------------------------------------------------------------------------
# Segment top-k: topk_nodes / topk_edges, SortPooling (csrc/segment_topk.hip)
# ---------------------------------------------------------------------------
class _SegmentTopk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, segs, k, descending, sortby):
        N, F = x2.shape
        B = segs.num_segments
        dev = x2.device
        values = torch.empty(B, k, F, dtype=torch.float32, device=dev)
        indices = torch.empty((B, k) if sortby >= 0 else (B, k, F), dtype=torch.int64,
                              device=dev)
        if N == 0:  # no rows (and no storage to point the library at): all padding
            values.zero_()
            indices.fill_(-1)
        else:
            off = segs.on(dev)
            xv, ldx = _rows_view(x2.detach(), F)
            if dev.type == "cuda":
                nbytes = 0
                if segs.max_rows < 0 or segs.max_rows > TOPK_CHUNK:
                    nbytes = LIB.dglhip_segment_topk_workspace_bytes(B, N, F, k, descending,
                                                                     sortby)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
                check_call(LIB.dglhip_segment_topk_device(
                    B, N, F, k, descending, sortby, ptr(off), ptr(xv), ldx, ptr(values),
                    ptr(indices), segs.max_rows, ptr(ws), _stream_of(dev)))
            else:
                check_call(LIB.dglhip_segment_topk_host(
                    B, N, F, k, descending, sortby, ptr(off), ptr(xv), ldx, ptr(values),
                    ptr(indices), 0))
        ctx.segs, ctx.args = segs, (N, F, k, descending, sortby)
        ctx.save_for_backward(indices)
        ctx.mark_non_differentiable(indices)
        return values, indices

    @staticmethod
    def backward(ctx, dy, _):
        indices, = ctx.saved_tensors
        N, F, k, descending, sortby = ctx.args
        segs = ctx.segs
        dev = indices.device
        dy = _f32c(dy)
        dx = torch.empty(N, F, dtype=torch.float32, device=dev)
        fn = LIB.dglhip_segment_topk_bwd_device if dev.type == "cuda" \
            else LIB.dglhip_segment_topk_bwd_host
        check_call(fn(segs.num_segments, N, F, k, descending, sortby, ptr(segs.on(dev)), ptr(dy),
                      ptr(indices), ptr(dx), _stream_of(dev) if dev.type == "cuda" else 0))
        return dx, None, None, None, None


def segment_topk(x, offsets, k, descending=True, sortby=None):
    """The first ``k`` rows of every segment ``x[offsets[s] : offsets[s+1]]``
    in sorted order, differentiable in ``x``.

    ``x`` is ``(N, *fshape)`` float32 (any strides) with ``F`` elements per
    row, ``offsets`` what :func:`segment_reduce` takes, ``1 <= k <=
    TOPK_CHUNK``. ``sortby=None`` ranks every column on its own and returns
    ``values (B, k, *fshape)`` and int64 ``indices (B, k, *fshape)``:
    ``values[s, j, f]`` is the j-th element of column ``f`` of segment ``s``
    and ``indices[s, j, f]`` its row within the segment. ``sortby=c`` (``-F <=
    c < F``, a position of the flattened row) ranks whole rows by column ``c``
    and returns the selected rows ``values (B, k, *fshape)`` and ``indices (B,
    k)``.

    The order is that of ``torch.sort(stable=True, descending=descending)`` on
    the CPU: descending puts NaN first and then decreasing values, ascending
    increasing values and NaN last; ``+0.0 == -0.0``, all NaNs are equal, and
    among equal keys the lower row comes first. Values are moved, never
    computed, so the output bits are the input bits. A segment of fewer than
    ``k`` rows fills the remaining slots with ``+0.0`` and index ``-1``. Same
    bits on the host and on the device, no atomics; ``k > TOPK_CHUNK`` is an
    error, not another path."""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise DGLError("segment_topk expects a tensor of rows")
    if x.dtype != torch.float32:
        raise DGLError("segment_topk ranks float32, got %s" % x.dtype)
    k = int(k)
    if k < 1 or k > TOPK_CHUNK:
        raise DGLError("segment_topk serves 1 <= k <= TOPK_CHUNK = %d, got k = %d"
                       % (TOPK_CHUNK, k))
    segs = _segment_offsets(offsets)
    N = x.shape[0]
    fshape = tuple(x.shape[1:])
    if segs.num_rows >= 0 and segs.num_rows != N:
        raise DGLError("offsets end at %d, expected the %d rows" % (segs.num_rows, N))
    B = segs.num_segments
    F = 1
    for d in fshape:
        F *= d
    col = -1
    if sortby is not None:
        col = int(sortby)
        if col < -F or col >= F:
            raise DGLError("sortby = %d is no column of rows of %d elements" % (col, F))
        col %= F
    if B == 0 or F == 0:
        return (x.new_zeros((B, k) + fshape),
                torch.full((B, k) + (fshape if col < 0 else ()), -1, dtype=torch.int64,
                           device=x.device))
    values, indices = _SegmentTopk.apply(x.reshape(N, F), segs, k, 1 if descending else 0, col)
    values = values.view((B, k) + fshape)
    return values, (indices if col >= 0 else indices.view((B, k) + fshape))


# ---------------------------------------------------------------------------
# Segment k-nearest neighbours: knn_graph / segmented_knn_graph (csrc/segment_knn.hip)
# ---------------------------------------------------------------------------
def segment_knn(x, offsets, k, exclude_self=False):
    """For every row ``i`` of every segment ``x[offsets[s] : offsets[s+1]]``
    the ``k`` rows ``j`` of the same segment nearest to it: ``(nbr, dist)``,
    ``nbr (N, k)`` int64 global row ids and ``dist (N, k)`` float32 squared
    Euclidean distances, both ascending. Not differentiable.

    ``x`` is ``(N, D)`` float32 (read in place through its row stride),
    ``offsets`` what :func:`segment_reduce` takes, ``1 <= k <= KNN_MAX_K`` and
    ``D <= KNN_MAX_DIM``; outside is an error, not another path.

    In float32, ``d(i, j) = n_i + n_j - 2 <x_i, x_j>`` with ``n_i = <x_i,
    x_i>``; a value not above zero is ``+0.0``, a NaN stays NaN, ``d(i, i)``
    is ``+0.0`` by definition and with ``exclude_self`` the pair ``(i, i)`` is
    no candidate. The order is ascending by ``(d, j)``, NaN last: an ascending
    stable sort, so no tie is left to chance. A row with fewer than ``k``
    candidates fills the remaining slots with ``-1`` and ``+inf``. On a ROCm
    device the dot products run on the f32 MFMA and the selection in the same
    pass: no distance matrix is written. Host and device each return the
    exact top-k under their own float32 distances; where the arithmetic is
    exact they agree index for index."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise DGLError("segment_knn expects an (N, D) tensor of points")
    if x.dtype != torch.float32:
        raise DGLError("segment_knn computes in float32, got %s" % x.dtype)
    k = int(k)
    if k < 1 or k > KNN_MAX_K:
        raise DGLError("segment_knn serves 1 <= k <= KNN_MAX_K = %d, got k = %d" % (KNN_MAX_K, k))
    N, D = x.shape
    if D > KNN_MAX_DIM:
        raise DGLError("segment_knn serves D <= KNN_MAX_DIM = %d, got D = %d" % (KNN_MAX_DIM, D))
    segs = _segment_offsets(offsets)
    if segs.num_rows >= 0 and segs.num_rows != N:
        raise DGLError("offsets end at %d, expected the %d rows" % (segs.num_rows, N))
    B, dev = segs.num_segments, x.device
    nbr = torch.full((N, k), -1, dtype=torch.int64, device=dev)
    dist = torch.full((N, k), float("inf"), dtype=torch.float32, device=dev)
    if N == 0 or B == 0:
        return nbr, dist
    if D == 0:  # no storage to point the library at: every distance is +0.0
        x, D = x.new_zeros(N, 1), 1
    off = segs.on(dev)
    xv, ldx = _rows_view(x.detach(), D)
    if dev.type == "cuda":
        ws = torch.empty(LIB.dglhip_segment_knn_workspace_bytes(B, N, D, k), dtype=torch.uint8,
                         device=dev)
        check_call(LIB.dglhip_segment_knn_device(
            B, N, D, k, int(bool(exclude_self)), ptr(off), ptr(xv), ldx, ptr(nbr), ptr(dist),
            ptr(ws), _stream_of(dev)))
    else:
        check_call(LIB.dglhip_segment_knn_host(
            B, N, D, k, int(bool(exclude_self)), ptr(off), ptr(xv), ldx, ptr(nbr), ptr(dist), 0))
    return nbr, dist


# ---------------------------------------------------------------------------
# Segment farthest point sampling: dgl.geometry (csrc/segment_fps.hip)
# ---------------------------------------------------------------------------
def _fps_without_coordinates(segs, m, start, dev):
    """D == 0: every distance is +0.0, so after the first pick the rows follow
    in order. From the offsets alone, where they are."""
    off = segs.on(dev)
    beg, n = off[:-1, None], (off[1:] - off[:-1])[:, None]
    st = torch.zeros_like(n) if start is None else \
        torch.minimum(start[:, None].clamp(min=0), (n - 1).clamp(min=0))
    j = torch.arange(m, dtype=torch.int64, device=dev)[None, :]
    row = torch.where(j == 0, st, torch.where(j - 1 < st, j - 1, j))
    idx = torch.where(j < n, beg + row, torch.full_like(row, -1))
    dist = torch.zeros(idx.shape, dtype=torch.float32, device=dev)
    dist[:, 0] = torch.where(n[:, 0] > 0, float("inf"), 0.0)
    return idx, dist


def segment_fps(x, offsets, m, start=None):
    """Farthest point sampling of every segment ``x[offsets[s] :
    offsets[s+1]]``: ``(idx, dist)``, ``idx (B, m)`` int64 global row ids in
    pick order and ``dist (B, m)`` float32, the pick's squared distance to
    the nearest earlier pick when it was picked (``+inf`` for the first). Not
    differentiable.

    ``x`` is ``(N, D)`` float32 (read in place through its row stride) with
    ``D <= FPS_MAX_DIM``, ``offsets`` what :func:`segment_reduce` takes, ``m
    >= 1``; ``start`` is None (every segment starts at its row 0) or a
    ``(B,)`` int64 tensor of rows within the segments. A ``start`` on the
    host is checked against host-side sizes (outside ``[0, rows)`` is a
    DGLError); one on the device is clamped into its segment.

    In float32, ``d(p, j)`` is the chain ``s = fma(t, t, s)`` over ``t = x_j[c]
    - x_p[c]``, ``c`` ascending, from ``+0.0``. Every row keeps the minimum of
    its distances to the picks so far, from ``+inf``; a NaN distance never
    lowers it. A picked row is never picked again; each later pick is the
    row with the largest minimum, the lowest row among equals: no tie is left
    to chance, and a row with a NaN coordinate (whose minimum stays ``+inf``)
    is picked early. A segment of fewer than ``m`` rows fills the remaining
    slots with ``-1`` and ``+0.0``. Same bits on the host and on the device,
    where one workgroup keeps a segment on chip for all ``m`` picks; no
    atomics, no host synchronisation."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise DGLError("segment_fps expects an (N, D) tensor of points")
    if x.dtype != torch.float32:
        raise DGLError("segment_fps computes in float32, got %s" % x.dtype)
    m = int(m)
    if m < 1:
        raise DGLError("segment_fps picks m >= 1 rows, got m = %d" % m)
    N, D = x.shape
    if D > FPS_MAX_DIM:
        raise DGLError("segment_fps serves D <= FPS_MAX_DIM = %d, got D = %d" % (FPS_MAX_DIM, D))
    segs = _segment_offsets(offsets)
    if segs.num_rows >= 0 and segs.num_rows != N:
        raise DGLError("offsets end at %d, expected the %d rows" % (segs.num_rows, N))
    B, dev = segs.num_segments, x.device
    if start is not None:
        if not isinstance(start, torch.Tensor) or start.dtype != torch.int64 \
                or tuple(start.shape) != (B,):
            raise DGLError("start must be an int64 tensor of the %d segments' first picks" % B)
        if not start.is_cuda and segs.host is not None:
            n = segs.host[1:] - segs.host[:-1]
            if bool(((n > 0) & ((start < 0) | (start >= n))).any()):
                raise DGLError("start names a row outside its segment")
        start = start.detach().to(dev).contiguous()
    if N == 0 or B == 0:
        return (torch.full((B, m), -1, dtype=torch.int64, device=dev),
                torch.zeros(B, m, dtype=torch.float32, device=dev))
    if D == 0:
        return _fps_without_coordinates(segs, m, start, dev)
    idx = torch.empty(B, m, dtype=torch.int64, device=dev)
    dist = torch.empty(B, m, dtype=torch.float32, device=dev)
    off = segs.on(dev)
    xv, ldx = _rows_view(x.detach(), D)
    if dev.type == "cuda":
        nbytes = LIB.dglhip_segment_fps_workspace_bytes(B, N, D, m, segs.max_rows)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check_call(LIB.dglhip_segment_fps_device(
            B, N, D, m, ptr(off), ptr(xv), ldx, ptr(start), ptr(idx), ptr(dist), segs.max_rows,
            ptr(ws), _stream_of(dev)))
    else:
        check_call(LIB.dglhip_segment_fps_host(
            B, N, D, m, ptr(off), ptr(xv), ldx, ptr(start), ptr(idx), ptr(dist), 0))
    return idx, dist


# ---------------------------------------------------------------------------
# Segment fixed-radius neighbours: ball_query, radius_graph (csrc/segment_radius.hip)
# ---------------------------------------------------------------------------
def segment_radius(x, offsets, r, k, q=None, q_offsets=None, exclude_self=False,
                   pad_first=False):
    """For every query row ``i`` of every segment ``q[q_offsets[s] :
    q_offsets[s+1]]`` the first ``k`` rows ``j`` of ``x[offsets[s] :
    offsets[s+1]]``, in row order, closer than ``r``: ``(nbr, cnt, dist)``,
    ``nbr (M, k)`` int64 global rows of ``x``, ``cnt (M,)`` int32 ``min(members,
    k)`` and ``dist (M, k)`` float32 squared distances. Not differentiable.

    ``x (N, D)`` and ``q (M, D)`` are float32 (read in place through their row
    strides), ``offsets`` and ``q_offsets`` what :func:`segment_reduce` takes,
    with the same number of segments; ``q=None`` searches ``x`` round its own
    rows (the graph case). ``1 <= k <= RADIUS_MAX_K`` and ``D <=
    RADIUS_MAX_DIM``; outside is an error, not another path.

    In float32, ``d(i, j)`` is the chain ``s = fma(t, t, s)`` over ``t = x_j[c]
    - q_i[c]``, ``c`` ascending, from ``+0.0``; ``j`` is a member when ``d <
    float32(r) * float32(r)``, strictly (a NaN distance is outside), and with
    ``exclude_self`` not when it is the query's own global row. The members
    are the first ``k`` in row order, not the nearest. Slots past ``cnt[i]``
    hold ``-1`` and ``+inf``, with ``pad_first`` the first member and its
    distance (PointNet++'s grouping); a query without a member keeps ``-1`` and
    ``+inf``. Same bits on the host and on the device, where a workgroup
    walks a cloud once for 64 queries and stops when all of them are full: no
    distance matrix, no atomics, no host synchronisation."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise DGLError("segment_radius expects an (N, D) tensor of points")
    if q is None:
        if q_offsets is not None:
            raise DGLError("q_offsets without q")
        q, q_offsets = x, offsets
    elif q_offsets is None:
        raise DGLError("queries need their own q_offsets")
    if not isinstance(q, torch.Tensor) or q.dim() != 2 or q.shape[1] != x.shape[1]:
        raise DGLError("segment_radius expects (M, D) queries of the points' width")
    if x.dtype != torch.float32 or q.dtype != torch.float32:
        raise DGLError("segment_radius computes in float32, got %s and %s" % (x.dtype, q.dtype))
    if q.device != x.device:
        raise DGLError("points on %s, queries on %s" % (x.device, q.device))
    k = int(k)
    if k < 1 or k > RADIUS_MAX_K:
        raise DGLError("segment_radius serves 1 <= k <= RADIUS_MAX_K = %d, got k = %d"
                       % (RADIUS_MAX_K, k))
    (N, D), M = x.shape, q.shape[0]
    if D > RADIUS_MAX_DIM:
        raise DGLError("segment_radius serves D <= RADIUS_MAX_DIM = %d, got D = %d"
                       % (RADIUS_MAX_DIM, D))
    segs = _segment_offsets(offsets)
    qsegs = segs if q_offsets is offsets else _segment_offsets(q_offsets)
    if segs.num_rows >= 0 and segs.num_rows != N:
        raise DGLError("offsets end at %d, expected the %d rows" % (segs.num_rows, N))
    if qsegs.num_rows >= 0 and qsegs.num_rows != M:
        raise DGLError("q_offsets end at %d, expected the %d queries" % (qsegs.num_rows, M))
    if qsegs.num_segments != segs.num_segments:
        raise DGLError("%d segments of points, %d of queries"
                       % (segs.num_segments, qsegs.num_segments))
    B, dev = segs.num_segments, x.device
    r2 = np.float32(r) * np.float32(r)
    nbr = torch.full((M, k), -1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(M, dtype=torch.int32, device=dev)
    dist = torch.full((M, k), float("inf"), dtype=torch.float32, device=dev)
    if N == 0 or M == 0 or B == 0:
        return nbr, cnt, dist
    if D == 0:  # no storage to point the library at: every distance is +0.0
        x, q, D = x.new_zeros(N, 1), q.new_zeros(M, 1), 1
    flags = (_RADIUS_EXCLUDE_SELF if exclude_self else 0) | (_RADIUS_PAD_FIRST if pad_first else 0)
    xv, ldx = _rows_view(x.detach(), D)
    qv, ldq = (xv, ldx) if q is x else _rows_view(q.detach(), D)
    if dev.type == "cuda":
        check_call(LIB.dglhip_segment_radius_device(
            B, N, M, D, k, r2, flags, ptr(segs.on(dev)), ptr(xv), ldx, ptr(qsegs.on(dev)),
            ptr(qv), ldq, ptr(nbr), ptr(cnt), ptr(dist), None, _stream_of(dev)))
    else:
        check_call(LIB.dglhip_segment_radius_host(
            B, N, M, D, k, r2, flags, ptr(segs.on(dev)), ptr(xv), ldx, ptr(qsegs.on(dev)),
            ptr(qv), ldq, ptr(nbr), ptr(cnt), ptr(dist), 0))
    return nbr, cnt, dist
