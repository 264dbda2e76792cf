"""R-GCN's operators: gather_rows, the DistMult decoder and its loss, and
the typed-edge block-diagonal g-SpMM (csrc/typed_block.hip)."""
from __future__ import absolute_import

import os

import torch

from .._ffi import LIB, check_call, ptr, stream_of as _stream_of
from ..base import DGLError
from ..device_graph import _workspace
from .policy import ORDER_EID
from .csr import build_csr
from .spmm import _f32c, _fwd_slot_of_bwd

# ---------------------------------------------------------------------------
# Typed-edge block-diagonal g-SpMM (R-GCN block layer)
# ---------------------------------------------------------------------------
class _Segments(object):
    """A CSR-like view for the typed-block kernels: rows with slot ranges
    ``indptr`` over column ids ``indices`` (int32)."""

    def __init__(self, indptr, indices):
        self.indptr, self.indices = indptr, indices
        self.num_rows = indptr.numel() - 1
        self.nnz = indices.numel()
        self._plans = {}


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx):
        ctx.num_rows = x.shape[0]
        ctx.save_for_backward(idx)
        return x.index_select(0, idx)

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        m, n = idx.numel(), ctx.num_rows
        if m == 0:
            return dy.new_zeros((n,) + tuple(dy.shape[1:])), None
        dy2 = _f32c(dy.reshape(m, -1))
        F = dy2.shape[1]
        dev = dy2.device
        # positions grouped by row, in increasing position (a stable sort; the
        # counts by an integer scatter-add): no host sync
        ptr_, order = _position_groups(idx, n)
        # the sum per row as the typed-block kernel over F blocks of 1 x 1
        # ones (fma(1, x, acc) == acc + x): chains of TYPED_CHUNK positions,
        # the chunks of a long row added in order
        seg = _Segments(ptr_, order)
        ones = torch.ones(1, F, 1, 1, dtype=torch.float32, device=dev)
        rel = torch.zeros(m, dtype=torch.int32, device=dev)
        dx = _run_typed_block(seg, dy2, ones, rel, None, F, 1, 1)
        return dx.view((n,) + tuple(dy.shape[1:])), None


def gather_rows(x, idx):
    """``x[idx]`` (rows) whose gradient sums each row's duplicates
    deterministically: dx[r] = the dy[i] with idx[i] == r in increasing i, as
    chains of TYPED_CHUNK positions whose partials are added in order (the
    typed-block kernel with unit weights; no atomics, no host sync). torch's
    index backward accumulates duplicates in an implementation-defined order
    and walks a hub row's duplicates serially (R-GCN's DistMult decoder: 3 of
    the 8 ms step, tools/rgcn_step.py)."""
    idx = idx.to(device=x.device, dtype=torch.int64).reshape(-1)
    return _GatherRows.apply(x, idx)


TYPED_CHUNK = 64  # DGLHIP_TYPED_CHUNK: slots per chain of the typed-block kernels


def set_typed_block_width(slices):
    """Study knob: at most ``slices`` (1, 2, 4, 8) slices of 64 outputs per
    wave of the typed-block g-SpMM (default 1; 8 was slower at configs[4]).
    Same bits."""
    check_call(LIB.dglhip_set_typed_block_width(int(slices)))


_DEBUG_GROUPS = os.environ.get("DGLHIP_DEBUG_GROUPS", "0") not in ("", "0")


def _check_groups(ptr_, order, idx, num_rows):
    """DGLHIP_DEBUG_GROUPS=1: check a position grouping on the host before a
    kernel walks it (one sync; skipped under HIP-graph capture)."""
    if idx.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    p, o, ix = ptr_.cpu(), order.cpu().long(), idx.cpu()
    m = ix.numel()
    problems = []
    if p.numel() != num_rows + 1 or int(p[0]) != 0 or int(p[-1]) != m:
        problems.append("ptr ends %s..%s for %d positions" % (p[:1].tolist(), p[-1:].tolist(), m))
    if bool((p[1:] < p[:-1]).any()):
        problems.append("ptr not monotone")
    if m and (int(o.min()) < 0 or int(o.max()) >= m or
              not torch.equal(torch.sort(o)[0], torch.arange(m))):
        problems.append("order is not a permutation of the positions")
    if m and (int(ix.min()) < 0 or int(ix.max()) >= num_rows):
        problems.append("ids span [%d, %d] for %d rows" % (int(ix.min()), int(ix.max()), num_rows))
    if problems:
        raise DGLError("malformed position grouping: " + "; ".join(problems))


def _position_groups_items(idx, num_rows):
    """_position_groups on a device with the typed-block item list over it,
    in one library call (dglhip_group_positions_device: ≈80 µs of host time
    as a CSR build plus _typed_items, r06): (ptr, order, item_ptr, item_row)."""
    dev = idx.device
    m = idx.numel()
    R = max(int(num_rows), 1)
    bound = R + -(-m // TYPED_CHUNK)
    nb = LIB.dglhip_group_positions_workspace_bytes(R, m)
    ptr_ = torch.empty(R + 1, dtype=torch.int64, device=dev)
    order = torch.empty(max(m, 1), dtype=torch.int32, device=dev)[:m]
    item_ptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
    item_row = torch.empty(bound, dtype=torch.int32, device=dev)
    ws = _workspace(nb, dev)
    check_call(LIB.dglhip_group_positions_device(
        R, m, ptr(idx.contiguous()), bound, ptr(ptr_), ptr(order), ptr(item_ptr),
        ptr(item_row), ptr(ws), int(nb), _stream_of(dev)))
    return ptr_, order, item_ptr, item_row


def _position_groups(idx, num_rows):
    """Positions of ``idx`` grouped by row in increasing position, no host
    sync: (ptr int64[R+1], order int32[m]). On a device, the library's CSR
    builder over (idx, position) — an LSD radix sort, stable, and each row's
    first slot found by the fill — instead of torch's merge sort, scatter-add
    and scan (a quarter of the launches); the same arrays."""
    m = idx.numel()
    if idx.is_cuda and m:
        return _position_groups_items(idx, num_rows)[:2]
    order = torch.sort(idx, stable=True)[1].to(torch.int32)
    counts = torch.zeros(num_rows, dtype=torch.int64, device=idx.device).scatter_add_(
        0, idx, torch.ones_like(idx))
    ptr_ = torch.zeros(num_rows + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(counts, 0, out=ptr_[1:])
    return ptr_, order


class _DistMult(torch.autograd.Function):
    """score[i] = sum_f (h[s_i] * w[r_i] * h[o_i])_f in one kernel (no
    [n, F] gathers or products), and its gradients as ordered chains per node
    and relation (dglhip_distmult_*): each position's term as torch's autograd
    of the three-way product computes it, chained as gather_rows' backward
    chains them, so dh and dw carry the bits of the torch formulation
    ``gather_rows(h, s) * gather_rows(w, r) * gather_rows(h, o)`` with its
    duplicates summed by gather_rows; the score's sum runs in the kernel's
    order (lane chains + butterfly) instead of torch's."""

    @staticmethod
    def forward(ctx, h, w, s, r, o):
        n, F = s.numel(), h.shape[1]
        score = torch.empty(n, dtype=torch.float32, device=h.device)
        args = (n, F, h.shape[0], w.shape[0], ptr(s), ptr(r), ptr(o), ptr(h), ptr(w), ptr(score))
        if h.is_cuda:
            check_call(LIB.dglhip_distmult_score_device(*(args + (_stream_of(h.device),))))
        else:
            check_call(LIB.dglhip_distmult_score_host(*(args + (0,))))
        ctx.save_for_backward(h, w, s, r, o)
        return score

    @staticmethod
    def backward(ctx, dscore):
        h, w, s, r, o = ctx.saved_tensors
        ds = _f32c(dscore.reshape(-1))
        n, F = s.numel(), h.shape[1]
        grads = [None, None]
        for task, (need, rows, idx) in enumerate(
                ((ctx.needs_input_grad[0], h.shape[0], lambda: torch.cat([s, o])),
                 (ctx.needs_input_grad[1], w.shape[0], lambda: r))):
            if not need:
                continue
            ix = idx()
            if h.is_cuda and ix.numel():
                ptr_, order, item_ptr, item_row = _position_groups_items(ix, rows)
            else:
                ptr_, order = _position_groups(ix, rows)
                item_ptr = item_row = None
            if _DEBUG_GROUPS:
                _check_groups(ptr_, order, ix, rows)
            out = torch.empty(rows, F, dtype=torch.float32, device=h.device)
            common = (n, h.shape[0], w.shape[0])
            tail = (ptr(order), ptr(s), ptr(r), ptr(o), ptr(ds), ptr(h), ptr(w), ptr(out))
            if h.is_cuda:
                if item_ptr is None:
                    item_ptr, item_row = _typed_items(ptr_, ix.numel())
                part = torch.empty(item_row.numel(), F, dtype=torch.float32, device=h.device)
                check_call(LIB.dglhip_distmult_grad_device(
                    task, rows, item_row.numel(), F, *common, ptr(ptr_), ptr(item_ptr),
                    ptr(item_row), *tail, ptr(part), _stream_of(h.device)))
            else:
                check_call(LIB.dglhip_distmult_grad_host(task, rows, F, *common, ptr(ptr_),
                                                         *tail, 0))
            grads[task] = out
        return grads[0], grads[1], None, None, None


def distmult_score(h, w_rel, subj, rel, obj):
    """DistMult scores of (subj, rel, obj) triples over node embeddings ``h``
    and relation vectors ``w_rel`` (the reference's calc_score,
    examples/pytorch/rgcn/link_predict.py:50-55) in one kernel; differentiable
    in h and w_rel with deterministic gradients (see _DistMult). Indices out of
    range raise IndexError, as the torch formulation's index_select does: ids
    given on the host are checked there before they move; ids already on a
    device are checked when ``set_validate_indices(True)`` (or
    DGLHIP_VALIDATE_INDICES=1) asks for it, with one min/max reduction and a
    host sync per call. Unchecked, the kernel never reads past its tables: an
    out-of-range position scores NaN and adds nothing to the gradients."""
    return _DistMult.apply(_f32c(h), _f32c(w_rel), *_distmult_ids(h, w_rel, subj, rel, obj))


def _distmult_ids(h, w_rel, subj, rel, obj):
    """The triples' ids as int64 on h's device, checked (distmult_score)."""
    dev = h.device
    if w_rel.shape[1:] != h.shape[1:] or h.dim() != 2:
        raise DGLError("distmult_score: h and w_rel must be 2-D of one width")
    trip = [torch.as_tensor(t) for t in (subj, rel, obj)]
    if not (trip[0].numel() == trip[1].numel() == trip[2].numel()):
        raise DGLError("distmult_score: subj, rel, obj lengths differ")
    on_host = all(t.device.type == "cpu" for t in trip)
    if trip[0].numel() and (on_host or (_VALIDATE_INDICES and not (
            dev.type == "cuda" and torch.cuda.is_current_stream_capturing()))):
        lo_hi = torch.stack([torch.stack([t.min(), t.max()]).to(torch.int64)
                             for t in trip]).tolist()
        for (lo, hi), bound, what in zip(lo_hi, (h.shape[0], w_rel.shape[0], h.shape[0]),
                                         ("subj", "rel", "obj")):
            if lo < 0 or hi >= bound:
                raise IndexError("distmult_score: %s ids span [%d, %d], out of range for %d rows"
                                 % (what, lo, hi, bound))
    # one stacking copy (the triples usually arrive as the columns of one
    # (n, 3) sample tensor: three strided views) instead of three
    ids = torch.stack([t.to(device=dev, dtype=torch.int64).reshape(-1) for t in trip])
    return [ids[0], ids[1], ids[2]]


class _DistMultLoss(torch.autograd.Function):
    """distmult_link_loss on a device: the loss and the scores in two
    launches, the gradients as _DistMult's chains with the BCE gradient formed
    in the kernel and the regulariser's term added to every row
    (dglhip_distmult_loss_*)."""

    @staticmethod
    def forward(ctx, h, w, s, r, o, labels, reg):
        n, F = s.numel(), h.shape[1]
        dev = h.device
        score = torch.empty(n, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        nws = LIB.dglhip_distmult_loss_workspace_floats(n, h.shape[0], w.shape[0], F)
        ws = torch.empty(max(int(nws), 1), dtype=torch.float32, device=dev)
        check_call(LIB.dglhip_distmult_loss_fwd_device(
            n, F, h.shape[0], w.shape[0], ptr(s), ptr(r), ptr(o), ptr(h), ptr(w), ptr(labels),
            float(reg), ptr(score), ptr(loss), ptr(ws), int(nws), _stream_of(dev)))
        ctx.save_for_backward(h, w, s, r, o, labels, score)
        ctx.reg = float(reg)
        return loss

    @staticmethod
    def backward(ctx, g):
        h, w, s, r, o, labels, score = ctx.saved_tensors
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        n, F = s.numel(), h.shape[1]
        dev = h.device
        grads = [None, None]
        for task, (need, rows, idx) in enumerate(
                ((ctx.needs_input_grad[0], h.shape[0], lambda: torch.cat([s, o])),
                 (ctx.needs_input_grad[1], w.shape[0], lambda: r))):
            if not need:
                continue
            ptr_, order, item_ptr, item_row = _position_groups_items(idx(), rows)
            out = torch.empty(rows, F, dtype=torch.float32, device=dev)
            part = torch.empty(item_row.numel(), F, dtype=torch.float32, device=dev)
            check_call(LIB.dglhip_distmult_loss_grad_device(
                task, rows, item_row.numel(), F, n, h.shape[0], w.shape[0], ptr(ptr_),
                ptr(item_ptr), ptr(item_row), ptr(order), ptr(s), ptr(r), ptr(o), ptr(score),
                ptr(labels), ptr(g), ctx.reg, ptr(h), ptr(w), ptr(out), ptr(part),
                _stream_of(dev)))
            grads[task] = out
        return grads[0], grads[1], None, None, None, None, None


def distmult_link_loss(h, w_rel, subj, rel, obj, labels, reg):
    """The R-GCN link-prediction loss (the reference's get_loss,
    examples/pytorch/rgcn/link_predict.py:57-66):

        F.binary_cross_entropy_with_logits(distmult_score(h, w_rel, subj, rel, obj), labels)
            + reg * (h.pow(2).mean() + w_rel.pow(2).mean())

    On a ROCm device one forward launch pair and the decoder's gradient
    launches (the BCE and regulariser gradients formed inside them) instead of
    about twenty small kernels; values within fp32 rounding of that
    expression (its sums associate differently). Ids are checked as
    distmult_score checks them."""
    ids = _distmult_ids(h, w_rel, subj, rel, obj)
    labels = torch.as_tensor(labels)
    if (h.is_cuda and h.dtype == torch.float32 and w_rel.dtype == torch.float32 and
            ids[0].numel() > 0 and h.numel() > 0):
        lab = labels.to(device=h.device, dtype=torch.float32).reshape(-1).contiguous()
        if lab.numel() != ids[0].numel():
            raise DGLError("distmult_link_loss: %d labels for %d triples"
                           % (lab.numel(), ids[0].numel()))
        return _DistMultLoss.apply(_f32c(h), _f32c(w_rel), *ids, lab, float(reg))
    score = _DistMult.apply(_f32c(h), _f32c(w_rel), *ids)
    return (torch.nn.functional.binary_cross_entropy_with_logits(score, labels.to(score)) +
            reg * (h.pow(2).mean() + w_rel.pow(2).mean()))


_VALIDATE_INDICES = os.environ.get("DGLHIP_VALIDATE_INDICES", "0") not in ("", "0")


def set_validate_indices(on):
    """Check device-resident index arguments (distmult_score's triples,
    typed_block_spmm's relations) on the host before launching (one sync per
    call); returns the old setting. Host-resident ones are always checked."""
    global _VALIDATE_INDICES
    old, _VALIDATE_INDICES = _VALIDATE_INDICES, bool(on)
    return old


def _typed_items(rowptr, nnz):
    """The typed-block kernels' work items over a CSR-like ``rowptr`` with
    ``nnz`` slots, built on the device with no host sync (cached by the
    caller): (item_ptr int64[R+1] — each row's first item, a row of deg slots
    having max(1, ceil(deg / TYPED_CHUNK)) items —, item_row int32[I_max],
    I_max = R + ceil(nnz / TYPED_CHUNK) >= the item count, the entries past
    the last item = R (padding the kernels skip))."""
    R = rowptr.numel() - 1
    if rowptr.is_cuda:  # three launches in the library (nit, rocPRIM scan, search)
        bound = R + -(-nnz // TYPED_CHUNK)
        item_ptr = torch.empty(R + 1, dtype=torch.int64, device=rowptr.device)
        item_row = torch.empty(max(bound, 1), dtype=torch.int32, device=rowptr.device)[:bound]
        nb = LIB.dglhip_typed_items_workspace_bytes(R)
        ws = _workspace(nb, rowptr.device)
        check_call(LIB.dglhip_typed_items_device(R, ptr(rowptr), bound,
                                                 ptr(item_ptr), ptr(item_row), ptr(ws), int(nb),
                                                 _stream_of(rowptr.device)))
        return item_ptr, item_row
    deg = rowptr[1:] - rowptr[:-1]
    nit = torch.clamp((deg + (TYPED_CHUNK - 1)) // TYPED_CHUNK, min=1)
    item_ptr = torch.zeros(R + 1, dtype=torch.int64, device=rowptr.device)
    torch.cumsum(nit, 0, out=item_ptr[1:])
    bound = R + -(-nnz // TYPED_CHUNK)
    item_row = torch.searchsorted(item_ptr[1:], torch.arange(bound, device=rowptr.device),
                                  right=True).to(torch.int32)
    return item_ptr, item_row


def _run_typed_block(csr, ufeat2, weight, slot_rel, slot_norm, nb, si, so):
    dev = ufeat2.device
    out = torch.empty(csr.num_rows, nb * so, dtype=torch.float32, device=dev)
    if dev.type == "cuda":
        items = csr._plans.get("typed_items")
        if items is None:
            items = csr._plans["typed_items"] = _typed_items(csr.indptr, csr.nnz)
        item_ptr, item_row = items
        part = torch.empty(item_row.numel(), nb * so, dtype=torch.float32, device=dev)
        check_call(LIB.dglhip_typed_block_spmm_device(
            csr.num_rows, item_row.numel(), nb, si, so, ptr(csr.indptr), ptr(item_ptr),
            ptr(item_row), csr.num_rows, None, ptr(csr.indices), ptr(slot_rel),
            ptr(slot_norm), ptr(ufeat2), ptr(weight), ptr(out), ptr(part), _stream_of(dev)))
    else:
        check_call(LIB.dglhip_typed_block_spmm_host(
            csr.num_rows, nb, si, so, ptr(csr.indptr), ptr(csr.indices), ptr(slot_rel),
            ptr(slot_norm), ptr(ufeat2), ptr(weight), ptr(out), 0))
    return out


def set_typed_block_messages(on):
    """The typed-block g-SpMM as relation-major messages + a slot-order sum,
    and its weight gradient with LDS-staged rows (csrc/typed_block.hip, r06),
    instead of the one-kernel forms; the same bits."""
    check_call(LIB.dglhip_set_typed_block_messages(1 if on else 0))


def _typed_msg_ok(nb, si, so):
    return LIB.dglhip_typed_block_msg_ok(nb, si, so) == 1


def _relation_groups(adj, etype, num_rels):
    g = getattr(adj, "_rel_groups", None)
    if g is None or not g.matches(etype):
        g = adj._rel_groups = _RelationGroups(adj.fwd, etype, num_rels)
    return g


def _run_typed_msg(csr, slot_map, groups, pos_row, ufeat2, weight, slot_norm, nb, si, so,
                   operand_scale=None, out_scale=None, weight_transposed=False):
    """out = the typed-block g-SpMM over ``csr`` in two launches: every edge's
    message (blockdiag(weight[r]) applied to ufeat2[pos_row], that row scaled
    by ``operand_scale[pos_row]`` when given) stored at its forward slot,
    walked relation-major; then each row's sum over its slots, reading message
    ``slot_map[k]`` (None: k) for slot k, times ``out_scale[row]``."""
    dev = ufeat2.device
    Fo = nb * so
    R = groups.ptr.numel() - 1
    msg = torch.empty(max(csr.nnz, 1), Fo, dtype=torch.float32, device=dev)
    g_ptr, g_rel = groups.items
    stream = _stream_of(dev)
    check_call(LIB.dglhip_typed_block_msg_device(
        R, g_rel.numel(), nb, si, so, ptr(groups.ptr), ptr(g_ptr), ptr(g_rel), ptr(pos_row),
        ptr(groups.slot), ptr(ufeat2), ptr(operand_scale), ptr(weight),
        1 if weight_transposed else 0, ptr(msg), stream))
    items = csr._plans.get("typed_items")
    if items is None:
        items = csr._plans["typed_items"] = _typed_items(csr.indptr, csr.nnz)
    item_ptr, item_row = items
    out = torch.empty(csr.num_rows, Fo, dtype=torch.float32, device=dev)
    part = torch.empty(item_row.numel(), Fo, dtype=torch.float32, device=dev)
    check_call(LIB.dglhip_typed_msg_sum_device(
        csr.num_rows, item_row.numel(), Fo, ptr(csr.indptr), ptr(item_ptr), ptr(item_row),
        csr.num_rows, None, ptr(slot_map), ptr(slot_norm), ptr(msg), ptr(out_scale), ptr(out),
        ptr(part), stream))
    return out


def _slot_values(csr, etype, enorm):
    """The per-edge relation (int32) and norm in ``csr``'s slot order."""
    rel = etype.index_select(0, csr.eid).to(torch.int32)
    nrm = None if enorm is None else enorm.index_select(0, csr.eid)
    return rel, nrm


class _RelationGroups(object):
    """Relation-major grouping of an adjacency's edges for the weight
    gradient: ptr[R+1], the source and destination of each edge (forward
    slot order within a relation), ``slot`` the forward slot each came from,
    and the chunked items (_typed_items)."""

    def __init__(self, fwd, etype, num_rels):
        # relations are checked where they were given (typed_block_spmm: host
        # ids always, device ids on request), not with a sync here; the
        # grouping never stores outside its arrays for any value
        if fwd.device.type == "cuda":
            self._build_device(fwd, etype, num_rels)
        else:
            rel_of_slot = etype.index_select(0, fwd.eid)
            rel = build_csr(num_rels, max(fwd.num_cols, 1), rel_of_slot, fwd.indices.long(),
                            ORDER_EID, fwd.device, schedule=False, validate=False)
            self.ptr = rel.indptr
            self.src = rel.indices
            self.slot = rel.eid  # forward slot of each relation-major position
            self.dst = fwd.row_ids().index_select(0, self.slot).to(torch.int32)
            self.items = None
        self.etype = etype  # the relations it was built for (held: see matches)
        self.version = etype._version

    def _build_device(self, fwd, etype, num_rels):
        """The same arrays in one library call (dglhip_relation_groups_device:
        ≈100 µs of host time as a CSR build, gathers, repeat_interleave and
        the item list, r06)."""
        dev, nnz, R = fwd.device, fwd.nnz, max(int(num_rels), 1)
        bound = R + -(-nnz // TYPED_CHUNK)
        nb = LIB.dglhip_relation_groups_workspace_bytes(R, nnz)
        self.ptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
        self.src = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
        self.slot = torch.empty(max(nnz, 1), dtype=torch.int64, device=dev)[:nnz]
        self.dst = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
        item_ptr = torch.empty(R + 1, dtype=torch.int64, device=dev)
        item_rel = torch.empty(bound, dtype=torch.int32, device=dev)
        ws = _workspace(nb, dev)
        check_call(LIB.dglhip_relation_groups_device(
            R, fwd.num_rows, nnz, ptr(etype), ptr(fwd.indptr), ptr(fwd.indices), ptr(fwd.eid),
            bound, ptr(self.ptr), ptr(self.src), ptr(self.slot), ptr(self.dst), ptr(item_ptr),
            ptr(item_rel), ptr(ws), int(nb), _stream_of(dev)))
        self.items = (item_ptr, item_rel)

    def matches(self, etype):
        # typed_block_spmm hands a new 1-D view of the relations at every call
        # (r04 ADVICE: compared by object, the cache never hit). The held
        # tensor keeps its memory from being reused, so the same address and
        # length is the same memory, and views share one version counter
        return (self.etype.device == etype.device and self.etype.numel() == etype.numel() and
                self.etype.data_ptr() == etype.data_ptr() and self.version == etype._version)


def _typed_scale_fused(dev, nb, si, so):
    """A destination row scale rides in the message path's kernels (forward
    sum, dH messages, staged dW) for these widths on a device."""
    return (dev.type == "cuda" and _typed_msg_ok(nb, si, so) and _typed_msg_ok(nb, so, si) and
            nb * si * so <= 4096)


class _TypedBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, adj, etype, num_rels, ufeat2, weight, enorm, row_scale=None):
        R, nb, si, so = weight.shape
        if ufeat2.is_cuda and _typed_msg_ok(nb, si, so):
            g = _relation_groups(adj, etype, R)
            nrm = None if enorm is None else enorm.index_select(0, adj.fwd.eid)
            out = _run_typed_msg(adj.fwd, None, g, g.src, ufeat2, weight, nrm, nb, si, so,
                                 out_scale=row_scale)
        else:
            assert row_scale is None  # typed_block_spmm scales outside otherwise
            rel, nrm = _slot_values(adj.fwd, etype, enorm)
            out = _run_typed_block(adj.fwd, ufeat2, weight, rel, nrm, nb, si, so)
        ctx.adj, ctx.num_rels = adj, num_rels
        ctx.save_for_backward(etype, ufeat2, weight, enorm, row_scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        etype, ufeat2, weight, enorm, row_scale = ctx.saved_tensors
        adj = ctx.adj
        R, nb, si, so = weight.shape
        dout = dout.contiguous()
        du = dw = None
        if ctx.needs_input_grad[3]:
            if dout.is_cuda and _typed_msg_ok(nb, so, si):
                # messages Wt[r] dout[dst] at the forward slots, read along the
                # transpose (the weight read transposed in the kernel)
                g = _relation_groups(adj, etype, R)
                nrm = None if enorm is None else enorm.index_select(0, adj.bwd.eid)
                du = _run_typed_msg(adj.bwd, _fwd_slot_of_bwd(adj), g, g.dst, dout, weight, nrm,
                                    nb, so, si, operand_scale=row_scale, weight_transposed=True)
            else:
                wt = weight.transpose(2, 3).contiguous()  # (R, nb, so, si)
                rel, nrm = _slot_values(adj.bwd, etype, enorm)
                du = _run_typed_block(adj.bwd, dout, wt, rel, nrm, nb, so, si)
        if ctx.needs_input_grad[4]:
            g = _relation_groups(adj, etype, R)
            fwd_nrm = None if enorm is None else enorm.index_select(0, adj.fwd.eid)
            nrm = None if fwd_nrm is None else fwd_nrm.index_select(0, g.slot)
            dw = torch.empty_like(weight)
            if dout.is_cuda:
                item_ptr, item_rel = g.items
                part = torch.empty(item_rel.numel(), nb * si * so, dtype=torch.float32,
                                   device=dout.device)
                check_call(LIB.dglhip_typed_block_wgrad_scaled_device(
                    R, item_rel.numel(), nb, si, so, ptr(g.ptr), ptr(item_ptr), ptr(item_rel),
                    R, None, ptr(g.src), ptr(g.dst), ptr(nrm), ptr(ufeat2), ptr(dout),
                    ptr(row_scale), ptr(dw), ptr(part), _stream_of(dout.device)))
            else:
                check_call(LIB.dglhip_typed_block_wgrad_host(
                    R, nb, si, so, ptr(g.ptr), ptr(g.src), ptr(g.dst), ptr(nrm), ptr(ufeat2),
                    ptr(dout), ptr(dw), 0))
        return None, None, None, du, dw, None, None


def typed_block_spmm(adj, ufeat, weight, etype, enorm=None, row_scale=None):
    """R-GCN block-diagonal message passing in one kernel:
    out[v] = sum_{e=(u->v)} enorm[e] * blockdiag(weight[etype[e]]) applied to ufeat[u].

    adj    : SparseAdj (rows = destinations) on the features' device
    ufeat  : (num_src, nb * si) float32
    weight : (num_rels, nb, si, so) float32 (autograd)
    etype  : (num_edges,) int64 relation of each edge id
    enorm  : optional (num_edges,) float32 per-edge scale (not differentiated)
    row_scale : optional (num_rows,) float32 scale of each output row (not
             differentiated): the value of ``out * row_scale.unsqueeze(1)`` —
             the R-GCN layer's 1 / in-degree, rounded as that product is —
             applied inside the kernels when the message path runs (no
             elementwise pass either way, r06), else by that product
    """
    dev = ufeat.device
    adj = adj.to(dev)
    R, nb, si, so = weight.shape
    if ufeat.shape[1] != nb * si:
        raise DGLError("ufeat width %d != num_blocks * in_block %d" % (ufeat.shape[1], nb * si))
    etype = torch.as_tensor(etype)
    if etype.numel() and (etype.device.type == "cpu" or (
            _VALIDATE_INDICES and not (dev.type == "cuda" and
                                       torch.cuda.is_current_stream_capturing()))):
        lo, hi = torch.stack([etype.min(), etype.max()]).tolist()
        if lo < 0 or hi >= R:
            raise IndexError("typed_block_spmm: relations span [%d, %d], out of range for %d "
                             "relation weights" % (lo, hi, R))
    etype = etype.to(device=dev, dtype=torch.int64).contiguous().reshape(-1)
    en = None if enorm is None else _f32c(enorm.to(dev).reshape(-1).detach())
    # one relation (and norm) per edge id: the kernels gather them by edge id
    E = adj.fwd.nnz
    if etype.numel() != E or (en is not None and en.numel() != E):
        raise DGLError("typed_block_spmm: %d edges but etype has %d and enorm %s entries"
                       % (E, etype.numel(), "no" if en is None else en.numel()))
    if row_scale is None:
        return _TypedBlock.apply(adj, etype, R, _f32c(ufeat), _f32c(weight), en)
    rs = _f32c(torch.as_tensor(row_scale).to(dev).reshape(-1).detach())
    if rs.numel() != adj.fwd.num_rows:
        raise DGLError("typed_block_spmm: row_scale has %d entries for %d rows"
                       % (rs.numel(), adj.fwd.num_rows))
    if _typed_scale_fused(dev, nb, si, so):
        return _TypedBlock.apply(adj, etype, R, _f32c(ufeat), _f32c(weight), en, rs)
    return _TypedBlock.apply(adj, etype, R, _f32c(ufeat), _f32c(weight), en) * rs.unsqueeze(1)
