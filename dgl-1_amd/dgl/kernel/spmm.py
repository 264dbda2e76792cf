"""The g-SpMM / g-SDDMM operators: one product on a CSR's native plan, the
autograd functions over it, the raw products of the pipelined forward, and
call timing."""
from __future__ import absolute_import

import ctypes

import numpy as np
import torch

from .. import _handoff
from .._ffi import LIB, check_call, ptr, stream_of as _stream_of
from ..base import DGLError
from .policy import (
    MSG_COPY_U, MSG_U_MUL_E, MSG_COPY_E, MSG_COPY_U_BF16, RED_SUM, RED_MAX, RED_MEAN,
    RED_SUM_ACCUM, RED_MEAN_ACCUM, _ACCUM, SLOT, _MSG_NAMES, _RED_NAMES, schedule_policy)
from .plan import PLAN_PATH_BLOCKED, _block_cuts

# ---------------------------------------------------------------------------
# Raw kernel calls
# ---------------------------------------------------------------------------
def _edge_len(eshape, fshape):
    """Values per edge for an edge feature of trailing shape ``eshape`` against
    node features of trailing shape ``fshape``: 1 (scalar), F (same shape) or
    H (leading dims of fshape, broadcast over the rest: GAT's (H, 1) vs (H, D))."""
    eshape, fshape = tuple(eshape), tuple(fshape)
    F = int(np.prod(fshape)) if fshape else 1
    if all(d == 1 for d in eshape):  # (), (1,), (1, 1): one scalar per edge
        return 1
    if eshape == fshape:
        return F
    k = len(eshape)
    while k > 0 and eshape[k - 1] == 1:
        k -= 1
    if 0 < k < len(fshape) and eshape[:k] == fshape[:k] and \
            all(d == 1 for d in eshape[k:]) and len(eshape) <= len(fshape):
        return int(np.prod(fshape[:k]))
    raise DGLError("edge feature shape %s does not broadcast against node feature shape %s"
                   % (eshape, fshape))


_EDGE_BY_SLOT, _EDGE_BY_EID, _EDGE_BY_MAP = 0, 1, 2


def _edge_layout(csr, msg, emap):
    """(layout, rows tensor) of the edge values for the plan: by slot, by the
    CSR's edge ids (the plan caches what it derives from them), or a map."""
    if msg in (MSG_COPY_U, MSG_COPY_U_BF16) or emap is SLOT:
        return _EDGE_BY_SLOT, None
    if emap is None:
        return _EDGE_BY_EID, csr.eid
    return _EDGE_BY_MAP, emap.contiguous()


def _run_gspmm(csr, msg, red, ufeat2, efeat2, elen, feat_len, want_arg, out=None, emap=None):
    """ufeat2: (num_cols, F) or None; efeat2: (E, elen) or None. Returns (out, arg).
    ``out`` (optional) receives the result; RED_SUM_ACCUM adds into it.
    ``emap`` says where slot k's edge values are: None = row eid[k] (edge-id
    order), SLOT = row k (efeat2 laid out in this CSR's slot order), or an
    int64 tensor of rows per slot."""
    dev = (ufeat2 if ufeat2 is not None else efeat2).device
    if _CALL_EVENTS is None or dev.type != "cuda":
        return _run_gspmm_call(csr, msg, red, ufeat2, efeat2, elen, feat_len, want_arg, out,
                               emap, dev)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(torch.cuda.current_stream(dev))
    res = _run_gspmm_call(csr, msg, red, ufeat2, efeat2, elen, feat_len, want_arg, out, emap,
                          dev)
    end.record(torch.cuda.current_stream(dev))
    _CALL_EVENTS.append((start, end))
    return res


def _run_gspmm_call(csr, msg, red, ufeat2, efeat2, elen, feat_len, want_arg, out, emap, dev):
    """One product on the CSR's native plan (dglhip_spmm_plan_run): the plan
    picks the source-blocked schedule, the heavy-row split, the short-row
    tiers, the padded-stride copy and the edge values' order exactly as it
    does for a C-ABI caller."""
    if csr.device != dev:
        raise DGLError("adjacency on %s but features on %s" % (csr.device, dev))
    if out is None:
        out = torch.empty(csr.num_rows, feat_len, dtype=torch.float32, device=dev)
    arg = None
    if red == RED_MAX and want_arg:
        arg = torch.empty(csr.num_rows, feat_len, dtype=torch.int64, device=dev)
    plan = csr.plan
    emode, erow = _edge_layout(csr, msg, emap)
    ldu = 0
    if ufeat2 is not None and ufeat2.shape[0] > 1 and _row_strided(ufeat2, feat_len):
        ldu = ufeat2.stride(0)
    urows = 0 if ufeat2 is None else ufeat2.shape[0]
    elen = 0 if efeat2 is None else elen
    nbytes = plan.workspace(msg, red, feat_len, ldu, urows, elen, emode, erow)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    check_call(LIB.dglhip_spmm_plan_run(
        plan.handle, msg, red, feat_len, ptr(ufeat2), ldu, urows, ptr(efeat2), elen, emode,
        ptr(erow), ptr(out), ptr(arg), ptr(ws), nbytes, plan.stream()))
    return out, arg


_PADDED = {}


def padded_width(F):
    """Row stride (floats) for the source rows of a g-SpMM gather: F itself,
    or F rounded up to 16 / 32 floats when that cuts the 128-B lines a row
    touches by at least 5 % (F = 41: 2.28 -> 2.0 lines at a 48-float stride;
    F = 24: 1.5 -> 1.0 at 32); the plan's rule (dglhip_spmm_padded_width)."""
    w = _PADDED.get(F)
    if w is None:
        o = ctypes.c_int64()
        check_call(LIB.dglhip_spmm_padded_width(int(F), ctypes.byref(o)))
        w = _PADDED[F] = int(o.value)
    return w


def _pad_rows(msg, red, ufeat2, feat_len):
    """Whether the plan gathers these rows from a padded copy (the same rule:
    callers that produce such rows write them padded instead)."""
    if msg not in (MSG_COPY_U, MSG_U_MUL_E) or red not in (RED_SUM, RED_MEAN) + _ACCUM or \
            ufeat2 is None or ufeat2.dtype != torch.float32:
        return False
    pol = schedule_policy()
    return (bool(pol["pad_rows"]) and ufeat2.numel() * 4 >= pol["pad_min_bytes"] and
            padded_width(feat_len) != feat_len)


def blocked_schedule(adj, ufeat):
    """The number of source-blocked launches the copy_u sum / mean g-SpMM of
    ``ufeat`` over ``adj`` runs in (0: one launch), as the plan schedules it."""
    adj = adj.to(ufeat.device)
    if ufeat.device.type != "cuda":
        return 0
    u2 = ufeat.reshape(ufeat.shape[0], -1)
    F = u2.shape[1]
    ldu = u2.stride(0) if (u2.shape[0] > 1 and _row_strided(u2, F)) else 0
    msg = MSG_COPY_U_BF16 if u2.dtype == torch.bfloat16 else MSG_COPY_U
    path, launches = adj.fwd.plan.schedule(msg, RED_SUM, F, ldu, u2.shape[0])
    return launches if path == PLAN_PATH_BLOCKED else 0


def segment_blocks(csrs, feat_len, dtypes):
    """Launches of the source-blocked schedule over CSRs gathered at
    ``feat_len`` features of the given row dtypes (one per CSR; a pipelined
    partition's own and halo segments), 0 for a CSR that keeps one launch."""
    total = 0
    for csr, dt in zip(csrs, dtypes):
        if csr.device.type != "cuda" or csr.nnz == 0:
            continue
        msg = MSG_COPY_U_BF16 if dt == torch.bfloat16 else MSG_COPY_U
        path, launches = csr.plan.schedule(msg, RED_SUM_ACCUM, feat_len, 0, csr.num_cols)
        total += launches if path == PLAN_PATH_BLOCKED else 0
    return total


def _run_sddmm_dot(csr, lhs2, rhs2, num_edges, heads=1, slot=False):
    """out[eid, h] = <lhs[row, head h], rhs[col, head h]>; returns (num_edges, heads).
    ``slot``: out[k] for slot k of ``csr`` instead (values in its slot order)."""
    dev = lhs2.device
    out = torch.zeros(num_edges, heads, dtype=torch.float32, device=dev)
    F = lhs2.shape[1]
    eid = None if slot else csr.eid
    if dev.type == "cuda":
        # rows longest-first; the gathered rows one source block at a time
        # where the CSR has a blocked schedule (per-edge values: same bits)
        cuts = (_block_cuts(csr, F * 4, schedule_policy()["block_bytes"]) or
                [csr.indptr, csr.indptr[1:]])
        for b in range(len(cuts) - 1):
            check_call(LIB.dglhip_gsddmm_ranges_device(
                0, csr.num_rows, F, heads, ptr(cuts[b]), ptr(cuts[b + 1]), ptr(csr.row_order),
                ptr(csr.indices), ptr(eid), ptr(lhs2), ptr(rhs2), ptr(out), _stream_of(dev)))
    else:
        check_call(LIB.dglhip_gsddmm_host(0, csr.num_rows, F, heads, ptr(csr.indptr),
                                          ptr(csr.indices), ptr(eid), ptr(lhs2), ptr(rhs2),
                                          ptr(out), 0))
    return out


def _fwd_slot_of_bwd(adj):
    """For each slot of the transposed CSR, the forward-CSR slot holding the
    same edge: how an edge tensor laid out in forward slot order is read along
    the transpose (backward of slot-ordered edge values). Cached on ``adj``."""
    m = getattr(adj, "_bwd_fslot", None)
    if m is None:
        fwd, bwd = adj.fwd, adj.bwd
        # (the identity check is a host sync: used only when already made)
        if fwd._slot_eid is None:  # forward slots known to run in edge-id order
            m = bwd.eid
        else:
            inv = torch.empty_like(fwd.eid)
            inv[fwd.eid] = torch.arange(fwd.nnz, dtype=fwd.eid.dtype, device=fwd.eid.device)
            m = inv.index_select(0, bwd.eid)
            del inv
        adj._bwd_fslot = m
    return m


def edge_order_of(adj, edge_order):
    """Validate an ``edge_order`` argument ("eid" or "slot")."""
    if edge_order not in ("eid", "slot"):
        raise DGLError("edge_order must be 'eid' or 'slot', got %r" % (edge_order,))
    return edge_order == "slot"


def slot_permutation(adj):
    """int64[nnz]: the edge id held by each forward-CSR slot of ``adj``. An
    edge tensor ``x`` in edge-id order is ``x[slot_permutation(adj)]`` in slot
    order; a slot-ordered ``y`` goes back with ``out[perm] = y``."""
    return adj.fwd.eid


def _eid_major(adj):
    """(csr, transposed): the CSR of ``adj`` whose slots walk the edge ids most
    nearly in order, for kernels that store one value per edge at out[eid]
    (g-SDDMM): the stores are then sequential instead of a scatter. The
    forward CSR unless the transpose's edge ids run clearly more in order
    (edges added source-major, as the (src, dst)-sorted loaders add them).
    Every per-edge value is symmetric in its two endpoint operands (a*b ==
    b*a, fma(a, b, c) == fma(b, a, c), a + b == b + a, all exact), so both
    walks give the same bits."""
    fwd = adj.fwd
    if fwd.slot_eid is None:
        return fwd, False
    bwd = adj.bwd
    if bwd.eid_locality > max(0.5, 2.0 * fwd.eid_locality):
        return bwd, True
    return fwd, False


def _row_strided(t, F):
    """A (rows, F) float32 view whose rows sit at an even stride > F (a
    row-padded buffer): the strided g-SpMM entries read it as it is."""
    return (t.dim() == 2 and t.dtype == torch.float32 and t.shape[1] == F and
            t.stride(1) == 1 and t.stride(0) > F and t.stride(0) % 2 == 0)


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise DGLError("g-SpMM computes in float32, got %s" % t.dtype)
    return t.contiguous()


def _operand_rows(grad, rows):
    """``grad`` (a row per column of the adjacency) as the gradient of an
    operand of ``rows`` rows: an operand may carry more rows than the
    adjacency has columns (gspmm, gat_aggregate), and no edge reads those, so
    their gradient is zero."""
    if grad is None or grad.shape[0] == rows:
        return grad
    out = grad.new_zeros((rows,) + tuple(grad.shape[1:]))
    out[:grad.shape[0]] = grad
    return out


def _mean_scaled(fwd, dout, padded_ok):
    """dC / deg, the mean reducer's backward ahead of the transposed product;
    with ``padded_ok`` (only the node gradient reads it) written straight into
    the padded rows that product gathers when the rows straddle lines (one pass
    instead of the division's and the padding copy's)."""
    deg = fwd.mean_divisor()
    F = dout.shape[1]
    if padded_ok and dout.is_cuda and _pad_rows(MSG_COPY_U, RED_SUM, dout, F):
        ld = padded_width(F)
        buf = dout.new_empty(dout.shape[0], ld)
        check_call(LIB.dglhip_div_rows_device(
            dout.shape[0], F, ptr(dout), dout.stride(0), ptr(deg), ptr(buf), ld,
            _stream_of(dout.device)))
        return buf[:, :F]
    return (dout / deg).contiguous()


class _GSpMM(torch.autograd.Function):
    """out = REDUCE over in-slots of MSG(ufeat[col], efeat[eid]).

    Backward (SUM/MEAN): dU = the same product over the transposed CSR (the
    reference's autograd of torch.sparse.mm computes Aᵀ·dC the same way,
    accumulating over out-edges in edge-id order); dE by g-SDDMM.

    ``slot``: efeat is laid out in the forward CSR's slot order (row k = slot
    k), so the forward reads it without the eid indirection and dE comes back
    in the same layout (the SDDMM walks the forward CSR, sequential stores)."""

    @staticmethod
    def forward(ctx, adj, msg, red, feat_len, num_edges, ufeat2, efeat2, slot=False):
        elen = 0 if efeat2 is None else efeat2.shape[1]
        need_arg = red == RED_MAX and (
            (ufeat2 is not None and ufeat2.requires_grad) or
            (efeat2 is not None and efeat2.requires_grad))
        out, arg = _run_gspmm(adj.fwd, msg, red, ufeat2, efeat2, elen, feat_len, need_arg,
                              emap=SLOT if slot else None)
        ctx.adj, ctx.msg, ctx.red, ctx.num_edges, ctx.slot = adj, msg, red, num_edges, slot
        # keep an operand alive only when the backward reads its values: the
        # node rows for u_mul_e's edge gradient, the edge values for its node
        # gradient. copy_u/copy_e + sum/mean save nothing (in a partitioned
        # layer ufeat2 is the whole gathered halo, GBs per layer)
        u_mul_e = msg == MSG_U_MUL_E
        need_u = ufeat2 is not None and ufeat2.requires_grad
        need_e = efeat2 is not None and efeat2.requires_grad
        ctx.ushape = None if ufeat2 is None else tuple(ufeat2.shape)
        ctx.eshape = None if efeat2 is None else tuple(efeat2.shape)
        ctx.save_for_backward(ufeat2 if (u_mul_e and need_e) else None,
                              efeat2 if (u_mul_e and need_u) else None, arg)
        return out

    @staticmethod
    def backward(ctx, dout):
        ufeat2, efeat2, arg = ctx.saved_tensors
        adj, msg, red, slot = ctx.adj, ctx.msg, ctx.red, ctx.slot
        dout = dout.contiguous()
        fwd = adj.fwd
        du = de = None
        need_u = ctx.needs_input_grad[5]
        need_e = ctx.needs_input_grad[6]
        F = dout.shape[1]
        if red == RED_MEAN:
            dout = _mean_scaled(fwd, dout, padded_ok=need_u and not need_e)
            red_b = RED_SUM
        else:
            red_b = red
        if red_b == RED_SUM:
            if need_u:
                elen = 0 if efeat2 is None else efeat2.shape[1]
                reads_e = msg == MSG_U_MUL_E
                du, _ = _run_gspmm(adj.bwd, msg if msg != MSG_COPY_E else MSG_COPY_U, RED_SUM,
                                   dout, efeat2 if reads_e else None, elen if reads_e else 0, F,
                                   False, emap=_fwd_slot_of_bwd(adj) if (slot and reads_e)
                                   else None)
                du = _operand_rows(du, ctx.ushape[0])
            if need_e:
                rows = fwd.row_ids()
                if msg == MSG_COPY_E:
                    g = dout.index_select(0, rows)
                    if ctx.eshape[1] == 1:
                        g = g.sum(1, keepdim=True)
                elif ctx.eshape[1] < F:  # scalar or per-head weights: g-SDDMM dot
                    u2 = ufeat2.contiguous()
                    if slot:  # forward walk, de[k] stored in slot order
                        de = _run_sddmm_dot(fwd, dout, u2, ctx.num_edges, ctx.eshape[1],
                                            slot=True)
                    else:
                        csr, tr = _eid_major(adj)
                        de = _run_sddmm_dot(csr, u2 if tr else dout, dout if tr else u2,
                                            ctx.num_edges, ctx.eshape[1])
                    g = None
                else:
                    g = dout.index_select(0, rows) * ufeat2.index_select(0, fwd.indices.long())
                if g is not None:
                    if slot:
                        de = g.reshape(ctx.eshape)
                    else:
                        de = dout.new_zeros(ctx.eshape)
                        de.index_copy_(0, fwd.eid, g)
        else:  # MAX: route each output element's gradient to its argmax slot
            valid = arg >= 0
            slots = arg.clamp(min=0)
            rowsel = valid.nonzero(as_tuple=True)
            sl = slots[rowsel]
            g = dout[rowsel]
            fidx = rowsel[1]
            dpe = F // ctx.eshape[1] if ctx.eshape is not None else 1
            if need_u:
                src = fwd.indices.long()[sl]
                gu = g
                if msg == MSG_U_MUL_E:
                    e = sl if slot else fwd.eid[sl]
                    gu = g * efeat2[e, fidx // dpe]
                du = dout.new_zeros(ctx.ushape)
                du.index_put_((src, fidx), gu, accumulate=True)
            if need_e:
                e = sl if slot else fwd.eid[sl]
                ge = g
                if msg == MSG_U_MUL_E:
                    ge = g * ufeat2[fwd.indices.long()[sl], fidx]
                de = dout.new_zeros(ctx.eshape)
                de.index_put_((e, fidx // dpe), ge, accumulate=True)
        return None, None, None, None, None, du, de, None


def gspmm(adj, msg, reduce, ufeat=None, efeat=None, num_edges=None, edge_order="eid"):
    """Generalised SpMM over ``adj`` (a SparseAdj on the features' device).

    ufeat : (num_cols, *fshape) node features or None (copy_e)
    efeat : (num_edges,) / (num_edges, 1) scalar or (num_edges, *fshape) edge
            features indexed by the adjacency's eid, or None (copy_u)
    edge_order : "eid" (efeat row e = edge id e, the frame's layout) or
            "slot" (row k = the forward CSR's slot k, as edge_attention /
            gsddmm_dot return with edge_order="slot": no eid indirection)
    returns (num_rows, *fshape) float32
    """
    slot = edge_order_of(adj, edge_order)
    msg = _MSG_NAMES.get(msg, msg)
    red = _RED_NAMES.get(reduce, reduce)
    if msg != MSG_COPY_E and ufeat is None:
        raise DGLError("message needs source node features")
    if msg != MSG_COPY_U and efeat is None:
        raise DGLError("message needs edge features")
    if ufeat is not None:
        fshape = tuple(ufeat.shape[1:])
    else:
        fshape = tuple(efeat.shape[1:]) if efeat.dim() > 1 else ()
        if fshape == (1,):
            fshape = (1,)
    F = 1
    for s in fshape:
        F *= int(s)
    dev = (ufeat if ufeat is not None else efeat).device
    adj = adj.to(dev)
    if ufeat is not None and _row_strided(ufeat, F) and dev.type == "cuda" and \
            msg == MSG_COPY_U and red in (RED_SUM, RED_MEAN):
        u2 = ufeat  # rows at a padded stride: gathered in place (_run_gspmm)
    else:
        u2 = None if ufeat is None else _f32c(ufeat.reshape(ufeat.shape[0], F))
    e2 = None
    if efeat is not None:
        ne = efeat.shape[0]
        elen = _edge_len(efeat.shape[1:], fshape) if ufeat is not None else F
        e2 = _f32c(efeat.reshape(ne, elen))
    if num_edges is None:
        num_edges = 0 if e2 is None else e2.shape[0]
    out = _GSpMM.apply(adj, msg, red, F, num_edges, u2, e2, slot)
    shape = (adj.shape[0],) + fshape if fshape else (adj.shape[0],)
    # the product's own tensor when no reshape is needed: a view would make
    # a caller's in-place update of the result rebase its autograd graph
    # (CopySlices: a zero fill and a copy of the whole gradient)
    return out if tuple(out.shape) == shape else out.reshape(shape)


class _MeanAddInto(torch.autograd.Function):
    """out <- out + mean over in-slots of ufeat[col] (copy_u + mean whose
    store adds the row's mean to the value in ``out``, in place). Backward:
    the incoming gradient for ``out``'s old value, the mean's transposed
    product for ufeat."""

    @staticmethod
    def forward(ctx, adj, ufeat2, out, feat_len):
        _run_gspmm(adj.fwd, MSG_COPY_U, RED_MEAN_ACCUM, ufeat2, None, 0, feat_len, False,
                   out=out)
        ctx.mark_dirty(out)
        ctx.adj = adj
        # what the backward's operand dC / deg looks like when padded: a
        # producer of dC (the node-row loss kernel) can write it as it stores
        # dC and hand it over as ``prescaled`` (nn.pytorch.sage_dense)
        ctx.scale_spec = None
        if out.is_cuda and _pad_rows(MSG_COPY_U, RED_SUM, out, feat_len):
            ctx.scale_spec = (adj.fwd.mean_divisor(), padded_width(feat_len))
        ctx.prescaled = None
        return out

    @staticmethod
    def backward(ctx, dout):
        adj = ctx.adj
        dout = dout.contiguous()
        given, ctx.prescaled = ctx.prescaled, None
        du = None
        if ctx.needs_input_grad[1]:
            d = _handoff.take(given, dout)  # dC / deg, written by dC's producer
            if d is None:
                d = _mean_scaled(adj.fwd, dout, padded_ok=True)
            du, _ = _run_gspmm(adj.bwd, MSG_COPY_U, RED_SUM, d, None, 0, dout.shape[1], False)
        return None, du, dout if ctx.needs_input_grad[2] else None, None


def gspmm_mean_add(adj, ufeat, out):
    """out <- out + mean over in-edges of ufeat[src] (copy_u + mean), in place
    and differentiable: the value of ``out + gspmm(adj, "copy_u", "mean",
    ufeat)`` bit for bit (a sum of two terms; rows without in-edges store
    out + 0.0, so a -0.0 there becomes +0.0), with the addition in the aggregation's own store instead of a pass
    over both tensors (GraphSAGE's fc_self(h) + mean(fc_neigh(h)),
    nn.pytorch.sage_dense). ``out``: contiguous float32 (num_rows, F) on the
    features' device; ufeat may be row-padded (F columns of a wider row)."""
    F = out.shape[1] if out.dim() == 2 else -1
    dev = ufeat.device
    if (out.dtype != torch.float32 or out.dim() != 2 or not out.is_contiguous() or
            out.device != dev or ufeat.dim() != 2 or ufeat.shape[1] != F):
        raise DGLError("gspmm_mean_add: out must be a contiguous float32 (num_rows, F) "
                       "tensor beside (num_cols, F) features")
    adj = adj.to(dev)
    if out.shape[0] != adj.shape[0] or ufeat.shape[0] < adj.shape[1]:
        raise DGLError("gspmm_mean_add: shapes do not match the adjacency")
    u2 = ufeat if (_row_strided(ufeat, F) and dev.type == "cuda") else _f32c(ufeat)
    return _MeanAddInto.apply(adj, u2, out, F)


def gsddmm_dot(adj, lhs, rhs, num_edges, heads=1, edge_order="eid"):
    """out[eid, h] = <lhs[row, h], rhs[col, h]> for every slot of ``adj``
    (rows of lhs are the adjacency's rows, of rhs its columns; no autograd).
    edge_order="slot" returns row k = forward CSR slot k instead."""
    slot = edge_order_of(adj, edge_order)
    dev = lhs.device
    adj = adj.to(dev)
    lhs2 = _f32c(lhs.reshape(lhs.shape[0], -1))
    rhs2 = _f32c(rhs.reshape(rhs.shape[0], -1))
    if slot:
        return _run_sddmm_dot(adj.fwd, lhs2, rhs2, num_edges, heads, slot=True)
    csr, tr = _eid_major(adj)
    return _run_sddmm_dot(csr, rhs2 if tr else lhs2, lhs2 if tr else rhs2, num_edges, heads)


def gspmm_into(csr, out, ufeat, accumulate=False):
    """Raw copy_u + sum over ``csr`` into ``out`` (num_rows, F), no autograd:
    out = A·ufeat (ufeat float32, or bfloat16 rows widened exactly to fp32 in
    the kernel), or with ``accumulate`` out += A·ufeat with every row's chain
    continued from the value already in ``out`` (one product evaluated segment
    by segment: dgl.distributed's pipelined forward). Degree-descending
    schedule and, under set_row_split, heavy rows cut into chunks whose
    partials are added in order (deterministic)."""
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise DGLError("out must be a contiguous float32 tensor")
    if out.shape[0] != csr.num_rows or out.device != csr.device:
        raise DGLError("out does not match the adjacency")
    if ufeat.shape[0] < csr.num_cols:
        raise DGLError("ufeat has %d rows, the adjacency %d columns"
                       % (ufeat.shape[0], csr.num_cols))
    F = out.shape[1]
    if ufeat.dtype == torch.bfloat16:  # rows read as bf16, summed in fp32 (exact widening)
        u2, msg = ufeat.reshape(ufeat.shape[0], F).contiguous(), MSG_COPY_U_BF16
    else:
        u2, msg = _f32c(ufeat.reshape(ufeat.shape[0], F)), MSG_COPY_U
    _run_gspmm(csr, msg, RED_SUM_ACCUM if accumulate else RED_SUM, u2, None, 0, F,
               False, out=out)
    return out


def gspmm_ranges(msg, beg, end, accumulate, indices, out, ufeat=None, efeat=None, eid=None):
    """out[i] (=|+=) sum over slots [beg[i], end[i]) of MSG(ufeat[indices[k]], efeat[eid[k]]),
    each row one sequential chain (continued from ``out`` when ``accumulate``).
    Raw op without autograd (the pipelined distributed forward)."""
    msg = _MSG_NAMES.get(msg, msg)
    dev = out.device
    F = out.shape[1]
    elen = 0 if efeat is None else efeat.shape[1]
    args = (msg, beg.numel(), F, ptr(beg), ptr(end), 1 if accumulate else 0, ptr(indices),
            ptr(eid), ptr(ufeat), ptr(efeat), elen, ptr(out))
    if dev.type == "cuda":
        check_call(LIB.dglhip_gspmm_ranges_device(*(args + (_stream_of(dev),))))
    else:
        check_call(LIB.dglhip_gspmm_ranges_host(*(args + (0,))))
    return out


# per-call timing (timing_enable(per_call=True)): (start, end) event pairs
_CALL_EVENTS = None


def timing_enable(flag=True, per_call=False):
    """Bracket every g-SpMM/g-SDDMM launch with hipEvents (bench support).
    With ``per_call`` instead one event pair on the current stream around each
    g-SpMM call on a ROCm device (all of the call's launches and its output's
    zero fill, no markers between the launches: the blocked schedule's 19
    launches per call had paid 0.18 ms for them); timing_read then counts
    calls."""
    global _CALL_EVENTS
    _CALL_EVENTS = [] if (flag and per_call) else None
    check_call(LIB.dglhip_timing_enable(1 if (flag and not per_call) else 0))


def timing_read():
    """(total kernel ms, launches — calls under per-call timing) since the
    last timing_enable."""
    if _CALL_EVENTS is not None:
        for _, end in _CALL_EVENTS:
            end.synchronize()
        return sum(a.elapsed_time(b) for a, b in _CALL_EVENTS), len(_CALL_EVENTS)
    ms = ctypes.c_double()
    n = ctypes.c_int64()
    check_call(LIB.dglhip_timing_read(ctypes.byref(ms), ctypes.byref(n)))
    return ms.value, n.value
