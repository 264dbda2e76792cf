"""The edge-attention operators: GAT's per-edge attention, its fused
aggregation layer with its backwards and its attention logits
(csrc/gat_fused.hip), and the softmax over a node's edges
(csrc/edge_softmax.hip)."""
from __future__ import absolute_import

import os
import weakref

import numpy as np
import torch

from .._ffi import LIB, check_call, ptr, stream_of as _stream_of
from ..base import DGLError
from ..device_graph import _workspace
# the block sizes are read as _plan.<name> at call time: plan owns them
from . import plan as _plan
from .policy import MSG_U_MUL_E, MSG_COPY_E, RED_SUM, SLOT, schedule_policy
from .plan import _block_cuts, _block_edge_rows, _block_plan, _cuts_native
from .spmm import (
    _eid_major, _f32c, _fwd_slot_of_bwd, _operand_rows, _run_gspmm, _run_sddmm_dot,
    edge_order_of, gspmm_ranges)

# ---------------------------------------------------------------------------
# GAT edge attention (fused u_add_v g-SDDMM + leaky_relu + exp + clamp)
# ---------------------------------------------------------------------------
class _EdgeAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, adj, num_edges, alpha, lo, hi, apply_exp, a_src, a_dst, slot=False):
        # lhs is gathered by column, rhs read per row: over the transpose the
        # roles swap (a_dst[v] + a_src[u] == a_src[u] + a_dst[v] exactly).
        # slot: the forward CSR, out[k] per slot (no eid, sequential stores)
        csr, tr = (adj.fwd, False) if slot else _eid_major(adj)
        H = a_src.shape[1]
        lhs, rhs = (a_dst, a_src) if tr else (a_src, a_dst)
        out = torch.empty(num_edges, H, dtype=torch.float32, device=a_src.device)
        args = (csr.num_rows, H, ptr(csr.indptr), ptr(csr.indices),
                ptr(None if slot else csr.eid), ptr(lhs), ptr(rhs), float(alpha), float(lo),
                float(hi), 1 if apply_exp else 0, ptr(out))
        if a_src.is_cuda:
            check_call(LIB.dglhip_gsddmm_attention_device(*(args + (_stream_of(a_src.device),))))
        else:
            check_call(LIB.dglhip_gsddmm_attention_host(*(args + (0,))))
        ctx.adj, ctx.alpha, ctx.lo, ctx.hi, ctx.apply_exp = adj, alpha, lo, hi, apply_exp
        ctx.slot, ctx.tr = slot, tr
        ctx.save_for_backward(out, a_src, a_dst)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, a_src, a_dst = ctx.saved_tensors
        adj = ctx.adj
        # d/dx clamp(exp(lrelu(x))): out * lrelu'(x) where not clamped, the
        # slope alpha where the logit x <= 0 (x == 0 included), as torch's
        # leaky_relu backward: from x itself, recomputed in out's order
        # (out <= 1 would differ for 0 < x < 2^-24, where exp(x) rounds to 1)
        x = _edge_logits(adj, a_src, a_dst, ctx.slot, ctx.tr, out.shape[0])
        inside = (out > ctx.lo) & (out < ctx.hi)
        slope = torch.where(x <= 0, torch.full_like(out, ctx.alpha), torch.ones_like(out))
        g = dout * out * slope if ctx.apply_exp else dout * slope
        g = torch.where(inside, g, torch.zeros_like(g)).contiguous()
        # sum the per-edge gradient at the source (transposed CSR) and destination
        H = g.shape[1]
        d_src, _ = _run_gspmm(adj.bwd, MSG_COPY_E, RED_SUM, None, g, H, H, False,
                              emap=_fwd_slot_of_bwd(adj) if ctx.slot else None)
        d_dst, _ = _run_gspmm(adj.fwd, MSG_COPY_E, RED_SUM, None, g, H, H, False,
                              emap=SLOT if ctx.slot else None)
        return (None, None, None, None, None, None, _operand_rows(d_src, a_src.shape[0]), d_dst,
                None)


def _edge_logits(adj, a_src, a_dst, slot, tr, num_edges):
    """x = a_src[u] + a_dst[v] per edge u -> v (the attention kernels' sum,
    float32): by forward slot, or by edge id through the CSR the forward ran
    over (tr: the transpose, whose rows are the sources)."""
    if slot:
        fwd = adj.fwd
        return a_src.index_select(0, fwd.indices.long()) + \
            a_dst.index_select(0, fwd.row_ids())
    csr, _ = _eid_major(adj)
    rows, cols = csr.row_ids(), csr.indices.long()
    u, v = (rows, cols) if tr else (cols, rows)
    x = torch.empty(num_edges, a_src.shape[1], dtype=torch.float32, device=a_src.device)
    x[csr.eid.long()] = a_src.index_select(0, u) + a_dst.index_select(0, v)
    return x


def edge_attention(adj, a_src, a_dst, num_edges, alpha=0.2, clamp=(-10.0, 10.0),
                   apply_exp=True, edge_order="eid"):
    """Per-edge, per-head GAT attention in one kernel:
    clamp(exp(leaky_relu(a_src[u] + a_dst[v], alpha))) for every edge u -> v,
    returned as (num_edges, H) indexed by edge id (edge_order="slot": by
    forward CSR slot, for gspmm(..., edge_order="slot")). Differentiable in
    a_src/a_dst."""
    slot = edge_order_of(adj, edge_order)
    dev = a_src.device
    adj = adj.to(dev)
    H = a_src.reshape(a_src.shape[0], -1).shape[1]
    return _EdgeAttention.apply(adj, int(num_edges), float(alpha), float(clamp[0]),
                                float(clamp[1]), bool(apply_exp),
                                _f32c(a_src.reshape(-1, H)), _f32c(a_dst.reshape(-1, H)), slot)


# ---------------------------------------------------------------------------
# Fused GAT aggregation: attention + dropout + normaliser + head-broadcast sum
# ---------------------------------------------------------------------------
_GAT_SEED = {}
# the GAT backward: "auto" (the one-pass transposed kernel where it applies,
# 8 heads x 16) or "three" (r03's three passes, the attention stored)
_GAT_BWD = os.environ.get("DGLHIP_GAT_BWD", "auto")


def set_gat_backward(policy):
    """Study / test knob for the fused GAT layer's backward: "auto" or
    "three"; returns the old policy. Same bits either way."""
    global _GAT_BWD
    old = _GAT_BWD
    _GAT_BWD = str(policy)
    return old


def _gat_seed_counter(dev):
    """The per-device int64 counter of captured calls. Made at the first call
    on the device outside a capture (the warm-up a capture needs anyway), so
    its zero fill is not part of any graph; made first inside a capture its
    start value is arbitrary (torch.empty: a captured fill would reset it at
    every replay)."""
    key = str(dev)
    if key not in _GAT_SEED:
        if torch.cuda.is_current_stream_capturing():
            _GAT_SEED[key] = torch.empty(1, dtype=torch.int64, device=dev)
        else:
            _GAT_SEED[key] = torch.zeros(1, dtype=torch.int64, device=dev)
    return _GAT_SEED[key]


def _gat_seed_offset(dev):
    """For a call captured in a HIP graph: a base seed from torch's generator
    (drawn at capture) and the device counter the fused kernel adds to it,
    advanced on the device at every replay: every replay draws a new mask
    with no host round trip."""
    off = _gat_seed_counter(dev)
    off.add_(1)
    return int(torch.randint(0, 1 << 62, (1,)).item()), off


def set_gat_variant(variant):
    """Study knob for the fused GAT kernel: 0 automatic (default), 1 the
    attention computed in every lane that consumes it, 2 once per (slot,
    head) through LDS (1/2/4/8/16 heads) with each batch's feature rows
    gathered after its attention, 3 the LDS kernel with them gathered before
    it (what 0 picks on two-float lanes). Same bits."""
    check_call(LIB.dglhip_set_gat_variant(int(variant)))


def gat_dropout_scale(p):
    """The kept attention's scale 1 / (1 - p) as the fused kernel computes it
    (float32 operands), so host compositions match its bits."""
    one = np.float32(1.0)
    return float(one / (one - np.float32(p)))


def gat_dropout_mask(num_slots, num_heads, p, seed):
    """bool (num_slots, num_heads): the (slot, head) pairs the fused kernel
    keeps at dropout probability ``p`` under seed ``seed`` (its counter hash,
    computed on the host)."""
    keep = torch.empty(num_slots, num_heads, dtype=torch.uint8)
    check_call(LIB.dglhip_gat_dropout_mask_host(num_slots, num_heads, float(p), int(seed),
                                                ptr(keep)))
    return keep.bool()


def _attention_slots(fwd, el, er, alpha, lo, hi, apply_exp):
    out = torch.empty(fwd.nnz, el.shape[1], dtype=torch.float32, device=el.device)
    args = (fwd.num_rows, el.shape[1], ptr(fwd.indptr), ptr(fwd.indices), None, ptr(el),
            ptr(er), float(alpha), float(lo), float(hi), 1 if apply_exp else 0, ptr(out))
    if el.is_cuda:
        check_call(LIB.dglhip_gsddmm_attention_device(*(args + (_stream_of(el.device),))))
    else:
        check_call(LIB.dglhip_gsddmm_attention_host(*(args + (0,))))
    return out


class _GATAggregate(torch.autograd.Function):
    """(ft_sum, z) = (sum_k w[k,h] ft[u_k, h, :], sum_k a[k,h]) per destination
    row and head, a = clamp(exp(leaky_relu(el[u] + er[v]))), w = dropout(a),
    all in one kernel on the device (dglhip_gat_aggregate_device); a and w are
    kept in CSR slot order only when a gradient is needed. The backward is the
    three-kernel path's (the u_mul_e product over the transpose, the g-SDDMM
    dot, the copy_e gather, the attention's backward): same bits."""

    @staticmethod
    def forward(ctx, adj, alpha, lo, hi, apply_exp, p, seed, seed_off, el, er, ft2, D, grad_mode,
                attn_l=None):
        fwd = adj.fwd
        H = el.shape[1]
        F = ft2.shape[1]
        dev = ft2.device
        # needs_input_grad follows requires_grad even under torch.no_grad():
        # the caller's grad mode decides whether a backward can follow
        need = grad_mode and any(ctx.needs_input_grad[8:11])
        a = w = None
        # the one-pass backward over the transpose recomputes the attention:
        # nothing per edge is stored (8 heads x 16, _gat_backward_t)
        ctx.use_t = (need and dev.type == "cuda" and _GAT_BWD == "auto" and
                     LIB.dglhip_gat_backward_t_ok(H, D) == 1 and ft2.data_ptr() % 8 == 0)
        if dev.type == "cuda":
            out_ft = torch.empty(fwd.num_rows, F, dtype=torch.float32, device=dev)
            out_z = torch.empty(fwd.num_rows, H, dtype=torch.float32, device=dev)
            if need and not ctx.use_t:
                a = torch.empty(fwd.nnz, H, dtype=torch.float32, device=dev)
                w = torch.empty_like(a) if p > 0 else None
            # source-blocked (exact where the blocks never decrease along a
            # row): one launch per block, both chains continued; with nothing
            # stored, smaller blocks (_GAT_BLOCK_BYTES_NOGRAD)
            cuts = _block_cuts(fwd, (F + H) * 4,
                               None if a is not None else _plan._GAT_BLOCK_BYTES_NOGRAD)
            if cuts is None:
                cuts = [fwd.indptr, fwd.indptr[1:]]
            # attn_l (el known to be gat_logits(ft, attn_l)): the 8 x 16
            # blocked kernel recomputes each source's logit from its row
            for b in range(len(cuts) - 1):
                check_call(LIB.dglhip_gat_aggregate_logits_ranges_device(
                    fwd.num_rows, ft2.shape[0], H, D, ptr(cuts[b]), ptr(cuts[b + 1]),
                    1 if b else 0, ptr(fwd.indices), ptr(fwd.row_order), ptr(el), ptr(er),
                    ptr(ft2), ptr(attn_l), float(alpha), float(lo), float(hi),
                    1 if apply_exp else 0, float(p), int(seed), ptr(seed_off), ptr(out_ft),
                    ptr(out_z), ptr(a), ptr(w), _stream_of(dev)))
        else:  # host: the same per-edge values and chains from the host kernels
            a = _attention_slots(fwd, el, er, alpha, lo, hi, apply_exp)
            w = None
            if p > 0:
                keep = gat_dropout_mask(fwd.nnz, H, p, seed)
                w = torch.where(keep, a * gat_dropout_scale(p), torch.zeros_like(a))
            out_ft, _ = _run_gspmm(fwd, MSG_U_MUL_E, RED_SUM, ft2, w if p > 0 else a, H, F,
                                   False, emap=SLOT)
            out_z, _ = _run_gspmm(fwd, MSG_COPY_E, RED_SUM, None, a, H, H, False, emap=SLOT)
            if not need:
                a = w = None
        ctx.adj, ctx.alpha, ctx.lo, ctx.hi, ctx.apply_exp, ctx.p = adj, alpha, lo, hi, \
            apply_exp, p
        # the dropout seed as this call used it (a captured call's device
        # counter moves on at the next call): the backward recomputes keep bits
        ctx.seed = int(seed)
        ctx.seed_off = None if (seed_off is None or p == 0 or not need) else seed_off.clone()
        if ctx.use_t:
            ctx.D = D
            ctx.save_for_backward(ft2, el, er)
        else:  # (el, er: the logits' sign gives the leaky_relu slope)
            ctx.save_for_backward(ft2, a, w, el, er)
        return out_ft, out_z

    @staticmethod
    def backward(ctx, d_ft, d_z):
        if ctx.use_t:
            return _gat_backward_t(ctx, d_ft, d_z) + (None,)
        ft2, a, w, el, er = ctx.saved_tensors
        adj = ctx.adj
        fwd = adj.fwd
        H = a.shape[1]
        F = ft2.shape[1]
        need_el, need_er, need_ft = ctx.needs_input_grad[8:11]
        d_el = d_er = d_ft2 = None
        # (fs unused: its zero gradient has the adjacency's rows, not ft's)
        d_ft = (torch.zeros(fwd.num_rows, F, dtype=torch.float32, device=ft2.device)
                if d_ft is None else d_ft.contiguous())
        wt = w if w is not None else a
        if need_ft:
            # (source-blocked where the transpose qualifies: _run_gspmm)
            d_ft2, _ = _run_gspmm(adj.bwd, MSG_U_MUL_E, RED_SUM, d_ft, wt, H, F, False,
                                  emap=_fwd_slot_of_bwd(adj))
        if need_el or need_er:
            scale = gat_dropout_scale(ctx.p) if w is not None else 1.0
            if ft2.is_cuda:
                # the dot, dropout, normaliser and activation gradients in one
                # pass (the g-SDDMM dot with the GAT epilogue): the torch ops
                # below, fused, same bits
                g = torch.empty_like(a)
                dz = None if d_z is None else d_z.contiguous()
                # every slot's value is its own: the source blocks' sub-ranges
                # (ft rows of one block at a time) give the same bits
                cuts = _block_cuts(fwd, F * 4) or [fwd.indptr, fwd.indptr[1:]]
                ft2c = ft2.contiguous()
                # er's gradient (the copy_edge sum of g over each row's slots)
                # summed in the same pass, in slot order across the blocks:
                # the same chain as the separate sum, one E x H read less
                fuse_er = (need_er and LIB.dglhip_gat_attention_grad_rowsum_ok(F, H) == 1 and
                           d_ft.data_ptr() % 16 == 0 and ft2c.data_ptr() % 16 == 0)
                er_sum = (torch.zeros(fwd.num_rows, H, dtype=torch.float32, device=ft2.device)
                          if fuse_er else None)
                # keep bits from the forward's hash (drop_p), not w != 0; the
                # slope from the logits el[u] + er[v]
                p_hash = float(ctx.p) if w is not None else 0.0
                for b in range(len(cuts) - 1):
                    check_call(LIB.dglhip_gat_attention_grad_logits_ranges_device(
                        fwd.num_rows, F, H, ptr(cuts[b]), ptr(cuts[b + 1]),
                        ptr(fwd.row_order), ptr(fwd.indices), ptr(d_ft), ptr(ft2c), ptr(a),
                        None, ptr(dz), ptr(el), ptr(er), float(ctx.alpha), float(ctx.lo),
                        float(ctx.hi), 1 if ctx.apply_exp else 0, 1.0, p_hash, ctx.seed,
                        ptr(ctx.seed_off), ptr(g), ptr(er_sum), _stream_of(ft2.device)))
                if fuse_er:
                    d_er = er_sum
            else:
                d_a = _run_sddmm_dot(fwd, d_ft, ft2.contiguous(), fwd.nnz, H, slot=True)
                if w is not None:  # dropout's backward: the kept pairs (the hash), scaled
                    keep = gat_dropout_mask(fwd.nnz, H, ctx.p, ctx.seed).to(d_a.device)
                    d_a = torch.where(keep, d_a * scale, torch.zeros_like(d_a))
                if d_z is not None:
                    d_a = d_a + d_z.contiguous().index_select(0, fwd.row_ids())
                # the attention's backward (_EdgeAttention.backward, slot order)
                x = _edge_logits(adj, el, er, True, False, fwd.nnz)
                inside = (a > ctx.lo) & (a < ctx.hi)
                slope = torch.where(x <= 0, torch.full_like(a, ctx.alpha), torch.ones_like(a))
                g = d_a * a * slope if ctx.apply_exp else d_a * slope
                g = torch.where(inside, g, torch.zeros_like(g)).contiguous()
            if need_el:
                d_el = _gat_el_grad(adj, g, H)
            if need_er and d_er is None:
                d_er, _ = _run_gspmm(fwd, MSG_COPY_E, RED_SUM, None, g, H, H, False, emap=SLOT)
        return (None,) * 8 + (_operand_rows(d_el, el.shape[0]), d_er,
                              _operand_rows(d_ft2, ft2.shape[0]), None, None, None)


def _gat_backward_t(ctx, d_ft, d_z):
    """The GAT layer's backward as ONE pass over the transpose
    (dglhip_gat_backward_t_device): d_ft and d_el chained in the transpose's
    slot order — over its source-blocked plan when it has one, each block's
    launch continuing the chains — and the attention gradient g stored at its
    forward slot; d_er is the copy_e sum of g over the forward CSR. The
    attention and the dropout keep bits are recomputed from el, er and the
    seed, so the forward stored nothing per edge. Same bits as the r03
    three-pass backward (attention gradient over the CSR, d_ft and d_el over
    the transpose through the slot map)."""
    ft2, el, er = ctx.saved_tensors
    adj = ctx.adj
    fwd, bwd = adj.fwd, adj.bwd
    H, F, D = el.shape[1], ft2.shape[1], ctx.D
    need_el, need_er, need_ft = ctx.needs_input_grad[8:11]
    dev = ft2.device
    dout = (torch.zeros(fwd.num_rows, F, dtype=torch.float32, device=dev) if d_ft is None
            else _f32c(d_ft))
    if dout.data_ptr() % 8:
        # the entry reads dout's rows in 8-byte vectors and rejects others; the
        # forward stored nothing for the two-pass backward, so a gradient that
        # arrives as a view at an odd float offset is copied to rows of its own
        dout = dout.clone()
    dz = None if d_z is None else _f32c(d_z)
    emap = _fwd_slot_of_bwd(adj)
    d_ft2 = torch.empty(bwd.num_rows, F, dtype=torch.float32, device=dev)
    d_el = torch.empty(bwd.num_rows, H, dtype=torch.float32, device=dev)
    # the attention gradient at its forward slot, for d_er's sum (none when
    # er needs no gradient: the kernel then stores nothing)
    g = torch.empty(fwd.nnz, H, dtype=torch.float32, device=dev) if need_er else None
    common = (fwd.num_rows, ft2.shape[0], H, D)
    rest = (float(ctx.alpha), float(ctx.lo), float(ctx.hi), 1 if ctx.apply_exp else 0,
            float(ctx.p), ctx.seed, ptr(ctx.seed_off), ptr(d_ft2), ptr(d_el), ptr(g),
            _stream_of(dev))
    if dz is not None:
        # er and dz side by side in one [rows, 2H] table: a pair's two
        # destination operands in one 64-B run, one line per slot instead of
        # two (same bits)
        erdz = torch.cat([er, dz], 1)
        tail = (ptr(ft2), ptr(el), ptr(erdz), ptr(dout)) + rest
        entry = LIB.dglhip_gat_backward_t_packed_device
    else:
        tail = (ptr(ft2), ptr(el), ptr(er), ptr(dz), ptr(dout)) + rest
        entry = LIB.dglhip_gat_backward_t_device
    plan = _block_plan(bwd, dout, F, _plan._GAT_BWD_BLOCK_BYTES) if bwd.nnz else None
    if plan is None:
        check_call(entry(
            bwd.num_rows, ptr(bwd.row_order), ptr(bwd.indptr), ptr(bwd.indptr[1:]), 1, 0,
            *(common + (ptr(bwd.indices), ptr(emap)) + tail)))
    else:
        # the plan's launches over its global slot arrays: item offsets (ptr)
        # are global, so every launch takes the same column-id and map bases
        erows = _block_edge_rows(bwd, plan, emap)
        if plan.absent.numel():
            d_ft2.index_fill_(0, plan.absent.long(), 0.0)
            d_el.index_fill_(0, plan.absent.long(), 0.0)
        for i, it in enumerate(plan):
            check_call(entry(
                it.rows.numel(), ptr(it.rows), ptr(it.ptr), ptr(it.ptr[1:]), 0, 1 if i else 0,
                *(common + (ptr(plan.indices), ptr(erows)) + tail)))
    d_er = None
    if need_er:  # the copy_e sum of g over the CSR, one wave per row (same chain)
        d_er = torch.empty(fwd.num_rows, H, dtype=torch.float32, device=dev)
        check_call(LIB.dglhip_rowsum_heads8_device(fwd.num_rows, ptr(fwd.indptr),
                                                   ptr(fwd.row_order), ptr(g), ptr(d_er),
                                                   _stream_of(dev)))
    return ((None,) * 8 + (_operand_rows(d_el, el.shape[0]) if need_el else None, d_er,
                           _operand_rows(d_ft2, ft2.shape[0]) if need_ft else None, None, None))


def _gat_el_grad(adj, g, H):
    """d_el[u, h] = sum of g[forward slot of k, h] over the transpose's slots k
    of source u, in slot order (the copy_edge sum of the attention gradient
    along the transpose). On a ROCm device with a graph numbered source-major
    it runs over destination blocks (row sub-ranges of the transpose, each
    continuing the rows' chains: the same bits); else in one launch."""
    bwd = adj.bwd
    emap = _fwd_slot_of_bwd(adj)
    cuts = None
    pol = schedule_policy()
    if g.is_cuda and pol["blocked"] and bwd.nnz and bwd.nnz < (1 << 31):
        B = -(-(g.numel() * g.element_size()) // _plan._EL_GRAD_BLOCK_BYTES)
        B = min(B, bwd.nnz // (pol["block_min_slots"] * max(bwd.num_nonempty, 1)))
        if B >= 2:
            cuts = _cuts_native(bwd, 0, 0, B)
    if cuts is None:
        return _run_gspmm(bwd, MSG_COPY_E, RED_SUM, None, g, H, H, False, emap=emap)[0]
    out = torch.empty(bwd.num_rows, H, dtype=torch.float32, device=g.device)
    for b in range(len(cuts) - 1):
        gspmm_ranges(MSG_COPY_E, cuts[b], cuts[b + 1], b > 0, bwd.indices, out, efeat=g,
                     eid=emap)
    return out


def gat_aggregate(adj, ft, el, er, alpha=0.2, clamp=(-10.0, 10.0), attn_drop=0.0,
                  training=True, apply_exp=True, seed=None):
    """One GAT layer's aggregation in one kernel (examples/pytorch/gat/train.py:74-96):
    for every destination row v and head h, over v's in-edges u -> v in CSR
    slot order,

        a      = clamp(exp(leaky_relu(el[u, h] + er[v, h], alpha)), *clamp)
        ft_sum = sum a_drop * ft[u, h, :]    (a_drop = dropout(a), training only)
        z      = sum a

    returned as (ft_sum (R, H, D), z (R, H, 1)), differentiable in ft, el, er.
    ft (N, H, D); el (N, H[, 1]); er (R, H[, 1]); ft and el may carry more rows
    than the adjacency has columns (their gradients' extra rows are zero).
    Equals edge_attention(...,
    edge_order="slot") followed by gspmm(u_mul_e, sum) and gspmm(copy_e, sum)
    bit for bit. The dropout mask is the kernel's counter hash of (seed,
    slot, head) (gat_dropout_mask), not torch's generator; ``seed`` None draws
    the seed from torch's generator at every call (inside a HIP graph capture:
    once per device, plus a device counter advanced at every replay)."""
    p = float(attn_drop) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise DGLError("attention dropout must be in [0, 1), got %r" % (attn_drop,))
    dev = ft.device
    adj = adj.to(dev)
    N, H, D = ft.shape
    el2 = _f32c(el.reshape(el.shape[0], H))
    er2 = _f32c(er.reshape(er.shape[0], H))
    ft2 = _f32c(ft.reshape(N, H * D))
    if el2.shape[0] < adj.shape[1] or er2.shape[0] != adj.shape[0] or N < adj.shape[1]:
        raise DGLError("gat_aggregate: feature rows do not match the adjacency")
    seed_off = None
    if p > 0 and seed is None:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            seed, seed_off = _gat_seed_offset(dev)
        else:  # torch's generator, every call: torch.manual_seed repeats the masks
            if dev.type == "cuda":
                _gat_seed_counter(dev)  # ready for a later capture
            seed = int(torch.randint(0, 1 << 62, (1,)).item())
    ft_sum, z = _GATAggregate.apply(adj, float(alpha), float(clamp[0]), float(clamp[1]),
                                    bool(apply_exp), p, int(seed or 0), seed_off, el2, er2,
                                    ft2, D, torch.is_grad_enabled(), _logits_source(el, ft))
    return ft_sum.view(-1, H, D), z.view(-1, H, 1)


class _GATLogits(torch.autograd.Function):
    """(el, er) = ((ft * attn_l).sum(-1), (ft * attn_r).sum(-1)) per node and
    head in the library's fixed association (dglhip_gat_logits_*); backward
    in torch: d_ft = d_el * attn_l + d_er * attn_r, d_attn = sum_n d_e * ft."""

    @staticmethod
    def forward(ctx, ft, attn_l, attn_r):
        N, H, D = ft.shape
        el = torch.empty(N, H, dtype=torch.float32, device=ft.device)
        er = torch.empty_like(el)
        args = (N, H, D, ptr(ft), ptr(attn_l), ptr(attn_r), ptr(el), ptr(er))
        if ft.is_cuda:
            check_call(LIB.dglhip_gat_logits_device(*(args + (_stream_of(ft.device),))))
        else:
            check_call(LIB.dglhip_gat_logits_host(*(args + (0,))))
        ctx.save_for_backward(ft, attn_l, attn_r)
        return el, er

    @staticmethod
    def backward(ctx, d_el, d_er):
        ft, attn_l, attn_r = ctx.saved_tensors
        H, D = attn_l.shape
        d_el = torch.zeros(ft.shape[:2], device=ft.device) if d_el is None else d_el
        d_er = torch.zeros(ft.shape[:2], device=ft.device) if d_er is None else d_er
        d_ft = d_attn_l = d_attn_r = None
        if ctx.needs_input_grad[0]:
            d_ft = d_el.unsqueeze(-1) * attn_l + d_er.unsqueeze(-1) * attn_r
        if ctx.needs_input_grad[1]:
            d_attn_l = (d_el.unsqueeze(-1) * ft).sum(0)
        if ctx.needs_input_grad[2]:
            d_attn_r = (d_er.unsqueeze(-1) * ft).sum(0)
        return d_ft, d_attn_l, d_attn_r


def gat_logits(ft, attn_l, attn_r):
    """The GAT layer's attention logits (examples/pytorch/gat/train.py:66-67,
    ``bmm(head_ft, attn_l)``): el, er (N, H, 1) with el[n, h] = sum_d
    ft[n, h, d] * attn_l[h, d], in the library's association
    (dglhip_gat_logits_*). Differentiable in ft, attn_l and attn_r. When
    gat_aggregate is then given this el with the same ft, its 8-head x 16
    source-blocked forward recomputes each source's logit from the feature
    row it gathers anyway (same bits, a fifth fewer line requests)."""
    N, H, D = ft.shape
    ftc = _f32c(ft)
    al = _f32c(attn_l.reshape(H, D))
    ar = _f32c(attn_r.reshape(H, D))
    el, er = _GATLogits.apply(ftc, al, ar)
    el, er = el.view(N, H, 1), er.view(N, H, 1)
    # what the aggregation may recompute el from: this ft (data, shape,
    # version, and the tensor itself, held weakly: once it is freed its
    # address may come back as another tensor's) and attn_l's values at this
    # call; el's own version too (an in-place change of el voids the tag)
    el._dglhip_logits = (ftc.data_ptr(), tuple(ftc.shape), ftc._version, el._version,
                         al.detach().clone(), weakref.ref(ftc))
    return el, er


def _logits_source(el, ft):
    """attn_l when ``el`` came from gat_logits(ft, attn_l, ...) on this very ft
    (same data, shape and version) at 8 heads x 16 on a device, else None."""
    tag = getattr(el, "_dglhip_logits", None)
    if tag is None or not ft.is_cuda or tuple(ft.shape[1:]) != (8, 16):
        return None
    ptr_, shape, version, el_version, al, ref = tag
    if (ref() is None or ft.data_ptr() != ptr_ or tuple(ft.shape) != shape or
            ft._version != version or el._version != el_version):
        return None
    return al if al.device == ft.device else None


# ---------------------------------------------------------------------------
# Edge softmax: the softmax of per-edge scores over each row's slots
# (csrc/edge_softmax.hip)
# ---------------------------------------------------------------------------
EDGE_SOFTMAX_CHUNK = 1024  # DGLHIP_EDGE_SOFTMAX_CHUNK: a longer row is cut into pieces


def _softmax_run(rows, x, dy):
    """The forward over the scores ``x`` (``dy`` None) or the backward from
    the forward's ``x`` = y and ``dy``, both (nnz, H) float32 contiguous.
    ``rows``: (num_rows, indptr, eid or None, row_order or None, the longest
    row or -1)."""
    R, indptr, eid, row_order, max_len = rows
    nnz, H = x.shape
    dev = x.device
    out = torch.empty_like(x)
    if dev.type == "cuda":
        nbytes = 0
        if max_len < 0 or max_len > EDGE_SOFTMAX_CHUNK:
            nbytes = LIB.dglhip_edge_softmax_workspace_bytes(R, nnz, H)
        ws = _workspace(nbytes, dev) if nbytes else None
        head = (R, nnz, H, ptr(indptr), ptr(eid), ptr(row_order))
        tail = (ptr(out), max_len, ptr(ws), _stream_of(dev))
        if dy is None:
            check_call(LIB.dglhip_edge_softmax_device(*(head + (ptr(x),) + tail)))
        else:
            check_call(LIB.dglhip_edge_softmax_bwd_device(*(head + (ptr(x), ptr(dy)) + tail)))
    elif dy is None:
        check_call(LIB.dglhip_edge_softmax_host(R, nnz, H, ptr(indptr), ptr(eid), ptr(x),
                                                ptr(out), 0))
    else:
        check_call(LIB.dglhip_edge_softmax_bwd_host(R, nnz, H, ptr(indptr), ptr(eid), ptr(x),
                                                    ptr(dy), ptr(out), 0))
    return out


class _EdgeSoftmax(torch.autograd.Function):
    """y = softmax of x over the slots of each row; dx = y * (dy - sum y dy)."""

    @staticmethod
    def forward(ctx, x, rows):
        y = _softmax_run(rows, x, None)
        ctx.rows = rows
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _softmax_run(ctx.rows, y, _f32c(dy)), None


def _softmax_columns(x, what):
    """``x`` (rows, ...) as (rows, H) float32 contiguous."""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise DGLError("%s expects a tensor of rows" % what)
    H = 1
    for d in x.shape[1:]:
        H *= d
    return _f32c(x.reshape(x.shape[0], H))


def edge_softmax(adj, logits, norm_by="dst", edge_order="eid"):
    """The softmax of the edge scores ``logits`` over the in-edges of every
    destination (``norm_by="dst"``, the rows of ``adj.fwd``) or the out-edges
    of every source (``"src"``, the rows of ``adj.bwd``), one kernel forward
    and one backward (csrc/edge_softmax.hip). ``logits`` is ``(E,)`` or
    ``(E, ...)`` float32 indexed by edge id, every trailing position its own
    softmax; the result has its shape. ``edge_order="slot"``
    (``norm_by="dst"`` only) takes and returns values in forward-CSR slot
    order, as ``gspmm`` and ``edge_attention`` do.

    Per group: y = expf(x - max x) / sum, in float32; a NaN or +inf makes the
    group NaN, -inf beside a finite maximum gives 0, a node without edges
    contributes nothing. The same bits on every call (no atomics); the sum's
    order is the kernel's, not the slot order."""
    if norm_by not in ("dst", "src"):
        raise DGLError("norm_by must be 'dst' or 'src', got %r" % (norm_by,))
    slot = edge_order_of(adj, edge_order)
    if slot and norm_by != "dst":
        raise DGLError("edge_order='slot' is the forward CSR's order: norm_by='dst' only")
    x = _softmax_columns(logits, "edge_softmax")
    adj = adj.to(logits.device)
    csr = adj.fwd if norm_by == "dst" else adj.bwd
    if x.shape[0] != csr.nnz:
        raise DGLError("edge_softmax: %d rows of logits for %d edges" % (x.shape[0], csr.nnz))
    if x.numel() == 0:
        return torch.empty_like(logits)
    rows = (csr.num_rows, csr.indptr, None if slot else csr.slot_eid, csr.row_order,
            csr.max_degree)
    return _EdgeSoftmax.apply(x, rows).view(logits.shape)


def segment_softmax(x, segments):
    """The softmax of ``x`` (N, ...) float32 over each consecutive row range
    of ``segments`` (a :class:`SegmentOffsets`), every trailing position its
    own softmax: the edge-softmax kernel with the offsets as its row pointer
    and no edge ids. Differentiable; the result has ``x``'s shape."""
    x2 = _softmax_columns(x, "segment_softmax")
    N = x2.shape[0]
    if segments.num_rows >= 0 and segments.num_rows != N:
        raise DGLError("offsets end at %d, expected the %d rows" % (segments.num_rows, N))
    if x2.numel() == 0 or segments.num_segments == 0:
        return torch.empty_like(x)
    rows = (segments.num_segments, segments.on(x.device), None, None, segments.max_rows)
    return _EdgeSoftmax.apply(x2, rows).view(x.shape)
