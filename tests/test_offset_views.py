"""Tensor views at a non-zero storage offset through every entry that picks a
vector width, or a whole kernel, from the run-time address of its operands.

``torch.zeros(n * F + 1)[1:].view(n, F)`` is contiguous, so ``.contiguous()``
hands it on as it is, 4 bytes past a 16-byte boundary: what a slice of a flat
parameter or gradient buffer looks like. Every case below runs one operation
with its operands, its caller-supplied outputs or its incoming gradients
replaced by such views (``offset_view``: 4 bytes off defeats the 8- and
16-byte gates, 8 bytes off passes the 8-byte gates and defeats the 16-byte
ones) and asserts

1. the result, against the reference and with the kind of assertion the
   kernel's aligned test uses (the oracle's bits for sum and max; rtol 1e-5 /
   atol 1e-6 for mean; float64 within rtol 1e-5 / atol 1e-4 for the g-SDDMM
   dot), and, where every schedule keeps one chain per output element, the
   bits of the same call on aligned tensors;
2. the schedule the case names (read from the plan or the gate's Python twin);
3. the guard floats around every view the call wrote.

The g-SpMM cases share one graph: 300 rows, 5,000 slots, source-sorted edge
ids (so the blocked schedules apply), 10 rows without slots and one hub row
of 1,052.

The gates and their cases:

* pick_vec (gspmm_impl.h): test_rows_*, test_heavy_row_split (the chunked
  launch), test_max (one launch and the row ranges);
* dglhip_gspmm_short_rows_device: test_short_row_tiers;
* the blocked item gate (gspmm_items.hip): test_blocked_*, beside
  test_items_columns / _pair / _gate;
* the sweep (sweep.hip, spmm_plan.cc): test_sweep_falls_back_on_misaligned_rows;
* launch_sddmm_dot: test_gsddmm_dot, and test_gat_layer's two-pass backward;
* dglhip_gsddmm_attention_device: test_attention_entry;
* dglhip_div_rows_device: test_div_rows (the pad columns tell the kernels apart);
* the xent kernels' flat staging and store (node_loss.hip): test_cross_entropy;
* gat_fused.hip's aggregate and dglhip_gat_backward_t_*'s check, with
  kernel.py's twin of it: test_gat_layer;
* node_linear.hip's checks and linear.py's twins: test_sage_dense_and_node_linear;
* segment_reduce.hip's aligned16: test_segment_reduce.py, as before.

Where both sides of a gate give the same bits (pick_vec, the short rows, the
item gate, the attention entry, xent) a case pins the result and the guards
for offset operands, whichever kernel runs; only the sweep (by its count and
its entries' errors), div_rows (by the pad), the rejecting entries (by their
errors) and the Python twins (asserted directly) show which side was taken.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dgl import kernel
from dgl._ffi import LIB, check_call, ptr
from dgl.base import DGLError
from dgl.nn.pytorch import linear as L
from dgl.nn.pytorch import NodeLinear, node_epilogue, sage_dense, weighted_cross_entropy
from oracle import oracle as O

SENTINEL = 1234.5
N, M = 300, 5000


def offset_view(t, k, guard=SENTINEL):
    """(view, guards): a contiguous tensor with ``t``'s shape and values whose
    data_ptr() is 4 * k bytes past a 16-byte boundary (k = 0..3), carved from
    a flat buffer filled with ``guard``; ``guards`` are the buffer's slices in
    front of the view (16 + 4 k bytes) and behind it (16 bytes)."""
    item = t.element_size()
    assert k in (0, 1, 2, 3) and (4 * k) % item == 0
    g, off, n = 16 // item, 4 * k // item, t.numel()
    buf = torch.full((g + off + n + g,), guard, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[g + off:g + off + n].view(t.shape)
    view.copy_(t)
    return view, (buf[:g + off], buf[g + off + n:])


def guards_intact(guards, guard=SENTINEL):
    return all(bool((g == guard).all()) for g in guards)


def test_offset_view_layout():
    t = torch.arange(35, dtype=torch.float32).view(5, 7)
    for k in (0, 1, 2, 3):
        v, (front, back) = offset_view(t, k)
        assert v.data_ptr() % 16 == 4 * k
        assert v.is_contiguous() and v.shape == t.shape and torch.equal(v, t)
        assert v.contiguous().data_ptr() == v.data_ptr()
        assert front.numel() == 4 + k and back.numel() == 4
        # the guards touch the view on both sides, in one storage
        assert front.data_ptr() + 4 * front.numel() == v.data_ptr()
        assert back.data_ptr() == v.data_ptr() + 4 * v.numel()
        assert guards_intact((front, back))
        v.fill_(SENTINEL + 1)  # a write into the view leaves them alone
        assert guards_intact((front, back))
        back[0] = 0.0
        assert not guards_intact((front, back))
    b, (front, back) = offset_view(t.to(torch.bfloat16), 1)  # 2-byte elements: 4 bytes off
    assert b.data_ptr() % 16 == 4 and front.numel() == 10 and back.numel() == 8
    assert guards_intact((front, back))


# ---------------------------------------------------------------------------
# The shared graph, tables and references
# ---------------------------------------------------------------------------
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda", 0)


@functools.lru_cache(None)
def _graph():
    """(src, dst, deg): destinations drawn as test_max_reducer's _graph draws
    them, edge ids in source order."""
    rng = np.random.default_rng(5)
    p = 1.0 / np.arange(1, N + 1) ** 1.1
    dst = rng.choice(N, size=M, p=p / p.sum()).astype(np.int64)
    src = rng.integers(0, N, M).astype(np.int64)
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    deg = np.bincount(dst, minlength=N)
    assert deg.max() == 1052 and (deg == 0).sum() == 10 and np.sort(deg)[-2] < 500
    return src, dst, deg


def _adj(dev):
    src, dst, _ = _graph()
    return kernel.from_coo(N, N, torch.from_numpy(dst).to(dev), torch.from_numpy(src).to(dev),
                           kernel.ORDER_EID, dev)


@functools.lru_cache(None)
def _table(F, seed=1, ints=False):
    rng = np.random.default_rng(1000 * seed + F)
    if ints:  # frequent ties for max
        return rng.integers(-4, 5, (N, F)).astype(np.float32)
    return rng.uniform(-1, 1, (N, F)).astype(np.float32)


def _elen(layout, F):
    return {None: 0, "scalar": 1, "head": 2, "full": F}[layout]


@functools.lru_cache(None)
def _weights(layout, F, ints=False):
    rng = np.random.default_rng(77 + F)
    shape = (M, _elen(layout, F))
    if ints:
        return rng.integers(-2, 3, shape).astype(np.float32)
    return rng.uniform(0.5, 1.5, shape).astype(np.float32)


def _wide(layout, F, ints=False):
    """The edge values repeated to one per feature, (M, F)."""
    W = _weights(layout, F, ints)
    return np.repeat(W, F // W.shape[1], axis=1)


@functools.lru_cache(None)
def _sum_ref(F, layout):
    """The oracle's chain per output element (O.spmm_coo)."""
    src, dst, _ = _graph()
    H = _table(F)
    if layout is None:
        return O.spmm_coo(N, dst, src, H)
    if layout == "scalar":
        return O.spmm_coo(N, dst, src, H, _weights(layout, F)[:, 0])
    W = _wide(layout, F)
    ref = np.empty((N, F), np.float32)
    for f in range(F):
        ref[:, f] = O.spmm_coo(N, dst, src, H[:, f:f + 1], np.ascontiguousarray(W[:, f]))[:, 0]
    return ref


@functools.lru_cache(None)
def _mean_ref(F, layout):
    src, dst, _ = _graph()
    msgs = _table(F)[src]
    if layout is not None:
        msgs = msgs * _wide(layout, F)
    return O.mean_mailbox(N, dst, msgs.astype(np.float32))


@functools.lru_cache(None)
def _base(F):
    return np.random.default_rng(31 + F).uniform(-1, 1, (N, F)).astype(np.float32)


@functools.lru_cache(None)
def _accum_ref(F):
    """Every row's chain continued from _base(F): the oracle's chain with the
    base rows as each row's first slot (0 + base == base exactly)."""
    src, dst, _ = _graph()
    rows = np.concatenate([np.arange(N), dst])
    cols = np.concatenate([N + np.arange(N), src])
    return O.spmm_coo(N, rows, cols, np.vstack([_table(F), _base(F)]))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, ref):
    assert np.array_equal(_np(got), ref)


def _close_mean(got, ref):
    np.testing.assert_allclose(_np(got), ref, rtol=1e-5, atol=1e-6)


def _views(k, dev, **arrays):
    """Offset views (4 k bytes) of the given arrays, checked."""
    out = {}
    for name, a in arrays.items():
        v, _ = offset_view(a if torch.is_tensor(a) else _t(a, dev), k)
        assert v.data_ptr() % 16 == 4 * k and v.is_contiguous()
        out[name] = v
    return out


def _assert_rows_path(csr, msg, red, F, elen=0):
    """One launch, one wave per row: no blocks, no heavy-row split, no tiers
    (test_special_values._assert_rows_path)."""
    assert csr.plan.schedule(msg, red, F, 0, N, elen, 0) == (kernel.PLAN_PATH_ROWS, 1)
    assert csr.plan.stats()["heavy_threshold"] == 0
    n_long, _ = csr.tiers()
    assert N - n_long < kernel.schedule_policy()["tier_min_rows"]


def _blocked_policy(F):
    """Blocks of about a fifth of the source table: several launches
    (test_special_values._blocked_policy)."""
    return dict(block_table_min=0, block_bytes=max(256, N * F * 4 // 5), block_min_row_bytes=0,
                block_min_slots=1)


# ---------------------------------------------------------------------------
# pick_vec (csrc/gspmm_impl.h): one wave per row, sum and mean
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", [None, "scalar", "head", "full"])
@pytest.mark.parametrize("F", [4, 8, 128, 130, 256])
def test_rows_sum_mean(F, layout):
    """F = 4 and 8 share a wave at VEC 2, 128 and up take a whole wave at VEC
    2 (130: a last pass with idle lanes; two heads of 65 keep VEC 1)."""
    dev = _dev()
    adj = _adj(dev)
    msg = "copy_u" if layout is None else "u_mul_e"
    elen = _elen(layout, F)
    for red in (kernel.RED_SUM, kernel.RED_MEAN):
        _assert_rows_path(adj.fwd, kernel._MSG_NAMES[msg], red, F, elen)
    h0 = _t(_table(F), dev)
    w0 = None if layout is None else _t(_weights(layout, F), dev)
    if layout == "head":  # two heads: (N, 2, F / 2) rows against (M, 2, 1) weights
        h0, w0 = h0.view(N, 2, F // 2), w0.view(M, 2, 1)

    def run(red, h, w):
        return kernel.gspmm(adj, msg, red, h, w).reshape(N, F)

    aligned = run("sum", h0, w0)
    _same(aligned, _sum_ref(F, layout))
    for k in (1, 2):
        v = _views(k, dev, h=h0, **({} if w0 is None else {"w": w0}))
        combos = [(v["h"], w0)] if w0 is None else [(v["h"], w0), (h0, v["w"]), (v["h"], v["w"])]
        for h, w in combos:
            got = run("sum", h, w)
            _same(got, _sum_ref(F, layout))
            assert torch.equal(got, aligned)
            _close_mean(run("mean", h, w), _mean_ref(F, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [4, 128, 130])
def test_rows_backward_offset_gradient(F):
    """The incoming gradient is the transposed product's source table
    (dout.contiguous() keeps the view): dH = A^T dC in the oracle's bits, for
    mean A^T (dC / deg); u_mul_e's weight gradient is the g-SDDMM dot."""
    dev = _dev()
    src, dst, deg = _graph()
    adj = _adj(dev)
    _assert_rows_path(adj.bwd, kernel.MSG_COPY_U, kernel.RED_SUM, F)
    _assert_rows_path(adj.bwd, kernel.MSG_U_MUL_E, kernel.RED_SUM, F, 1)
    G = _table(F, seed=2)
    Gm = (G / np.maximum(deg, 1).astype(np.float32)[:, None]).astype(np.float32)
    W = _weights("scalar", F)
    for k in (1, 2):
        g = _views(k, dev, g=G)["g"]
        for red, ref in (("sum", O.spmm_coo(N, src, dst, G)), ("mean", O.spmm_coo(N, src, dst, Gm))):
            h = _views(k, dev, h=_table(F))["h"].requires_grad_(True)
            kernel.gspmm(adj, "copy_u", red, h).backward(g)
            _same(h.grad, ref)
        h = _t(_table(F), dev).requires_grad_(True)
        w = _views(k, dev, w=W)["w"].requires_grad_(True)
        kernel.gspmm(adj, "u_mul_e", "sum", h, w).backward(g)
        _same(h.grad, O.spmm_coo(N, src, dst, G, W[:, 0]))
        # test_gpu_kernels.test_backward_transposed's tolerance
        np.testing.assert_allclose(_np(w.grad)[:, 0], O.sddmm_dot(dst, src, G, _table(F)),
                                   rtol=1e-5, atol=1e-4)


@pytest.mark.gpu
def test_rows_bf16_source():
    """MSG_COPY_U_BF16 at F = 128: the bf16 table 4 and 8 bytes off (two and
    four elements), and the output 4 and 8 bytes off."""
    dev = _dev()
    src, dst, _ = _graph()
    F = 128
    csr = _adj(dev).fwd
    assert csr.plan.schedule(kernel.MSG_COPY_U_BF16, kernel.RED_SUM, F, 0, N) == \
        (kernel.PLAN_PATH_ROWS, 1)
    hb0 = _t(_table(F), dev).to(torch.bfloat16)
    ref = O.spmm_coo(N, dst, src, hb0.to(torch.float32).cpu().numpy())
    for k in (1, 2):
        hb = _views(k, dev, h=hb0)["h"]
        out, guards = offset_view(torch.full((N, F), 7.0, device=dev), k)
        _same(kernel.gspmm_into(csr, torch.full((N, F), 7.0, device=dev), hb), ref)
        _same(kernel.gspmm_into(csr, out, hb0), ref)
        _same(kernel.gspmm_into(csr, out.fill_(7.0), hb), ref)
        assert guards_intact(guards)


# ---------------------------------------------------------------------------
# dglhip_gspmm_short_rows_device, and the accumulating stores into a view
# ---------------------------------------------------------------------------
def _accumulating_cases(adj, F, k, dev, exact=True):
    """sum-accumulate and mean-add into an ``out`` 4 k bytes off (guards), from
    a table 4 k bytes off: the chains' bits (``exact``), the aligned run's bits."""
    h0, b0 = _t(_table(F), dev), _t(_base(F), dev)
    h = _views(k, dev, h=h0)["h"]
    want = kernel.gspmm_into(adj.fwd, b0.clone(), h0, accumulate=True)
    out, guards = offset_view(b0, k)
    got = kernel.gspmm_into(adj.fwd, out, h, accumulate=True)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)
    if exact:
        _same(got, _accum_ref(F))
    assert guards_intact(guards)
    want = kernel.gspmm_mean_add(adj, h0, b0.clone())
    out, guards = offset_view(b0, k)
    got = kernel.gspmm_mean_add(adj, h, out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)
    np.testing.assert_allclose(_np(got), _base(F) + _mean_ref(F, None), rtol=1e-5, atol=1e-6)
    assert guards_intact(guards)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [4, 128])
def test_short_row_tiers(F):
    dev = _dev()
    old = kernel.set_short_rows(True)
    try:
        with kernel.scheduled(tier_min_rows=0):
            adj = _adj(dev)
            for red in (kernel.RED_SUM, kernel.RED_MEAN, kernel.RED_SUM_ACCUM,
                        kernel.RED_MEAN_ACCUM):
                assert adj.fwd.plan.schedule(kernel.MSG_COPY_U, red, F, 0, N) == \
                    (kernel.PLAN_PATH_ROWS, 1)
            assert adj.fwd.plan.stats()["heavy_threshold"] == 0
            n_long, tiers = adj.fwd.tiers()
            assert 0 < n_long < N and [t[0] for t in tiers] == [8, 4, 0]
            assert all(t[2] >= 10 for t in tiers)
            h0 = _t(_table(F), dev)
            aligned = kernel.gspmm(adj, "copy_u", "sum", h0)
            for k in (1, 2):
                h = _views(k, dev, h=h0)["h"]
                got = kernel.gspmm(adj, "copy_u", "sum", h)
                _same(got, _sum_ref(F, None))
                assert torch.equal(got, aligned)
                _close_mean(kernel.gspmm(adj, "copy_u", "mean", h), _mean_ref(F, None))
                _accumulating_cases(adj, F, k, dev)
    finally:
        kernel.set_short_rows(old)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [4, 128])
def test_rows_accumulate_into_offset_out(F):
    """The same stores from the one-wave-per-row kernels (no tiers)."""
    dev = _dev()
    adj = _adj(dev)
    _assert_rows_path(adj.fwd, kernel.MSG_COPY_U, kernel.RED_SUM_ACCUM, F)
    _assert_rows_path(adj.fwd, kernel.MSG_COPY_U, kernel.RED_MEAN_ACCUM, F)
    for k in (1, 2):
        _accumulating_cases(adj, F, k, dev)


# ---------------------------------------------------------------------------
# The chunked heavy-row launch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("F", [4, 128])
def test_heavy_row_split(F):
    """set_row_split(64): rows of more than 64 slots (the hub's 1,052 among
    them) are cut into chunks whose partials are added in order. As
    test_gpu_kernels.test_heavy_row_split: light rows keep the chain's bits,
    chunked rows stay within 1e-5 of it; and the aligned run's bits."""
    dev = _dev()
    _, _, deg = _graph()
    light = deg <= 64
    old = kernel.set_row_split(64)
    try:
        adj = _adj(dev)
        assert adj.fwd.plan.stats()["heavy_threshold"] == 64
        assert adj.fwd.split_plan(64, chunk=64)["num_chunks"] >= 1052 // 64 + (~light).sum()
        for red in (kernel.RED_SUM, kernel.RED_MEAN, kernel.RED_SUM_ACCUM):
            assert adj.fwd.plan.schedule(kernel.MSG_COPY_U, red, F, 0, N) == \
                (kernel.PLAN_PATH_ROWS, 1)
        h0, b0 = _t(_table(F), dev), _t(_base(F), dev)
        d = np.maximum(deg, 1).astype(np.float32)[:, None]
        exact = {"sum": _sum_ref(F, None),
                 "mean": np.where(deg[:, None] > 1, _sum_ref(F, None) / d, _sum_ref(F, None))}
        aligned = {red: kernel.gspmm(adj, "copy_u", red, h0) for red in exact}
        acc = kernel.gspmm_into(adj.fwd, b0.clone(), h0, accumulate=True)
        for k in (1, 2):
            h = _views(k, dev, h=h0)["h"]
            for red, ref in exact.items():
                got = kernel.gspmm(adj, "copy_u", red, h)
                assert torch.equal(got, aligned[red])
                assert np.array_equal(_np(got)[light], ref.astype(np.float32)[light])
                np.testing.assert_allclose(_np(got), ref, rtol=1e-5,
                                           atol=1e-5 * np.abs(ref).max())
            out, guards = offset_view(b0, k)
            got = kernel.gspmm_into(adj.fwd, out, h, accumulate=True)
            assert torch.equal(got, acc) and guards_intact(guards)
            assert np.array_equal(_np(got)[light], _accum_ref(F)[light])
            np.testing.assert_allclose(_np(got), _accum_ref(F), rtol=1e-5,
                                       atol=1e-5 * np.abs(_accum_ref(F)).max())
    finally:
        kernel.set_row_split(old)


# ---------------------------------------------------------------------------
# max: one launch and the blocked row ranges, with and without the argmax
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("layout", [None, "scalar", "full"])
@pytest.mark.parametrize("F", [4, 128])
def test_max(F, layout, blocked):
    dev = _dev()
    src, dst, _ = _graph()
    msg = "copy_u" if layout is None else "u_mul_e"
    elen = _elen(layout, F)
    H = _table(F, ints=True)
    msgs = H[src] if layout is None else (H[src] * _wide(layout, F, True)).astype(np.float32)
    ref = O.max_mailbox(N, dst, msgs)
    # integer-valued gradients: the scatter to the winning slots is exact in any order
    G = _t(_table(F, seed=3, ints=True), dev)
    policy = _blocked_policy(F) if blocked else {}
    with kernel.scheduled(**policy):
        adj = _adj(dev)
        path, launches = adj.fwd.plan.schedule(kernel._MSG_NAMES[msg], kernel.RED_MAX, F, 0, N,
                                               elen, 0)
        if blocked:
            assert path == kernel.PLAN_PATH_MAX_BLOCKED and launches > 2
        else:
            assert (path, launches) == (kernel.PLAN_PATH_ROWS, 1)
        h0 = _t(H, dev)
        # edge values by slot: row k of w is the forward CSR's slot k
        w0 = None if layout is None else \
            _t(_weights(layout, F, True), dev).index_select(0, adj.fwd.eid).contiguous()

        def run(k_h, k_w, grad):
            h = offset_view(h0, k_h)[0]
            w = None if w0 is None else offset_view(w0, k_w)[0]
            assert h.data_ptr() % 16 == 4 * k_h
            if grad:  # the argmax is written, and routes the gradient
                h.requires_grad_(True)
            out = kernel.gspmm(adj, msg, "max", h, w, edge_order="slot")
            if grad:
                out.backward(G)
            return out.detach(), h.grad

        want, want_grad = run(0, 0, True)
        _same(want, ref)
        for k in (1, 2):
            for k_h, k_w in ((k, 0),) if w0 is None else ((k, 0), (0, k), (k, k)):
                got, _ = run(k_h, k_w, False)
                _same(got, ref)
                got, grad = run(k_h, k_w, True)
                _same(got, ref)
                assert torch.equal(grad, want_grad)


# ---------------------------------------------------------------------------
# The blocked sum beyond test_items_columns / test_items_pair (they send an
# offset ufeat and an offset out through copy_u + sum at F = 128): u_mul_e
# with offset edge values, and mean_add, whose chains run in workspace rows
# and are added to the offset out at the end
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["scalar", "full"])
def test_blocked_u_mul_e(layout):
    dev = _dev()
    F = 128
    with kernel.scheduled(**_blocked_policy(F)):
        adj = _adj(dev)
        path, launches = adj.fwd.plan.schedule(kernel.MSG_U_MUL_E, kernel.RED_SUM, F, 0, N,
                                               _elen(layout, F), 1, adj.fwd.eid)
        assert path == kernel.PLAN_PATH_BLOCKED and launches > 2
        h0, w0 = _t(_table(F), dev), _t(_weights(layout, F), dev)
        aligned = kernel.gspmm(adj, "u_mul_e", "sum", h0, w0)
        _same(aligned, _sum_ref(F, layout))
        for k in (1, 2):
            v = _views(k, dev, h=h0, w=w0)
            for h, w in ((v["h"], w0), (h0, v["w"]), (v["h"], v["w"])):
                got = kernel.gspmm(adj, "u_mul_e", "sum", h, w)
                _same(got, _sum_ref(F, layout))
                assert torch.equal(got, aligned)
                _close_mean(kernel.gspmm(adj, "u_mul_e", "mean", h, w), _mean_ref(F, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [8, 128])
def test_blocked_accumulate_into_offset_out(F):
    dev = _dev()
    old = LIB.dglhip_set_blocked_mean_add(1)
    try:
        with kernel.scheduled(**_blocked_policy(F)):
            adj = _adj(dev)
            for red in (kernel.RED_SUM_ACCUM, kernel.RED_MEAN_ACCUM):
                path, launches = adj.fwd.plan.schedule(kernel.MSG_COPY_U, red, F, 0, N)
                assert path == kernel.PLAN_PATH_BLOCKED and launches > 2
            for k in (1, 2):
                _accumulating_cases(adj, F, k, dev)
    finally:
        LIB.dglhip_set_blocked_mean_add(old)


# ---------------------------------------------------------------------------
# The source sweep (csrc/sweep.hip): 8-byte vectors at F = 128 and no scalar
# form, so a run whose rows are 4 bytes off takes the sweep-off schedule
# ---------------------------------------------------------------------------
SWEEP_SRC, SWEEP_DST, SWEEP_M = 2048, 48, 48 * 160


@functools.lru_cache(None)
def _sweep_graph():
    """2,048 source rows of 128 floats: a 1-MiB table, the smallest the knobs
    below route to the sweep in four 256-KiB blocks; 44 rows of about 175
    slots (the sweep wants 128 per non-empty row) and 4 without slots."""
    rng = np.random.default_rng(9)
    src = rng.integers(0, SWEEP_SRC, SWEEP_M)
    dst = rng.integers(0, SWEEP_DST - 4, SWEEP_M)
    o = np.lexsort((dst, src))
    return src[o].astype(np.int64), dst[o].astype(np.int64)


@pytest.mark.gpu
def test_sweep_falls_back_on_misaligned_rows():
    dev = _dev()
    F = 128
    src, dst = _sweep_graph()
    rng = np.random.default_rng(10)
    H = rng.uniform(-1, 1, (SWEEP_SRC, F)).astype(np.float32)
    B = rng.uniform(-1, 1, (SWEEP_DST, F)).astype(np.float32)
    ref = O.spmm_coo(SWEEP_DST, dst, src, H)
    ref_acc = O.spmm_coo(SWEEP_DST, np.concatenate([np.arange(SWEEP_DST), dst]),
                         np.concatenate([SWEEP_SRC + np.arange(SWEEP_DST), src]),
                         np.vstack([H, B]))
    ref_mean = O.mean_mailbox(SWEEP_DST, dst, H[src])
    old = kernel.set_sweep_schedule(on=True, table_min=512 << 10, accum_table_min=512 << 10,
                                    block_bytes=256 << 10)
    try:
        adj = kernel.from_coo(SWEEP_DST, SWEEP_SRC, torch.from_numpy(dst).to(dev),
                              torch.from_numpy(src).to(dev), kernel.ORDER_EID, dev)
        csr = adj.fwd
        for red in (kernel.RED_SUM, kernel.RED_MEAN, kernel.RED_SUM_ACCUM):
            path, launches = csr.plan.schedule(kernel.MSG_COPY_U, red, F, 0, SWEEP_SRC)
            assert (path, launches) == (kernel.PLAN_PATH_SWEEP, 1), red
        h0, b0 = _t(H, dev), _t(B, dev)

        def run(h, k_out):
            """(sum, mean, sum-accum into an out 4 k_out bytes off, fallbacks)"""
            kernel.sweep_fallbacks(reset=True)
            s = kernel.gspmm(adj, "copy_u", "sum", h)
            m = kernel.gspmm(adj, "copy_u", "mean", h)
            out, guards = offset_view(b0, k_out)
            kernel.gspmm_into(csr, out, h, accumulate=True)
            torch.cuda.synchronize()
            assert guards_intact(guards)
            return s, m, out, kernel.sweep_fallbacks(reset=True)

        # aligned, and 8 bytes off (the kernel's vector width): the sweep runs
        for k_h, k_out in ((0, 0), (2, 0), (0, 2), (2, 2)):
            h = h0 if k_h == 0 else _views(k_h, dev, h=h0)["h"]
            s, m, acc, fell = run(h, k_out)
            assert fell == 0, (k_h, k_out)
            _same(s, ref)
            _close_mean(m, ref_mean)
            _same(acc, ref_acc)
        # 4 or 12 bytes off: the run takes the schedule it takes with the sweep
        # off (here one wave per row), by count and by bits
        for k_h, k_out, want in ((1, 0, 3), (3, 0, 3), (0, 1, 1), (1, 1, 3)):
            h = h0 if k_h == 0 else _views(k_h, dev, h=h0)["h"]
            s, m, acc, fell = run(h, k_out)
            assert fell == want, (k_h, k_out)
            _same(s, ref)
            _close_mean(m, ref_mean)
            _same(acc, ref_acc)
        kernel.set_sweep_schedule(on=False)
        off_path = csr.plan.schedule(kernel.MSG_COPY_U, kernel.RED_SUM, F, 0, SWEEP_SRC)
        assert off_path == (kernel.PLAN_PATH_ROWS, 1)
        kernel.set_sweep_schedule(on=True)
        # a direct caller gets an error, not the access
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        h1 = _views(1, dev, h=h0)["h"]
        o1, guards = offset_view(torch.zeros(SWEEP_DST, F, device=dev), 1)
        o0 = torch.full((SWEEP_DST, F), SENTINEL, device=dev)
        for h, o in ((h1, o0), (h0, o1)):
            with pytest.raises(DGLError, match="aligned"):
                check_call(LIB.dglhip_gspmm_sweep_device(
                    SWEEP_DST, F, ptr(csr.indptr), ptr(csr.indices), ptr(h), ptr(o),
                    ptr(csr.row_order), 0, 512, 4, 0, 10, stream))
            with pytest.raises(DGLError, match="aligned"):
                check_call(LIB.dglhip_gspmm_sweep_stream_device(
                    SWEEP_DST, 0, None, None, 4, None, None, ptr(csr.indptr), ptr(h), ptr(o), 0,
                    19, 0, None, 0, 0, 0, stream))
        torch.cuda.synchronize()
        assert guards_intact(guards) and bool((o0 == SENTINEL).all())
    finally:
        kernel.set_sweep_schedule(**old)


# ---------------------------------------------------------------------------
# g-SDDMM: the dot (launch_sddmm_dot takes the sliced kernel on 16-byte
# aligned rows only) and the attention entry
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("F,H", [(32, 1), (128, 1), (128, 4), (128, 8)])
def test_gsddmm_dot(F, H):
    """Every shape here is one the sliced kernel takes when aligned; the
    generic kernel orders a dot product differently, hence
    test_gsddmm_dot_heads' tolerance against float64."""
    dev = _dev()
    src, dst, _ = _graph()
    adj = _adj(dev)
    A, B = _table(F, seed=4), _table(F, seed=5)
    D = F // H
    ref = (A[dst].astype(np.float64).reshape(-1, H, D) *
           B[src].astype(np.float64).reshape(-1, H, D)).sum(-1)
    a0, b0 = _t(A, dev), _t(B, dev)
    np.testing.assert_allclose(_np(kernel.gsddmm_dot(adj, a0, b0, M, H)), ref, rtol=1e-5,
                               atol=1e-4)
    for k in (1, 2):
        v = _views(k, dev, a=a0, b=b0)
        for a, b in ((v["a"], b0), (a0, v["b"]), (v["a"], v["b"])):
            for order in ("eid", "slot"):
                got = kernel.gsddmm_dot(adj, a, b, M, H, edge_order=order)
                again = kernel.gsddmm_dot(adj, a, b, M, H, edge_order=order)
                assert torch.equal(got, again)
                want = ref if order == "eid" else ref[_np(adj.fwd.eid)]
                np.testing.assert_allclose(_np(got), want, rtol=1e-5, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 2, 4, 8, 16])
def test_attention_entry(H):
    """dglhip_gsddmm_attention_device with lhs and the caller's out off their
    vector width (4 H bytes, 16 from 4 heads on): test_sddmm_walk's
    reference, and the aligned call's bits."""
    dev = _dev()
    src, dst, _ = _graph()
    fwd = _adj(dev).fwd
    a1, a2 = _t(_table(H, seed=6), dev), _t(_table(H, seed=7), dev)
    s, d = fwd.indices.long(), fwd.row_ids()
    x = a1[s] + a2[d]
    ref = torch.exp(torch.where(x > 0, x, 0.2 * x)).clamp(-10, 10)
    stream = kernel._stream_of(dev)

    def run(lhs, out):
        check_call(LIB.dglhip_gsddmm_attention_device(
            fwd.num_rows, H, ptr(fwd.indptr), ptr(fwd.indices), None, ptr(lhs), ptr(a2), 0.2,
            -10.0, 10.0, 1, ptr(out), stream))
        return out

    aligned = run(a1, torch.empty(M, H, device=dev))
    torch.testing.assert_close(aligned, ref, rtol=1e-6, atol=0)
    for k in (1, 2, 3):
        lhs = _views(k, dev, a=a1)["a"]
        for l, k_out in ((lhs, 0), (a1, k), (lhs, k)):
            out, guards = offset_view(torch.zeros(M, H, device=dev), k_out)
            assert torch.equal(run(l, out), aligned)
            assert guards_intact(guards)


# ---------------------------------------------------------------------------
# dglhip_div_rows_device: the tiled kernel on 16-byte aligned x and out only
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,F,ld", [(130, 41, 48), (130, 64, 64), (257, 7, 8)])
def test_div_rows(n, F, ld):
    """Every shape is one the tiled kernel takes when both addresses are
    aligned: it writes whole padded rows, the pad columns as zeros (the
    header's promise). From an offset x or into an offset out the general
    kernel runs, which leaves the pad as it found it."""
    dev = _dev()
    rng = np.random.default_rng(n + F)
    x0 = _t(rng.standard_normal((n, F)).astype(np.float32), dev)
    x0[::5] *= 1e-38  # subnormal quotients too
    d = _t(rng.integers(1, 5000, (n, 1)).astype(np.float32), dev)
    want = x0 / d
    for kx, ko in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (1, 1), (2, 2), (3, 1)):
        x = x0 if kx == 0 else _views(kx, dev, x=x0)["x"]
        buf, guards = offset_view(torch.full((n, ld), 7.0, device=dev), ko)
        check_call(LIB.dglhip_div_rows_device(n, F, ptr(x), F, ptr(d), ptr(buf), ld,
                                              kernel._stream_of(dev)))
        assert torch.equal(buf[:, :F], want), (kx, ko)
        tiled = kx == 0 and ko == 0
        assert bool((buf[:, F:] == (0.0 if tiled else 7.0)).all()), (kx, ko)
        assert guards_intact(guards), (kx, ko)


# ---------------------------------------------------------------------------
# Cross entropy (csrc/node_loss.hip): rows packed at an odd width from an
# aligned start are staged as one float4 run (C = 41); even widths never are
# ---------------------------------------------------------------------------
def _xent_ref(z, y, w, g):
    z64 = z.detach().double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(z64, y, reduction="none")
    loss = (ce * w.double()).sum() if w is not None else ce.sum()
    (loss * g).backward()
    return loss.detach(), z64.grad


@pytest.mark.gpu
@pytest.mark.parametrize("C", [41, 64])
def test_cross_entropy(C):
    """test_node_loss.test_fused_matches_expression's tolerances; the stored
    gradient rows (dglhip_xent_bwd_device into a caller's view) keep the
    aligned call's bits."""
    dev = _dev()
    gen = torch.Generator().manual_seed(C)
    z0 = (torch.randn(N, C, generator=gen) * 3.0).to(dev)
    y = torch.randint(0, C, (N,), generator=gen)
    y[::37] = -100
    y = y.to(dev)
    w = (torch.rand(N, generator=gen) < 0.6).float().to(dev)
    from dgl.nn.pytorch import loss as LS
    stream = kernel._stream_of(dev)
    one = torch.ones((), device=dev)

    def stored(z, k_out):
        dz, guards = offset_view(torch.zeros(N, C, device=dev), k_out)
        check_call(LIB.dglhip_xent_bwd_device(N, C, ptr(z), C, ptr(y), ptr(w), ptr(one), ptr(dz),
                                              C, stream))
        torch.cuda.synchronize()
        assert guards_intact(guards)
        return dz

    dz0 = stored(z0, 0)
    for k in (0, 1, 2):
        z = (z0.clone() if k == 0 else _views(k, dev, z=z0)["z"]).requires_grad_(True)
        assert LS._fused_ok(z, y, w) and z.data_ptr() % 16 == 4 * k
        for weight in (w, None):
            z.grad = None
            loss = weighted_cross_entropy(z, y, weight)
            (loss * 2.5).backward()
            rl, rg = _xent_ref(z, y, weight, 2.5)
            assert abs(loss.item() - rl.item()) <= 1e-5 * max(1.0, abs(rl.item()))
            assert torch.allclose(z.grad.double(), rg, atol=2.5e-6, rtol=1e-5)
            assert bool((z.grad[y < 0] == 0).all())
        for k_out in (0, 1, 2):
            assert torch.equal(stored(z.detach(), k_out), dz0), (k, k_out)


# ---------------------------------------------------------------------------
# The fused GAT layer (csrc/gat_fused.hip)
# ---------------------------------------------------------------------------
def _gat_node(fs):
    """The _GATAggregate node behind gat_aggregate's reshaped output."""
    node = fs.grad_fn
    while not hasattr(node, "use_t"):
        node = node.next_functions[0][0]
    return node


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,one_pass", [(8, 16, True), (4, 32, False), (2, 5, False)])
def test_gat_layer(H, D, one_pass):
    """Forward, and both backwards: 8 x 16 takes the one-pass backward over
    the transpose (dglhip_gat_backward_t_*, which rejects ft / dout / d_ft off
    8 bytes: the forward keeps to the two-pass backward for such an ft, and an
    incoming gradient that arrives 4 bytes off is copied), the other shapes
    the two-pass one. Offset ft, offset logits, offset incoming gradients:
    the aligned call's bits, which test_gat_fused pins to the three-kernel
    composition. One exception, with its bound: the two-pass backward takes
    the per-slot dot <dout, ft> from launch_sddmm_dot, whose sliced kernel
    (16-byte aligned rows) and generic kernel order the D products
    differently, so d_el and d_er from an ft or a dout off 16 bytes are
    another fp32 evaluation of the same sums. Both stay within the a-priori
    bound of a dot of D terms feeding a chain of n = degree terms,
    (D + n + 8) * 2^-24 of the terms' magnitudes each, hence twice that
    between them (8: the epilogue's roundings per slot)."""
    dev = _dev()
    adj = _adj(dev)
    assert (LIB.dglhip_gat_backward_t_ok(H, D) == 1) == one_pass and kernel._GAT_BWD == "auto"
    gen = torch.Generator().manual_seed(H * D)
    ft0 = torch.randn(N, H, D, generator=gen).to(dev)
    el0 = torch.randn(N, H, generator=gen).to(dev)
    er0 = torch.randn(N, H, generator=gen).to(dev)
    gf0 = torch.randn(N, H, D, generator=gen).to(dev)
    gz0 = torch.randn(N, H, 1, generator=gen).to(dev)

    def run(k_ft, k_log, k_grad, use_t):
        ft, el, er = (offset_view(t, k)[0].requires_grad_(True)
                      for t, k in ((ft0, k_ft), (el0, k_log), (er0, k_log)))
        gf, gz = offset_view(gf0, k_grad)[0], offset_view(gz0, k_grad)[0]
        assert ft.data_ptr() % 16 == 4 * k_ft and gf.data_ptr() % 16 == 4 * k_grad
        fs, z = kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.3, seed=77)
        assert _gat_node(fs).use_t == use_t, (k_ft, k_log, k_grad)
        torch.autograd.backward([fs, z], [gf, gz])
        return fs.detach(), z.detach(), ft.grad, el.grad, er.grad

    want = run(0, 0, 0, one_pass)
    # the magnitudes of d_er's terms (per destination) and d_el's (per source):
    # a * (scale * sum |dout * ft| + |dz|) per slot and head, in float64
    fwd = adj.fwd
    s, d = fwd.indices.long(), fwd.row_ids()
    a = kernel.edge_attention(adj, el0, er0, M, edge_order="slot").double()
    dots = (gf0[d].double() * ft0[s].double()).abs().sum(-1)
    m = a * (dots / (1.0 - 0.3) + gz0[d].double().abs().squeeze(-1))
    zero = torch.zeros(N, H, dtype=torch.float64, device=dev)
    ones = torch.ones(M, 1, dtype=torch.float64, device=dev)
    bound = {}
    for name, rows in (("d_el", s), ("d_er", d)):
        n_terms = torch.zeros(N, 1, dtype=torch.float64, device=dev).index_add_(0, rows, ones)
        bound[name] = 2 * (D + n_terms + 8) * 2.0 ** -24 * zero.index_add(0, rows, m)
    # the two backwards agree bit for bit (test_transposed_backward_same_bits),
    # so one aligned run is the reference for both
    names = ("ft_sum", "z", "d_ft", "d_el", "d_er")
    for k_ft, k_log, k_grad in ((1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2),
                                (1, 1, 1), (2, 2, 2), (2, 1, 1)):
        use_t = one_pass and k_ft % 2 == 0
        got = run(k_ft, k_log, k_grad, use_t)
        # the sliced dot applies at these shapes (F = 128) and not at 2 x 5
        same_dot = use_t or H * D != 128 or (k_ft == 0 and k_grad == 0)
        for name, x, y in zip(names, got, want):
            if same_dot or name not in bound:
                assert torch.equal(x, y), (k_ft, k_log, k_grad, name)
            else:
                err = (x.double() - y.double()).abs()
                assert bool((err <= bound[name]).all()), (k_ft, k_log, k_grad, name,
                                                          float((err - bound[name]).max()))


# ---------------------------------------------------------------------------
# NodeLinear, sage_dense (csrc/node_linear.hip rejects inputs off 16 bytes:
# linear.py asks _mfma_fwd_ok / _mfma_cat_ok first), node_epilogue, gather_rows
# ---------------------------------------------------------------------------
def _ints(rng, shape, lo=-3, hi=4):
    return torch.from_numpy(rng.integers(lo, hi, shape).astype(np.float32))


def _int_linear(rng, fin, fout, bias, dev):
    lin = NodeLinear(fin, fout, bias=bias).to(dev)
    with torch.no_grad():
        lin.weight.copy_(_ints(rng, (fout, fin), -2, 3))
        if bias:
            lin.bias.copy_(_ints(rng, (fout,)))
    return lin


@pytest.mark.gpu
@pytest.mark.parametrize("fin,fout,relu", [(128, 41, False), (64, 41, False), (64, 64, True),
                                           (128, 128, True), (96, 41, False), (96, 96, True)])
def test_sage_dense_and_node_linear(fin, fout, relu):
    """Integer-valued operands keep every f32 product and sum exact, so the
    MFMA kernels (test_node_linear's layout tests) and torch's GEMMs both
    equal the float64 layer bit for bit: 64 and 128 inputs take the MFMA
    entries when aligned (narrowing: both products in one pass, then the
    one-pass input gradient; square with ReLU: the concatenated product),
    96 never does, and no offset input may."""
    dev = _dev()
    src, dst, _ = _graph()
    adj = _adj(dev)
    rng = np.random.default_rng(fin * 1000 + fout)
    fs, fn_ = _int_linear(rng, fin, fout, True, dev), _int_linear(rng, fin, fout, False, dev)
    x0, dy0 = _ints(rng, (N, fin)).to(dev), _ints(rng, (N, fout)).to(dev)
    act = torch.relu if relu else None

    def aggregate(t):
        return kernel.gspmm(adj, "copy_u", "sum", t)

    # the float64 layer: fc_self(x) + fc_neigh(A x), torch's autograd
    A = torch.zeros(N, N, dtype=torch.float64)
    A.index_put_((torch.from_numpy(dst), torch.from_numpy(src)),
                 torch.ones(M, dtype=torch.float64), accumulate=True)
    x64 = x0.cpu().double().requires_grad_(True)
    ws, wn, b = (p.detach().cpu().double().requires_grad_(True)
                 for p in (fs.weight, fn_.weight, fs.bias))
    ref = x64 @ ws.t() + b + (A @ x64) @ wn.t()
    ref = ref.relu() if relu else ref
    ref.backward(dy0.cpu().double())
    narrowing = fin > fout
    fast = fin in (64, 128)
    for k_x, k_dy in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (1, 1)):
        x = offset_view(x0, k_x)[0].requires_grad_(True)
        dy = offset_view(dy0, k_dy)[0]
        if narrowing:
            assert L._mfma_fwd_ok(x, fout, fout) == (fast and k_x == 0)
        else:
            assert L._mfma_cat_ok(x, aggregate(x.detach()), fout, relu) == (fast and k_x == 0)
        for p in (fs.weight, fs.bias, fn_.weight):
            p.grad = None
        out = sage_dense(x, aggregate, fs, fn_, act)
        out.backward(dy)
        assert torch.equal(out.detach().cpu().double(), ref.detach()), (k_x, k_dy)
        for got, want in ((x.grad, x64.grad), (fs.weight.grad, ws.grad), (fs.bias.grad, b.grad),
                          (fn_.weight.grad, wn.grad)):
            assert torch.equal(got.cpu().double(), want), (k_x, k_dy)
        # NodeLinear alone (torch's GEMMs at any address)
        fs.weight.grad = fs.bias.grad = None
        x = offset_view(x0, k_x)[0].requires_grad_(True)
        y = fs(x)
        y.backward(dy)
        assert torch.equal(y.detach().cpu().double(),
                           (x64 @ ws.t() + b).detach()), (k_x, k_dy)
        assert torch.equal(x.grad.cpu().double(), dy0.cpu().double() @ ws.detach())


@pytest.mark.gpu
@pytest.mark.parametrize("F", [7, 128])
def test_node_epilogue(F):
    """act(x * row_scale + bias): the bits of torch's three operations both
    ways (the bias gradient: integer-valued gradients, exact in any order)."""
    dev = _dev()
    rng = np.random.default_rng(F)
    x0 = _t(rng.standard_normal((N, F)).astype(np.float32), dev)
    rs = _t(rng.uniform(0.1, 1, (N,)).astype(np.float32), dev)
    b0 = _t(rng.standard_normal(F).astype(np.float32), dev)
    dy0 = _ints(rng, (N, F)).to(dev)

    def run(k, fused):
        x = offset_view(x0, k)[0].requires_grad_(True)
        b = offset_view(b0, k)[0].requires_grad_(True)
        dy = offset_view(dy0, k)[0]
        if fused:
            out = node_epilogue(x, rs, b, torch.relu)
        else:
            out = torch.relu(x * rs.reshape(-1, 1) + b)
        out.backward(dy)
        return out.detach(), x.grad, b.grad

    want = run(0, False)
    for k in (0, 1, 2, 3):
        for a, b in zip(run(k, True), want):
            assert torch.equal(a, b), k


@pytest.mark.gpu
@pytest.mark.parametrize("F", [7, 128])
def test_gather_rows(F):
    """x[idx] and its gradient (each row's duplicates summed in order by the
    typed-block kernel): integer-valued gradients, exact in any order."""
    dev = _dev()
    rng = np.random.default_rng(F + 1)
    idx = torch.from_numpy(rng.integers(0, N, 2000)).to(dev)
    idx[:700] = 3  # a hub row: chunks of TYPED_CHUNK positions
    x0 = _t(rng.standard_normal((N, F)).astype(np.float32), dev)
    dy0 = _ints(rng, (2000, F)).to(dev)
    want = torch.zeros(N, F, device=dev).index_add_(0, idx, dy0)
    for k in (0, 1, 2):
        x = offset_view(x0, k)[0].requires_grad_(True)
        y = kernel.gather_rows(x, idx)
        y.backward(offset_view(dy0, k)[0])
        assert torch.equal(y.detach(), x0[idx]) and torch.equal(x.grad, want), k
