"""The source-blocked schedule of copy_u + sum / mean (kernel._block_plan,
DESIGN.md §4.1): B launches over per-block segment CSRs, each row's chain
continued block by block. It is used only when, along every row's slots
(edge-id order), the source blocks never decrease — then the blocked chain IS
the row's chain and the results are bit-identical to the one-launch schedule
(and the oracle). These tests check the plan's gate (monotone graphs get it,
others do not), the bits on the host and on the device (forward, mean, the
transposed backward, line-straddling F), and that the bench graph takes it.
"""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import kernel
from oracle import oracle as O


def _graph(n, m, seed, sorted_src):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    if sorted_src:  # edges numbered source-major, as (src, dst)-sorted loaders give them
        o = np.lexsort((dst, src))
        src, dst = src[o], dst[o]
    return src, dst


@pytest.fixture
def small_blocks():
    with kernel.scheduled(block_table_min=0, block_bytes=1 << 16):
        yield


def _chains_kept(csr, plan):
    """Every row's slots, read block by block in plan order (each block's
    items in their slot order), are the row's CSR slots in order; every
    block's indices are the CSR's at its positions."""
    rows, segs, pos = [], [], []
    for i, it in enumerate(plan):
        assert torch.equal(it.indices, csr.indices[it.pos])
        cnt = it.ptr[1:] - it.ptr[:-1]
        assert bool((cnt > 0).all()) and bool((cnt[:-1] >= cnt[1:]).all())  # longest first
        rows.append(torch.repeat_interleave(it.rows.long(), cnt))
        segs.append(torch.full((it.nnz,), i, dtype=torch.int64))
        pos.append(it.pos)
    rows, segs, pos = torch.cat(rows), torch.cat(segs), torch.cat(pos)
    order = torch.sort(rows * len(plan) + segs, stable=True)[1]
    return torch.equal(pos[order], torch.arange(csr.nnz))


def test_plan_gate_and_host_bits(small_blocks):
    n, m = 2000, 200_000
    src, dst = _graph(n, m, 0, True)
    csr = kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                           kernel.ORDER_EID, "cpu")
    h = torch.randn(n, 128, generator=torch.Generator().manual_seed(1))
    plan = kernel._block_plan(csr, h, 128)
    assert plan is not None and len(plan) >= 2 and not plan[-1].suffix
    assert sum(p.nnz for p in plan) == csr.nnz
    assert _chains_kept(csr, plan)
    # the same chains through the host kernel, item by item: the oracle's bits
    ref = torch.from_numpy(O.spmm_coo(n, dst, src, h.numpy()))
    out = torch.zeros(n, 128)
    for it in plan:
        part = kernel.build_csr(n, n, torch.repeat_interleave(it.rows.long(),
                                                              it.ptr[1:] - it.ptr[:-1]),
                                it.indices.long(), kernel.ORDER_EID, "cpu")
        kernel._run_gspmm(part, kernel.MSG_COPY_U, kernel.RED_SUM_ACCUM, h, None, 0, 128,
                          False, out=out)
    assert torch.equal(out, ref)
    # edges in random order: some row's blocks decrease -> no plan
    src2, dst2 = _graph(n, m, 0, False)
    csr2 = kernel.build_csr(n, n, torch.from_numpy(dst2), torch.from_numpy(src2),
                            kernel.ORDER_EID, "cpu")
    assert kernel._block_plan(csr2, h, 128) is None
    # off switch
    old = kernel.set_blocked("off")
    try:
        assert kernel._block_plan(csr, h, 128) is None
    finally:
        kernel.set_blocked(old)


def test_suffix_after_monotone_prefix(small_blocks):
    """Edges appended after a source-major list (GCN's self-loops): each row's
    monotone prefix is blocked and the rest runs last, in order; the host
    run of the plan equals the oracle's chain bit for bit. A random-order
    graph's suffixes are too long: no plan."""
    n, m = 2000, 200_000
    src, dst = _graph(n, m, 0, True)
    ar = np.arange(n)
    src, dst = np.concatenate([src, ar]), np.concatenate([dst, ar])
    csr = kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                           kernel.ORDER_EID, "cpu")
    h = torch.randn(n, 128, generator=torch.Generator().manual_seed(1))
    plan = kernel._block_plan(csr, h, 128)
    assert plan is not None and len(plan) >= 3 and plan[-1].suffix
    assert sum(p.nnz for p in plan) == csr.nnz
    assert 0 < plan[-1].nnz <= n  # at most each row's self-loop
    assert _chains_kept(csr, plan)
    cuts = kernel._block_cuts(csr, 128 * 4, 1 << 16)
    assert cuts is not None and len(cuts) == len(plan) + 1
    assert torch.equal(cuts[-1], csr.indptr[1:]) and torch.equal(cuts[0], csr.indptr[:-1])


@pytest.mark.gpu
@pytest.mark.parametrize("F", [128, 41])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_blocked_device_bits(F, reduce):
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m = 120_000, 8_000_000  # 61 MB table at F = 128: 8 blocks; 3 at F = 41
    src, dst = _graph(n, m, 3, True)
    g = dgl.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)))
    gen = torch.Generator().manual_seed(4)
    H = torch.randn(n, F, generator=gen)
    G = torch.randn(n, F, generator=gen)
    red = fn.sum if reduce == "sum" else fn.mean

    def run(policy):
        old = kernel.set_blocked(policy)
        try:
            h = H.to(dev).requires_grad_(True)
            g.ndata["h"] = h
            kernel.timing_enable(True)
            g.update_all(fn.copy_src("h", "m"), red("m", "o"))
            g.ndata["o"].backward(G.to(dev))
            torch.cuda.synchronize()
            _, launches = kernel.timing_read()
            kernel.timing_enable(False)
            return g.ndata["o"].detach().cpu(), h.grad.cpu(), launches
        finally:
            kernel.set_blocked(old)
    o1, g1, n1 = run("auto")
    o0, g0, n0 = run("off")
    adj = g.sparse_adjacency(dev)
    assert kernel._block_plan(adj.fwd, H.to(dev), F) is not None
    assert n1 > n0  # the blocked launches ran, forward and backward
    assert torch.equal(o1, o0) and torch.equal(g1, g0)
    if reduce == "sum":
        assert np.array_equal(o1.numpy(), O.spmm_coo(n, dst, src, H.numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [16, 32, 41, 48, 64])
def test_blocked_narrow_rows_same_bits(F):
    """Narrow source rows (<= 64 floats: F = 41 runs at its 48-float padded
    stride) on the blocked schedule: forward, the transposed backward, mean
    and a continued (SUM_ACCUM) product equal the one-launch run bit for bit,
    and the oracle's chains; rows of 1, 2 and 3 slots and odd tails
    included."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m = 120_000, 8_000_000
    src, dst = _graph(n, m, 5, True)
    # a few rows with 1..3 slots in the source-major order (short items)
    src = np.concatenate([src, [7, 8, 9, 10, 11, 12]]).astype(np.int64)
    dst = np.concatenate([dst, [n - 1, n - 2, n - 2, n - 3, n - 3, n - 3]]).astype(np.int64)
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    g = dgl.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)))
    gen = torch.Generator().manual_seed(6)
    H = torch.randn(n, F, generator=gen)
    G = torch.randn(n, F, generator=gen)
    base = torch.randn(n, F, generator=gen)
    adj = g.sparse_adjacency(dev)

    def run(policy):
        old = kernel.set_blocked(policy)
        try:
            h = H.to(dev).requires_grad_(True)
            g.ndata["h"] = h
            g.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
            g.ndata["o"].backward(G.to(dev))
            g.update_all(fn.copy_src("h", "m"), fn.mean("m", "mo"))
            acc = base.to(dev).clone()
            kernel.gspmm_into(adj.fwd, acc, H.to(dev), accumulate=True)
            torch.cuda.synchronize()
            return [g.ndata["o"].detach().cpu(), h.grad.cpu(), g.ndata["mo"].cpu(), acc.cpu()]
        finally:
            kernel.set_blocked(old)
    # small tables: blocks of 2 MiB so that every width takes the blocked schedule
    with kernel.scheduled(block_table_min=0, block_bytes=2 << 20, block_min_row_bytes=0):
        assert kernel._block_plan(adj.fwd, H.to(dev), F) is not None
        blocked, single = run("auto"), run("off")
    for a, b in zip(blocked, single):
        assert torch.equal(a, b)
    assert np.array_equal(blocked[0].numpy(), O.spmm_coo(n, dst, src, H.numpy()))
    assert np.array_equal(blocked[1].numpy(), O.spmm_coo(n, src, dst, G.numpy()))


@pytest.mark.gpu
def test_random_order_graph_keeps_one_launch():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m = 60_000, 6_000_000
    src, dst = _graph(n, m, 5, False)
    adj = kernel.from_coo(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                          kernel.ORDER_EID, dev)
    h = torch.randn(n, 128, device=dev)
    assert kernel._block_plan(adj.fwd, h, 128) is None
    out = kernel.gspmm(adj, "copy_u", "sum", h)
    assert np.array_equal(out.cpu().numpy(), O.spmm_coo(n, dst, src, h.cpu().numpy()))


@pytest.mark.gpu
def test_bench_graph_takes_the_blocked_schedule():
    """The Reddit-shaped bench graph (edges numbered source-major by the
    generator) qualifies in both directions."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from dgl import data
    dev = torch.device("cuda", 0)
    src, dst, n = data.reddit_like(device=dev)
    adj = kernel.from_coo(n, n, dst, src, kernel.ORDER_EID, dev)
    h = torch.empty(n, 128, device=dev)
    plan = kernel._block_plan(adj.fwd, h, 128)
    assert plan is not None and len(plan) >= 8
    assert kernel._block_plan(adj.bwd, h, 128) is not None


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_blocked_accumulate_over_a_column_span(dtype):
    """gspmm_into with accumulate over a CSR whose slots reference one range
    of a larger buffer (a pipelined partition's halo chunk): the blocks cut
    that range, every block adds to ``out``; bits equal the one-launch path."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m, base = 120_000, 8_000_000, 150_000
    src, dst = _graph(n, m, 6, True)
    csr = kernel.build_csr(n, 3 * n, torch.from_numpy(dst), torch.from_numpy(src + base),
                           kernel.ORDER_EID, dev)
    gen = torch.Generator().manual_seed(7)
    buf = (torch.rand(3 * n, 128, generator=gen) * 2 - 1).to(dev).to(dtype)
    init = (torch.rand(n, 128, generator=gen) * 2 - 1).to(dev)

    def run(policy, accumulate):
        old = kernel.set_blocked(policy)
        try:
            out = init.clone()
            kernel.timing_enable(True)
            kernel.gspmm_into(csr, out, buf, accumulate=accumulate)
            torch.cuda.synchronize()
            _, launches = kernel.timing_read()
            kernel.timing_enable(False)
            return out.cpu(), launches
        finally:
            kernel.set_blocked(old)
    assert kernel._column_span(csr) == (base + int(src.min()), base + int(src.max()) + 1)
    for acc in (False, True):
        o1, n1 = run("auto", acc)
        o0, n0 = run("off", acc)
        assert n1 > n0
        assert torch.equal(o1, o0)


@pytest.mark.gpu
def test_gcn_self_loops_blocked_bits():
    """The GCN example's graph (edges, then self-loops appended) takes the
    blocked schedule with a suffix launch; forward and backward equal the
    one-launch path and the oracle."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m = 120_000, 8_000_000
    src, dst = _graph(n, m, 12, True)
    g = dgl.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)))
    g.add_edges(g.nodes(), g.nodes())
    adj = g.sparse_adjacency(dev)
    H = torch.randn(n, 128, generator=torch.Generator().manual_seed(2))
    plan = kernel._block_plan(adj.fwd, H.to(dev), 128)
    assert plan is not None and plan[-1].nnz > 0

    def run(policy):
        old = kernel.set_blocked(policy)
        try:
            h = H.to(dev).requires_grad_(True)
            g.ndata["h"] = h
            g.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
            g.ndata["o"].backward(torch.ones(n, 128, device=dev))
            return g.ndata["o"].detach().cpu(), h.grad.cpu()
        finally:
            kernel.set_blocked(old)
    o1, g1 = run("auto")
    o0, g0 = run("off")
    assert torch.equal(o1, o0) and torch.equal(g1, g0)
    s2 = np.concatenate([src, np.arange(n)])
    d2 = np.concatenate([dst, np.arange(n)])
    assert np.array_equal(o1.numpy(), O.spmm_coo(n, d2, s2, H.numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["eid", "slot"])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_blocked_u_mul_e_bits(order, reduce):
    """u_mul_e (scalar and per-head edge values) over the blocks' row ranges:
    forward and both gradients equal the one-launch kernels."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m = 120_000, 8_000_000
    src, dst = _graph(n, m, 13, True)
    adj = kernel.from_coo(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                          kernel.ORDER_EID, dev)
    gen = torch.Generator().manual_seed(14)
    H = torch.randn(n, 128, generator=gen).to(dev)
    for w in (torch.rand(m, 1, generator=gen), torch.rand(m, 4, 1, generator=gen)):
        w = w.to(dev)
        h3 = H if w.dim() == 2 else H.view(n, 4, 32)

        def run(policy):
            old = kernel.set_blocked(policy)
            try:
                h = h3.clone().requires_grad_(True)
                we = w.clone().requires_grad_(True)
                kernel.timing_enable(True)
                o = kernel.gspmm(adj, "u_mul_e", reduce, h, we, edge_order=order)
                torch.cuda.synchronize()
                _, launches = kernel.timing_read()
                kernel.timing_enable(False)
                o.backward(torch.ones_like(o))
                return o.detach().cpu(), h.grad.cpu(), we.grad.cpu(), launches
            finally:
                kernel.set_blocked(old)
        a = run("auto")
        b = run("off")
        assert a[3] > b[3]
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y)
        # pinned to the oracle directly (r03 verdict, "Next" 7): per head the
        # forward is the reference's fma chain over COO (dst, src) in edge
        # order with that head's weights (mean: that chain over max(deg, 1),
        # IEEE division); dH the same chain over the transpose with dC's
        # rows; the weight gradient within 1e-5 of the float64 dot
        wc = w.cpu().reshape(m, -1).numpy()
        # edge_order "slot": the values are in the CSR's slot order (edges
        # grouped by destination in edge order); map them to edge ids
        inv = np.argsort(np.argsort(dst, kind="stable"), kind="stable")
        if order == "slot":
            wc = wc[inv]
        Hh = wc.shape[1]
        Hc = H.cpu().numpy().reshape(n, Hh, -1)
        deg = np.maximum(np.bincount(dst, minlength=n), 1).astype(np.float32)
        dC = np.ones((n, Hh, Hc.shape[2]), np.float32)
        if reduce == "mean":
            dC = dC / deg[:, None, None]
        for hh in range(Hh):
            ref = O.spmm_coo(n, dst, src, Hc[:, hh], wc[:, hh])
            if reduce == "mean":
                ref = ref / deg[:, None]
            assert np.array_equal(a[0].reshape(n, Hh, -1)[:, hh].numpy(), ref)
            dref = O.spmm_coo(n, src, dst, dC[:, hh], wc[:, hh])
            assert np.array_equal(a[1].reshape(n, Hh, -1)[:, hh].numpy(), dref)
            dw = O.sddmm_dot(dst, src, dC[:, hh], Hc[:, hh])
            gw = a[2].reshape(m, Hh)[:, hh].numpy()
            if order == "slot":
                gw = gw[inv]
            assert np.allclose(gw, dw, rtol=1e-5, atol=1e-5 * float(np.abs(dw).max()))


def test_u_mul_e_plan_slot_map(small_blocks):
    """The blocked plan's slot map (blocks in order, suffix last) covers
    every slot once and maps through the edge ids; a per-slot row tensor is
    composed once per object and anew after an in-place change."""
    n, m = 2000, 200_000
    src, dst = _graph(n, m, 3, True)
    ar = np.arange(n)
    src, dst = np.concatenate([src, ar]), np.concatenate([dst, ar])
    csr = kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                           kernel.ORDER_EID, "cpu")
    gen = torch.Generator().manual_seed(5)
    h = torch.randn(n, 128, generator=gen)
    w = torch.rand(csr.nnz, 1, generator=gen)
    plan = kernel._block_plan(csr, h, 128)
    slots = kernel._block_slots(csr, plan)
    assert torch.equal(torch.sort(slots)[0], torch.arange(csr.nnz))
    assert torch.equal(slots, torch.cat([it.pos for it in plan]))
    rows = kernel._block_edge_rows(csr, plan, None)
    eid = csr.slot_eid if csr.slot_eid is not None else torch.arange(csr.nnz)
    assert torch.equal(rows, eid[slots])
    # a per-slot row map: composed once per tensor object, anew when it changes
    emap = torch.randperm(csr.nnz)
    r1 = kernel._block_edge_rows(csr, plan, emap)
    assert kernel._block_edge_rows(csr, plan, emap) is r1
    assert torch.equal(r1, emap[slots])
    emap[:5] = emap[:5].flip(0)
    r2 = kernel._block_edge_rows(csr, plan, emap)
    assert r2 is not r1 and torch.equal(r2, emap[slots])


@pytest.mark.gpu
@pytest.mark.parametrize("halo", ["allgather", "alltoall"])
def test_pipelined_segments_blocked_bits(halo):
    """An emulated rank of a 2-rank partition (no communication: the halo
    rows are the rank's own random landing buffer): its pipelined segments
    (own rows, then each halo chunk, continued with SUM_ACCUM) take the
    blocked schedule over their column spans, with the one-launch bits."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from dgl.distributed import PartitionedGraph, balanced_bounds
    dev = torch.device("cuda", 0)
    n, m, W = 200_000, 24_000_000, 2
    src, dst = _graph(n, m, 15, True)
    src, dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    bounds = balanced_bounds(torch.bincount(dst, minlength=n), W)
    lo, hi = int(bounds[0]), int(bounds[1])
    sel = (dst >= lo) & (dst < hi)
    pg = PartitionedGraph(n, src[sel], dst[sel], bounds, dev, pipeline_chunks=4, rank=0,
                          world=W, halo=halo)
    h_local = torch.rand(hi - lo, 128, generator=torch.Generator().manual_seed(16)).to(dev)
    pg.update_all(h_local)  # lands the emulated halo rows
    assert kernel._block_plan(pg.seg_csrs[0], h_local, 128) is not None

    def run(policy):
        old = kernel.set_blocked(policy)
        try:
            return pg.update_all(h_local).cpu()
        finally:
            kernel.set_blocked(old)
    assert torch.equal(run("auto"), run("off"))


@pytest.mark.gpu
@pytest.mark.parametrize("msg", ["copy_u", "u_mul_e"])
def test_blocked_max_bits_with_ties(msg):
    """The max reducer over the blocks' row ranges: values, and (features
    drawn from a few integers: ties everywhere) the argmax routing of the
    gradient, equal the one-launch kernel's."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m = 120_000, 8_000_000
    src, dst = _graph(n, m, 17, True)
    adj = kernel.from_coo(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                          kernel.ORDER_EID, dev)
    gen = torch.Generator().manual_seed(18)
    H = torch.randint(-3, 4, (n, 128), generator=gen).float().to(dev)
    w = torch.randint(1, 3, (m, 1), generator=gen).float().to(dev)
    assert kernel._block_cuts(adj.fwd, 128 * 4, kernel.schedule_policy()["block_bytes"]) is not None

    def run(policy):
        old = kernel.set_blocked(policy)
        try:
            h = H.clone().requires_grad_(True)
            kernel.timing_enable(True)
            if msg == "copy_u":
                o = kernel.gspmm(adj, "copy_u", "max", h)
            else:  # weights in slot order (blocked); by edge id they keep one launch
                o = kernel.gspmm(adj, "u_mul_e", "max", h, w, edge_order="slot")
            torch.cuda.synchronize()
            _, launches = kernel.timing_read()
            kernel.timing_enable(False)
            o.backward(torch.arange(n * 128, device=dev, dtype=torch.float32).view(n, 128))
            return o.detach().cpu(), h.grad.cpu(), launches
        finally:
            kernel.set_blocked(old)
    o1, g1, n1 = run("auto")
    o0, g0, n0 = run("off")
    assert n1 > n0
    assert torch.equal(o1, o0) and torch.equal(g1, g0)
    # pinned to the oracle directly (r03 verdict, "Next" 7): the values are
    # the degree-bucketing max over each row's mailbox (messages in edge
    # order; empty rows 0); with the upstream gradient zero past row R0, each
    # (row, feature)'s value routes to the source of its first maximal message
    # in edge order (strict >): integers throughout, exact
    inv = np.argsort(np.argsort(dst, kind="stable"), kind="stable")
    w_edge = w.cpu().numpy()[inv]  # slot-ordered weights, per edge id
    Hn = H.cpu().numpy()
    full = Hn[src] if msg == "copy_u" else Hn[src] * w_edge
    assert np.array_equal(o1.numpy(), O.max_mailbox(n, dst, full))
    R0 = 3000
    G = np.zeros((n, 128), np.float32)
    G[:R0] = np.arange(R0 * 128, dtype=np.float32).reshape(R0, 128)
    old = kernel.set_blocked("auto")
    try:
        h = H.clone().requires_grad_(True)
        if msg == "copy_u":
            o = kernel.gspmm(adj, "copy_u", "max", h)
        else:
            o = kernel.gspmm(adj, "u_mul_e", "max", h, w, edge_order="slot")
        o.backward(torch.from_numpy(G).to(dev))
        got = h.grad.cpu().numpy()
    finally:
        kernel.set_blocked(old)
    expect = np.zeros((n, 128), np.float64)
    es = np.nonzero(dst < R0)[0]  # edge order
    rows = dst[es]
    srt = np.argsort(rows, kind="stable")
    es, rows = es[srt], rows[srt]
    starts = np.searchsorted(rows, np.arange(R0))
    ends = np.searchsorted(rows, np.arange(R0), side="right")
    for r in range(R0):
        if starts[r] == ends[r]:
            continue
        e = es[starts[r]:ends[r]]
        block = full[e]
        first = np.argmax(block == block.max(0), axis=0)  # first maximal message
        wgt = 1.0 if msg == "copy_u" else w_edge[e[first], 0]
        np.add.at(expect, (src[e[first]], np.arange(128)), G[r] * wgt)
    assert np.array_equal(got, expect.astype(np.float32))


def _tagged_graph():
    """A CSR whose blocked plan has a suffix at B = 2 but none at B = 3: most
    rows are source-sorted below column 600; a few end with sources 1000
    then 999 (blocks 1 then 0 at B = 2 — a decrease, so a suffix; both in
    block 1 at B = 3); one row references column 1999 (the span)."""
    rng = np.random.default_rng(21)
    n = 2000
    src, dst = [], []
    for r in range(n):
        s = np.sort(rng.integers(0, 600, 40))
        src.append(s)
        dst.append(np.full(40, r))
    for r in range(0, n, 50):
        src.append(np.array([1000, 999]))
        dst.append(np.array([r, r]))
    src.append(np.array([1999]))
    dst.append(np.array([7]))
    return n, np.concatenate(src), np.concatenate(dst)


def test_plan_caches_keyed_on_blocks_not_length():
    """Caches derived from a blocked plan (slot map, edge rows) are keyed on
    its block count and suffix, not its length: B = 2 plus a suffix and B = 3
    without one are both three launches (the slot map of one was
    reused for the other)."""
    n, src, dst = _tagged_graph()
    csr = kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                           kernel.ORDER_EID, "cpu")
    p2 = kernel._block_items(csr, 2)
    p3 = kernel._block_items(csr, 3)
    assert len(p2) == len(p3) == 3 and p2[-1].suffix and not p3[-1].suffix
    assert _chains_kept(csr, p2) and _chains_kept(csr, p3)
    s2 = kernel._block_slots(csr, p2)
    s3 = kernel._block_slots(csr, p3)
    assert torch.equal(s2, torch.cat([it.pos.long() for it in p2]))
    assert torch.equal(s3, torch.cat([it.pos.long() for it in p3]))
    assert not torch.equal(s2, s3)
    emap = torch.randperm(csr.nnz)
    assert torch.equal(kernel._block_edge_rows(csr, p2, emap), emap[s2])
    assert torch.equal(kernel._block_edge_rows(csr, p3, emap), emap[s3])
    eid = csr.slot_eid if csr.slot_eid is not None else torch.arange(csr.nnz)
    assert torch.equal(kernel._block_edge_rows(csr, p2, None), eid[s2])
    assert torch.equal(kernel._block_edge_rows(csr, p3, None), eid[s3])


@pytest.mark.gpu
def test_one_csr_two_block_counts_device():
    """One CSR through the blocked u_mul_e at two widths whose plans are
    B = 2 + suffix and B = 3 (three launches each): both equal the oracle's
    chain bit for bit, in either order of first use."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, src, dst = _tagged_graph()
    gen = torch.Generator().manual_seed(22)
    w = torch.rand(len(src), 1, generator=gen)
    old = kernel.set_schedule_policy(block_table_min=0, block_min_slots=1)
    try:
        for widths in ((64, 96), (96, 64)):
            adj = kernel.from_coo(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                                  kernel.ORDER_EID, dev)
            for F in widths:
                # F = 64: 512 KB table -> 2 blocks; F = 96: 768 KB -> 3 blocks
                kernel.set_schedule_policy(block_bytes=256_000)
                H = torch.randn(n, F, generator=gen)
                plan = kernel._block_plan(adj.fwd, H.to(dev), F)
                assert plan is not None and len(plan) == 3
                assert plan[-1].suffix == (F == 64)
                out = kernel.gspmm(adj, "u_mul_e", "sum", H.to(dev), w.to(dev)).cpu()
                ref = O.spmm_coo(n, dst, src, H.numpy(), w.numpy().ravel())
                assert np.array_equal(out.numpy(), ref)
                out = kernel.gspmm(adj, "copy_u", "sum", H.to(dev)).cpu()
                assert np.array_equal(out.numpy(), O.spmm_coo(n, dst, src, H.numpy()))
    finally:
        kernel.set_schedule_policy(**old)


@pytest.mark.gpu
def test_readonly_random_order_graph_is_blocked_and_exact():
    """The edge-order precondition concerns mutable graphs only. A readonly
    graph's adjacency keeps its slots sorted by (dst, src), as the
    reference's ImmutableGraph CSR (immutable_graph.cc:206-237), so its
    chains run in source order and the source-blocked schedule applies to an
    edge list in random order: blocked launches, and the oracle's bits for
    that slot order (the in-edges of each row sorted by source, stable)."""
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    dev = torch.device("cuda", 0)
    n, m = 120_000, 12_000_000
    gen = torch.Generator().manual_seed(21)
    src = torch.randint(0, n, (m,), generator=gen)
    dst = torch.randint(0, n, (m,), generator=gen)
    h = torch.rand(n, 128, generator=gen) * 2 - 1
    out = {}
    for ro in (False, True):
        g = dgl.DGLGraph((src, dst), readonly=ro) if ro else dgl.DGLGraph((src, dst))
        g.ndata["h"] = h.to(dev)
        launches = kernel.blocked_schedule(g.sparse_adjacency(dev), g.ndata["h"])
        assert (launches > 1) == ro, (ro, launches)
        g.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
        out[ro] = g.ndata["o"].cpu().numpy()
    s_np, d_np = src.numpy(), dst.numpy()
    hn = h.numpy()
    # mutable: the edge-id chains; readonly: the (dst, src)-sorted chains
    ip, ix, pos = O.coo_to_csr(n, d_np, s_np)
    assert np.array_equal(out[False], O.spmm_csr(ip, ix, pos, hn, num_threads=16))
    order = np.lexsort((s_np, d_np))
    ip, ix, pos = O.coo_to_csr(n, d_np[order], s_np[order])
    assert np.array_equal(out[True], O.spmm_csr(ip, ix, pos, hn, num_threads=16))


def test_readonly_and_mutable_chain_orders_host():
    """The two slot orders on the host: a mutable graph's chains run in edge-id
    order (the reference's COO adjacency, graph.cc:509-524), a readonly
    graph's in (dst, src) order (ImmutableGraph's CSR,
    immutable_graph.cc:206-237); each equals the oracle over that order."""
    n, m = 3000, 300_000
    gen = torch.Generator().manual_seed(21)
    src = torch.randint(0, n, (m,), generator=gen)
    dst = torch.randint(0, n, (m,), generator=gen)
    h = torch.rand(n, 16, generator=gen) * 2 - 1
    s_np, d_np, hn = src.numpy(), dst.numpy(), h.numpy()
    for ro in (False, True):
        g = dgl.DGLGraph((src, dst), readonly=ro) if ro else dgl.DGLGraph((src, dst))
        g.ndata["h"] = h
        g.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
        order = np.lexsort((s_np, d_np)) if ro else np.arange(m)
        ip, ix, pos = O.coo_to_csr(n, d_np[order], s_np[order])
        assert np.array_equal(g.ndata["o"].numpy(), O.spmm_csr(ip, ix, pos, hn))
