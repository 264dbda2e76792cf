"""Two items per wave (gspmm_items_pair_kernel): the blocked
schedule's launches for copy_u over fp32 rows of 128 floats, lanes 0-31 on
one item and lanes 32-63 on the next, 16 bytes per lane. The schedule policy's
``items_per_wave`` (2, or 1 for the one-item kernel) selects it; every lane's
chain is the one-item kernel's, so the two give the same bits. These tests
compare them — bit patterns, so NaN payloads and the sign of zero count —
on small graphs cut into source blocks of 128 rows: item pairs of equal and
very unequal lengths, lengths around the batch depth, odd item counts, first
and accumulating launches, the suffix launch, special values, the gate
(unaligned views, other widths), the transposed backward and a pipelined
partition's segments. Every test asserts that the plan schedules the blocked
path with more than one launch.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import _ffi, kernel
from oracle import oracle as O

F = 128
DEPTH = 10       # gathers a wave has in flight per batch (launch_items_pair)
BLOCK_ROWS = 128  # source rows per block at F = 128 under small_blocks()


@contextlib.contextmanager
def small_blocks(**more):
    with kernel.scheduled(block_table_min=0, block_bytes=BLOCK_ROWS * F * 4, block_min_slots=1,
                          **more):
        yield


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _random_graph(n, m, seed, hub=None):
    """Source-major random edges; ``hub``: a row with an edge from every source."""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    if hub is not None:
        src = np.concatenate([src, np.arange(n)])
        dst = np.concatenate([dst, np.full(n, hub)])
    o = np.lexsort((dst, src))
    return src[o].astype(np.int64), dst[o].astype(np.int64)


def _graph_of_lengths(blocks, seed=0):
    """Edges such that block b's launch has exactly the items ``blocks[b]``: a
    list of (row, slots), the slots' sources drawn from block b's rows without
    repetition. Source-major, so every row's blocks never decrease. The first
    and the last source row are referenced, so the plan's even cut of the
    referenced column range is these blocks."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for b, items in enumerate(blocks):
        for i, (row, length) in enumerate(items):
            assert 0 < length <= BLOCK_ROWS
            s = np.sort(rng.choice(BLOCK_ROWS, size=length, replace=False)) + b * BLOCK_ROWS
            if i == 0 and b == 0:
                s[0] = 0
            if i == 0 and b == len(blocks) - 1:
                s[-1] = len(blocks) * BLOCK_ROWS - 1
            src.append(s)
            dst.append(np.full(length, row))
    src, dst = np.concatenate(src), np.concatenate(dst)
    o = np.lexsort((dst, src))
    return src[o].astype(np.int64), dst[o].astype(np.int64)


def _csr(n, src, dst, dev, cols=None):
    return kernel.build_csr(n, cols or n, torch.from_numpy(dst), torch.from_numpy(src),
                            kernel.ORDER_EID, dev)


def _launches(csr, u2, red=kernel.RED_SUM):
    """Launches of the blocked path this product takes (asserted blocked, > 1)."""
    feat = u2.shape[1]
    ldu = u2.stride(0) if kernel._row_strided(u2, feat) else 0
    path, launches = csr.plan.schedule(kernel.MSG_COPY_U, red, feat, ldu, u2.shape[0])
    assert path == kernel.PLAN_PATH_BLOCKED and launches > 1
    return launches


def _item_lengths(csr, u2):
    plan = kernel._block_plan(csr, u2, u2.shape[1])
    assert plan is not None
    return [(it.ptr[1:] - it.ptr[:-1]).tolist() for it in plan]


def _run(csr, u2, red, ipw, init=None):
    """One product under items_per_wave = ipw; ``init`` pre-fills out (the
    accumulating reducers continue from it, the others must overwrite it)."""
    out = (torch.full((csr.num_rows, u2.shape[1]), float("nan"), device=u2.device)
           if init is None else init.clone())
    with kernel.scheduled(items_per_wave=ipw):
        kernel._run_gspmm(csr, kernel.MSG_COPY_U, red, u2, None, 0, u2.shape[1], False, out=out)
    torch.cuda.synchronize()
    return out


def _rows(n, feat, seed, dev):
    return (torch.rand(n, feat, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)


# ---------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------
def test_policy_roundtrips_items_per_wave_and_rejects_other_values():
    pol = kernel.schedule_policy()
    assert pol["items_per_wave"] in (1, 2)
    for v in (1, 2):
        with kernel.scheduled(items_per_wave=v):
            assert kernel.schedule_policy()["items_per_wave"] == v
            raw = kernel._Policy()
            _ffi.check_call(_ffi.LIB.dglhip_spmm_get_policy(ctypes.addressof(raw)))
            assert raw.items_per_wave == v
    assert kernel.schedule_policy() == pol
    for bad in (0, 3, -1):
        with pytest.raises(kernel.DGLError):
            kernel.set_schedule_policy(items_per_wave=bad)
        assert kernel.schedule_policy() == pol
        # the launch entry checks its own argument, ahead of every pointer
        with pytest.raises(kernel.DGLError):
            _ffi.check_call(_ffi.LIB.dglhip_gspmm_items_table_device(
                kernel.MSG_COPY_U, 0, F, None, None, 0, None, None, None, 0, 0, bad, None, 0,
                None, None))
    _ffi.check_call(_ffi.LIB.dglhip_gspmm_items_table_device(
        kernel.MSG_COPY_U, 0, F, None, None, 0, None, None, None, 0, 0, 2, None, 0, None, None))


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------
N = 640  # 5 source blocks of 128 rows

# block -> (row, slots); rows 16.. are in no block at all
SHAPED = [
    [(3, 40), (5, 1)],                                          # 1 against 40: five batches apart
    [(3, DEPTH - 1), (5, DEPTH), (7, DEPTH + 1), (9, 2 * DEPTH + 1)],   # around the batch depth
    [(11, 5)],                                                  # a launch of exactly one item
    [(3, 9), (7, 9), (13, 3)],                                  # odd item count
    [(3, 33), (5, 2), (9, 2), (11, 1), (15, 1)],
]


@pytest.fixture(scope="module")
def shaped():
    dev = _dev()
    src, dst = _graph_of_lengths(SHAPED, seed=1)
    H = torch.rand(N, F, generator=torch.Generator().manual_seed(2)) * 2 - 1
    return {"dev": dev, "src": src, "dst": dst, "csr": _csr(N, src, dst, dev), "H": H,
            "ref": O.spmm_coo(N, dst, src, H.numpy())}


@pytest.mark.gpu
def test_shaped_launches_have_the_intended_items(shaped):
    with small_blocks():
        h = shaped["H"].to(shaped["dev"])
        assert _launches(shaped["csr"], h) == len(SHAPED)
        got = _item_lengths(shaped["csr"], h)
    assert got == [sorted((n for _, n in items), reverse=True) for items in SHAPED]
    assert [len(x) % 2 for x in got] == [0, 0, 1, 1, 1] and len(got[2]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("red", ["sum", "mean", "sum_accum", "mean_add"])
def test_shaped_pairs_same_bits(shaped, red):
    """Unequal pairs, lengths at D - 1, D, D + 1 and 2D + 1, odd counts and a
    one-item launch; rows absent from block 0 (zero-filled ahead of the first
    launch) and from middle blocks; first and accumulating launches."""
    dev = shaped["dev"]
    code = {"sum": kernel.RED_SUM, "mean": kernel.RED_MEAN, "sum_accum": kernel.RED_SUM_ACCUM,
            "mean_add": kernel.RED_MEAN_ACCUM}[red]
    h = shaped["H"].to(dev)
    init = _rows(N, F, 3, dev) if red in ("sum_accum", "mean_add") else None
    with small_blocks():
        _launches(shaped["csr"], h, code)
        two = _run(shaped["csr"], h, code, 2, init)
        one = _run(shaped["csr"], h, code, 1, init)
    assert _same_bits(two, one)
    if red == "sum":
        assert np.array_equal(two.cpu().numpy(), shaped["ref"])
        assert not bool(two[16:].any())  # rows without slots: zero, not the pre-fill


@pytest.mark.gpu
@pytest.mark.parametrize("m", [20_000, 60_000])
def test_random_graph_with_a_hub_row(m):
    dev = _dev()
    n = 600
    src, dst = _random_graph(n, m, 10 + m, hub=17)
    csr = _csr(n, src, dst, dev)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(4)) * 2 - 1
    h = H.to(dev)
    init = _rows(n, F, 5, dev)
    with small_blocks():
        assert _launches(csr, h) >= 3
        lengths = _item_lengths(csr, h)
        assert all(x[0] >= 100 for x in lengths)  # the hub: a slot from every source
        for code, start in ((kernel.RED_SUM, None), (kernel.RED_MEAN, None),
                            (kernel.RED_SUM_ACCUM, init), (kernel.RED_MEAN_ACCUM, init)):
            two, one = _run(csr, h, code, 2, start), _run(csr, h, code, 1, start)
            assert _same_bits(two, one)
            if code == kernel.RED_SUM:
                assert np.array_equal(two.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))


@pytest.mark.gpu
def test_suffix_launch_after_self_loops():
    dev = _dev()
    n = 600
    src, dst = _random_graph(n, 30_000, 21)
    src, dst = np.concatenate([src, np.arange(n)]), np.concatenate([dst, np.arange(n)])
    csr = _csr(n, src, dst, dev)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(6)) * 2 - 1
    h = H.to(dev)
    with small_blocks():
        _launches(csr, h)
        plan = kernel._block_plan(csr, h, F)
        assert plan[-1].suffix and plan[-1].nnz > 0
        two, one = _run(csr, h, kernel.RED_SUM, 2), _run(csr, h, kernel.RED_SUM, 1)
    assert _same_bits(two, one)
    assert np.array_equal(two.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))


@pytest.mark.gpu
def test_special_values_and_switched_off_lanes():
    """Pairs of a short and a long item over source rows of NaN, +-inf, -0.0
    and denormals: the short half's lanes add nothing while the long item's
    slots run, so a row of -0.0 slots continued from -0.0 stays -0.0."""
    dev = _dev()
    blocks = [
        [(3, 40), (5, 1)],             # row 5: one slot, beside 40
        [(3, 20), (5, 2), (7, 19)],    # row 5 again: accumulating, beside 20 and 19
        [(5, 1), (9, 2 * DEPTH + 3)],
    ]
    n = 3 * BLOCK_ROWS
    src, dst = _graph_of_lengths(blocks, seed=7)
    csr = _csr(n, src, dst, dev)
    rng = np.random.default_rng(8)
    H = (rng.random((n, F), dtype=np.float32) * 2 - 1)
    H[rng.choice(n, 24, replace=False)] = np.float32(1e-41)       # denormal rows
    H[rng.choice(n, 12, replace=False), ::3] = np.float32("inf")
    H[rng.choice(n, 12, replace=False), 1::3] = np.float32("-inf")
    H[rng.choice(n, 12, replace=False), 2::5] = np.float32("nan")
    H[src[dst == 5]] = np.float32(-0.0)  # every source of row 5
    h = torch.from_numpy(H).to(dev)
    init = _rows(n, F, 9, dev)
    init[5] = -0.0
    with small_blocks():
        _launches(csr, h)
        assert _item_lengths(csr, h) == [[40, 1], [20, 19, 2], [2 * DEPTH + 3, 1]]
        for code, start in ((kernel.RED_SUM, None), (kernel.RED_SUM_ACCUM, init)):
            two, one = _run(csr, h, code, 2, start), _run(csr, h, code, 1, start)
            assert _same_bits(two, one)
            assert bool(torch.isnan(two).any()) and bool(torch.isinf(two).any())
    # continued from -0.0 over -0.0 slots only: -0.0 (a zero fed to the idle
    # lanes would have made it +0.0)
    assert bool((_bits(two[5]) == -2 ** 31).all())
    # from zero the same slots give +0.0, as in the one-item kernel
    with small_blocks():
        first = _run(csr, h, kernel.RED_SUM, 2)
    assert bool((_bits(first[5]) == 0).all())


@pytest.mark.gpu
def test_gate_unaligned_views_keep_the_one_item_kernel_bits():
    dev = _dev()
    n = 600
    src, dst = _random_graph(n, 30_000, 31)
    csr = _csr(n, src, dst, dev)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(11)) * 2 - 1
    ref = O.spmm_coo(n, dst, src, H.numpy())
    flat = torch.zeros(n * F + 2, device=dev)
    off8 = flat[2:].view(n, F)       # 8 bytes past a 16-byte boundary
    off8.copy_(H)
    assert off8.data_ptr() % 16 == 8
    padded = torch.zeros(n, F + 2, device=dev)[:, :F]  # stride 130: rows not 16-byte aligned
    padded.copy_(H)
    assert kernel._row_strided(padded, F) and padded.stride(0) % 4 != 0
    with small_blocks(pad_rows=0):
        for view in (off8, padded):
            _launches(csr, view)
            two, one = _run(csr, view, kernel.RED_SUM, 2), _run(csr, view, kernel.RED_SUM, 1)
            assert _same_bits(two, one)
            assert np.array_equal(two.cpu().numpy(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("feat", [64, 256])
def test_gate_other_widths_unchanged(feat):
    dev = _dev()
    n = 600
    src, dst = _random_graph(n, 30_000, 41)
    csr = _csr(n, src, dst, dev)
    H = torch.rand(n, feat, generator=torch.Generator().manual_seed(12)) * 2 - 1
    h = H.to(dev)
    with kernel.scheduled(block_table_min=0, block_bytes=BLOCK_ROWS * feat * 4,
                          block_min_slots=1, block_min_row_bytes=0):
        _launches(csr, h)
        two, one = _run(csr, h, kernel.RED_SUM, 2), _run(csr, h, kernel.RED_SUM, 1)
    assert _same_bits(two, one)
    assert np.array_equal(two.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))


@pytest.mark.gpu
def test_transposed_backward_same_gradients():
    dev = _dev()
    n = 600
    src, dst = _random_graph(n, 40_000, 51, hub=3)
    g = dgl.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)))
    gen = torch.Generator().manual_seed(13)
    H = torch.rand(n, F, generator=gen) * 2 - 1
    G = torch.rand(n, F, generator=gen) * 2 - 1

    def run(ipw):
        with kernel.scheduled(items_per_wave=ipw):
            h = H.to(dev).requires_grad_(True)
            g.ndata["h"] = h
            kernel.timing_enable(True)
            g.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
            g.ndata["o"].backward(G.to(dev))
            torch.cuda.synchronize()
            _, launches = kernel.timing_read()
            kernel.timing_enable(False)
            # the backward ran blocked launches of its own
            assert launches > _launches(g.sparse_adjacency(dev).fwd, h.detach()) + 1
            return g.ndata["o"].detach(), h.grad
    with small_blocks():
        o2, g2 = run(2)
        o1, g1 = run(1)
    assert _same_bits(o2, o1) and _same_bits(g2, g1)
    assert np.array_equal(g2.cpu().numpy(), O.spmm_coo(n, src, dst, G.numpy()))


@pytest.mark.gpu
def test_pipelined_segments_with_the_pair_kernel():
    """An emulated rank of a 2-rank partition: own rows, then each halo chunk
    continued with SUM_ACCUM, every segment blocked over its column span."""
    dev = _dev()
    from dgl.distributed import PartitionedGraph, balanced_bounds
    n, W = 2400, 2
    src, dst = _random_graph(n, 120_000, 61)
    src, dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    bounds = balanced_bounds(torch.bincount(dst, minlength=n), W)
    lo, hi = int(bounds[0]), int(bounds[1])
    sel = (dst >= lo) & (dst < hi)
    with small_blocks():
        pg = PartitionedGraph(n, src[sel], dst[sel], bounds, dev, pipeline_chunks=2, rank=0,
                              world=W, halo="allgather")
        h_local = _rows(hi - lo, F, 14, dev)
        pg.update_all(h_local)  # lands the emulated halo rows
        for csr in pg.seg_csrs:
            path, launches = csr.plan.schedule(kernel.MSG_COPY_U, kernel.RED_SUM_ACCUM, F, 0,
                                               csr.num_cols)
            assert path == kernel.PLAN_PATH_BLOCKED and launches > 1
        with kernel.scheduled(items_per_wave=2):
            two = pg.update_all(h_local).clone()
        with kernel.scheduled(items_per_wave=1):
            one = pg.update_all(h_local).clone()
        old = kernel.set_blocked("off")
        try:
            flat = pg.update_all(h_local).clone()
        finally:
            kernel.set_blocked(old)
    assert _same_bits(two, one) and _same_bits(two, flat)
