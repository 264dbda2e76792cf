"""Column halves (gspmm_items_columns_kernel): the launches of
the pair kernel — the blocked schedule's items for copy_u over fp32 rows of
128 floats — with four items to a wave, one per 16-lane quarter, over one half
of the columns; a workgroup's half is its XCD label's low bit, so each L2
holds half of the source slice. The schedule policy's ``column_parts`` (2, or
1 for the pair kernel) selects it on top of ``items_per_wave`` = 2. Every
lane's chain is the one-item kernel's, so all three give the same bits. These
tests compare them — bit patterns, so NaN payloads and the sign of zero count
— and the oracle's chains on small graphs cut into source blocks of 128 rows:
groups of four items of equal and very unequal lengths, lengths around the
batch depth in every quarter, item counts that leave partial waves, partial
workgroups and block counts that are no multiple of 8, first, accumulating and
suffix launches, special values, the gate (unaligned views, strides, other
widths), the transposed backward and a pipelined partition's segments. Every
test asserts that the plan schedules the blocked path with more than one
launch.
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
DEPTH = 12        # gathers a wave has in flight per batch (launch_items_columns)
BLOCK_ROWS = 128  # source rows per block at F = 128 under small_blocks()

COLS = {"items_per_wave": 2, "column_parts": 2}   # the kernel under test
PAIR = {"items_per_wave": 2, "column_parts": 1}
ONE = {"items_per_wave": 1, "column_parts": 1}


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
        assert len({row for row, _ in items}) == len(items)
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


def _run(csr, u2, red, pol, init=None, out=None):
    """One product under the policy words ``pol``; ``init`` pre-fills out (the
    accumulating reducers continue from it, the others must overwrite it);
    ``out``: the tensor to run into, as it is."""
    if out is None:
        out = (torch.full((csr.num_rows, u2.shape[1]), float("nan"), device=u2.device)
               if init is None else init.clone())
    with kernel.scheduled(**pol):
        kernel._run_gspmm(csr, kernel.MSG_COPY_U, red, u2, None, 0, u2.shape[1], False, out=out)
    torch.cuda.synchronize()
    return out


def _three(csr, u2, red, init=None):
    """The product under the column halves, asserted bit-equal to the pair
    kernel's and the one-item kernel's; returns it."""
    cols = _run(csr, u2, red, COLS, init)
    assert _same_bits(cols, _run(csr, u2, red, ONE, init))
    assert _same_bits(cols, _run(csr, u2, red, PAIR, init))
    return cols


def _rows(n, feat, seed, dev):
    return (torch.rand(n, feat, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)


RED = {"sum": kernel.RED_SUM, "mean": kernel.RED_MEAN, "sum_accum": kernel.RED_SUM_ACCUM,
       "mean_add": kernel.RED_MEAN_ACCUM}


# ---------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------
def test_policy_roundtrips_column_parts_and_rejects_other_values():
    pol = kernel.schedule_policy()
    assert pol["column_parts"] in (1, 2)
    for v in (1, 2):
        with kernel.scheduled(column_parts=v):
            now = kernel.schedule_policy()
            assert now["column_parts"] == v
            # every other word keeps its value across the set / get
            assert {k: x for k, x in now.items() if k != "column_parts"} == \
                {k: x for k, x in pol.items() if k != "column_parts"}
            raw = kernel._Policy()
            _ffi.check_call(_ffi.LIB.dglhip_spmm_get_policy(ctypes.addressof(raw)))
            assert raw.column_parts == v and raw.items_per_wave == pol["items_per_wave"]
            assert raw.block_bytes == pol["block_bytes"]
            assert raw.pad_min_bytes == pol["pad_min_bytes"]
    assert kernel.schedule_policy() == pol
    for bad in (0, 3, 4, -1):
        with pytest.raises(kernel.DGLError):
            kernel.set_schedule_policy(column_parts=bad)
        assert kernel.schedule_policy() == pol
        # the launch entry checks its own argument, ahead of every pointer
        with pytest.raises(kernel.DGLError):
            _ffi.check_call(_ffi.LIB.dglhip_gspmm_items_columns_device(
                kernel.MSG_COPY_U, 0, F, None, None, 0, None, None, None, 0, 0, 2, bad, None, 0,
                None, None))
    for ipw in (1, 2):
        for parts in (1, 2):
            _ffi.check_call(_ffi.LIB.dglhip_gspmm_items_columns_device(
                kernel.MSG_COPY_U, 0, F, None, None, 0, None, None, None, 0, 0, ipw, parts, None,
                0, None, None))
    # the existing words are set and read back beside the new one
    with kernel.scheduled(column_parts=2, items_per_wave=1, block_bytes=1 << 20, pad_rows=0,
                          block_max_stretch=2.5, pad_min_bytes=12345):
        now = kernel.schedule_policy()
        assert (now["column_parts"], now["items_per_wave"], now["block_bytes"], now["pad_rows"],
                now["block_max_stretch"], now["pad_min_bytes"]) == (2, 1, 1 << 20, 0, 2.5, 12345)
    assert kernel.schedule_policy() == pol


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------
AROUND = [2 * DEPTH + 1, 2 * DEPTH, 2 * DEPTH - 1, DEPTH + 1, DEPTH, DEPTH - 1]

# block -> (row, slots). Items run longest first, four to a wave.
SHAPED = [
    [(1, 7), (3, 7), (5, 7), (7, 7)],                  # a group of equal lengths
    [(1, 128), (3, 40), (5, 3), (7, 1)],               # very unequal: 1 / 3 / 40 / 128
    # the lengths around the batch depth behind 0, 1, 2 and 3 longer items:
    # each of them in every quarter of its wave
    [(2 * i, n) for i, n in enumerate(AROUND)],
    [(0, 128)] + [(2 * i + 3, n) for i, n in enumerate(AROUND)],
    [(0, 128), (1, 128)] + [(2 * i + 2, n) for i, n in enumerate(AROUND)],
    [(0, 128), (1, 128), (2, 128)] + [(2 * i + 5, n) for i, n in enumerate(AROUND)],
    [(9, 2 * DEPTH), (1, DEPTH), (4, DEPTH), (6, DEPTH)],  # whole batches only
]
N = len(SHAPED) * BLOCK_ROWS


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
    # quarter (position % 4) of every length around the depth, over blocks 2-5
    seen = {n: set() for n in AROUND}
    for lengths in got[2:6]:
        for pos, n in enumerate(lengths):
            if n in seen:
                seen[n].add(pos % 4)
    assert all(q == {0, 1, 2, 3} for q in seen.values())


@pytest.mark.gpu
@pytest.mark.parametrize("red", sorted(RED))
def test_shaped_groups_same_bits(shaped, red):
    """Equal and very unequal groups, every length around the depth in every
    quarter, partial waves; rows absent from block 0 (zero-filled ahead of the
    first launch) and from middle blocks; first and accumulating launches."""
    dev = shaped["dev"]
    h = shaped["H"].to(dev)
    init = _rows(N, F, 3, dev) if red in ("sum_accum", "mean_add") else None
    with small_blocks():
        _launches(shaped["csr"], h, RED[red])
        cols = _three(shaped["csr"], h, RED[red], init)
    if red == "sum":
        assert np.array_equal(cols.cpu().numpy(), shaped["ref"])
        assert not bool(cols[20:].any())  # rows without slots: zero, not the NaN pre-fill
    if red == "sum_accum":
        assert _same_bits(cols[20:], init[20:])  # rows without slots keep the running value


COUNTS = [1, 2, 3, 5, 15, 16, 17, 33]  # items per launch: 2, 4 and 6 blocks of 16 items


@pytest.mark.gpu
def test_item_counts_partial_waves_and_block_counts():
    """Launches of 1 to 33 items: waves with one to three quarters off, a
    workgroup with waves off, and 2, 4 and 6 blocks (no multiple of 8)."""
    dev = _dev()
    rng = np.random.default_rng(20)
    blocks = []
    for b, c in enumerate(COUNTS):
        rows = rng.choice(40, size=c, replace=False)  # rows shared among launches
        blocks.append([(int(r), int(rng.integers(1, 31))) for r in rows])
    n = len(COUNTS) * BLOCK_ROWS
    src, dst = _graph_of_lengths(blocks, seed=21)
    csr = _csr(n, src, dst, dev)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(22)) * 2 - 1
    h = H.to(dev)
    init = _rows(n, F, 23, dev)
    with small_blocks():
        assert _launches(csr, h) == len(COUNTS)
        assert [len(x) for x in _item_lengths(csr, h)] == COUNTS
        cols = _three(csr, h, kernel.RED_SUM)
        _three(csr, h, kernel.RED_SUM_ACCUM, init)
    assert np.array_equal(cols.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))


@pytest.fixture(scope="module")
def hub_graph():
    dev = _dev()
    n = 2000
    src, dst = _random_graph(n, 60_000, 30, hub=17)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(4)) * 2 - 1
    return {"dev": dev, "n": n, "src": src, "dst": dst, "csr": _csr(n, src, dst, dev), "H": H,
            "ref": O.spmm_coo(n, dst, src, H.numpy())}


@pytest.mark.gpu
def test_column_parts_1_against_2_on_a_random_graph_with_a_hub_row(hub_graph):
    dev, n, csr = hub_graph["dev"], hub_graph["n"], hub_graph["csr"]
    h = hub_graph["H"].to(dev)
    init = _rows(n, F, 5, dev)
    with small_blocks():
        assert _launches(csr, h) >= 15
        lengths = _item_lengths(csr, h)
        assert all(x[0] >= 64 for x in lengths)  # the hub: a slot from every source
        for red in sorted(RED):
            start = init if red in ("sum_accum", "mean_add") else None
            cols = _three(csr, h, RED[red], start)
            if red == "sum":
                assert np.array_equal(cols.cpu().numpy(), hub_graph["ref"])


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
        cols = _three(csr, h, kernel.RED_SUM)
    assert np.array_equal(cols.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))


@pytest.mark.gpu
def test_special_values_and_switched_off_lanes():
    """Groups of short and long items over source rows of NaN, +-inf, -0.0 and
    denormals: a short item's quarter adds nothing while the longer items'
    slots run, so a row of -0.0 slots continued from -0.0 stays -0.0."""
    dev = _dev()
    blocks = [
        [(3, 40), (5, 1), (7, 25), (9, 12)],     # row 5: one slot, beside 40, 25 and 12
        [(3, 20), (5, 2), (7, 19)],              # row 5 again: accumulating, a quarter off
        [(5, 1), (9, 2 * DEPTH + 3), (11, 4), (13, 3), (15, 2)],
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
        assert _item_lengths(csr, h) == [[40, 25, 12, 1], [20, 19, 2],
                                         [2 * DEPTH + 3, 4, 3, 2, 1]]
        first = _three(csr, h, kernel.RED_SUM)
        cont = _three(csr, h, kernel.RED_SUM_ACCUM, init)
    for got in (first, cont):
        assert bool(torch.isnan(got).any()) and bool(torch.isinf(got).any())
    # the oracle's chains: NaN where it has NaN, its bits everywhere else
    ref, got = O.spmm_coo(n, dst, src, H), first.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.where(np.isnan(ref), 0, got.view(np.int32)),
                          np.where(np.isnan(ref), 0, ref.view(np.int32)))
    # continued from -0.0 over -0.0 slots only: -0.0 (a zero fed to the idle
    # lanes would have made it +0.0), in both column halves
    assert bool((_bits(cont[5]) == -2 ** 31).all())
    # from zero the same slots give +0.0, as in the one-item kernel
    assert bool((_bits(first[5]) == 0).all())


@pytest.mark.gpu
def test_gate_views_and_strides_give_the_same_bits():
    """Tables the column halves do not take (4 bytes past a 16-byte boundary,
    a row stride that is no multiple of 4 floats) and one they do (a stride of
    132 floats), and an out 4 bytes past: the same bits through whichever
    kernel the gate picks."""
    dev = _dev()
    n = 600
    src, dst = _random_graph(n, 30_000, 31)
    csr = _csr(n, src, dst, dev)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(11)) * 2 - 1
    ref = O.spmm_coo(n, dst, src, H.numpy())
    h = H.to(dev)
    off4 = torch.zeros(n * F + 1, device=dev)[1:].view(n, F)  # 4 bytes past
    off4.copy_(H)
    assert off4.data_ptr() % 16 == 4
    ld130 = torch.zeros(n, F + 2, device=dev)[:, :F]  # rows not 16-byte aligned
    ld130.copy_(H)
    ld132 = torch.zeros(n, F + 4, device=dev)[:, :F]  # 16-byte aligned rows, 528 bytes apart
    ld132.copy_(H)
    assert kernel._row_strided(ld130, F) and ld130.stride(0) % 4 != 0
    assert kernel._row_strided(ld132, F) and ld132.stride(0) == 132
    with small_blocks(pad_rows=0):
        for view in (off4, ld130, ld132):
            _launches(csr, view)
            cols = _three(csr, view, kernel.RED_SUM)
            assert np.array_equal(cols.cpu().numpy(), ref)
        _launches(csr, h)
        outs = []
        for pol in (COLS, PAIR, ONE):
            out4 = torch.full((n * F + 1,), float("nan"), device=dev)[1:].view(n, F)
            assert out4.data_ptr() % 16 == 4
            outs.append(_run(csr, h, kernel.RED_SUM, pol, out=out4))
        assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
        assert np.array_equal(outs[0].cpu().numpy(), ref)


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
        cols = _three(csr, h, kernel.RED_SUM)
    assert np.array_equal(cols.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))


@pytest.mark.gpu
def test_transposed_backward_same_gradients():
    dev = _dev()
    n = 600
    src, dst = _random_graph(n, 40_000, 51, hub=3)
    g = dgl.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)))
    gen = torch.Generator().manual_seed(13)
    H = torch.rand(n, F, generator=gen) * 2 - 1
    G = torch.rand(n, F, generator=gen) * 2 - 1

    def run(pol):
        with kernel.scheduled(**pol):
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
        oc, gc = run(COLS)
        o1, g1 = run(ONE)
    assert _same_bits(oc, o1) and _same_bits(gc, g1)
    assert np.array_equal(oc.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))
    assert np.array_equal(gc.cpu().numpy(), O.spmm_coo(n, src, dst, G.numpy()))


@pytest.mark.gpu
def test_pipelined_segments_with_the_column_halves():
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
        with kernel.scheduled(**COLS):
            cols = pg.update_all(h_local).clone()
        with kernel.scheduled(**PAIR):
            pair = pg.update_all(h_local).clone()
        with kernel.scheduled(**ONE):
            one = pg.update_all(h_local).clone()
        old = kernel.set_blocked("off")
        try:
            flat = pg.update_all(h_local).clone()
        finally:
            kernel.set_blocked(old)
    assert _same_bits(cols, one) and _same_bits(cols, pair) and _same_bits(cols, flat)
