"""The id path of the column halves (gspmm_items_columns_kernel, DESIGN.md
§4.1 "Column halves"): a wave whose four items have at most
``dglhip_gspmm_items_columns_ids_cap()`` slots together reads its column ids
once, coalesced, keeps the rows' byte offsets in its own region of LDS and
feeds every batch from there; a wave above the cap loads its ids batch by
batch. Every lane's chain is the one-item kernel's either way, so
``column_parts`` 2, 1 and the one-item kernel give the same bits. These tests
compare them, bit patterns, on tiny graphs built from prescribed item lengths
per source block, at the smallest shapes at which the path can go wrong: wave
totals at the cap and one to either side of it with preloaded and other waves
in one workgroup, totals around the loader's 64-slot loads, lengths around the
batch depth and one long item beside three of one slot, last waves with one to
three live items, first and accumulating launches, and special values in rows
that only a switched-off lane's neighbours gather.
"""
import contextlib

import numpy as np
import pytest
import torch

from dgl import _ffi, kernel
from oracle import oracle as O

F = 128
DEPTH = 12  # gathers a wave has in flight per batch (launch_items_columns)

COLS = {"items_per_wave": 2, "column_parts": 2}   # the kernel under test
PAIR = {"items_per_wave": 2, "column_parts": 1}
ONE = {"items_per_wave": 1, "column_parts": 1}
RED = {"sum": kernel.RED_SUM, "mean": kernel.RED_MEAN, "sum_accum": kernel.RED_SUM_ACCUM}


def _cap():
    return int(_ffi.LIB.dglhip_gspmm_items_columns_ids_cap())


def _block_rows():
    """Source rows per block: an item's slots are distinct sources of one
    block, and the longest item here is a quarter of the cap plus 60."""
    return _cap() // 4 + 64


@contextlib.contextmanager
def small_blocks():
    with kernel.scheduled(block_table_min=0, block_bytes=_block_rows() * F * 4,
                          block_min_slots=1):
        yield


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _graph_of_lengths(blocks, seed):
    """Edges such that block b's launch has exactly the items ``blocks[b]``: a
    list of (row, slots), the slots' sources drawn from block b's rows without
    repetition. Source-major. The first and the last source row are
    referenced, so the plan's even cut of the referenced column range is these
    blocks."""
    rows = _block_rows()
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for b, items in enumerate(blocks):
        assert len({row for row, _ in items}) == len(items)
        for i, (row, length) in enumerate(items):
            assert 0 < length <= rows and 0 <= row < len(blocks) * rows
            s = np.sort(rng.choice(rows, size=length, replace=False)) + b * rows
            if i == 0 and b == 0:
                s[0] = 0
            if i == 0 and b == len(blocks) - 1:
                s[-1] = len(blocks) * rows - 1
            src.append(s)
            dst.append(np.full(length, row))
    src, dst = np.concatenate(src), np.concatenate(dst)
    o = np.lexsort((dst, src))
    return src[o].astype(np.int64), dst[o].astype(np.int64)


def _items(lengths, first_row=0, step=1):
    """(row, slots) for the lengths, rows first_row, first_row + step, ..."""
    return [(first_row + step * i, n) for i, n in enumerate(lengths)]


def _csr(n, src, dst, dev):
    return kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                            kernel.ORDER_EID, dev)


def _item_lengths(csr, h, launches):
    """Item lengths per launch of the blocked path (asserted taken)."""
    path, got = csr.plan.schedule(kernel.MSG_COPY_U, kernel.RED_SUM, F, 0, h.shape[0])
    assert path == kernel.PLAN_PATH_BLOCKED and got == launches
    plan = kernel._block_plan(csr, h, F)
    assert plan is not None
    return [(it.ptr[1:] - it.ptr[:-1]).tolist() for it in plan]


def _wave_totals(lengths):
    return [sum(lengths[i:i + 4]) for i in range(0, len(lengths), 4)]


def _run(csr, h, red, pol, init):
    out = (torch.full((csr.num_rows, F), float("nan"), device=h.device)
           if init is None else init.clone())
    with kernel.scheduled(**pol):
        kernel._run_gspmm(csr, kernel.MSG_COPY_U, red, h, None, 0, F, False, out=out)
    torch.cuda.synchronize()
    return out


def _three(csr, h, red, init=None):
    """The product under the column halves, asserted bit-equal to the pair
    kernel's and the one-item kernel's; returns it."""
    cols = _run(csr, h, red, COLS, init)
    assert _same_bits(cols, _run(csr, h, red, ONE, init))
    assert _same_bits(cols, _run(csr, h, red, PAIR, init))
    return cols


def _rows(n, seed, dev):
    return (torch.rand(n, F, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)


def _check_all(blocks, seed, want_totals=None):
    """The three reducers over the graph of ``blocks``, three kernels each,
    sum against the oracle. Returns the item lengths per launch."""
    dev = _dev()
    n = len(blocks) * _block_rows()
    src, dst = _graph_of_lengths(blocks, seed)
    csr = _csr(n, src, dst, dev)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1
    h = H.to(dev)
    init = _rows(n, seed + 2, dev)
    with small_blocks():
        got = _item_lengths(csr, h, len(blocks))
        assert got == [sorted((m for _, m in items), reverse=True) for items in blocks]
        if want_totals is not None:
            for lengths, want in zip(got, want_totals):
                assert _wave_totals(lengths) == want
        for red in sorted(RED):
            cols = _three(csr, h, RED[red], init if red == "sum_accum" else None)
            if red == "sum":
                assert np.array_equal(cols.cpu().numpy(), O.spmm_coo(n, dst, src, H.numpy()))
    return got


# ---------------------------------------------------------------------------
# host
# ---------------------------------------------------------------------------
def test_ids_cap_is_exported_and_fits_eight_workgroups():
    cap = _cap()
    # a quarter's share is whole, and a full batch of every quarter fits
    assert cap % 4 == 0 and cap >= 4 * DEPTH
    # four waves' regions of 32-bit offsets, eight workgroups in a CU's 160 KiB
    assert 8 * 4 * cap * 4 <= 160 * 1024
    assert 4 * cap * 4 <= 20 * 1024


# ---------------------------------------------------------------------------
# device
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_wave_totals_at_the_cap():
    """Waves of cap + 240 (several batches without the preload), cap + 1, cap
    and cap - 1 slots in one workgroup, in the first and in two accumulating
    launches."""
    c4 = _cap() // 4
    lengths = [c4 + 60] * 4 + [c4 + 1] + [c4] * 10 + [c4 - 1]
    totals = [4 * c4 + 240, 4 * c4 + 1, 4 * c4, 4 * c4 - 1]
    blocks = [_items(lengths, first_row=b, step=3) for b in range(3)]
    _check_all(blocks, 100, [totals] * 3)


@pytest.mark.gpu
def test_wave_totals_around_the_loader_loads():
    """Wave totals of 129, 128, 127, 65, 64, 63 and 1 slots (a load is 64
    slots, a group of loads 256), and of 257, 256, 255: every wave but the
    first of a launch starts at a slot that is no multiple of 32."""
    a = [33] + [32] * 10 + [31] + [17] + [16] * 10 + [15] + [1]
    ta = [129, 128, 127, 65, 64, 63, 1]
    b = [65] + [64] * 10 + [63] + [20, 3]
    tb = [257, 256, 255, 23]
    blocks = [_items(a, 0, 2), _items(b, 1, 2), _items(a, 3, 1), _items(b, 0, 3)]
    _check_all(blocks, 200, [ta, tb, ta, tb])


AROUND = [2 * DEPTH + 1, 2 * DEPTH, 2 * DEPTH - 1, DEPTH + 1, DEPTH, DEPTH - 1]


@pytest.mark.gpu
def test_predication_around_the_depth_and_beside_a_long_item():
    """One long item beside three of one slot, and the lengths around the batch
    depth behind 0 to 3 longer items: each of them in every quarter of its
    wave, every boundary between the full and the predicated loop."""
    blocks = [
        _items([200, 1, 1, 1], 1, 2),
        _items(AROUND, 0, 2),
        _items([100] + AROUND, 1, 2),
        _items([100, 100] + AROUND, 0, 2),
        _items([100, 100, 100] + AROUND, 1, 2),
        _items([2 * DEPTH, DEPTH, DEPTH, DEPTH], 0, 3),   # whole batches only
        _items([200, 1, 1, 1], 0, 2),
    ]
    got = _check_all(blocks, 300)
    seen = {m: set() for m in AROUND}
    for lengths in got[1:5]:
        for pos, m in enumerate(lengths):
            if m in seen:
                seen[m].add(pos % 4)
    assert all(q == {0, 1, 2, 3} for q in seen.values())


COUNTS = [1, 2, 3, 4, 5, 6, 7, 16, 17]  # items per launch


@pytest.mark.gpu
def test_item_counts_and_partial_last_waves():
    """Launches whose last wave has 1, 2, 3 and 4 live items, in one and in
    two workgroup pairs (16 and 17 items)."""
    rng = np.random.default_rng(400)
    blocks = []
    for c in COUNTS:
        rows = rng.choice(40, size=c, replace=False)  # rows shared among launches
        blocks.append([(int(r), int(rng.integers(1, 31))) for r in rows])
    got = _check_all(blocks, 401)
    assert [len(x) for x in got] == COUNTS


@pytest.mark.gpu
def test_special_values_only_the_neighbours_gather():
    """NaN, +-inf and -0.0 in source rows that only the long items of a wave
    gather: the short items beside them, whose lanes are switched off while
    those slots run, stay finite and keep the one-item kernel's bits, and a row
    of -0.0 slots continued from -0.0 stays -0.0 (a switched-off lane adds
    nothing, not even a zero)."""
    dev = _dev()
    long_rows, short_rows = (3, 7), (5, 9)
    blocks = [
        [(3, 40), (5, 1), (7, 25), (9, 12)],
        [(3, 20), (5, 2), (7, 19)],                      # accumulating, a quarter off
        [(5, 1), (9, 3), (3, 2 * DEPTH + 3), (7, 4), (11, 2)],
    ]
    n = len(blocks) * _block_rows()
    src, dst = _graph_of_lengths(blocks, 500)
    csr = _csr(n, src, dst, dev)
    rng = np.random.default_rng(501)
    H = rng.random((n, F), dtype=np.float32) * 2 - 1
    H[src[dst == 5]] = np.float32(-0.0)                  # every source of row 5
    only_long = np.setdiff1d(src[np.isin(dst, long_rows)],
                             src[np.isin(dst, short_rows + (11,))])
    assert len(only_long) >= 40
    special = [np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(-0.0)]
    for i, s in enumerate(only_long):
        H[s, i % 3::3] = special[i % 4]
    h = torch.from_numpy(H).to(dev)
    init = _rows(n, 502, dev)
    init[5] = -0.0
    with small_blocks():
        assert _item_lengths(csr, h, 3) == [[40, 25, 12, 1], [20, 19, 2],
                                            [2 * DEPTH + 3, 4, 3, 2, 1]]
        first = _three(csr, h, kernel.RED_SUM)
        cont = _three(csr, h, kernel.RED_SUM_ACCUM, init)
        _three(csr, h, kernel.RED_MEAN)
    for got in (first, cont):
        assert bool(torch.isnan(got[list(long_rows)]).any())
        assert bool(torch.isfinite(got[list(short_rows)]).all())
    # the oracle's chains: NaN where it has NaN, its bits everywhere else
    ref, got = O.spmm_coo(n, dst, src, H), first.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.where(np.isnan(ref), 0, got.view(np.int32)),
                          np.where(np.isnan(ref), 0, ref.view(np.int32)))
    assert bool((_bits(cont[5]) == -2 ** 31).all())      # -0.0 kept
    assert bool((_bits(first[5]) == 0).all())            # from zero: +0.0
