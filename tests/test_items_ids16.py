"""The column halves over 16-bit block-local ids (gspmm_items_columns_kernel's
IDS16 instantiation, DESIGN.md §4.1 "Column halves", slice-local ids): the
launch's slots hold uint16 ids local to its source block, the kernel's table
is the block alone, and every lane reads the same slots and adds in the same
order as over int32 ids, so the bits are the same.

Kernel entry (dglhip_gspmm_items_ids16_device) against the int32 entry over
col_lo + id, item arrays built by hand at the smallest shapes at which the id
path can go wrong: wave totals at the LDS cap and to either side of it, totals
around the loader's 64- and 256-slot loads, item lengths around the batch
depth, partial last waves, an odd first slot (ids 2-byte aligned only), col_lo
> 0 with local ids 0 and block_rows - 1, first and accumulating launches, and
special values in rows that only a switched-off lane's neighbours gather. Every
row of the table outside the block is NaN, so a gather one row off either end
shows. Then through the plan (policy word ids_wide 0 against 1 and the oracle,
device-built ids against host-built ones) and a table just past 4 GiB whose
block qualifies where the table does not.
"""
import ctypes

import numpy as np
import pytest
import torch

from dgl import kernel
from dgl._ffi import LIB, check_call, ptr, stream_of
from oracle import oracle as O

F = 128
DEPTH = 12  # gathers a wave has in flight per batch (launch_items_columns)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda", 0)


def _cap():
    return int(LIB.dglhip_gspmm_items_columns_ids_cap())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _u16(a, dev):
    """uint16 values as a device tensor of the same bits."""
    return torch.from_numpy(np.asarray(a, dtype=np.uint16).view(np.int16).copy()).to(dev)


class Launch(object):
    """One launch's arrays: items of the given lengths into distinct rows,
    their slots at plan offset ``off0`` on, local ids in [0, block_rows)."""

    def __init__(self, lengths, off0, col_lo, block_rows, out_rows, seed, local=None):
        rng = np.random.default_rng(seed)
        n = len(lengths)
        self.n, self.col_lo, self.block_rows, self.out_rows = n, col_lo, block_rows, out_rows
        self.rows = rng.choice(out_rows, size=n, replace=False).astype(np.int32)
        self.ptr = (off0 + np.concatenate([[0], np.cumsum(lengths)])).astype(np.int64)
        total = int(self.ptr[-1])
        loc = rng.integers(0, block_rows, total)
        if local is not None:
            loc[off0:] = local
        # both ends of the block are gathered
        loc[off0], loc[total - 1] = 0, block_rows - 1
        self.local = loc


def _table(urows, col_lo, block_rows, seed):
    """Random rows in the block, NaN everywhere else."""
    H = np.full((urows, F), np.nan, dtype=np.float32)
    rng = np.random.default_rng(seed)
    H[col_lo:col_lo + block_rows] = rng.random((block_rows, F), dtype=np.float32) * 2 - 1
    return H


def _run_ids16(L, h, init, accum):
    dev = h.device
    out = init.clone()
    rows, p = torch.from_numpy(L.rows).to(dev), torch.from_numpy(L.ptr).to(dev)
    ids = _u16(L.local, dev)
    check_call(LIB.dglhip_gspmm_items_ids16_device(
        L.n, ptr(rows), ptr(p), int(accum), ptr(ids), L.col_lo, L.block_rows, ptr(h), 0,
        h.shape[0], ptr(out), out.shape[0], stream_of(dev)))
    torch.cuda.synchronize()
    return out


def _run_int32(L, h, init, accum, parts=1):
    """The int32 entry over col_lo + id (the pair kernel: the entry does not
    know out's rows)."""
    dev = h.device
    out = init.clone()
    rows, p = torch.from_numpy(L.rows).to(dev), torch.from_numpy(L.ptr).to(dev)
    ind = torch.from_numpy((L.local + L.col_lo).astype(np.int32)).to(dev)
    check_call(LIB.dglhip_gspmm_items_columns_device(
        kernel.MSG_COPY_U, L.n, F, ptr(rows), ptr(p), int(accum), ptr(ind), None, ptr(h), 0,
        h.shape[0], 2, parts, None, 0, ptr(out), stream_of(dev)))
    torch.cuda.synchronize()
    return out


def _compare(L, H, accum, seed=9, finite=True):
    dev = _dev()
    h = torch.from_numpy(H).to(dev)
    init = (torch.rand(L.out_rows, F, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)
    got = _run_ids16(L, h, init, accum)
    want = _run_int32(L, h, init, accum)
    touched = torch.from_numpy(L.rows.astype(np.int64)).to(dev)
    if finite:
        assert bool(torch.isfinite(got[touched]).all())   # no row outside the block gathered
        assert torch.equal(got, want)
    assert torch.equal(_bits(got), _bits(want))           # signed zeros, NaN payloads
    # the chain itself, in float64-free terms: slot order from zero / from out
    if finite:
        i = 0
        r, b, e = int(L.rows[i]), int(L.ptr[i]), int(L.ptr[i + 1])
        acc = init[r].clone() if accum else torch.zeros(F, device=dev)
        for s in range(b, e):
            acc = acc + h[L.col_lo + int(L.local[s])]
        assert torch.equal(got[r], acc)
    # rows of out no item names keep their values
    rest = torch.ones(L.out_rows, dtype=torch.bool, device=dev)
    rest[touched] = False
    assert torch.equal(_bits(got[rest]), _bits(init[rest]))
    return got


def _cases():
    c4 = _cap() // 4
    a = [33] + [32] * 10 + [31] + [17] + [16] * 10 + [15] + [1]      # 129 128 127 65 64 63 1
    b = [65] + [64] * 10 + [63] + [20, 3]                            # 257 256 255 23
    around = [25, 24, 13, 12, 11]
    return {
        # wave totals cap + 240, cap + 1, cap, cap - 1 in one workgroup
        "cap": [c4 + 60] * 4 + [c4 + 1] + [c4] * 10 + [c4 - 1],
        "loads64": a,
        "loads256": b,
        # lengths around the depth behind 0..3 longer items: every quarter
        "depth0": around,
        "depth1": [100] + around,
        "depth2": [100, 100] + around,
        "depth3": [100, 100, 100] + around,
        "beside_long": [200, 1, 1, 1],
        # partial last waves: 1, 2, 3 live items; 17 items: two workgroup pairs
        "count1": [7],
        "count2": [30, 2],
        "count3": [5, 5, 29],
        "count17": list(range(40, 23, -1)),
    }


CASE_NAMES = ["cap", "loads64", "loads256", "depth0", "depth1", "depth2", "depth3",
              "beside_long", "count1", "count2", "count3", "count17"]


def test_entry_is_declared_and_checks_its_operands():
    # nothing to do: no pointer is looked at
    check_call(LIB.dglhip_gspmm_items_ids16_device(0, None, None, 0, None, 0, 1, None, 0, 1, None,
                                                   1, None))
    with pytest.raises(kernel.DGLError):
        check_call(LIB.dglhip_gspmm_items_ids16_device(1, None, None, 0, None, 0, 1, None, 0, 1,
                                                       None, 1, None))


@pytest.mark.gpu
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_ids16_entry_matches_int32_entry(name, accum):
    """col_lo > 0, the block in the middle of a NaN table, both end ids, an odd
    first slot: the ids start 2-byte aligned only."""
    lengths = _cases()[name]
    col_lo, block_rows, urows = 37, 333, 500
    L = Launch(lengths, off0=3, col_lo=col_lo, block_rows=block_rows, out_rows=64,
               seed=len(lengths))
    H = _table(urows, col_lo, block_rows, 5)
    _compare(L, H, accum)


@pytest.mark.gpu
@pytest.mark.parametrize("off0", [0, 1, 2, 63, 65])
def test_first_slot_alignments(off0):
    """First slots 0, odd (2-byte aligned ids), 2 (4-byte) and either side of a
    128-byte line of ids, with the block at the table's start and at its end."""
    lengths = [70, 33, 12, 5, 64, 3, 1]
    for col_lo, block_rows, urows in ((0, 200, 260), (60, 200, 260)):
        L = Launch(lengths, off0, col_lo, block_rows, 32, seed=off0 + col_lo)
        _compare(L, _table(urows, col_lo, block_rows, 6), accum=bool(off0 & 1))


@pytest.mark.gpu
def test_block_of_65536_rows_both_end_ids():
    """The widest block: local id 65,535 is gathered, at col_lo > 0."""
    dev = _dev()
    col_lo, block_rows = 11, 65536
    L = Launch([40, 13, 12, 1, 300], 1, col_lo, block_rows, 16, seed=3)
    assert L.local.max() == 65535 and L.local.min() == 0
    _compare(L, _table(col_lo + block_rows + 5, col_lo, block_rows, 7), accum=True)
    # one more row does not fit 16 bits: the entry declines, it is an error
    h = torch.zeros(col_lo + block_rows + 5, F, device=dev)
    out = torch.zeros(16, F, device=dev)
    rows, p = torch.from_numpy(L.rows).to(dev), torch.from_numpy(L.ptr).to(dev)
    with pytest.raises(kernel.DGLError):
        check_call(LIB.dglhip_gspmm_items_ids16_device(
            L.n, ptr(rows), ptr(p), 0, ptr(_u16(L.local, dev)), col_lo, block_rows + 1, ptr(h), 0,
            h.shape[0], ptr(out), 16, stream_of(dev)))
    # and so is a block that ends past the table
    with pytest.raises(kernel.DGLError):
        check_call(LIB.dglhip_gspmm_items_ids16_device(
            L.n, ptr(rows), ptr(p), 0, ptr(_u16(L.local, dev)), col_lo + 6, block_rows, ptr(h), 0,
            h.shape[0], ptr(out), 16, stream_of(dev)))


@pytest.mark.gpu
@pytest.mark.parametrize("accum", [False, True])
def test_special_values_only_the_neighbours_gather(accum):
    """The layout of tests/test_items_columns_ids.py: NaN, +-inf and -0.0 in
    source rows that only the long items of a wave gather, behind the slots the
    short items beside them have; the short items stay finite and every row has
    the int32 kernel's bits. A row of -0.0 slots continued from -0.0 stays -0.0."""
    dev = _dev()
    col_lo, block_rows, urows = 20, 300, 340
    lengths = [40, 1, 25, 12, 2 * DEPTH + 3, 4, 3, 2, 1]
    H = _table(urows, col_lo, block_rows, 8)
    special_rows = np.arange(200, 300)                    # local ids of special rows
    vals = [np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(-0.0)]
    for i, s in enumerate(special_rows):
        H[col_lo + s, i % 3::3] = vals[i % 4]
    H[col_lo + 150] = np.float32(-0.0)
    rng = np.random.default_rng(12)
    local = []
    for m in lengths:
        ids = rng.integers(1, 150, m)                     # finite rows
        if m >= 25:
            ids[13:] = rng.choice(special_rows, m - 13)   # past every short item's end
        if m == 2:
            ids[:] = 150                                  # -0.0 + -0.0
        local.append(ids)
    L = Launch(lengths, 1, col_lo, block_rows, 24, seed=13, local=np.concatenate(local))
    # (Launch pins the first and the last slot to the block's ends: a long
    # item's first slot, finite, and the 1-slot item's, the block's last row)
    H[col_lo + block_rows - 1] = 0.25
    h = torch.from_numpy(H).to(dev)
    init = (torch.rand(24, F, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(dev)
    two = int(L.rows[lengths.index(2)])
    init[two] = -0.0
    got = _run_ids16(L, h, init, accum)
    want = _run_int32(L, h, init, accum)
    assert torch.equal(_bits(got), _bits(want))
    long_rows = [int(L.rows[i]) for i, m in enumerate(lengths) if m >= 25]
    short_rows = [int(L.rows[i]) for i, m in enumerate(lengths) if m < 25]
    assert bool(torch.isnan(got[long_rows]).any())
    assert bool(torch.isfinite(got[short_rows]).all())
    want_two = -2 ** 31 if accum else 0                   # -0.0 kept / from zero: +0.0
    assert bool((_bits(got[two]) == want_two).all())


# ---------------------------------------------------------------------------
# through the plan
# ---------------------------------------------------------------------------
def _graph(n, seed, suffix):
    rng = np.random.default_rng(seed)
    deg = np.minimum((rng.pareto(1.3, n) * 8 + 1).astype(np.int64), 600)
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, dst.size)
    src = np.concatenate([src, [0, n - 1]])
    dst = np.concatenate([dst, [1, 2]])
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    if suffix:
        rows = np.arange(3, n, 97)
        src = np.concatenate([src, np.tile([n - 2, 4], rows.size)])
        dst = np.concatenate([dst, np.repeat(rows, 2)])
    return src.astype(np.int64), dst.astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("suffix", [False, True])
def test_through_the_plan_switch_and_oracle(suffix):
    """A power-law graph of 4,000 rows in 5 blocks of 800 (a suffix launch in
    one variant, its span within 16 bits): ids_wide 0 against 1, bit for bit,
    sum against the oracle's chain; the device-built ids16 against the host's."""
    dev = _dev()
    n = 4000
    src, dst = _graph(n, 31, suffix)
    csr = kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                           kernel.ORDER_EID, dev)
    H = torch.rand(n, F, generator=torch.Generator().manual_seed(32)) * 2 - 1
    h = H.to(dev)
    init = (torch.rand(n, F, generator=torch.Generator().manual_seed(33)) * 2 - 1).to(dev)
    with kernel.scheduled(block_table_min=0, block_bytes=800 * F * 4, block_min_slots=1):
        path, launches = csr.plan.schedule(kernel.MSG_COPY_U, kernel.RED_SUM, F, 0, n)
        assert path == kernel.PLAN_PATH_BLOCKED and launches == 5 + int(suffix) >= 3
        k = ctypes.c_int()
        check_call(LIB.dglhip_gspmm_items_kernel(kernel.MSG_COPY_U, F, 0, n, n, 2, 2, ptr(h),
                                                 ptr(init), ctypes.byref(k)))
        assert k.value == 2
        plan = kernel._block_plan(csr, h, F)
        assert plan.has_suffix == suffix and plan.bs == 800 and plan.ids16 is not None
        # device builder against host builder
        host = kernel._block_items(
            kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                             kernel.ORDER_EID, "cpu"), 5)
        assert torch.equal(plan.indices.cpu(), host.indices)
        assert torch.equal(plan.ids16.cpu(), host.ids16)
        for it in plan:
            assert torch.equal((it.ids16.to(torch.int64) & 0xFFFF) + it.col_lo,
                               it.indices.to(torch.int64))
        res = {}
        for red, start in ((kernel.RED_SUM, None), (kernel.RED_SUM_ACCUM, init),
                           (kernel.RED_MEAN, None)):
            for wide in (0, 1):
                out = (torch.full((n, F), float("nan"), device=dev) if start is None
                       else start.clone())
                with kernel.scheduled(ids_wide=wide):
                    kernel._run_gspmm(csr, kernel.MSG_COPY_U, red, h, None, 0, F, False, out=out)
                torch.cuda.synchronize()
                res[(red, wide)] = out
            assert torch.equal(res[(red, 0)], res[(red, 1)])
            assert torch.equal(_bits(res[(red, 0)]), _bits(res[(red, 1)]))
    assert np.array_equal(res[(kernel.RED_SUM, 0)].cpu().numpy(),
                          O.spmm_coo(n, dst, src, H.numpy()))


@pytest.mark.gpu
def test_table_past_4gib_with_a_short_block_near_its_end():
    """A table of 4 GiB + 2 MiB: no int32 kernel with 32-bit offsets takes it
    (the query says the one-item kernel), but a block of 300 rows ending at its
    last row takes the column halves over 16-bit ids (the entry launches that
    kernel or fails). Only the gathered rows are filled. Compared with the
    int32 pair kernel over the block as a table of its own."""
    dev = _dev()
    urows = (1 << 23) + 4096
    need = urows * F * 4 + (64 << 20)
    free, _ = torch.cuda.mem_get_info(dev)
    if free < need:
        pytest.skip("needs %.1f GiB of device memory" % (need / 2.0 ** 30))
    block_rows = 300
    col_lo = urows - block_rows
    table = torch.empty(urows, F, device=dev)
    Hb = _table(block_rows, 0, block_rows, 41)
    table[col_lo - 1] = float("nan")
    table[col_lo:] = torch.from_numpy(Hb).to(dev)
    k = ctypes.c_int()
    out0 = torch.zeros(32, F, device=dev)
    check_call(LIB.dglhip_gspmm_items_kernel(kernel.MSG_COPY_U, F, 0, urows, 32, 2, 2, ptr(table),
                                             ptr(out0), ctypes.byref(k)))
    assert k.value == 0
    L = Launch([70, 30, 13, 12, 11, 2, 1], 1, col_lo, block_rows, 32, seed=42)
    init = (torch.rand(32, F, generator=torch.Generator().manual_seed(43)) * 2 - 1).to(dev)
    for accum in (False, True):
        got = _run_ids16(L, table, init, accum)
        # the block as a table of its own: ids local, col_lo 0
        sub = Launch([70, 30, 13, 12, 11, 2, 1], 1, 0, block_rows, 32, seed=42)
        assert np.array_equal(sub.local, L.local) and np.array_equal(sub.rows, L.rows)
        want = _run_int32(sub, table[col_lo:], init, accum)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, want) and torch.equal(_bits(got), _bits(want))
    del table
    torch.cuda.empty_cache()
