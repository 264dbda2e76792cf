"""The wave schedule of the column halves (gspmm_items_columns_kernel,
DESIGN.md §4.1 "Column halves"): a wave's nine item records behind one wait
(every wave but a launch's last, which clamps them), the first ids ahead of the
running row, the next batch's ids consumed after the batch's adds, and one
store for the wave's four rows through a descriptor over all of out.

Every case runs F = 128 over 3 source blocks of 128 rows (a first launch that
only writes and two that continue the running rows), or over a random graph of
as many rows, under ``items_per_wave=2, column_parts=2`` and compares bit
patterns with ``items_per_wave=1, column_parts=1`` (the one-item kernel) and
with the oracle's chain: slot order, from zero or from the running row.

The plan makes no item without slots, so a length of 0 stands for what the
kernel sees as one: a quarter past the launch's last item (the clamped wave's
dead quarters, n = 0) and a row that has no slot in a launch and keeps its
value across it. A launch's items run longest first, four to a wave, so the
wave (24, 24, 24, 37) is the items 37, 24, 24, 24; (13, 1, 0, 25) the last
wave 25, 13, 1 and a dead quarter; (0, 0, 0, 1) a last wave of one item.
"""
import contextlib

import numpy as np
import pytest
import torch

from dgl import kernel
from oracle import oracle as O

F = 128
DEPTH = 12        # gathers a wave has in flight per batch (launch_items_columns)
BLOCK_ROWS = 128  # source rows per block under small_blocks()
N = 3 * BLOCK_ROWS

COLS = {"items_per_wave": 2, "column_parts": 2}   # the kernel under test
ONE = {"items_per_wave": 1, "column_parts": 1}

SENTINEL = 12345.0


@contextlib.contextmanager
def small_blocks(**more):
    with kernel.scheduled(block_table_min=0, block_bytes=BLOCK_ROWS * F * 4, block_min_slots=1,
                          **more):
        yield


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _graph_of_lengths(blocks, seed=0):
    """Edges such that block b's launch has exactly the items ``blocks[b]``: a
    list of (row, slots), the slots' sources drawn from block b's 128 rows
    (without repetition up to 128 slots, with it past them: a hub). Source-
    major, so every row's slots run in source order. The first and the last
    source row are referenced, so the plan's even cut of the referenced column
    range is these blocks."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for b, items in enumerate(blocks):
        assert len({row for row, _ in items}) == len(items)
        for i, (row, length) in enumerate(items):
            assert length > 0
            s = np.sort(rng.choice(BLOCK_ROWS, size=length, replace=length > BLOCK_ROWS))
            s = s + b * BLOCK_ROWS
            if i == 0 and b == 0:
                s[0] = 0
            if i == 0 and b == len(blocks) - 1:
                s[-1] = len(blocks) * BLOCK_ROWS - 1
            src.append(s)
            dst.append(np.full(length, row))
    src, dst = np.concatenate(src), np.concatenate(dst)
    o = np.lexsort((dst, src))
    return src[o].astype(np.int64), dst[o].astype(np.int64)


def _random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    o = np.lexsort((dst, src))
    return src[o].astype(np.int64), dst[o].astype(np.int64)


def _csr(n, src, dst, dev):
    return kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src), kernel.ORDER_EID,
                            dev)


def _launches(csr, u2):
    feat = u2.shape[1]
    ldu = u2.stride(0) if kernel._row_strided(u2, feat) else 0
    path, launches = csr.plan.schedule(kernel.MSG_COPY_U, kernel.RED_SUM, feat, ldu, u2.shape[0])
    assert path == kernel.PLAN_PATH_BLOCKED and launches > 1
    return launches


def _item_lengths(csr, u2):
    plan = kernel._block_plan(csr, u2, u2.shape[1])
    assert plan is not None
    return [(it.ptr[1:] - it.ptr[:-1]).tolist() for it in plan]


def _run(csr, u2, pol, init=None, out=None):
    """The product under the policy words ``pol``: RED_SUM into a NaN-filled
    out, or RED_SUM_ACCUM continued from ``init``; ``out``: run into it as it is."""
    red = kernel.RED_SUM if init is None else kernel.RED_SUM_ACCUM
    if out is None:
        out = (torch.full((csr.num_rows, F), float("nan"), device=u2.device)
               if init is None else init.clone())
    with kernel.scheduled(**pol):
        kernel._run_gspmm(csr, kernel.MSG_COPY_U, red, u2, None, 0, F, False, out=out)
    torch.cuda.synchronize()
    return out


def _chain(src, dst, H, init):
    """The oracle's chain continued from ``init``: every row adds its slots'
    source rows in slot order (fp32, one add per slot)."""
    out = np.array(init, dtype=np.float32, copy=True)
    for s, d in zip(src.tolist(), dst.tolist()):
        out[d] = out[d] + H[s]
    return out


def _assert_oracle_bits(got, ref):
    """NaN where the oracle has NaN, its bits everywhere else."""
    got = got.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.where(np.isnan(ref), 0, got.view(np.int32)),
                          np.where(np.isnan(ref), 0, ref.view(np.int32)))


def _check(dev, blocks, seed, H=None, init=None):
    """Both reducers over the graph of ``blocks`` under the column halves,
    against the one-item kernel and the oracle; returns (first, continued)."""
    src, dst = _graph_of_lengths(blocks, seed)
    csr = _csr(N, src, dst, dev)
    if H is None:
        H = (torch.rand(N, F, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1).numpy()
    if init is None:
        init = (torch.rand(N, F, generator=torch.Generator().manual_seed(seed + 2)) * 2 - 1).numpy()
    h, start = torch.from_numpy(H).to(dev), torch.from_numpy(init).to(dev)
    with small_blocks():
        assert _launches(csr, h) == len(blocks)
        assert _item_lengths(csr, h) == [sorted((n for _, n in items), reverse=True)
                                         for items in blocks]
        first, cont = _run(csr, h, COLS), _run(csr, h, COLS, start)
        assert _same_bits(first, _run(csr, h, ONE))
        assert _same_bits(cont, _run(csr, h, ONE, start))
    _assert_oracle_bits(first, O.spmm_coo(N, dst, src, H))
    _assert_oracle_bits(cont, _chain(src, dst, H, init))
    return first, cont


# the lengths around one, two and three batches, and a hub; rows 40 and up
# have no slot anywhere
LENGTHS = [1, 11, 12, 13, 23, 24, 25, 36, 37, 200]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_item_lengths_in_every_quarter(dev, shift):
    """Ten items per launch, sorted 200, 37, 36, 25 | 24, 23, 13, 12 | 11, 1
    and two dead quarters; ``shift`` more items of 30 slots move every length
    through the four quarters (and the last wave through 2, 3, 4 and 1 live
    quarters). Every row's length differs from launch to launch, and rows 20-29
    have slots in one launch only: they keep their value across the others."""
    blocks = []
    for b in range(3):
        items = [(2 * ((i + 3 * b) % len(LENGTHS)), n) for i, n in enumerate(LENGTHS)]
        items += [(20 + 3 * b + j, 30) for j in range(shift)]
        blocks.append(items)
    first, cont = _check(dev, blocks, seed=100 + shift)
    assert not bool(first[40:].any())  # rows without slots: zero, not the NaN pre-fill


# (24, 24, 24, 37): two full batches, then a predicated one for one quarter;
# (12, 12, 12, 12): the full-batch loop alone
FULL_WAVES = [(1, 37), (3, 24), (5, 24), (7, 24), (9, 12), (11, 12), (13, 12), (15, 12)]
LAST_THREE = [(3, 25), (5, 13), (7, 1)]  # (13, 1, 0, 25)
LAST_ONE = [(5, 1)]                      # (0, 0, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("turn", [0, 1, 2])
def test_waves_of_given_items(dev, turn):
    """The issue's four waves, each of them in the first launch (``turn``) and
    in an accumulating one."""
    blocks = [FULL_WAVES, LAST_THREE, LAST_ONE]
    blocks = blocks[turn:] + blocks[:turn]
    _check(dev, blocks, seed=200 + turn)


@pytest.mark.gpu
@pytest.mark.parametrize("counts", [(4, 5, 6), (5, 6, 7), (6, 7, 8), (7, 8, 4), (8, 4, 5)])
def test_item_counts_per_launch(dev, counts):
    """4 and 8 items: every wave takes its records unclamped; 5, 6 and 7: a
    clamped last wave of 1, 2 and 3 live quarters. Each count once in the first
    launch."""
    rng = np.random.default_rng(300 + counts[0])
    blocks = []
    for c in counts:
        rows = rng.choice(24, size=c, replace=False)  # rows shared among the launches
        blocks.append([(int(r), int(rng.integers(1, 40))) for r in rows])
    _check(dev, blocks, seed=310 + counts[0])


@pytest.mark.gpu
def test_special_running_rows_and_unowned_quarters(dev):
    """Running rows of -0.0, NaN and +-inf beside ended items, absent rows and
    dead quarters. Row 5 continues from -0.0 over -0.0 slots only, one or two per
    launch beside longer items: it stays -0.0 (a zero added for a switched-off
    lane would make it +0.0). Row 21 holds -0.0 and has no slot: untouched. The
    last launch ends on a wave of one live quarter whose item is the highest
    row; a dead quarter that stored would overwrite that row, and nothing may
    be written past it."""
    blocks = [
        [(3, 40), (5, 1), (7, 25), (9, 12), (11, 2 * DEPTH + 1)],
        [(3, 20), (5, 1), (7, 19)],
        [(5, 2), (9, 2 * DEPTH + 3), (11, 4), (13, 3), (30, 1)],
    ]
    src, dst = _graph_of_lengths(blocks, seed=7)
    rng = np.random.default_rng(8)
    H = rng.random((N, F), dtype=np.float32) * 2 - 1
    H[rng.choice(N, 24, replace=False)] = np.float32(1e-41)  # denormal rows
    H[rng.choice(N, 12, replace=False), ::3] = np.float32("inf")
    H[rng.choice(N, 12, replace=False), 2::5] = np.float32("nan")
    H[src[dst == 5]] = np.float32(-0.0)  # every source of row 5
    init = rng.random((N, F), dtype=np.float32) * 2 - 1
    init[5] = init[21] = -0.0
    init[3, ::2] = np.float32("nan")
    init[7, 1::4] = np.float32("inf")
    init[9, 2::4] = np.float32("-inf")
    init[13] = np.float32("-inf")
    init[31:] = SENTINEL  # past the last item's row
    first, cont = _check(dev, blocks, seed=7, H=H, init=init)
    for got in (first, cont):
        assert bool(torch.isnan(got).any()) and bool(torch.isinf(got).any())
    assert bool((_bits(cont[5]) == -2 ** 31).all())
    assert bool((_bits(cont[21]) == -2 ** 31).all())
    assert bool((_bits(first[5]) == 0).all())  # from zero the same slots give +0.0
    assert bool((cont[31:] == SENTINEL).all())


@pytest.fixture(scope="module")
def random_graph(dev):
    src, dst = _random_graph(N, 9000, 31)
    H = torch.rand(N, F, generator=torch.Generator().manual_seed(11)) * 2 - 1
    init = torch.rand(N, F, generator=torch.Generator().manual_seed(12)) * 2 - 1
    return {"src": src, "dst": dst, "csr": _csr(N, src, dst, dev), "H": H, "init": init,
            "ref": O.spmm_coo(N, dst, src, H.numpy()),
            "ref_cont": _chain(src, dst, H.numpy(), init.numpy())}


@pytest.mark.gpu
def test_strided_input(dev, random_graph):
    """Source rows at a stride of 132 floats (16-byte aligned, 528 bytes apart)."""
    g = random_graph
    ld132 = torch.zeros(N, F + 4, device=dev)[:, :F]
    ld132.copy_(g["H"])
    assert kernel._row_strided(ld132, F) and ld132.stride(0) == 132
    start = g["init"].to(dev)
    with small_blocks(pad_rows=0):
        assert _launches(g["csr"], ld132) >= 3
        first, cont = _run(g["csr"], ld132, COLS), _run(g["csr"], ld132, COLS, start)
        assert _same_bits(first, _run(g["csr"], ld132, ONE))
        assert _same_bits(cont, _run(g["csr"], ld132, ONE, start))
    assert np.array_equal(first.cpu().numpy(), g["ref"])
    assert np.array_equal(cont.cpu().numpy(), g["ref_cont"])


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [4, 5 * F + 8])
def test_output_inside_a_larger_tensor(dev, random_graph, lead):
    """out starts ``lead`` floats into a larger tensor (16-byte aligned: 16
    bytes, and five rows and 32 bytes): the store's offsets start from that
    base, and nothing ahead of out or behind it is written."""
    g = random_graph
    h = g["H"].to(dev)
    with small_blocks():
        assert _launches(g["csr"], h) == 3
        for init, ref in ((None, g["ref"]), (g["init"], g["ref_cont"])):
            big = torch.full((lead + N * F + 3 * F,), SENTINEL, device=dev)
            out = big[lead:lead + N * F].view(N, F)
            assert out.data_ptr() % 16 == 0 and out.data_ptr() != big.data_ptr()
            if init is not None:
                out.copy_(init)
            _run(g["csr"], h, COLS, None if init is None else out, out=out)
            assert np.array_equal(out.cpu().numpy(), ref)
            assert bool((big[:lead] == SENTINEL).all())
            assert bool((big[lead + N * F:] == SENTINEL).all())
