"""The blocked plan's 16-bit ids (BlockedPlan::ids16, DESIGN.md §4.1 "Column
halves", slice-local ids): one uint16 per plan slot, the slot's column less
the first column of its launch's source block (the suffix launch: less the
first referenced column). The host builder writes them in the same pass as
``indices``; they exist when a block has at most 65,536 columns. These tests
run the host builder: ``ids16`` plus each launch's ``col_lo`` gives back
``indices`` exactly, on a power-law graph cut into 3 blocks with and without
a suffix launch; the array is there at 65,536 columns per block and not at
65,537; local ids 0 and ``bs`` - 1 both occur. (The device builder is
compared with the host's in tests/test_items_ids16.py.)
"""
import numpy as np
import torch

from dgl import kernel

N = 3000


def _local(ids16):
    """The uint16 ids (handed out as int16 bits) as int64."""
    return ids16.to(torch.int64) & 0xFFFF


def _power_law(seed, suffix):
    """Source-major edges over N nodes with power-law in-degrees; the first and
    the last node are sources, so 3 blocks are 1,000 columns each, and the
    first and last column of every block are referenced. ``suffix``: a few
    rows end, in edge-id order, with a source of block 2 and then one of
    block 0: a decrease, so their last slot runs in the suffix launch."""
    rng = np.random.default_rng(seed)
    deg = np.minimum((rng.pareto(1.2, N) * 6 + 1).astype(np.int64), 400)
    dst = np.repeat(np.arange(N), deg)
    src = rng.integers(0, N, dst.size)
    edge = np.arange(0, N + 1, 1000)
    ends = np.concatenate([edge[:-1], edge[1:] - 1])      # 0, 1000, 2000, 999, 1999, 2999
    src = np.concatenate([src, ends])
    dst = np.concatenate([dst, np.arange(ends.size) * 7 % N])
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    if suffix:
        rows = np.arange(5, N, 211)
        src = np.concatenate([src, np.tile([2500, 3], rows.size)])
        dst = np.concatenate([dst, np.repeat(rows, 2)])
    return src.astype(np.int64), dst.astype(np.int64)


def _host_plan(src, dst, n, blocks):
    csr = kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src),
                           kernel.ORDER_EID, "cpu")
    return csr, kernel._block_items(csr, blocks)


def _check_reproduces(suffix):
    src, dst = _power_law(17, suffix)
    csr, plan = _host_plan(src, dst, N, 3)
    assert plan is not None and plan.B == 3 and plan.has_suffix == suffix
    assert len(plan) == 3 + int(suffix)
    assert (plan.lo, plan.bs, plan.span) == (0, 1000, N)
    assert plan.ids16 is not None and plan.ids16.dtype == torch.int16
    assert plan.ids16.numel() == plan.indices.numel() == csr.nnz
    for i, it in enumerate(plan):
        assert it.nnz > 0
        assert it.col_lo == (plan.lo if it.suffix else plan.lo + i * plan.bs)
        loc = _local(it.ids16)
        # exact, slot by slot
        assert torch.equal(loc + it.col_lo, it.indices.to(torch.int64))
        assert int(loc.max()) < (plan.span if it.suffix else plan.bs)
        if not it.suffix:
            # the block's first and last column are referenced
            assert int(loc.min()) == 0 and int(loc.max()) == plan.bs - 1
    # the plan's slots are a permutation of the CSR's: the same through pos
    assert torch.equal(csr.indices[plan.pos.long()], plan.indices)
    return plan


def test_ids16_and_col_lo_reproduce_indices_three_blocks():
    _check_reproduces(suffix=False)


def test_ids16_and_col_lo_reproduce_indices_with_a_suffix_launch():
    plan = _check_reproduces(suffix=True)
    sfx = plan[-1]
    assert sfx.suffix and sfx.col_lo == 0
    # the suffix slots are the sources of block 0 behind those of block 2
    assert set(sfx.indices.tolist()) == {3}


def _two_blocks_of(bs):
    """Two blocks of ``bs`` columns: a handful of edges whose sources are the
    first and last column of each block."""
    n = 2 * bs
    src = np.array([0, bs - 1, bs, n - 1, 5, bs + 5], dtype=np.int64)
    dst = np.array([0, 0, 1, 1, 2, 2], dtype=np.int64)
    o = np.lexsort((dst, src))
    csr, plan = _host_plan(src[o], dst[o], n, 2)
    assert plan is not None and plan.B == 2 and plan.bs == bs and not plan.has_suffix
    return plan


def test_blocks_of_65536_columns_build_ids16_with_both_end_ids():
    plan = _two_blocks_of(65536)
    assert plan.ids16 is not None
    for it in plan:
        loc = _local(it.ids16)
        assert sorted(loc.tolist()) == [0, 5, 65535]
        assert torch.equal(loc + it.col_lo, it.indices.to(torch.int64))


def test_blocks_of_65537_columns_build_no_ids16():
    plan = _two_blocks_of(65537)
    assert plan.ids16 is None
    assert all(it.ids16 is None for it in plan)
    assert sorted(plan[1].indices.tolist()) == [65537, 65542, 2 * 65537 - 1]


def test_policy_word_ids_wide_roundtrips_and_rejects_other_values():
    import ctypes

    import pytest

    from dgl import _ffi
    pol = kernel.schedule_policy()
    assert pol["ids_wide"] in (0, 1)
    assert ctypes.sizeof(kernel._Policy) == 104     # the word was there: `reserved`
    for v in (0, 1):
        with kernel.scheduled(ids_wide=v):
            now = kernel.schedule_policy()
            assert now["ids_wide"] == v
            assert {k: x for k, x in now.items() if k != "ids_wide"} == \
                {k: x for k, x in pol.items() if k != "ids_wide"}
            raw = kernel._Policy()
            _ffi.check_call(_ffi.LIB.dglhip_spmm_get_policy(ctypes.addressof(raw)))
            assert raw.ids_wide == v and raw.column_parts == pol["column_parts"]
    assert kernel.schedule_policy() == pol
    for bad in (2, -1):
        with pytest.raises(kernel.DGLError):
            kernel.set_schedule_policy(ids_wide=bad)
        assert kernel.schedule_policy() == pol
