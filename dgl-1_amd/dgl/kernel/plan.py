"""Python views of a CSR's native launch plan (dglhip_spmm_plan_*,
csrc/spmm_plan.*): the handle, the source-blocked schedule as launches or as
row ranges, and the block sizes of the kernels that walk those ranges
themselves. CSRs are taken duck-typed (csr.py imports this module)."""
from __future__ import absolute_import

import ctypes
import os
import weakref

import torch

from .. import _ffi
from .._ffi import LIB, check_call, ptr, stream_of as _stream_of
from ..base import DGLError
from .policy import SLOT, _POLICY_GEN, schedule_policy

# ---------------------------------------------------------------------------
# The native launch plan of a CSR (dglhip_spmm_plan_*, csrc/spmm_plan.*)
# ---------------------------------------------------------------------------
def _retry_oom(fn):
    """Run ``fn``; when the library's hipMalloc fails, hand torch's cached
    blocks back to the device once and retry (plan structures live in memory
    the library allocates beside torch's caching allocator)."""
    try:
        return fn()
    except DGLError as err:
        msg = str(err)
        if "hipMalloc" not in msg and "out of memory" not in msg.lower():
            raise
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return fn()


def _capi(name):
    return _ffi.get_global_func("dglhip._CAPI_" + name)


class _NativePlan(object):
    """Handle on a CSR's launch plan (dglhip_spmm_plan_create / _free). The
    plan borrows the CSR's indptr / indices / row_order (the CSR holds them for
    as long as it holds the plan) and keeps the schedules the g-SpMM runs over
    them, built natively on first use: the same object the
    C-ABI and dglhip._CAPI_GSpMM hand out, so one implementation serves the
    Python operators and every C / PackedFunc caller."""

    __slots__ = ("handle", "device", "_ws", "_cache", "__weakref__")

    def __init__(self, csr):
        dev = csr.device
        self.handle = None
        self.device = dev
        self._ws = {}
        self._cache = {}
        h = ctypes.c_void_p()
        if dev.type == "cuda":
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            kind, stream = (10, idx), _stream_of(dev)
            hip = csr._host_indptr
        else:
            kind, stream, hip = (1, 0), None, None

        def make():
            check_call(LIB.dglhip_spmm_plan_create(
                kind[0], kind[1], csr.num_rows, csr.num_cols, csr.nnz, ptr(csr.indptr),
                ptr(csr.indices) if csr.nnz else None, ptr(hip), ptr(csr.row_order), stream,
                ctypes.byref(h)))
        _retry_oom(make)
        self.handle = h.value

    @property
    def arg(self):
        return ("handle", self.handle)

    def stream(self):
        return _stream_of(self.device) if self.device.type == "cuda" else None

    def stream_arg(self):
        return ("handle", self.stream().value) if self.device.type == "cuda" else None

    def __del__(self):
        h, self.handle = self.handle, None
        if h:
            try:
                LIB.dglhip_spmm_plan_free(h)
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass

    def workspace(self, msg, red, F, ldu, urows, elen, emode, erow):
        key = (msg, red, F, ldu, urows, elen, emode, _POLICY_GEN[0])
        nbytes = self._ws.get(key)
        if nbytes is None:
            b = ctypes.c_int64()
            _retry_oom(lambda: check_call(LIB.dglhip_spmm_plan_workspace(
                self.handle, msg, red, F, ldu, urows, elen, emode, ptr(erow), self.stream(),
                ctypes.byref(b))))
            nbytes = self._ws[key] = int(b.value)
        return nbytes

    def schedule(self, msg, red, F, ldu=0, urows=0, elen=0, emode=0, erow=None):
        """(path, launches) a run with these arguments takes
        (DGLHIP_PLAN_PATH_*: 0 host, 1 rows, 2 blocked, 3 blocked max, 4 sweep)."""
        path, launches = ctypes.c_int(), ctypes.c_int64()
        _retry_oom(lambda: check_call(LIB.dglhip_spmm_plan_schedule(
            self.handle, msg, red, F, ldu, urows, elen, emode, ptr(erow), self.stream(),
            ctypes.byref(path), ctypes.byref(launches))))
        return int(path.value), int(launches.value)

    def stats(self):
        """dict: rows, cols, nnz, max_degree, nonempty, waves, heavy_threshold."""
        s = (ctypes.c_int64 * 7)()
        check_call(LIB.dglhip_spmm_plan_stats(self.handle, s))
        return dict(zip(("rows", "cols", "nnz", "max_degree", "nonempty", "waves",
                         "heavy_threshold"), list(s)))


PLAN_PATH_HOST, PLAN_PATH_ROWS, PLAN_PATH_BLOCKED, PLAN_PATH_MAX_BLOCKED, PLAN_PATH_SWEEP = \
    0, 1, 2, 3, 4


# the fused GAT kernels' blocks: their per-row work (the attention through LDS)
# makes a row's pass per block dearer than copy_u's, so fewer, larger blocks
_GAT_BLOCK_BYTES = int(os.environ.get("DGLHIP_GAT_BLOCK_BYTES", 11 << 20))  # 11 MiB
# the fused forward when no attention is stored (inference, and training with
# the one-pass backward, which recomputes it): with the batch's logits loaded
# ahead of its row gathers the per-row pass got cheaper, so smaller blocks pay
# (Reddit-shaped 8 x 16: 4.96 ms at 7 MiB, 4.98 at 8, 5.22 at 9, 5.81 at 11;
# tools/gat_block_percall.py, profiles/r04/gat_bwd/fwd_block_sweep.log)
_GAT_BLOCK_BYTES_NOGRAD = int(os.environ.get("DGLHIP_GAT_BLOCK_BYTES_NOGRAD", 7 << 20))
# the one-pass GAT backward over the transpose (its own per-row work: the
# attention recomputed per pair, the dot's exchanges, the epilogue): larger
# slices, as the forward's (Reddit-shaped 8 x 16, forward + backward: 4 / 6 /
# 8 / 11 / 14 / 18 MiB 17.97 / 16.86 / 16.48 / 16.18 / 16.25 / 16.39 ms, the
# same bits; tools/gat_bwd_sweep.py, profiles/r04/gat_bwd_sweep.json); at 5
# waves per SIMD (r05) 6 / 8 / 11 / 14 / 18 / 24 MiB 14.63 / 14.30 / 14.15 /
# 14.06 / 14.29 / 14.65 ms (profiles/r05/gat_fwd/bwd_block_sweep_*.json)
_GAT_BWD_BLOCK_BYTES = int(os.environ.get("DGLHIP_GAT_BWD_BLOCK_BYTES", 14 << 20))


# el's gradient reads the E x H attention gradient (forward slot order)
# through the transpose's slot map: 32-B values at random forward slots, a
# 128-B line each. Cut by destination block, each launch's values come from
# one contiguous forward-slot range of about this many bytes, which the
# Infinity Cache holds (Reddit-shaped graph, 8 heads: one launch 3.72 ms;
# 32 / 128 / 256 / 512 MiB blocks 3.34 / 3.19 / 3.13 / 3.20 ms, the same
# bits; tools/el_grad_sweep.py)
_EL_GRAD_BLOCK_BYTES = int(os.environ.get("DGLHIP_EL_GRAD_BLOCK_BYTES", 256 << 20))


class _PlanLaunch(object):
    """One launch of the plan's source-blocked schedule (views of the plan's
    arrays): ``rows`` (int32) the rows with slots in the block, longest first
    (stable by row id); item i's slots are [ptr[i], ptr[i+1]) of the plan's
    global slot arrays (``ptr`` holds global offsets); ``indices`` / ``pos``
    this launch's slots (column ids, and the CSR slot each came from);
    ``col_lo`` the first column of the launch's source block (the suffix: of
    the whole span) and ``ids16`` its slots' 16-bit ids local to it, as an
    int16 view of the bits (None where the plan has none)."""
    __slots__ = ("rows", "ptr", "indices", "pos", "nnz", "off", "suffix", "col_lo", "ids16")


class _BlockedSchedule(list):
    """The plan's source-blocked schedule: its launches (B blocks, then the
    suffix if any) plus the global arrays: ``indices`` / ``pos`` (plan
    order), ``absent`` (rows the first launch does not list), ``lo`` / ``bs``
    / ``span`` (the first referenced column, columns per block, columns
    referenced) and ``ids16`` (the uint16 block-local ids of every slot as an
    int16 tensor of the same bits, built when ``bs`` <= 65,536, else None)."""


def _blocked_native(csr, row_bytes, block_bytes, blocks=0):
    """The native plan's blocked schedule for gathered rows of ``row_bytes``
    in ``block_bytes`` slices (or exactly ``blocks`` blocks), as torch views
    of its arrays (cached per policy); None when none applies."""
    plan = csr.plan
    key = ("blocked", int(row_bytes), int(block_bytes), int(blocks), _POLICY_GEN[0])
    if key in plan._cache:
        return plan._cache[key]
    f = _retry_oom(lambda: _capi("SpmmPlanBlocked")(plan.arg, int(row_bytes), int(block_bytes),
                                                    int(blocks), plan.stream_arg()))
    res = None
    if f is not None:
        meta = f(0).tolist()
        B, sfx, _, L = meta[:4]
        res = _BlockedSchedule()
        res.indices, res.pos, res.absent = f(1), f(2), f(3)
        res.B, res.has_suffix = int(B), bool(sfx)
        res.lo, res.bs, res.span, has16 = (int(x) for x in meta[4 + 4 * int(L):8 + 4 * int(L)])
        res.ids16 = f(4 + 2 * int(L)) if has16 else None
        for i in range(int(L)):
            n_items, nnz, off, suffix = meta[4 + 4 * i:8 + 4 * i]
            it = _PlanLaunch()
            it.rows, it.ptr = f(4 + 2 * i), f(5 + 2 * i)
            it.indices = res.indices[off:off + nnz]
            it.pos = res.pos[off:off + nnz]
            it.nnz, it.off, it.suffix = int(nnz), int(off), bool(suffix)
            it.col_lo = res.lo if it.suffix else res.lo + i * res.bs
            it.ids16 = None if res.ids16 is None else res.ids16[off:off + nnz]
            res.append(it)
    plan._cache[key] = res
    return res


def _block_plan(csr, ufeat2, feat_len, block_bytes=None):
    """The blocked schedule the plan runs for these source rows (None when
    the product keeps one launch): the blocks cut the referenced column range
    evenly (``block_bytes`` of source rows each, default the policy's)."""
    ld = ufeat2.stride(0) if (ufeat2.dim() == 2 and ufeat2.shape[0] > 1) else feat_len
    row_bytes = max(ld, feat_len) * ufeat2.element_size()
    if csr.nnz == 0:
        return None
    return _blocked_native(csr, row_bytes, block_bytes or schedule_policy()["block_bytes"])


def _block_items(csr, blocks):
    """The plan's blocked schedule at exactly ``blocks`` source blocks (None:
    some rows' suffixes exceed the policy's share)."""
    return _blocked_native(csr, 0, 0, blocks)


def _column_span(csr):
    """(lo, hi): the range of columns the slots reference."""
    if csr.nnz == 0:
        return (0, 0)
    ind = csr.indices
    lo, hi = torch.aminmax(ind) if ind.is_cuda else (ind.min(), ind.max())
    return int(lo), int(hi) + 1


def _cuts_native(csr, row_bytes, block_bytes, blocks=0):
    plan = csr.plan
    key = ("cuts", int(row_bytes), int(block_bytes), int(blocks), _POLICY_GEN[0])
    if key in plan._cache:
        return plan._cache[key]
    arr = _retry_oom(lambda: _capi("SpmmPlanCuts")(plan.arg, int(row_bytes), int(block_bytes),
                                                   int(blocks), plan.stream_arg()))
    res = None if arr is None else [arr[i] for i in range(arr.shape[0])]
    plan._cache[key] = res
    return res


def _block_cuts(csr, row_bytes, block_bytes=None):
    """The blocked schedule as row ranges (the plan's, cached): B + 1 int64
    arrays (B + 2 when some rows have a suffix), row r's slots of range i
    being [cuts[i][r], cuts[i + 1][r]) of the CSR itself (cuts[0] =
    indptr[:-1], the last = indptr[1:]), for kernels that keep the CSR's slot
    indices (the fused GAT layer, the g-SDDMM). ``row_bytes``: bytes gathered
    per source. None when the schedule does not apply."""
    if csr.nnz == 0:
        return None
    return _cuts_native(csr, row_bytes, block_bytes or _GAT_BLOCK_BYTES)


def _plan_tag(plan):
    """(source blocks, has a suffix launch): the key of caches derived from a
    blocked plan. The plan's length alone is ambiguous: B blocks plus a suffix
    and B + 1 blocks without one are both B + 1 launches, and one CSR gets
    different B at different widths or dtypes."""
    sfx = bool(plan[-1].suffix)
    return (len(plan) - int(sfx), sfx)


def _block_slots(csr, plan):
    """int64: for each slot of the blocked plan, blocks in order, the slot of
    ``csr`` it came from (cached; for edge-valued messages)."""
    key = ("blocked_slots",) + _plan_tag(plan)
    if key not in csr._plans:
        csr._plans[key] = plan.pos.long()
    return csr._plans[key]


def _block_edge_rows(csr, plan, emap):
    """Rows of the edge-value tensor for the blocked plan's slots, for the
    layout ``emap`` names (_run_gspmm): None = edge ids, SLOT = the CSR's
    slots, or a per-slot row tensor (e.g. the transpose's forward-slot map).
    Cached: per layout, and for a row tensor per tensor object (held weakly:
    a new tensor, or one changed in place, composes anew)."""
    tag = _plan_tag(plan)
    slots = _block_slots(csr, plan)
    if emap is SLOT or (emap is None and csr.slot_eid is None):
        return slots
    if emap is None:
        key = ("blocked_eid",) + tag
        if key not in csr._plans:
            csr._plans[key] = csr.slot_eid.index_select(0, slots)
        return csr._plans[key]
    key = ("blocked_emap",) + tag
    hit = csr._plans.get(key)
    if hit is not None and hit[0]() is emap and hit[1] == emap._version:
        return hit[2]
    rows = emap.index_select(0, slots)
    csr._plans[key] = (weakref.ref(emap), emap._version, rows)
    return rows
