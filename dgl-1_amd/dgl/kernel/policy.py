"""The operators' constants and the g-SpMM schedule policy: the native launch
plan's (dglhip_spmm_get_policy / dglhip_spmm_set_policy), its sweep knobs and
the heavy-row split's gate. The bottom of the package: it imports none of the
package's other modules."""
from __future__ import absolute_import

import contextlib
import ctypes

import torch

from .._ffi import LIB, check_call
from ..base import DGLError

MSG_COPY_U, MSG_U_MUL_E, MSG_COPY_E = 0, 1, 2
MSG_COPY_U_BF16 = 3  # copy_u over bf16 source rows, widened exactly to fp32 (dgl_hip.h)
RED_SUM, RED_MAX, RED_MEAN = 0, 1, 2
RED_SUM_ACCUM = 3  # out += sum, each row's chain continued from out (include/dgl_hip.h)
RED_MEAN_ACCUM = 4  # out = out + mean (include/dgl_hip.h)
_ACCUM = (RED_SUM_ACCUM, RED_MEAN_ACCUM)
ORDER_EID, ORDER_COL = 0, 1
# edge values laid out in the forward CSR's slot order (edge_order="slot"):
# kernels read / write slot k at row k, no eid indirection
SLOT = "slot"

_MSG_NAMES = {"copy_src": MSG_COPY_U, "copy_u": MSG_COPY_U, "src_mul_edge": MSG_U_MUL_E,
              "u_mul_e": MSG_U_MUL_E, "copy_edge": MSG_COPY_E, "copy_e": MSG_COPY_E}
_RED_NAMES = {"sum": RED_SUM, "max": RED_MAX, "mean": RED_MEAN}


# ---------------------------------------------------------------------------
# Schedule policy: the native launch plan's (dglhip_spmm_get_policy /
# dglhip_spmm_set_policy, include/dgl_hip.h). One policy serves the engine's
# own operators and every C-ABI / PackedFunc caller of the plan.
#
# Heavy-row policy ("row_split") of the sum / mean kernels, sized from the
# device: R = the headline kernel's resident waves
# (dglhip_gspmm_resident_waves: compute units x waves per CU at its occupancy;
# MI355X 256 x 28 = 7,168).
#   "auto" : (default) a row is one wave's sequential chain, a launch spreads
#            its slots over the R resident waves and rows start longest-first,
#            so a row longer than twice a wave's share (nnz / (R / 2) slots)
#            outlasts the rest of the launch. Only then — and only for rows
#            longer than 16,384 slots (~1.5 ms of chained gathers), below which
#            the loss is bounded and every row stays one exact chain — are the
#            rows longer than max(4096, (7168 / 12000) x nnz / R) slots (nnz /
#            12,000 on MI355X) cut into chunks, sized to spread their slots
#            over 4R/7 waves (4,096 on MI355X). A floor of 65,536 left the
#            60k-slot hub rows of RMAT-26's pipelined segments at 1/8 unsplit:
#            13.2 -> 24.3 ms per step (bench.py --emulate-world 8 --workload rmat).
#            RMAT-26 (max in-degree ~855k, 2.9x the share) is split: GraphSAGE-
#            mean epoch 0.693 -> 0.640 s (profiles/r02/graphsage_rmat26_row_split.log);
#            Reddit (max 21,657 <= 114.8M / 3584 = 32,045) is not, and stays
#            bit-exact. A part with fewer resident waves has a longer share per
#            wave and splits less.
#   "off"  : every row is one sequential chain — bit-exact with the reference
#            on every graph (the documented bit-exact switch)
#   <int>  : explicit chunk length, applied whenever some row is longer
# (DGLHIP_ROW_SPLIT sets it from the environment.)
# ---------------------------------------------------------------------------
_REF_WAVES = 7168       # MI355X (and the host path, which never splits)
_WAVES = {}


class _Policy(ctypes.Structure):
    _fields_ = [("row_split", ctypes.c_int64), ("blocked", ctypes.c_int32),
                ("short_rows", ctypes.c_int32), ("pad_rows", ctypes.c_int32),
                ("items_per_wave", ctypes.c_int32), ("block_bytes", ctypes.c_int64),
                ("block_table_min", ctypes.c_int64), ("block_table_max", ctypes.c_int64),
                ("block_min_slots", ctypes.c_int64), ("block_max_stretch", ctypes.c_double),
                ("block_max_suffix", ctypes.c_double), ("block_min_row_bytes", ctypes.c_int64),
                ("tier_min_rows", ctypes.c_int64), ("pad_min_bytes", ctypes.c_int64),
                ("column_parts", ctypes.c_int32), ("ids_wide", ctypes.c_int32)]


_POLICY_KEYS = tuple(n for n, _ in _Policy._fields_)
# bumped at every policy change: part of the keys of the Python-side caches
# of native plan structures (a new policy may give a CSR another schedule)
_POLICY_GEN = [0]


def schedule_policy():
    """The g-SpMM schedule policy as a dict (row_split -1 auto / 0 off / a
    chunk length, blocked, short_rows, pad_rows, items_per_wave (1 or 2: the
    blocked schedule's items a wave takes), block_bytes, block_table_min,
    block_table_max, block_min_slots, block_max_stretch, block_max_suffix,
    block_min_row_bytes, tier_min_rows, pad_min_bytes, column_parts (1, or 2:
    those launches over column halves, one half per XCD), ids_wide (0: the
    column halves read 16-bit ids local to the launch's source block where a
    block has at most 65,536 rows, 1: always int32 ids))."""
    p = _Policy()
    check_call(LIB.dglhip_spmm_get_policy(ctypes.addressof(p)))
    return {k: getattr(p, k) for k in _POLICY_KEYS}


def set_schedule_policy(**changes):
    """Change fields of the schedule policy; returns the old policy (a dict
    that set_schedule_policy(**old) restores)."""
    p = _Policy()
    check_call(LIB.dglhip_spmm_get_policy(ctypes.addressof(p)))
    old = {k: getattr(p, k) for k in _POLICY_KEYS}
    for k, v in changes.items():
        if k not in _POLICY_KEYS:
            raise DGLError("unknown schedule policy field %r" % (k,))
        setattr(p, k, v)
    check_call(LIB.dglhip_spmm_set_policy(ctypes.addressof(p)))
    _POLICY_GEN[0] += 1
    return old


@contextlib.contextmanager
def scheduled(**changes):
    """Context manager: the schedule policy with ``changes`` for its body."""
    old = set_schedule_policy(**changes)
    try:
        yield
    finally:
        set_schedule_policy(**old)


def sweep_schedule():
    """The source-sweep schedule's knobs (DESIGN.md §4.1 "Source sweep"):
    {"on", "table_min", "block_bytes", "lag", "max_spin", "accum_table_min",
    "accum_min_slots", "accum_per_cu"}."""
    on, lag, spin, apc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    tmin, bb, atm, ams = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    check_call(LIB.dglhip_get_sweep_schedule(ctypes.byref(on), ctypes.byref(tmin),
                                             ctypes.byref(bb), ctypes.byref(lag),
                                             ctypes.byref(spin), ctypes.byref(atm),
                                             ctypes.byref(ams), ctypes.byref(apc)))
    return {"on": bool(on.value), "table_min": tmin.value, "block_bytes": bb.value,
            "lag": lag.value, "max_spin": spin.value, "accum_table_min": atm.value,
            "accum_min_slots": ams.value, "accum_per_cu": apc.value}


def sweep_barrier_expiries(reset=False):
    """Waits of the accumulating sweep's soft barrier that ran out of polls
    (max_spin) on the current device since the last reset (a synchronous read;
    ``reset`` zeroes the count after reading). Results never depend on them."""
    v = ctypes.c_int64()
    check_call(LIB.dglhip_sweep_barrier_expiries(1 if reset else 0, ctypes.byref(v)))
    return int(v.value)


def sweep_fallbacks(reset=False):
    """Runs the plan routed to the sweep that took the sweep-off schedule
    instead because ``ufeat`` or ``out`` was not 8-byte aligned (a view at an
    odd float offset of its storage), since the last reset."""
    v = ctypes.c_int64()
    check_call(LIB.dglhip_sweep_fallbacks(1 if reset else 0, ctypes.byref(v)))
    return int(v.value)


def set_sweep_schedule(**changes):
    """Change the source-sweep knobs; returns the old ones (for restoring).
    A plan keeps the sweep layouts it built; the choice is made per call."""
    old = sweep_schedule()
    new = dict(old, **changes)
    unknown = set(changes) - set(old)
    if unknown:
        raise DGLError("unknown sweep knobs: %s" % sorted(unknown))
    check_call(LIB.dglhip_set_sweep_schedule(int(bool(new["on"])), int(new["table_min"]),
                                             int(new["block_bytes"]), int(new["lag"]),
                                             int(new["max_spin"]), int(new["accum_table_min"]),
                                             int(new["accum_min_slots"]),
                                             int(new["accum_per_cu"])))
    return old


def _resident_waves(device=None):
    """R: the headline g-SpMM kernel's resident waves on ``device`` (queried
    once per device from the library); _REF_WAVES for host / unknown devices."""
    if device is None or torch.device(device).type != "cuda":
        return _REF_WAVES
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _WAVES:
        w = ctypes.c_int64()
        check_call(LIB.dglhip_gspmm_resident_waves(idx, ctypes.byref(w)))
        _WAVES[idx] = int(w.value)
    return _WAVES[idx]


def _row_split_name(v):
    return "auto" if v < 0 else ("off" if v == 0 else str(v))


def get_row_split():
    """The heavy-row policy: "auto", "off" or a chunk length (as a string)."""
    return _row_split_name(schedule_policy()["row_split"])


def set_row_split(policy):
    """Set the heavy-row policy ("auto", "off" or a chunk length); returns the old one."""
    pol = str(policy)
    if pol == "auto":
        v = -1
    elif pol in ("off", "0", "", "none", "None"):
        v = 0
    else:
        v = int(pol)
    return _row_split_name(set_schedule_policy(row_split=v)["row_split"])


def _split_threshold(csr, waves=None):
    """Rows longer than this many slots are chunked (0: none), for a launch
    over ``csr`` on a part with ``waves`` resident waves (None: csr's device):
    the native plan's gate (dglhip_spmm_split_threshold)."""
    R = waves if waves is not None else _resident_waves(getattr(csr, "device", None))
    t = ctypes.c_int64()
    check_call(LIB.dglhip_spmm_split_threshold(int(csr.nnz), int(csr.max_degree), int(R),
                                               ctypes.byref(t)))
    return int(t.value)


def set_short_rows(on):
    """Route short / empty rows to the batched short-row kernel (default on);
    returns the old setting."""
    return bool(set_schedule_policy(short_rows=1 if on else 0)["short_rows"])


def set_blocked(policy):
    """Source-blocked schedule for copy_u / u_mul_e with sum / mean / max and
    the fused GAT layer: "auto" (default: where it keeps the chains
    bit-identical and the table size pays) or "off". Returns the old
    policy."""
    old = set_schedule_policy(blocked=0 if str(policy) == "off" else 1)
    return "auto" if old["blocked"] else "off"


def set_pad_rows(policy):
    """Padded-stride gathers for line-straddling rows: "auto" (default) or
    "off"; returns the old policy."""
    old = set_schedule_policy(pad_rows=1 if str(policy) == "auto" else 0)
    return "auto" if old["pad_rows"] else "off"
