"""Sparse adjacency objects and the g-SpMM / g-SDDMM operators.

This package is the engine's replacement for what the reference delegates to
the tensor framework:

* ``F.sparse_matrix`` + ``F.spmm`` = ``torch.sparse_coo_tensor`` +
  ``torch.sparse.mm`` (python/dgl/backend/pytorch/tensor.py:45-51,145-146),
  driven by SPMVExecutor / SPMVWithDataExecutor
  (python/dgl/runtime/ir/executor.py:452-473,535-566);
* the adjacency index built by ``Graph::GetAdj`` (src/graph/graph.cc:506-554)
  and copied to the device on first use (python/dgl/graph_index.py:575-579).

A :class:`SparseAdj` holds a destination-major CSR (rows = reduce targets)
plus, built lazily, the source-major CSR of the transpose used by the
backward. Slot order within a row is the order in which torch's CPU sparse
product consumes the reference's uncoalesced COO (edge-id order for mutable
graphs), so the HIP kernels reproduce the reference's results bit for bit.

Every compute call goes to libdgl_hip.so (HIP kernels for tensors on a ROCm
device, the library's host kernels for CPU tensors). There is no other path.
Each CSR's schedules (the source-blocked plan, the heavy-row split, the
short-row tiers) live in its native launch plan (csrc/spmm_plan.*,
dglhip_spmm_plan_*): the package passes tensors to it and wraps what it
hands back, so the C-ABI and these operators run one schedule choice.

One module per operator family, imported one way, policy -> plan -> csr ->
spmm -> {rgcn, gat, segment}: ``policy`` (constants, the schedule policy),
``plan`` (the views of the native launch plan), ``csr`` (CSR, SparseAdj and
their builders), ``spmm`` (g-SpMM / g-SDDMM, call timing), ``rgcn``
(gather_rows, DistMult, the typed-block operator), ``gat`` (edge attention,
the fused GAT layer, the edge softmax), ``segment`` (the segment reduction). This file only
re-exports them, so callers keep ``kernel.<name>``.

A setting that is rebound after import lives in one module, which reads it at
call time: write it there (``kernel.plan._GAT_BLOCK_BYTES = n``). Reading
``kernel.<setting>`` forwards to the owner (``__getattr__`` below); assigning
to it here would only shadow the owner's value.
"""
from __future__ import absolute_import

import torch  # noqa: F401

from .._ffi import LIB, check_call, ptr, stream_of as _stream_of  # noqa: F401
from ..base import DGLError  # noqa: F401
# graph_index, the tools and the tests reach the device graph builders as kernel.<name>
from ..device_graph import (  # noqa: F401
    SUBGRAPH_CHUNK, LINE_GRAPH_TILE, TRAVERSAL_CHUNK, SAMPLE_REG_SLOTS, SAMPLE_LDS_SLOTS,
    BUCKET_CHUNK, _workspace,
    induced_subgraph_count, induced_subgraph_fill, induced_subgraph,
    line_graph_count, line_graph_fill, line_graph,
    DegreeBuckets, degree_buckets_count, degree_buckets_fill, degree_buckets,
    bfs_frontiers, topological_frontiers, sample_mix, neighbor_sample)
from . import plan, spmm, rgcn, gat
from .policy import (  # noqa: F401
    MSG_COPY_U, MSG_U_MUL_E, MSG_COPY_E, MSG_COPY_U_BF16, RED_SUM, RED_MAX, RED_MEAN,
    RED_SUM_ACCUM, RED_MEAN_ACCUM, ORDER_EID, ORDER_COL, SLOT, _MSG_NAMES, _RED_NAMES,
    _REF_WAVES, _Policy, schedule_policy, set_schedule_policy, scheduled, sweep_schedule,
    sweep_barrier_expiries, sweep_fallbacks, set_sweep_schedule, _resident_waves,
    get_row_split, set_row_split, _split_threshold, set_short_rows, set_blocked, set_pad_rows)
from .plan import (  # noqa: F401
    PLAN_PATH_HOST, PLAN_PATH_ROWS, PLAN_PATH_BLOCKED, PLAN_PATH_MAX_BLOCKED, PLAN_PATH_SWEEP,
    _NativePlan, _block_plan, _block_items, _column_span, _cuts_native, _block_cuts,
    _block_slots, _block_edge_rows)
from .csr import CSR, SparseAdj, _upload, build_csr, coo_of, from_coo  # noqa: F401
from .spmm import (  # noqa: F401
    _edge_len, _run_gspmm, padded_width, _pad_rows, blocked_schedule, segment_blocks,
    _run_sddmm_dot, _fwd_slot_of_bwd, edge_order_of, slot_permutation, _eid_major,
    _row_strided, _mean_scaled, gspmm, gspmm_mean_add, gsddmm_dot, gspmm_into, gspmm_ranges,
    timing_enable, timing_read)
from .rgcn import (  # noqa: F401
    TYPED_CHUNK, gather_rows, set_typed_block_width, _position_groups_items,
    _position_groups, _DistMult, distmult_score, distmult_link_loss, set_validate_indices,
    _typed_items, set_typed_block_messages, _typed_msg_ok, _run_typed_msg, _RelationGroups,
    _typed_scale_fused, typed_block_spmm)
from .gat import (  # noqa: F401
    edge_attention, set_gat_backward, set_gat_variant, gat_dropout_scale, gat_dropout_mask,
    _GATAggregate, _gat_el_grad, gat_aggregate, gat_logits, _logits_source,
    EDGE_SOFTMAX_CHUNK, edge_softmax, segment_softmax)
from .segment import SEGMENT_CHUNK, SegmentOffsets, segment_reduce  # noqa: F401

__all__ = ["CSR", "SparseAdj", "build_csr", "gspmm", "gsddmm_dot",
           "MSG_COPY_U", "MSG_U_MUL_E", "MSG_COPY_E", "RED_SUM", "RED_MAX", "RED_MEAN"]

# the settings rebound after import, by owner: never copied into this namespace
_SETTINGS = {"_GAT_BLOCK_BYTES": plan, "_GAT_BLOCK_BYTES_NOGRAD": plan,
             "_GAT_BWD_BLOCK_BYTES": plan, "_EL_GRAD_BLOCK_BYTES": plan,
             "_GAT_BWD": gat, "_VALIDATE_INDICES": rgcn, "_CALL_EVENTS": spmm}


def __getattr__(name):
    owner = _SETTINGS.get(name)
    if owner is None:
        raise AttributeError("module %r has no attribute %r" % (__name__, name))
    return getattr(owner, name)
