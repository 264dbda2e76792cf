"""dgl.kernel as a package: the facade still answers every ``kernel.<name>``
its callers use with the owning module's object, a setting rebound on its
owner is what ``kernel.<name>`` and the code that consumes it see, and no
module of the package imports inside a function (the one-way import order
policy -> plan -> csr -> spmm -> {rgcn, gat, segment} needs no deferred
import). Host only.
"""
import ast
import glob
import os

import numpy as np
import pytest
import torch

import dgl._ffi
import dgl.base
import dgl.device_graph
from dgl import kernel
from dgl.kernel import csr, gat, plan, policy, rgcn, segment, spmm

# every kernel.<name> that bench.py, bench_models.py, examples/, tools/, tests/
# and the dgl package referenced when kernel.py was split (a grep, pasted),
# by the module that owns it
NAMES = {
    policy: (
        "MSG_COPY_U", "MSG_COPY_U_BF16", "MSG_U_MUL_E", "ORDER_COL", "ORDER_EID", "RED_MAX",
        "RED_MEAN", "RED_MEAN_ACCUM", "RED_SUM", "RED_SUM_ACCUM", "_MSG_NAMES", "_Policy",
        "_RED_NAMES", "_REF_WAVES", "_resident_waves", "_split_threshold", "get_row_split",
        "schedule_policy", "scheduled", "set_blocked", "set_pad_rows", "set_row_split",
        "set_schedule_policy", "set_short_rows", "set_sweep_schedule",
        "sweep_barrier_expiries", "sweep_fallbacks"),
    plan: (
        "PLAN_PATH_BLOCKED", "PLAN_PATH_MAX_BLOCKED", "PLAN_PATH_ROWS", "PLAN_PATH_SWEEP",
        "_EL_GRAD_BLOCK_BYTES", "_GAT_BLOCK_BYTES", "_GAT_BLOCK_BYTES_NOGRAD",
        "_GAT_BWD_BLOCK_BYTES", "_block_cuts", "_block_edge_rows", "_block_items",
        "_block_plan", "_block_slots", "_column_span"),
    csr: ("CSR", "SparseAdj", "_upload", "build_csr", "coo_of", "from_coo"),
    spmm: (
        "_edge_len", "_eid_major", "_mean_scaled", "_pad_rows", "_row_strided", "_run_gspmm",
        "_run_sddmm_dot", "blocked_schedule", "gsddmm_dot", "gspmm", "gspmm_into",
        "gspmm_mean_add", "padded_width", "segment_blocks", "slot_permutation",
        "timing_enable", "timing_read"),
    rgcn: (
        "TYPED_CHUNK", "_DistMult", "_RelationGroups", "_position_groups",
        "_position_groups_items", "_run_typed_msg", "_typed_items", "_typed_msg_ok",
        "_typed_scale_fused", "distmult_link_loss", "distmult_score", "gather_rows",
        "set_typed_block_messages", "set_typed_block_width", "set_validate_indices",
        "typed_block_spmm"),
    gat: (
        "_GATAggregate", "_GAT_BWD", "_gat_el_grad", "_logits_source", "edge_attention",
        "gat_aggregate", "gat_dropout_mask", "gat_dropout_scale", "gat_logits",
        "set_gat_backward", "set_gat_variant"),
    segment: ("SEGMENT_CHUNK", "SegmentOffsets", "segment_reduce"),
    dgl.device_graph: (
        "BUCKET_CHUNK", "LINE_GRAPH_TILE", "SAMPLE_LDS_SLOTS", "SAMPLE_REG_SLOTS",
        "SUBGRAPH_CHUNK", "TRAVERSAL_CHUNK", "bfs_frontiers", "degree_buckets",
        "degree_buckets_count", "degree_buckets_fill", "induced_subgraph",
        "induced_subgraph_count", "line_graph", "line_graph_count", "line_graph_fill",
        "neighbor_sample", "sample_mix", "topological_frontiers"),
    dgl._ffi: ("LIB", "check_call", "ptr"),
    dgl.base: ("DGLError",),
}

# the settings rebound after import, and the module that owns each
SETTINGS = (
    (plan, "_GAT_BLOCK_BYTES"), (plan, "_GAT_BLOCK_BYTES_NOGRAD"),
    (plan, "_GAT_BWD_BLOCK_BYTES"), (plan, "_EL_GRAD_BLOCK_BYTES"),
    (gat, "_GAT_BWD"), (rgcn, "_VALIDATE_INDICES"), (spmm, "_CALL_EVENTS"))


def test_every_name_resolves_to_its_owner():
    for owner, names in NAMES.items():
        for name in names:
            assert getattr(kernel, name) is getattr(owner, name), name
    assert kernel._stream_of is dgl._ffi.stream_of
    assert kernel.torch is torch


@pytest.mark.parametrize("owner,name", SETTINGS, ids=[n for _, n in SETTINGS])
def test_setting_rebound_on_owner_is_seen(monkeypatch, owner, name):
    assert name not in vars(kernel)  # forwarded, never copied
    assert getattr(kernel, name) is getattr(owner, name)
    new = object()
    monkeypatch.setattr(owner, name, new)
    assert getattr(kernel, name) is new


def test_gat_block_bytes_steers_block_cuts(monkeypatch):
    """_block_cuts' default block size is plan._GAT_BLOCK_BYTES, read at the
    call: 64 sources of 512 B in 8 KiB blocks are at least two ranges, in one
    block of the default size one range."""
    n, m, row_bytes = 64, 2048, 512
    rng = np.random.default_rng(0)
    src = np.sort(rng.integers(0, n, m))
    dst = rng.integers(0, n, m)
    a = kernel.build_csr(n, n, torch.from_numpy(dst), torch.from_numpy(src), kernel.ORDER_EID,
                         "cpu")
    with kernel.scheduled(block_table_min=0, block_min_slots=1, block_min_row_bytes=0):
        whole = kernel._block_cuts(a, row_bytes)
        monkeypatch.setattr(plan, "_GAT_BLOCK_BYTES", 16 * row_bytes)
        cut = kernel._block_cuts(a, row_bytes)
        assert kernel._block_cuts(a, row_bytes, None) is cut  # None: the same default
    assert cut is not None and len(cut) - 1 >= 2
    assert whole is None or len(whole) < len(cut)
    assert torch.equal(cut[0], a.indptr[:-1]) and torch.equal(cut[-1], a.indptr[1:])


def test_no_import_inside_a_function():
    files = sorted(glob.glob(os.path.join(os.path.dirname(kernel.__file__), "*.py")))
    assert len(files) == 8
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for fn in ast.walk(tree):
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                for node in ast.walk(fn):
                    assert not isinstance(node, (ast.Import, ast.ImportFrom)), \
                        "%s:%d imports inside %s" % (path, node.lineno,
                                                     getattr(fn, "name", "a lambda"))
