"""The GAT kernels against a float64 reference at every head shape.

kernel.gat_aggregate (csrc/gat_fused.hip, the attention-gradient epilogue of
the g-SDDMM in csrc/gspmm.hip, rowsum_heads8_kernel, the dispatch in
kernel._GATAggregate / _gat_backward_t) and the host path are compared with
gat_reference.gat_reference64: plain float64 torch on the CPU, leaky_relu's
own backward. Per element

    |got - ref| <= (L + Dg + 16) * 2^-24 * S + 1e-30,   exactly 0 where S == 0

(gat_reference.py: S the element's condition scale, L its chain length, Dg
the head width for d_el / d_er). The bound is derived, not measured, and for
short rows it is far tighter than 1e-5 * S. With rows and sources of at most
129 slots L + Dg + 16 <= 161 (9.6e-6 * S, inside the project's 1e-5 of the
condition scale) for fs, z, d_ft and for d_el / d_er at heads of up to 16
features; only d_el / d_er at the wide heads 1 x 128, 4 x 32, 3 x 40 and
5 x 40 on the longest rows and sources go past it, up to 273 * 2^-24 =
1.6e-5 * S at 1 x 128: the formula's D-term dot, not a widened allowance.

Inputs: a graph of about 400 sources and 3,000 edges whose designated rows
and sources carry degrees 0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127,
128, 129 (square, rectangular 70 x 300 and 300 x 70, and with 20 feature rows
more than the adjacency has columns); el, er and ft on the dyadic grid of
multiples of 1/8 in [-2, 2], so the logits are exact in float32, exact zeros
occur, and no pair lies within 1e-3 of a clamp bound: the clamp gate is the
same set in float32 and float64. Head shapes cover every kernel: the LDS kernel on
one-float lanes (8x8, 16x4, 8x3, 2x5, 1x1), two-float lanes (1x128, 4x32,
8x16 with the one-pass transposed backward), the per-lane kernel for head
counts outside {1, 2, 4, 8, 16} (3x5, 12x8), heads straddling a 64-lane pass
(3x40, 5x40) and 32 heads (the sliced epilogue <4, ., 32>).
"""
import numpy as np
import pytest
import torch

from dgl import kernel
from gat_reference import (HUB_DEGREES, assert_within, check_all, dyadic,
                           edge_graph as _edge_graph, gat_reference64 as _gat_reference64)

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
SHAPES = [(8, 16), (8, 8), (16, 4), (8, 3), (2, 5), (1, 1), (1, 128), (4, 32), (32, 4), (3, 5),
          (12, 8), (3, 40), (5, 40)]
LDS_SHAPES = [s for s in SHAPES if s[0] in (1, 2, 4, 8, 16)]
ALPHA = 0.2
SEED = 20240
# (R, N, extra feature rows)
VARIANTS = {"square": (400, 400, 0), "rect": (70, 300, 0), "extra": (400, 400, 20),
            "tall": (300, 70, 0)}
EXP_CLAMP = (-10.0, 10.0)
NOEXP_CLAMP = (-0.33, 1.3)  # off the grid of leaky_relu values (multiples of 1/8 and of 1/40)
NO_CLAMP = (-float("inf"), float("inf"))


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


_ADJ = {}


def _adjacency(variant, order, dev):
    """(graph, SparseAdj on dev, src / dst in forward-slot order)."""
    R, N, _ = VARIANTS[variant]
    g = _edge_graph(R, N, 7, order)
    key = (variant, order, str(dev))
    if key not in _ADJ:
        adj = kernel.from_coo(R, N, torch.from_numpy(g.dst), torch.from_numpy(g.src),
                              kernel.ORDER_EID, dev)
        _ADJ[key] = (adj, adj.fwd.indices.long().cpu(), adj.fwd.row_ids().cpu())
    return (g,) + _ADJ[key]


def _values(variant, H, D, seed=3):
    """ft, el, er on the dyadic grid; dout, dz standard normal (host float32).
    The one pair of hub row 1 (in-degree 1) is clamped at every head under
    (-10, 10) with exp: a row whose d_er has condition scale 0."""
    R, N, extra = VARIANTS[variant]
    gen = torch.Generator().manual_seed(seed + 1000 * H + D)
    ft = dyadic((N + extra, H, D), gen)
    el = dyadic((N + extra, H), gen)
    er = dyadic((R, H), gen)
    g = _edge_graph(R, N, 7, "shuffled")
    u = int(g.src[g.dst == 1][0])
    el[u] = 2.0
    er[1] = 2.0
    dout = torch.randn(R, H, D, generator=gen)
    dz = torch.randn(R, H, 1, generator=gen)
    return ft, el, er, dout, dz


def _ctx(t):
    """The _GATAggregate node behind an output (through the reshaping view)."""
    fn = t.grad_fn
    while not hasattr(fn, "use_t"):
        fn = fn.next_functions[0][0]
    return fn


def _clamp_of(apply_exp, clamp):
    if clamp == "none":
        return NO_CLAMP
    return EXP_CLAMP if apply_exp else NOEXP_CLAMP


def _reference(adjt, vals, clamp, apply_exp, p, use_fs=True, use_z=True):
    g, adj, u, v = adjt
    ft, el, er, dout, dz = vals
    E, H = u.numel(), el.shape[1]
    keep = kernel.gat_dropout_mask(E, H, p, SEED) if p > 0 else None
    return _gat_reference64(u, v, g.R, g.N, ft, el, er, ALPHA, clamp[0], clamp[1], apply_exp,
                            keep, p, dout if use_fs else None, dz if use_z else None)


def _run(adj, vals, dev, clamp, apply_exp, p, req=(True, True, True), use_fs=True, use_z=True):
    """gat_aggregate and its gradients on ``dev``: (fs, z, d_ft, d_el, d_er),
    None for an input that does not require grad."""
    ft, el, er, dout, dz = (t.to(dev) for t in vals)
    ft, el, er = (t.clone().requires_grad_(r) for t, r in zip((ft, el, er), req))
    fs, z = kernel.gat_aggregate(adj, ft, el, er, ALPHA, clamp=clamp, attn_drop=p,
                                 apply_exp=apply_exp, seed=SEED)
    outs = [o for o, used in ((fs, use_fs), (z, use_z)) if used]
    gouts = [o for o, used in ((dout, use_fs), (dz, use_z)) if used]
    torch.autograd.backward(outs, gouts)
    return fs.detach(), z.detach(), ft.grad, el.grad, er.grad


def test_comparator_rejects_what_it_must():
    """assert_within itself, on the host: a value at the bound passes; one
    just outside it, a NaN, an infinity (with S > 0 or S == 0) and a nonzero
    where S == 0 each raise, also under a row restriction."""
    ref = torch.tensor([[1.0, -2.0], [0.0, 0.5], [3.0, 0.0]], dtype=torch.float64)
    S = torch.tensor([[1.0, 2.0], [0.0, 0.5], [4.0, 0.0]], dtype=torch.float64)
    L = torch.tensor([0, 3, 129])
    u = 2.0 ** -24
    at = ref.clone()
    at[0, 0] += 16 * u * 1.0          # L 0: exactly the allowance
    at[2, 0] -= (129 + 16) * u * 4.0
    assert_within(at, ref, S, L, 0, "self")
    assert_within(ref.float(), ref, S, L, 5, "self")

    def raises(got, rows=None, Dg=0):
        with pytest.raises(AssertionError):
            assert_within(got, ref, S, L, Dg, "self", rows)
    out = at.clone()
    out[0, 0] += 2 * u                # just outside
    raises(out)
    raises(out, rows=[0])
    assert_within(out, ref, S, L, 2, "self")  # (Dg counts)
    assert_within(out, ref, S, L, 0, "self", rows=[1, 2])
    for bad in (float("nan"), float("inf"), -float("inf")):
        for i, j in ((0, 1), (1, 0), (2, 1)):  # S > 0, S == 0, S == 0
            got = ref.clone()
            got[i, j] = bad
            raises(got)
            raises(got, rows=[i])
    got = ref.clone()
    got[1, 0] = 1e-40                 # S == 0: exactly 0 or nothing
    raises(got)
    got[1, 0] = -0.0
    assert_within(got, ref, S, L, 0, "self")


def test_graph_and_grid_hold_their_conditions():
    """The generator's promises, on the host: the hub rows' in-degrees and the
    hub sources' out-degrees are the designated ones, no other degree exceeds
    129 (8 on the square graph), parallel edges and self-loops exist, the
    edge ids differ from the slot order when shuffled and the sources ascend
    along every row when numbered source-major; about 8 % of the pairs are
    clamped at 10."""
    for variant, (R, N, _) in VARIANTS.items():
        for order in ("shuffled", "src"):
            g = _edge_graph(R, N, 7, order)
            indeg = np.bincount(g.dst, minlength=R)
            outdeg = np.bincount(g.src, minlength=N)
            assert tuple(indeg[g.hub_rows]) == HUB_DEGREES
            assert tuple(outdeg[g.hub_srcs]) == HUB_DEGREES
            rest_in = np.delete(indeg, g.hub_rows)
            rest_out = np.delete(outdeg, g.hub_srcs)
            cap = 8 if R == N else 129  # (few rows or few sources: the hubs' edges crowd them)
            assert rest_in.max() <= cap and rest_out.max() <= cap
            assert 2500 <= g.src.size <= 3500 or R != N
            pairs = g.src * R + g.dst
            assert np.unique(pairs).size < pairs.size  # parallel edges
            if R == N:
                assert bool((g.src == g.dst).any())
            adj = kernel.from_coo(R, N, torch.from_numpy(g.dst), torch.from_numpy(g.src),
                                  kernel.ORDER_EID, "cpu")
            eid = adj.fwd.eid
            if order == "shuffled":
                assert not torch.equal(eid, torch.arange(eid.numel()))
            else:
                ind, ip = adj.fwd.indices.numpy(), adj.fwd.indptr.numpy()
                for r in range(R):
                    assert (np.diff(ind[ip[r]:ip[r + 1]]) >= 0).all()
    adjt = _adjacency("square", "shuffled", torch.device("cpu"))
    ref = _reference(adjt, _values("square", 8, 16), EXP_CLAMP, True, 0.0)
    assert 0.05 <= 1.0 - ref["inside_share"] <= 0.12


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("clamp", ["finite", "none"])
@pytest.mark.parametrize("apply_exp", [True, False])
def test_forward(device, H, D, clamp, apply_exp):
    """fs and z at every head shape, with and without dropout, clamped and
    not, with and without exp; the same under torch.no_grad(), the path that
    stores nothing."""
    dev = _dev(device)
    adjt = _adjacency("square", "shuffled", dev)
    vals = _values("square", H, D)
    cl = _clamp_of(apply_exp, clamp)
    for p in (0.0, 0.5):
        ref = _reference(adjt, vals, cl, apply_exp, p)
        ft, el, er = (t.to(dev).clone().requires_grad_(True) for t in vals[:3])
        for grad in (True, False):
            with torch.set_grad_enabled(grad):
                fs, z = kernel.gat_aggregate(adjt[1], ft, el, er, ALPHA, clamp=cl, attn_drop=p,
                                             apply_exp=apply_exp, seed=SEED)
            assert (fs.grad_fn is not None) == grad
            assert fs.shape == (400, H, D) and z.shape == (400, H, 1)
            check_all(ref, fs=fs, z=z.reshape(-1, H), what="p=%g grad=%s" % (p, grad))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("order,bwd,apply_exp", [
    ("shuffled", "auto", True), ("shuffled", "three", True), ("src", "auto", True),
    ("src", "three", True), ("shuffled", "auto", False)])
def test_gradients(device, H, D, order, bwd, apply_exp):
    """All three gradients at every head shape, p in {0, 0.5}, on the shuffled
    and the source-major graph, through the automatic backward and the three
    passes (they differ only where the one-pass transposed kernel applies: 8
    heads x 16 on the device, asserted)."""
    dev = _dev(device)
    adjt = _adjacency("square", order, dev)
    vals = _values("square", H, D)
    cl = _clamp_of(apply_exp, "finite")
    old = kernel.set_gat_backward(bwd)
    try:
        for p in (0.0, 0.5):
            ref = _reference(adjt, vals, cl, apply_exp, p)
            ft, el, er = (t.to(dev).clone().requires_grad_(True) for t in vals[:3])
            fs, z = kernel.gat_aggregate(adjt[1], ft, el, er, ALPHA, clamp=cl, attn_drop=p,
                                         apply_exp=apply_exp, seed=SEED)
            want_t = (dev.type == "cuda" and bwd == "auto" and
                      kernel.LIB.dglhip_gat_backward_t_ok(H, D) == 1)
            assert want_t == (dev.type == "cuda" and bwd == "auto" and (H, D) == (8, 16))
            assert bool(_ctx(fs).use_t) == want_t
            torch.autograd.backward([fs, z], [vals[3].to(dev), vals[4].to(dev)])
            check_all(ref, fs=fs, z=z.reshape(-1, H), d_ft=ft.grad, d_el=el.grad, d_er=er.grad,
                      D=D, what="p=%g" % p)
    finally:
        kernel.set_gat_backward(old)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", [(8, 16), (8, 3)])
@pytest.mark.parametrize("bwd", ["auto", "three"])
def test_partial_backward(device, H, D, bwd):
    """Only ft, only el, only er requiring grad; only fs used (d_z is None:
    the transposed backward's unpacked entry); only z used (d_ft is None).
    The gradients that are asked for hold the bound, the others stay None."""
    dev = _dev(device)
    adjt = _adjacency("square", "shuffled", dev)
    vals = _values("square", H, D)
    p = 0.5
    old = kernel.set_gat_backward(bwd)
    try:
        for req in ((True, False, False), (False, True, False), (False, False, True)):
            ref = _reference(adjt, vals, EXP_CLAMP, True, p)
            _, _, d_ft, d_el, d_er = _run(adjt[1], vals, dev, EXP_CLAMP, True, p, req=req)
            for got, r in zip((d_ft, d_el, d_er), req):
                assert (got is not None) == r, req
            check_all(ref, d_ft=d_ft, d_el=d_el, d_er=d_er, D=D, what="requires_grad=%s" % (req,))
        for use_fs, use_z in ((True, False), (False, True)):
            ref = _reference(adjt, vals, EXP_CLAMP, True, p, use_fs=use_fs, use_z=use_z)
            fs, z, d_ft, d_el, d_er = _run(adjt[1], vals, dev, EXP_CLAMP, True, p, use_fs=use_fs,
                                           use_z=use_z)
            check_all(ref, fs=fs, z=z.reshape(-1, H), d_ft=d_ft, d_el=d_el, d_er=d_er, D=D,
                      what="fs used=%s z used=%s" % (use_fs, use_z))
    finally:
        kernel.set_gat_backward(old)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", [(8, 16), (8, 8), (3, 5)])
@pytest.mark.parametrize("variant", ["rect", "extra"])
@pytest.mark.parametrize("bwd", ["auto", "three"])
def test_rectangular_and_extra_rows(device, H, D, variant, bwd):
    """A rectangular adjacency (er with 70 rows, ft / el with 300) and
    operands with 20 rows more than the adjacency has columns: forward and
    gradients; the gradients have the operands' own row counts, the rows
    beyond the adjacency's columns exactly zero (their condition scale is 0)."""
    dev = _dev(device)
    R, N, extra = VARIANTS[variant]
    adjt = _adjacency(variant, "shuffled", dev)
    vals = _values(variant, H, D)
    old = kernel.set_gat_backward(bwd)
    try:
        for p in (0.0, 0.5):
            ref = _reference(adjt, vals, EXP_CLAMP, True, p)
            fs, z, d_ft, d_el, d_er = _run(adjt[1], vals, dev, EXP_CLAMP, True, p)
            assert fs.shape == (R, H, D) and z.shape == (R, H, 1)
            assert d_ft.shape == (N + extra, H, D) and d_el.shape == (N + extra, H)
            assert d_er.shape == (R, H)
            check_all(ref, fs=fs, z=z.reshape(-1, H), d_ft=d_ft, d_el=d_el, d_er=d_er, D=D,
                      what="%s p=%g" % (variant, p))
    finally:
        kernel.set_gat_backward(old)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", [(8, 16), (8, 3)])
@pytest.mark.parametrize("bwd", ["auto", "three"])
def test_only_z_used_with_more_rows_than_sources(device, H, D, bwd):
    """300 rows over 70 sources, only z used downstream: the zero gradient
    that stands in for fs's has the adjacency's row count (the backward reads
    it at every destination), and every gradient holds the bound."""
    dev = _dev(device)
    adjt = _adjacency("tall", "shuffled", dev)
    vals = _values("tall", H, D)
    old = kernel.set_gat_backward(bwd)
    try:
        for p in (0.0, 0.5):
            ref = _reference(adjt, vals, EXP_CLAMP, True, p, use_fs=False)
            fs, z, d_ft, d_el, d_er = _run(adjt[1], vals, dev, EXP_CLAMP, True, p, use_fs=False)
            check_all(ref, fs=fs, z=z.reshape(-1, H), d_ft=d_ft, d_el=d_el, d_er=d_er, D=D,
                      what="p=%g" % p)
    finally:
        kernel.set_gat_backward(old)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("msg", ["copy_u", "u_mul_e"])
def test_gspmm_extra_rows_gradient(device, msg):
    """gspmm with 20 node rows more than the adjacency has columns: the node
    gradient has the operand's row count, the extra rows zero."""
    dev = _dev(device)
    R, N, extra = VARIANTS["extra"]
    g, adj, u, v = _adjacency("extra", "shuffled", dev)
    gen = torch.Generator().manual_seed(5)
    x = dyadic((N + extra, 6), gen).to(dev).requires_grad_(True)
    e = dyadic((u.numel(), 1), gen).to(dev)
    dout = dyadic((R, 6), gen)
    out = kernel.gspmm(adj, msg, "sum", x, e if msg == "u_mul_e" else None, edge_order="slot")
    out.backward(dout.to(dev))
    w = e.cpu().double() if msg == "u_mul_e" else torch.ones(u.numel(), 1, dtype=torch.float64)
    ref = torch.zeros(N + extra, 6, dtype=torch.float64).index_add(0, u, w * dout.double()[v])
    assert x.grad.shape == (N + extra, 6)
    # dyadic values, at most 129 terms of at most 4: every partial sum is exact
    assert torch.equal(x.grad.cpu().double(), ref)
    assert bool((x.grad[N:] == 0).all())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("order", ["eid", "slot"])
@pytest.mark.parametrize("H", [4, 3])
def test_edge_attention_on_the_grid(device, order, H):
    """kernel.edge_attention (the vector kernel at 4 heads, the generic one at
    3) on the dyadic grid, a_src with 20 rows more than the adjacency has
    columns: the attention within 16 * 2^-24 of its value (one term: L = 0),
    both gradients within the bound, a_src's with the operand's rows."""
    dev = _dev(device)
    R, N, extra = VARIANTS["extra"]
    g, adj, u, v = _adjacency("extra", "shuffled", dev)
    if order == "eid":
        u, v = torch.from_numpy(g.src), torch.from_numpy(g.dst)
    E = u.numel()
    gen = torch.Generator().manual_seed(17 + H)
    el, er = dyadic((N + extra, H), gen), dyadic((R, H), gen)
    W = torch.randn(E, H, generator=gen)
    a_src, a_dst = (t.to(dev).clone().requires_grad_(True) for t in (el, er))
    a = kernel.edge_attention(adj, a_src, a_dst, E, ALPHA, clamp=EXP_CLAMP, edge_order=order)
    (a * W.to(dev)).sum().backward()
    el64, er64 = (t.double().requires_grad_(True) for t in (el, er))
    x = el64[u] + er64[v]
    pre = torch.exp(torch.nn.functional.leaky_relu(x, ALPHA))
    assert bool(((pre - 10.0).abs() > 1e-2).all())
    a64 = pre.clamp(*EXP_CLAMP)
    (a64 * W.double()).sum().backward()
    none = torch.zeros(E, dtype=torch.int64)
    assert_within(a, a64.detach(), a64.detach().abs(), none, 0, "attention")
    with torch.no_grad():
        slope = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, ALPHA))
        S_g = (pre < 10.0).double() * slope * a64 * W.double().abs()
    assert a_src.grad.shape == (N + extra, H)
    for got, ref, idx, name in ((a_src.grad, el64.grad, u, "d_src"), (a_dst.grad, er64.grad, v,
                                                                       "d_dst")):
        n = ref.shape[0]
        S = torch.zeros(n, H, dtype=torch.float64).index_add(0, idx, S_g)
        assert_within(got, ref, S, torch.bincount(idx, minlength=n), 0, name)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(8, 16), (8, 8), (1, 128), (3, 5)])
@pytest.mark.parametrize("bwd", ["auto", "three"])
def test_source_blocked_small(monkeypatch, H, D, bwd):
    """The source-blocked schedule at small scale (blocks of a quarter of the
    400 sources): the forward runs over at least 3 row ranges, the transposed
    backward over at least 2 launches; outputs and gradients hold the bound
    and equal the one-launch schedule's bit for bit."""
    dev = _dev("cuda")
    adjt = _adjacency("square", "src", dev)
    adj = adjt[1]
    vals = _values("square", H, D)
    F = H * D
    monkeypatch.setattr(kernel.plan, "_GAT_BLOCK_BYTES", (F + H) * 4 * 100)
    monkeypatch.setattr(kernel.plan, "_GAT_BLOCK_BYTES_NOGRAD", (F + H) * 4 * 100)
    monkeypatch.setattr(kernel.plan, "_GAT_BWD_BLOCK_BYTES", F * 4 * 100)
    p = 0.5
    ref = _reference(adjt, vals, EXP_CLAMP, True, p)
    old = kernel.set_gat_backward(bwd)
    try:
        with kernel.scheduled(block_table_min=0, block_min_slots=1, block_min_row_bytes=0,
                              block_bytes=F * 4 * 100):
            cuts = kernel._block_cuts(adj.fwd, (F + H) * 4)
            assert cuts is not None and len(cuts) - 1 >= 3
            plan = kernel._block_plan(adj.bwd, vals[3].to(dev).view(-1, F), F,
                                      kernel._GAT_BWD_BLOCK_BYTES)
            assert plan is not None and len(plan) >= 2
            blocked = _run(adj, vals, dev, EXP_CLAMP, True, p)
            with torch.no_grad():
                fs_ng, z_ng = kernel.gat_aggregate(
                    adj, vals[0].to(dev), vals[1].to(dev), vals[2].to(dev), ALPHA,
                    clamp=EXP_CLAMP, attn_drop=p, seed=SEED)
            old_b = kernel.set_blocked("off")
            try:
                assert kernel._block_cuts(adj.fwd, (F + H) * 4) is None
                single = _run(adj, vals, dev, EXP_CLAMP, True, p)
            finally:
                kernel.set_blocked(old_b)
    finally:
        kernel.set_gat_backward(old)
    fs, z, d_ft, d_el, d_er = blocked
    check_all(ref, fs=fs, z=z.reshape(-1, H), d_ft=d_ft, d_el=d_el, d_er=d_er, D=D, what="blocked")
    for a, b, name in zip(blocked, single, ("fs", "z", "d_ft", "d_el", "d_er")):
        assert torch.equal(a, b), name
    assert torch.equal(fs_ng, fs) and torch.equal(z_ng, z)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", LDS_SHAPES)
def test_kernel_variants_small(H, D):
    """Fused-kernel variants 1, 2, 3 (per-lane attention, LDS attention with
    the rows gathered after / before it) give variant 0's bits, outputs and
    gradients, on the small graph whose rows end at every batch edge; variant
    0 holds the bound."""
    dev = _dev("cuda")
    adjt = _adjacency("square", "shuffled", dev)
    vals = _values("square", H, D)
    p = 0.5
    outs = {}
    try:
        for variant in (0, 1, 2, 3):
            kernel.set_gat_variant(variant)
            outs[variant] = _run(adjt[1], vals, dev, EXP_CLAMP, True, p)
    finally:
        kernel.set_gat_variant(0)
    fs, z, d_ft, d_el, d_er = outs[0]
    check_all(_reference(adjt, vals, EXP_CLAMP, True, p), fs=fs, z=z.reshape(-1, H), d_ft=d_ft,
              d_el=d_el, d_er=d_er, D=D, what="variant 0")
    for variant in (1, 2, 3):
        for a, b, name in zip(outs[variant], outs[0], ("fs", "z", "d_ft", "d_el", "d_er")):
            assert torch.equal(a, b), "variant %d: %s" % (variant, name)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", [(8, 16), (8, 8)])
@pytest.mark.parametrize("bwd", ["auto", "three"])
def test_row_length_edges(device, H, D, bwd):
    """The hub row and the hub source of each designated length on their own
    (the comparison restricted to them): a failure names the batch edge."""
    dev = _dev(device)
    adjt = _adjacency("square", "shuffled", dev)
    g = adjt[0]
    vals = _values("square", H, D)
    old = kernel.set_gat_backward(bwd)
    try:
        for p in (0.0, 0.5):
            ref = _reference(adjt, vals, EXP_CLAMP, True, p)
            fs, z, d_ft, d_el, d_er = _run(adjt[1], vals, dev, EXP_CLAMP, True, p)
            for i, deg in enumerate(HUB_DEGREES):
                row, s = [int(g.hub_rows[i])], [int(g.hub_srcs[i])]
                assert int(ref["L_in"][row[0]]) == deg and int(ref["L_out"][s[0]]) == deg
                check_all(ref, fs=fs, z=z.reshape(-1, H), d_ft=d_ft, d_el=d_el, d_er=d_er, D=D,
                          what="at length %d, p=%g" % (deg, p), rows=row, srcs=s)
    finally:
        kernel.set_gat_backward(old)
