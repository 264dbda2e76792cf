"""The fused GAT aggregation (kernel.gat_aggregate, csrc/gat_fused.hip).

* kernel level: attention + weighted sum + normaliser in one kernel equal the
  three-kernel path (attention g-SDDMM in slot order, u_mul_e and copy_e
  g-SpMMs) bit for bit, forward and every gradient, over head shapes
  including Pubmed's (8 x 8, 8 x 3) and a Reddit-like row (8 x 16);
* dropout: the kernel's mask is the host hash (gat_dropout_mask), so the
  fused output equals the composition over that mask bit for bit, keeps
  about 1 - p of the pairs, and a fresh device counter draws a fresh mask;
* configs[2] at full size (Pubmed, 8 heads, -m gpu): per epoch, from the same
  parameters, the fused model's logits and gradients equal the three-kernel
  model's bit for bit and the reference UDF formulation's
  (examples/pytorch/gat/train.py:61-96) within 1e-5, dropout 0.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dgl
from conftest import load_example
from dgl import kernel
from gat_reference import assert_within, check_all, gat_reference64

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
# (32 x 4, 3 x 5, 3 x 40, 5 x 40, 12 x 8: head counts and widths only the
# per-lane kernel and the generic / 32-head epilogues run)
SHAPES = [(8, 8), (8, 3), (8, 16), (1, 128), (4, 32), (2, 5), (16, 4), (32, 4), (3, 5), (3, 40),
          (5, 40), (12, 8)]


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


def _graph(n=3000, m=40000, seed=0):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, m)
    # a few hub destinations: rows longer than one batch of slots in flight
    dst = np.where(rng.random(m) < 0.1, rng.integers(0, 5, m), rng.integers(0, n, m))
    g = dgl.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)))
    g.add_edges(g.nodes(), g.nodes())
    return g


def _inputs(n, H, D, dev, seed=1):
    gen = torch.Generator().manual_seed(seed)
    ft = torch.randn(n, H, D, generator=gen).to(dev).requires_grad_(True)
    el = torch.randn(n, H, generator=gen).to(dev).requires_grad_(True)
    er = torch.randn(n, H, generator=gen).to(dev).requires_grad_(True)
    return ft, el, er


def _unfused(adj, ft, el, er, alpha, clamp, E, keep=None, p=0.0):
    a = kernel.edge_attention(adj, el, er, E, alpha, clamp=clamp, edge_order="slot")
    w = a if keep is None else torch.where(keep, a * kernel.gat_dropout_scale(p),
                                           torch.zeros_like(a))
    fs = kernel.gspmm(adj, "u_mul_e", "sum", ft, w.unsqueeze(-1), edge_order="slot")
    z = kernel.gspmm(adj, "copy_e", "sum", None, a.unsqueeze(-1), edge_order="slot")
    return fs, z


def _grads(outs, ins, seed=2):
    gen = torch.Generator().manual_seed(seed)
    loss = sum((o * torch.randn(o.shape, generator=gen).to(o.device)).sum() for o in outs)
    return torch.autograd.grad(loss, ins)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", SHAPES)
@pytest.mark.parametrize("clamp", [(-10.0, 10.0), (-float("inf"), float("inf"))])
def test_fused_equals_three_kernels(device, H, D, clamp):
    dev = _dev(device)
    g = _graph()
    adj = g.sparse_adjacency(dev)
    ft, el, er = _inputs(g.number_of_nodes(), H, D, dev)
    fs, z = kernel.gat_aggregate(adj, ft, el, er, 0.2, clamp=clamp)
    fs2, z2 = _unfused(adj, ft, el, er, 0.2, clamp, g.number_of_edges())
    assert fs.shape == (g.number_of_nodes(), H, D) and z.shape == (g.number_of_nodes(), H, 1)
    assert torch.equal(fs, fs2) and torch.equal(z, z2)
    for a, b in zip(_grads((fs, z), (ft, el, er)), _grads((fs2, z2), (ft, el, er))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("device", DEVICES)
def test_fused_no_grad_and_partial_grads(device):
    dev = _dev(device)
    g = _graph(n=500, m=5000)
    adj = g.sparse_adjacency(dev)
    ft, el, er = _inputs(g.number_of_nodes(), 8, 8, dev)
    with torch.no_grad():
        fs, z = kernel.gat_aggregate(adj, ft, el, er)
    fs2, z2 = _unfused(adj, ft, el, er, 0.2, (-10.0, 10.0), g.number_of_edges())
    assert torch.equal(fs, fs2) and torch.equal(z, z2.detach())
    # only z used downstream, only ft requiring grad
    ft2 = ft.detach().requires_grad_(True)
    fs, z = kernel.gat_aggregate(adj, ft2, el.detach(), er.detach())
    (d,) = torch.autograd.grad(fs.sum(), ft2)
    fs3, _ = _unfused(adj, ft2, el.detach(), er.detach(), 0.2, (-10.0, 10.0),
                      g.number_of_edges())
    (d3,) = torch.autograd.grad(fs3.sum(), ft2)
    assert torch.equal(d, d3)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("p", [0.1, 0.6])
def test_dropout_mask_is_the_host_hash(device, p):
    dev = _dev(device)
    g = _graph()
    adj = g.sparse_adjacency(dev)
    H, D, E = 8, 8, g.number_of_edges()
    ft, el, er = _inputs(g.number_of_nodes(), H, D, dev)
    seed = 12345
    fs, z = kernel.gat_aggregate(adj, ft, el, er, 0.2, attn_drop=p, seed=seed)
    keep = kernel.gat_dropout_mask(E, H, p, seed).to(dev)
    assert abs(float(keep.float().mean()) - (1 - p)) < 0.01
    fs2, z2 = _unfused(adj, ft, el, er, 0.2, (-10.0, 10.0), E, keep=keep, p=p)
    assert torch.equal(fs, fs2) and torch.equal(z, z2)
    for a, b in zip(_grads((fs, z), (ft, el, er)), _grads((fs2, z2), (ft, el, er))):
        assert torch.equal(a, b)
    # eval mode: no dropout
    fs3, _ = kernel.gat_aggregate(adj, ft, el, er, 0.2, attn_drop=p, training=False)
    fs4, _ = _unfused(adj, ft, el, er, 0.2, (-10.0, 10.0), E)
    assert torch.equal(fs3, fs4)


@pytest.mark.parametrize("device", DEVICES)
def test_masks_fresh_per_call_and_repeat_with_manual_seed(device):
    """seed None: every call draws its seed from torch's generator, so calls
    get fresh masks and torch.manual_seed repeats them (a seed
    cached per process did not)."""
    dev = _dev(device)
    g = _graph(n=500, m=5000)
    adj = g.sparse_adjacency(dev)
    ft, el, er = _inputs(g.number_of_nodes(), 4, 8, dev)
    with torch.no_grad():
        torch.manual_seed(7)
        a, _ = kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.5)
        b, _ = kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.5)
        torch.manual_seed(7)
        c, _ = kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.5)
        d, _ = kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.5)
    assert not torch.equal(a, b)
    assert torch.equal(a, c) and torch.equal(b, d)


@pytest.mark.gpu
def test_graph_replays_draw_fresh_masks():
    """Inside a HIP graph capture the device counter advances at every
    replay: each replay draws a new mask."""
    dev = _dev("cuda")
    g = _graph(n=500, m=5000)
    adj = g.sparse_adjacency(dev)
    ft, el, er = _inputs(g.number_of_nodes(), 4, 8, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.5)  # warm (plans, buffers)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph, stream=side):
        out, _ = kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.5)
    graph.replay()
    torch.cuda.synchronize()
    a = out.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(a, out)


def test_bad_dropout_rejected():
    g = _graph(n=50, m=200)
    adj = g.sparse_adjacency("cpu")
    ft, el, er = _inputs(g.number_of_nodes(), 2, 4, torch.device("cpu"))
    with pytest.raises(dgl.DGLError):
        kernel.gat_aggregate(adj, ft, el, er, attn_drop=1.0)


# -- configs[2] at full size -------------------------------------------------
gat_train = load_example("gat/train.py", "gat_train_fused")


def _gat_model(data, g, dev, udf=False, unfused=False):
    torch.manual_seed(0)
    m = gat_train.GAT(g, 1, data.features.shape[1], 8, data.num_labels, [8, 8], F.elu,
                      0.0, 0.0, 0.2, False, udf=udf, unfused=unfused)
    return m.to(dev)


def _step(model, data):
    model.zero_grad(set_to_none=True)
    logits = model(data.features)
    loss = F.cross_entropy(logits[data.train_mask], data.labels[data.train_mask])
    loss.backward()
    return logits.detach(), [p.grad.detach().clone() for p in model.parameters()]


@pytest.mark.gpu
def test_gat_pubmed_fused_per_epoch_parity():
    """BASELINE configs[2]: GAT, 8 heads, Pubmed shape (19,717 nodes, 88,651
    edges + self-loops, 500 features, 3 classes). Five Adam epochs of the
    fused model; at each, the three-kernel and UDF models take its parameters
    and must give the same logits and gradients."""
    dev = _dev("cuda")
    data = gat_train.load_data("pubmed", seed=0, device=dev)
    src, dst = data.graph
    g = dgl.DGLGraph((src.cpu(), dst.cpu()))
    g.add_edges(g.nodes(), g.nodes())
    assert g.number_of_nodes() == 19717
    fused = _gat_model(data, g, dev)
    three = _gat_model(data, g, dev, unfused=True)
    udf = _gat_model(data, g, dev, udf=True)
    opt = torch.optim.Adam(fused.parameters(), lr=0.005, weight_decay=5e-4)
    for epoch in range(5):
        for other in (three, udf):
            other.load_state_dict(copy.deepcopy(fused.state_dict()))
        lf, gf = _step(fused, data)
        lt, gt = _step(three, data)
        lu, gu = _step(udf, data)
        assert torch.equal(lf, lt), epoch
        assert all(torch.equal(a, b) for a, b in zip(gf, gt)), epoch
        torch.testing.assert_close(lf, lu, rtol=1e-5, atol=1e-5 * float(lu.abs().max()))
        for a, b in zip(gf, gu):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5 * float(b.abs().max()) + 1e-12)
        opt.step()


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,p", [(8, 16, 0.0), (8, 16, 0.3), (8, 8, 0.3)])
def test_source_blocked_gat_bits(H, D, p):
    """The fused layer over the source-blocked schedule (one launch per
    source block over each row's sub-range, both chains continued; the
    per-lane kernel at 8 x 16, the LDS one at 8 x 8): on a graph whose edges
    are numbered source-major the outputs, the kept attention and every
    gradient equal the one-launch kernel's bit for bit."""
    dev = _dev("cuda")
    n, m = 120_000, 8_000_000
    rng = np.random.default_rng(11)
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    o = np.lexsort((dst, src))
    g = dgl.DGLGraph((torch.from_numpy(src[o]), torch.from_numpy(dst[o])))
    adj = g.sparse_adjacency(dev)
    assert kernel._block_cuts(adj.fwd, (H * D + H) * 4) is not None
    ft, el, er = _inputs(n, H, D, dev)

    def run(policy):
        old = kernel.set_blocked(policy)
        try:
            kernel.timing_enable(True)
            fs, z = kernel.gat_aggregate(adj, ft, el, er, 0.2, attn_drop=p, seed=77)
            torch.cuda.synchronize()
            _, launches = kernel.timing_read()
            kernel.timing_enable(False)
            return fs, z, _grads((fs, z), (ft, el, er)), launches
        finally:
            kernel.set_blocked(old)
    fs1, z1, g1, n1 = run("auto")
    fs0, z0, g0, n0 = run("off")
    assert n1 > n0
    assert torch.equal(fs1, fs0) and torch.equal(z1, z0)
    for a, b in zip(g1, g0):
        assert torch.equal(a, b)


@pytest.mark.parametrize("device", DEVICES)
def test_no_grad_stores_no_attention(device):
    """Under torch.no_grad() the fused layer keeps no E x H attention even
    when its inputs require grad (needs_input_grad alone does not say a
    backward will follow); the outputs are the same bits."""
    dev = _dev(device)
    g = _graph(n=500, m=5000)
    adj = g.sparse_adjacency(dev)
    ft, el, er = _inputs(g.number_of_nodes(), 4, 8, dev)
    with torch.no_grad():
        fs, z = kernel.gat_aggregate(adj, ft, el, er)
    fs2, z2 = kernel.gat_aggregate(adj, ft, el, er)
    assert torch.equal(fs, fs2.detach()) and torch.equal(z, z2.detach())
    assert fs.grad_fn is None and fs2.grad_fn is not None


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", [(8, 16), (4, 32), (8, 8), (2, 3)])
@pytest.mark.parametrize("blocked", ["auto", "off"])
def test_kernel_variants_same_bits(H, D, blocked):
    """Every fused-kernel variant (dglhip_set_gat_variant: per-lane
    attention, LDS attention with the feature rows gathered after it, or
    before it) gives the automatic choice's outputs, kept attention and
    dropped attention bit for bit, blocked or in one launch."""
    dev = _dev("cuda")
    n, m = 60_000, 3_000_000
    rng = np.random.default_rng(5)
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    o = np.lexsort((dst, src))
    g = dgl.DGLGraph((torch.from_numpy(src[o]), torch.from_numpy(dst[o])))
    adj = g.sparse_adjacency(dev)
    ft, el, er = _inputs(n, H, D, dev)
    old = kernel.set_blocked(blocked)
    try:
        outs = {}
        for v in (0, 1, 2, 3):
            kernel.set_gat_variant(v)
            fs, z = kernel.gat_aggregate(adj, ft, el, er, 0.2, attn_drop=0.25, seed=19)
            outs[v] = (fs.detach(), z.detach()) + tuple(_grads((fs, z), (ft, el, er)))
    finally:
        kernel.set_gat_variant(0)
        kernel.set_blocked(old)
    for v in (1, 2, 3):
        for a, b in zip(outs[v], outs[0]):
            assert torch.equal(a, b), v


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("blocked", ["auto", "off"])
@pytest.mark.parametrize("use_z", [True, False])
def test_transposed_backward_same_bits(p, blocked, use_z):
    """The one-pass backward over the transpose (8 heads x 16: attention and
    keep bits recomputed, d_ft / d_el chained in the transpose's slot order,
    g stored at its forward slot for d_er) equals r03's three passes (the
    attention stored by the forward) bit for bit: every gradient, with and
    without dropout (fixed seed), source-blocked or in one launch, with and
    without the normaliser's gradient."""
    dev = _dev("cuda")
    n, m = 120_000, 6_000_000  # 61 MB of ft at 8 x 16: the transpose is blocked
    rng = np.random.default_rng(31)
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    o = np.lexsort((dst, src))
    g = dgl.DGLGraph((torch.from_numpy(src[o]), torch.from_numpy(dst[o])))
    adj = g.sparse_adjacency(dev)
    gen = torch.Generator().manual_seed(32)
    ft0 = torch.randn(n, 8, 16, generator=gen).to(dev)
    el0 = torch.randn(n, 8, generator=gen).to(dev)
    er0 = torch.randn(n, 8, generator=gen).to(dev)
    gout = torch.randn(n, 8, 16, generator=gen).to(dev)
    gz = torch.randn(n, 8, 1, generator=gen).to(dev)

    def run(policy):
        old_b, old_g = kernel.set_blocked(blocked), kernel.set_gat_backward(policy)
        try:
            ft, el, er = (x.clone().requires_grad_(True) for x in (ft0, el0, er0))
            fs, z = kernel.gat_aggregate(adj, ft, el, er, attn_drop=p, seed=77)
            if use_z:
                torch.autograd.backward([fs, z], [gout, gz])
            else:
                fs.backward(gout)
            return fs.detach(), z.detach(), ft.grad, el.grad, er.grad
        finally:
            kernel.set_blocked(old_b)
            kernel.set_gat_backward(old_g)
    if blocked == "auto":
        assert kernel._block_plan(adj.bwd, gout.view(n, 128), 128) is not None
    a = run("auto")
    b = run("three")
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.gpu
def test_rowsum_heads8_is_the_copy_e_chain():
    """dglhip_rowsum_heads8_device (GAT's d_er: a wave per row, 64 slots per
    step through LDS) equals the copy_e sum over slot-ordered values bit for
    bit, on rows from empty to a hub of 50,000 slots."""
    dev = _dev("cuda")
    rng = np.random.default_rng(41)
    n, m = 20_000, 400_000
    dst = np.where(rng.random(m) < 0.125, 7, rng.integers(0, n, m))
    src = rng.integers(0, n, m)
    adj = kernel.from_coo(n, n, torch.from_numpy(dst), torch.from_numpy(src), kernel.ORDER_EID,
                          dev)
    vals = torch.randn(m, 8, generator=torch.Generator().manual_seed(42)).to(dev)
    old = kernel.set_row_split("off")  # the reference chain: no heavy-row chunks
    try:
        ref = kernel.gspmm(adj, "copy_e", "sum", None, vals.unsqueeze(-1), edge_order="slot")
    finally:
        kernel.set_row_split(old)
    out = torch.empty(n, 8, device=dev)
    kernel.check_call(kernel.LIB.dglhip_rowsum_heads8_device(
        n, kernel.ptr(adj.fwd.indptr), kernel.ptr(adj.fwd.row_order), kernel.ptr(vals),
        kernel.ptr(out), kernel._stream_of(dev)))
    assert torch.equal(out, ref.reshape(n, 8))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", [(8, 8), (8, 16)])
def test_dropout_keeps_pairs_with_zero_attention(device, H, D):
    """A kept (slot, head) pair whose attention is exactly 0 (no exp, a zero
    logit) keeps its gradient: the backward's keep bits come from the
    forward's hash, not from the dropped copy being nonzero (r03 ADVICE).
    Checked against float64 torch autograd through the same mask, within
    gat_reference's bound ((L + Dg + 16) * 2^-24 of each element's condition
    scale)."""
    dev = _dev(device)
    g = _graph(n=400, m=6000, seed=9)
    adj = g.sparse_adjacency(dev)
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(10)
    ft0 = torch.randn(n, H, D, generator=gen)
    el0 = torch.randn(n, H, generator=gen)
    er0 = torch.randn(n, H, generator=gen)
    el0[: n // 2] = 0.0
    er0[: n // 2] = 0.0  # edges among the first half: logit exactly 0
    p, seed = 0.5, 4242
    gout = torch.randn(n, H, D, generator=gen)
    gz = torch.randn(n, H, 1, generator=gen)
    ft, el, er = (x.clone().to(dev).requires_grad_(True) for x in (ft0, el0, er0))
    fs, z = kernel.gat_aggregate(adj, ft, el, er, 0.2, clamp=(-10.0, 10.0), attn_drop=p,
                                 apply_exp=False, seed=seed)
    torch.autograd.backward([fs, z], [gout.to(dev), gz.to(dev)])
    # reference: torch autograd over the slot-ordered attention, same mask
    fwd = adj.fwd
    u = fwd.indices.long().cpu()
    v = fwd.row_ids().cpu()
    keep = kernel.gat_dropout_mask(E, H, p, seed)
    assert bool((((el0[u] + er0[v]) == 0) & keep).any())  # the case is present
    # (the clamp is never reached here: no shares of clamped pairs to ask for)
    ref = gat_reference64(u, v, n, n, ft0, el0, er0, 0.2, -10.0, 10.0, False, keep, p, gout, gz,
                          shares=False)
    check_all(ref, fs=fs, z=z.reshape(n, H), d_ft=ft.grad, d_el=el.grad, d_er=er.grad, D=D)


@pytest.mark.gpu
def test_transposed_backward_without_er_grad():
    """er not requiring grad: the one-pass backward stores no attention
    gradient (NULL buffer) and d_ft / d_el keep the bits of the full
    backward."""
    dev = _dev("cuda")
    n, m = 40_000, 1_500_000
    rng = np.random.default_rng(43)
    g = dgl.DGLGraph((torch.from_numpy(rng.integers(0, n, m)),
                      torch.from_numpy(rng.integers(0, n, m))))
    adj = g.sparse_adjacency(dev)
    ft0, el0, er0 = (x.detach() for x in _inputs(n, 8, 16, dev))
    gout = torch.randn(n, 8, 16, device=dev)
    outs = []
    for er_grad in (True, False):
        ft, el = ft0.clone().requires_grad_(True), el0.clone().requires_grad_(True)
        er = er0.clone().requires_grad_(er_grad)
        fs, _ = kernel.gat_aggregate(adj, ft, el, er, attn_drop=0.3, seed=5)
        fs.backward(gout)
        outs.append((ft.grad, el.grad))
        assert (er.grad is not None) == er_grad
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _tiny_logit_graph(n=96, seed=5):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, 6 * n)
    dst = rng.integers(0, n, 6 * n)
    g = dgl.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)))
    return g, src, dst


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", [(8, 16), (2, 5)])
@pytest.mark.parametrize("bwd", ["auto", "three"])
def test_slope_from_the_logit_sign(device, H, D, bwd):
    """logits of exactly 0 and just above 0 (0 < x < 2^-24, where
    exp(x) rounds to 1). torch's leaky_relu backward takes slope 1 for any
    x > 0 and alpha for x <= 0; every GAT backward (the fused one-pass kernel,
    the three-pass kernels, the host path) now takes it from x = el[u] + er[v]
    itself, so the gradients match float64 torch within gat_reference's bound
    ((L + Dg + 16) * 2^-24 of each element's condition scale) — with a slope
    read from a <= 1 the tiny positive logits' pairs would be off by the
    factor 1 / alpha = 5."""
    dev = _dev(device)
    g, src, dst = _tiny_logit_graph()
    n = g.number_of_nodes()
    adj = g.sparse_adjacency(dev)
    gen = torch.Generator().manual_seed(11)
    ft = torch.randn(n, H, D, generator=gen)
    # x = el[u] + 0: exactly 0, tiny positive (exp rounds to 1), tiny negative,
    # ordinary values
    choice = torch.tensor([0.0, 1e-8, 3e-8, -1e-8, 0.5, -0.5])
    el = choice[torch.randint(0, 6, (n, H), generator=gen)]
    er = torch.zeros(n, H)
    R = torch.randn(n, H, D, generator=gen)
    S = torch.randn(n, H, 1, generator=gen)
    ft, el, er = (t.to(dev).requires_grad_(True) for t in (ft, el, er))
    old = kernel.set_gat_backward(bwd)
    try:
        fs, z = kernel.gat_aggregate(adj, ft, el, er, 0.2, clamp=(-10.0, 10.0))
        got = torch.autograd.grad((fs * R.to(dev)).sum() + (z * S.to(dev)).sum(), (ft, el, er))
    finally:
        kernel.set_gat_backward(old)
    # float64 torch (leaky_relu's own backward: slope alpha where x <= 0, 1 where
    # x > 0, however small), within gat_reference's bound; the clamp is never
    # reached here, so no shares of clamped pairs to ask for
    ref = gat_reference64(src, dst, n, n, ft, el, er, 0.2, -10.0, 10.0, True, None, 0.0, R, S,
                          shares=False)
    check_all(ref, fs=fs, z=z.reshape(n, H), d_ft=got[0], d_el=got[1], d_er=got[2], D=D)
    # the tiny positive logits are where the old slope differed: el's gradient
    # at those sources carries slope 1
    pos = (el.detach().cpu() > 0) & (el.detach().cpu() < 1e-7)
    assert bool(pos.any())
    check_all(ref, d_el=got[1], D=D, what="at the tiny positive logits",
              srcs=pos.any(1).nonzero().squeeze(1))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("order", ["eid", "slot"])
def test_edge_attention_slope_from_the_logit_sign(device, order):
    """The same for kernel.edge_attention's backward (eid and slot order)."""
    dev = _dev(device)
    g, src, dst = _tiny_logit_graph()
    n, E = g.number_of_nodes(), g.number_of_edges()
    adj = g.sparse_adjacency(dev)
    gen = torch.Generator().manual_seed(12)
    choice = torch.tensor([0.0, 1e-8, -1e-8, 0.5])
    el = choice[torch.randint(0, 4, (n, 4), generator=gen)].to(dev).requires_grad_(True)
    er = torch.zeros(n, 4, device=dev, requires_grad=True)
    a = kernel.edge_attention(adj, el, er, E, 0.2, clamp=(-10.0, 10.0), edge_order=order)
    W = torch.randn(E, 4, generator=gen)
    got = torch.autograd.grad((a * W.to(dev)).sum(), (el, er))
    if order == "slot":  # forward slot order: the CSR's (dst-major) order of the edges
        fwd = adj.fwd
        s64 = fwd.indices.long().cpu()
        d64 = fwd.row_ids().cpu()
    else:
        s64, d64 = torch.from_numpy(src), torch.from_numpy(dst)
    el64 = el.detach().double().cpu().requires_grad_(True)
    er64 = er.detach().double().cpu().requires_grad_(True)
    a64 = torch.clamp(torch.exp(F.leaky_relu(el64[s64] + er64[d64], 0.2)), -10.0, 10.0)
    ref = torch.autograd.grad((a64 * W.double()).sum(), (el64, er64))
    # gat_reference's bound with L = 1 and Dg = 0 (a term is one product); the
    # condition scale: the gradient's terms |W| a slope, summed per node.
    # (L = 1 is tighter than the chain length, a node's degree of about 6,
    # which test_gat_reference.py::test_edge_attention_on_the_grid uses for
    # the same sums: these few terms stay well inside the 16 allowed)
    with torch.no_grad():
        x64 = el64[s64] + er64[d64]
        slope = torch.where(x64 > 0, torch.ones_like(x64), torch.full_like(x64, 0.2))
        S_g = W.double().abs() * a64 * slope
    ones = torch.ones(n, dtype=torch.int64)
    for x, r, idx, name in zip(got, ref, (s64, d64), ("d_el", "d_er")):
        S = torch.zeros(n, 4, dtype=torch.float64).index_add(0, idx, S_g)
        assert_within(x, r, S, ones, 0, name)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("H,D", [(8, 16), (8, 8), (2, 5)])
def test_gat_logits_association_and_grads(device, H, D):
    """kernel.gat_logits: el = (ft * attn_l).sum(-1) in the library's
    association (a pairwise tree at D = 16, one fma chain otherwise), host ==
    device, within 1e-6 of float64; gradients as torch's for the same
    formula."""
    dev = _dev(device)
    gen = torch.Generator().manual_seed(31)
    n = 700
    ft = torch.randn(n, H, D, generator=gen)
    al = torch.randn(H, D, 1, generator=gen)
    ar = torch.randn(H, D, 1, generator=gen)
    ft1, al1, ar1 = (t.to(dev).requires_grad_(True) for t in (ft, al, ar))
    el, er = kernel.gat_logits(ft1, al1, ar1)
    assert el.shape == (n, H, 1) and er.shape == (n, H, 1)
    ref_l = (ft.double() * al.double().view(1, H, D)).sum(-1, keepdim=True)
    ref_r = (ft.double() * ar.double().view(1, H, D)).sum(-1, keepdim=True)
    mag = (ft.double().abs() * al.double().abs().view(1, H, D)).sum(-1, keepdim=True)
    assert ((el.double().cpu() - ref_l).abs() <= 1e-6 * mag + 1e-30).all()
    assert ((er.double().cpu() - ref_r).abs() <= 1e-6 * mag.max() + 1e-30).all()
    if dev.type == "cuda":
        el_h, er_h = kernel.gat_logits(ft, al, ar)
        assert torch.equal(el.detach().cpu(), el_h) and torch.equal(er.detach().cpu(), er_h)
    gl = torch.randn(n, H, 1, generator=gen).to(dev)
    gr = torch.randn(n, H, 1, generator=gen).to(dev)
    got = torch.autograd.grad((el * gl).sum() + (er * gr).sum(), (ft1, al1, ar1))
    ft2, al2, ar2 = (t.detach().clone().to(dev).requires_grad_(True) for t in (ft, al, ar))
    e2 = (ft2 * al2.view(1, H, D)).sum(-1, keepdim=True)
    r2 = (ft2 * ar2.view(1, H, D)).sum(-1, keepdim=True)
    want = torch.autograd.grad((e2 * gl).sum() + (r2 * gr).sum(), (ft2, al2, ar2))
    for x, y in zip(got, want):
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_gat_forward_recomputes_logits_same_bits(p):
    """With el from kernel.gat_logits on the same ft and the recompute switched
    on (a study knob, off by default: slower), the 8 x 16 source-blocked
    forward recomputes every source's logit from its gathered row
    (dglhip_gat_aggregate_logits_ranges_device) instead of reading el: the
    outputs and every gradient equal the el-reading kernel's bit for bit."""
    dev = _dev("cuda")
    n, m = 60_000, 6_000_000
    gen = torch.Generator().manual_seed(33)
    src = torch.randint(0, n, (m,), generator=gen)
    dst = torch.randint(0, n, (m,), generator=gen)
    order = torch.from_numpy(np.lexsort((dst.numpy(), src.numpy())))  # source-major
    g = dgl.DGLGraph((src[order], dst[order]))
    adj = g.sparse_adjacency(dev)
    ft0 = torch.randn(n, 8, 16, generator=gen) * 0.5
    al0 = torch.randn(8, 16, 1, generator=gen) * 0.3
    ar0 = torch.randn(8, 16, 1, generator=gen) * 0.3
    R = torch.randn(n, 8, 16, generator=gen).to(dev)
    S = torch.randn(n, 8, 1, generator=gen).to(dev)
    cuts = kernel._block_cuts(adj.fwd, (128 + 8) * 4, None)
    assert cuts is not None and len(cuts) > 2  # the source-blocked forward
    res = []
    for recompute in (True, False):
        kernel.LIB.dglhip_set_gat_logit_recompute(1 if recompute else 0)
        try:
            ft, al, ar = (t.to(dev).requires_grad_(True) for t in (ft0, al0, ar0))
            el, er = kernel.gat_logits(ft, al, ar)
            assert kernel._logits_source(el, ft) is not None
            fs, z = kernel.gat_aggregate(adj, ft, el, er, 0.2, attn_drop=p, seed=77)
            grads = torch.autograd.grad((fs * R).sum() + (z * S).sum(), (ft, al, ar))
        finally:
            kernel.LIB.dglhip_set_gat_logit_recompute(0)
        res.append([fs.detach(), z.detach()] + [x.detach() for x in grads])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_gat_logits_tag_follows_versions():
    """gat_aggregate may only recompute el from ft when el is gat_logits'
    unchanged output for that very ft: another ft, an in-place change of ft
    or of el voids the tag (kernel._logits_source)."""
    ft = torch.randn(50, 8, 16)
    al, ar = torch.randn(8, 16, 1), torch.randn(8, 16, 1)
    el, _ = kernel.gat_logits(ft, al, ar)
    # (host tensors: the recompute is a device path, so the tag reads None here;
    # check the tag's fields directly)
    tag = el._dglhip_logits
    assert tag[0] == ft.data_ptr() and tag[1] == tuple(ft.shape)
    assert tag[2] == ft._version and tag[3] == el._version
    ft.add_(0.0)
    assert ft._version != tag[2]
    el2, _ = kernel.gat_logits(ft, al, ar)
    el2.mul_(1.0)
    assert el2._version != el2._dglhip_logits[3]


def test_gat_logits_tag_dies_with_its_ft():
    """The tag holds its ft weakly: once that ft is freed, a new
    tensor at the same address, shape and version 0 no longer matches."""
    import gc
    ft = torch.randn(50, 8, 16)
    al, ar = torch.randn(8, 16, 1), torch.randn(8, 16, 1)
    with torch.no_grad():
        el, _ = kernel.gat_logits(ft, al, ar)
    ref = el._dglhip_logits[5]
    assert ref() is ft
    del ft
    gc.collect()
    assert ref() is None
