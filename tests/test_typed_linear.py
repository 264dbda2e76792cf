"""kernel.typed_linear_spmm (csrc/typed_linear.hip: dense per-relation weights
on the f32 MFMA), nn.RelGraphConv(regularizer="basis") and the entity
classification example, on the chosen graph of test_typed_block_edges (rows of
0..200 slots, relations of 0..517 edges: every 64-position item, 16-position
strip and 4-position step edge) against the float64 bmm formulation."""
import importlib.util
import os

import pytest
import torch

import dgl
import dgl.nn.pytorch as dglnn
from dgl import kernel
from test_typed_block import reference
from test_typed_block_edges import DST, ETYPE, N, R, SRC, _poison

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
M = SRC.numel()

# (Fi, Fo): what each reaches in csrc/typed_linear.hip
SHAPES = [
    (1, 1),      # one output
    (4, 16),     # exactly one MFMA step and one column tile
    (5, 3),      # both sides ragged
    (16, 4),     # the example's output layer
    (16, 16),    # one full tile each way
    (17, 33),    # one past a tile both ways
    (64, 64),    # several tiles
    (100, 40),   # ragged and several K-tiles
    (256, 256),  # the gate's edge
    (257, 8),    # past it: the fallback
]
IDS = ["%dx%d" % s for s in SHAPES]
_ADJ, _REF = {}, {}


def _adj(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    if device not in _ADJ:
        _ADJ[device] = kernel.from_coo(N, N, DST, SRC, kernel.ORDER_EID, device)
    return _ADJ[device]


def _inputs(shape, exact):
    """(h, W, G, enorm, row_scale): small integers and powers of two (every
    partial sum an integer below 2^24: float32 is exact in any order), or
    randn operands with positive scales."""
    Fi, Fo = shape
    gen = torch.Generator().manual_seed(1000 * Fi + Fo)
    if exact:
        h, W, G = (torch.randint(-2, 3, s, generator=gen).float()
                   for s in ((N, Fi), (R, Fi, Fo), (N, Fo)))
        enorm = 2.0 ** torch.randint(-2, 2, (M,), generator=gen).float()
        scale = 2.0 ** torch.randint(-3, 2, (N,), generator=gen).float()
    else:
        h, W, G = torch.randn(N, Fi, generator=gen), torch.randn(R, Fi, Fo, generator=gen) * 0.3, \
            torch.randn(N, Fo, generator=gen)
        enorm = torch.rand(M, generator=gen) * 0.9 + 0.1
        scale = torch.rand(N, generator=gen) * 0.99 + 0.01
    return h, W, G, enorm, scale


def _float64(shape, exact, scaled, f=lambda t: t):
    """(out, dH, dW) of the float64 bmm formulation over f(operands), once."""
    key = (shape, exact, scaled, f is torch.abs)
    if key not in _REF:
        h, W, G, enorm, scale = _inputs(shape, exact)
        h2, W2 = f(h.double()).requires_grad_(True), f(W.double()).requires_grad_(True)
        out = reference(SRC, DST, ETYPE, h2, W2.view(R, 1, *shape), N,
                        enorm.double() if scaled else None)
        if scaled:
            out = out * scale.double().unsqueeze(1)
        out.backward(f(G.double()))
        _REF[key] = (out.detach(), h2.grad, W2.grad)
    return _REF[key]


def _run(shape, exact, scaled, device):
    h, W, G, enorm, scale = _inputs(shape, exact)
    dev = torch.device(device)
    adj = _adj(device)
    h1, W1 = h.to(dev).requires_grad_(True), W.to(dev).requires_grad_(True)
    _poison(dev, G.numel(), h.numel(), W.numel(), M * max(shape))
    out = kernel.typed_linear_spmm(adj, h1, W1, ETYPE.to(dev), enorm.to(dev) if scaled else None,
                                   scale.to(dev) if scaled else None)
    out.backward(G.to(dev))
    return out.detach().cpu(), h1.grad.cpu(), W1.grad.cpu()


def test_gate_and_byte_cap(monkeypatch):
    cuda = torch.device("cuda")
    for Fi, Fo in SHAPES:
        assert kernel._typed_linear_ok(cuda, M, R, Fi, Fo) is (Fi <= 256)
        assert not kernel._typed_linear_ok(torch.device("cpu"), M, R, Fi, Fo)
    monkeypatch.setattr(kernel.rgcn, "_TYPED_LINEAR_BYTES", 4 * M * 64)  # the messages alone
    assert not kernel._typed_linear_ok(cuda, M, R, 64, 64)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_integer_operands(device, shape):
    """out, dH and dW equal the float64 reference, with and without enorm and
    row_scale; unwritten elements would show as NaN, the two empty rows and the
    empty relation's dW are exact zeros."""
    for scaled in (False, True):
        got = _run(shape, True, scaled, device)
        for g, w in zip(got, _float64(shape, True, scaled)):
            assert torch.equal(g.double(), w)
        assert not got[0][[0, N - 1]].any() and not got[2][0].any()
        assert got[0][1:N - 1].abs().sum() > 0 and got[2][1:].abs().sum() > 0


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_accuracy_on_randn_operands(device, shape):
    """Every element of out, dH and dW within 1e-5 * Σ|terms| of float64, the
    bound test_typed_block_edges holds the scalar kernels to on this graph."""
    for scaled in (False, True):
        got = _run(shape, False, scaled, device)
        want, bound = _float64(shape, False, scaled), _float64(shape, False, scaled, torch.abs)
        for g, w, b in zip(got, want, bound):
            err = (g.double() - w).abs()
            ratio = float((err / (1e-5 * b + 1e-30)).max())
            print(shape, device, scaled, "worst err / bound = %.3g" % ratio)
            assert bool((err <= 1e-5 * b + 1e-30).all()), ratio


@pytest.mark.parametrize("device", DEVICES)
def test_two_runs_give_the_same_bits(device):
    a, b = _run((100, 40), False, True, device), _run((100, 40), False, True, device)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _graph():
    g = dgl.DGLGraph((SRC, DST), multigraph=True)
    if g.number_of_nodes() < N:
        g.add_nodes(N - g.number_of_nodes())
    return g


def _within_bound(got, want, bound):
    for g, w, b in zip(got, want, bound):
        err = (g.detach().double().cpu() - w).abs()
        assert bool((err <= 1e-5 * b + 1e-30).all()), float((err / (1e-5 * b + 1e-30)).max())


@pytest.mark.parametrize("device", DEVICES)
def test_basis_module_matches_float64(device):
    """RelGraphConv(regularizer="basis") forward and the gradients of feat,
    weight, w_comp and loop_weight against the float64 w_comp-composed bmm."""
    _adj(device)
    torch.manual_seed(3)
    conv = dglnn.RelGraphConv(8, 6, num_rels=R, num_bases=3, regularizer="basis").to(device)
    assert conv.weight.shape == (3, 8, 6) and conv.w_comp.shape == (R, 3)
    feat, G, norm = torch.randn(N, 8), torch.randn(N, 6), torch.rand(N) * 0.9 + 0.1
    enorm = torch.rand(M) * 0.9 + 0.1
    params = [conv.weight, conv.w_comp, conv.loop_weight]
    x = feat.to(device).requires_grad_(True)
    out = conv(_graph(), x, ETYPE.to(device), norm=norm.to(device), enorm=enorm.to(device))
    got = (out,) + torch.autograd.grad(out, [x] + params, G.to(device))
    res = []
    for f in (lambda t: t, torch.abs):
        h, w, c, lw = (f(t.detach().double().cpu()).requires_grad_(True) for t in [feat] + params)
        W = (c @ w.view(3, -1)).view(R, 1, 8, 6)
        ref = reference(SRC, DST, ETYPE, h, W, N, f(enorm.double())) * norm.double().unsqueeze(1)
        ref = ref + h @ lw + f(conv.bias.detach().double().cpu())
        res.append((ref.detach(),) + torch.autograd.grad(ref, [h, w, c, lw], f(G.double())))
    _within_bound(got, *res)


@pytest.mark.parametrize("device", DEVICES)
def test_featureless_input_layer(device):
    """feat = node ids: out[v] = Σ_e enorm_e W[etype_e, id_u, :], and the
    gradients of weight and w_comp, against the float64 embedding lookup."""
    _adj(device)
    torch.manual_seed(4)
    conv = dglnn.RelGraphConv(N, 6, R, 3, bias=False, self_loop=False,
                              regularizer="basis").to(device)
    enorm, G = torch.rand(M) * 0.9 + 0.1, torch.randn(N, 6)
    params = [conv.weight, conv.w_comp]
    out = conv(_graph(), torch.arange(N, device=device), ETYPE.to(device), enorm=enorm.to(device))
    got = (out,) + torch.autograd.grad(out, params, G.to(device))
    res = []
    for f in (lambda t: t, torch.abs):
        w, c = (f(t.detach().double().cpu()).requires_grad_(True) for t in params)
        embed = (c @ w.view(3, -1)).view(R * N, 6)
        msg = embed[ETYPE * N + SRC] * enorm.double().unsqueeze(1)
        ref = torch.zeros(N, 6, dtype=torch.float64).index_add(0, DST, msg)
        res.append((ref.detach(),) + torch.autograd.grad(ref, [w, c], f(G.double())))
    _within_bound(got, *res)


def test_bdd_constructs_the_same_parameters():
    torch.manual_seed(5)
    a = dglnn.RelGraphConv(8, 6, num_rels=4, num_bases=2).state_dict()
    torch.manual_seed(5)
    b = dglnn.RelGraphConv(8, 6, num_rels=4, num_bases=2, regularizer="bdd").state_dict()
    assert list(a) == list(b) == ["weight", "loop_weight", "bias"]
    assert a["weight"].shape == (4, 2, 4, 3) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(dgl.DGLError):
        dglnn.RelGraphConv(8, 6, 4, 2, regularizer="dense")


def test_example_trains_on_the_host():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples",
                        "rgcn", "entity_classify.py")
    spec = importlib.util.spec_from_file_location("entity_classify", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.run(mod.parser().parse_args(
        ["--num-nodes", "300", "--num-edges", "900", "--num-rels", "5", "--num-train", "40",
         "--num-test", "10", "--n-epochs", "2", "--n-bases", "3"]))
    assert res["fused"] and all(l == l and abs(l) < 1e9 for l in res["losses"])
    assert res["losses"][1] < res["losses"][0]
