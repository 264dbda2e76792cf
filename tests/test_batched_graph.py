"""dgl.batch / dgl.unbatch / BatchedDGLGraph and the readout functions
(sum_nodes, mean_nodes, max_nodes and their _edges twins), against the
reference's behaviour (python/dgl/batched_graph.py): structure of the union,
attribute selection, read-only batch, unbatch as the inverse, message passing
on the batch equal to the member graphs', readouts equal to the reference's
torch formulas bit for bit, and a small graph classifier trained end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import dgl
import dgl.function as fn
from dgl.base import ALL, DGLError
from dgl.nn.pytorch import GraphConv

from test_segment_reduce import _same_bits, _torch_formula

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]

EDGES = [[(0, 1), (1, 2), (2, 0), (0, 2)], [], [(0, 3), (3, 3), (2, 1), (1, 0), (2, 3)]]
NODES = [3, 0, 4]


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


def _graph(n, edges, dev=torch.device("cpu"), seed=0, feats=True):
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    if edges:
        g.add_edges([e[0] for e in edges], [e[1] for e in edges])
    if feats:
        gen = torch.Generator().manual_seed(seed)
        scale = torch.exp(3 * torch.randn(n, 1, generator=gen))
        g.ndata["h"] = (torch.randn(n, 5, generator=gen) * scale).to(dev)
        g.ndata["w"] = torch.randn(n, 1, generator=gen).to(dev)
        g.edata["e"] = torch.randn(len(edges), 2, 3, generator=gen).to(dev)
        g.edata["w"] = torch.randn(len(edges), 1, generator=gen).to(dev)
    return g


def _three(dev=torch.device("cpu")):
    return [_graph(n, e, dev, seed=i) for i, (n, e) in enumerate(zip(NODES, EDGES))]


def test_structure():
    gs = _three()
    bg = dgl.batch(gs)
    assert isinstance(bg, dgl.BatchedDGLGraph) and isinstance(bg, dgl.DGLGraph)
    assert bg.batch_size == 3
    assert bg.batch_num_nodes == [3, 0, 4] and bg.batch_num_edges == [4, 0, 5]
    assert bg.number_of_nodes() == 7 and bg.number_of_edges() == 9
    src, dst, eid = bg.all_edges("all")
    # ids offset by the running sizes, edges in their own order
    assert src.tolist() == [0, 1, 2, 0] + [3 + u for u, _ in EDGES[2]]
    assert dst.tolist() == [1, 2, 0, 2] + [3 + v for _, v in EDGES[2]]
    assert eid.tolist() == list(range(9))
    assert torch.equal(bg.ndata["h"], torch.cat([g.ndata["h"] for g in gs if len(g)]))
    assert torch.equal(bg.edata["e"], torch.cat([gs[0].edata["e"], gs[2].edata["e"]]))
    # a batch of a batch concatenates the size lists
    bb = dgl.batch([bg, gs[2], bg])
    assert bb.batch_size == 7
    assert bb.batch_num_nodes == [3, 0, 4, 4, 3, 0, 4]
    assert bb.batch_num_edges == [4, 0, 5, 5, 4, 0, 5]
    assert bb.number_of_nodes() == 18


def test_attributes_and_mutation():
    gs = _three()
    assert set(dgl.batch(gs, node_attrs=ALL).ndata.keys()) == {"h", "w"}
    bg = dgl.batch(gs, node_attrs=None, edge_attrs=None)
    assert len(bg.ndata) == 0 and len(bg.edata) == 0
    bg = dgl.batch(gs, node_attrs="h", edge_attrs=["w"])
    assert set(bg.ndata.keys()) == {"h"} and set(bg.edata.keys()) == {"w"}
    bg = dgl.batch(gs, node_attrs=["h", "w"], edge_attrs=("e",))
    assert set(bg.ndata.keys()) == {"h", "w"} and set(bg.edata.keys()) == {"e"}
    # the empty graph carries no fields and is no mismatch; a graph with nodes is
    bare = _graph(0, [], feats=False)
    assert set(dgl.batch([gs[0], bare]).ndata.keys()) == {"h", "w"}
    odd = _graph(2, [(0, 1)])
    odd.ndata["extra"] = torch.zeros(2, 1)
    with pytest.raises(ValueError):
        dgl.batch([gs[0], odd])
    with pytest.raises(ValueError):
        dgl.batch(gs, node_attrs=3)
    dgl.batch([gs[0], odd], node_attrs="h")  # named fields need no agreement
    bg = dgl.batch(gs)
    for call in (lambda: bg.add_nodes(1), lambda: bg.add_edge(0, 1),
                 lambda: bg.add_edges([0], [1])):
        with pytest.raises(DGLError, match="Readonly graph. Mutation is not allowed."):
            call()


def test_unbatch_round_trip():
    gs = _three()
    bg = dgl.batch(gs)
    bg.ndata["h"][0] = 123.0  # the batch owns its columns
    bg.edata["w"] = torch.zeros(9, 1)
    assert not (gs[0].ndata["h"] == 123.0).any() and gs[0].edata["w"].abs().sum() > 0
    back = dgl.unbatch(dgl.batch(gs))
    assert len(back) == 3
    for g, r in zip(gs, back):
        assert g.number_of_nodes() == r.number_of_nodes()
        for a, b in zip(g.all_edges("all"), r.all_edges("all")):
            assert torch.equal(a, b)
        for k in ("h", "w"):
            assert torch.equal(g.ndata[k], r.ndata[k])
        for k in ("e", "w"):
            assert torch.equal(g.edata[k], r.edata[k])
    with pytest.raises(DGLError):
        dgl.unbatch(gs[0])


@pytest.mark.parametrize("device", DEVICES)
def test_message_passing_on_batch(device):
    dev = _dev(device)
    gs = _three(dev)
    bg = dgl.batch(gs)
    for red in (fn.sum, fn.max):
        bg.update_all(fn.copy_src("h", "m"), red("m", "o"))
        outs = []
        for g in gs:
            if len(g):
                g.update_all(fn.copy_src("h", "m"), red("m", "o"))
                outs.append(g.ndata["o"])
        assert _same_bits(bg.ndata["o"].cpu().numpy(), torch.cat(outs).cpu().numpy())


@pytest.mark.parametrize("device", DEVICES)
def test_readouts(device):
    dev = _dev(device)
    gs = _three(dev)
    bg = dgl.batch(gs)
    table = [("sum", dgl.sum_nodes, dgl.sum_edges), ("mean", dgl.mean_nodes, dgl.mean_edges),
             ("max", dgl.max_nodes, dgl.max_edges)]
    for reduce, on_nodes, on_edges in table:
        for call, feat, sizes, data in ((on_nodes, "h", bg.batch_num_nodes, bg.ndata),
                                        (on_edges, "e", bg.batch_num_edges, bg.edata)):
            for weight in ((None,) if reduce == "max" else (None, "w")):
                args = (feat,) if weight is None else (feat, weight)
                y = call(bg, *args)
                fshape = tuple(data[feat].shape[1:])
                assert tuple(y.shape) == (3,) + fshape
                # the reference's formulas on the CPU, bit for bit
                x2 = data[feat].cpu().reshape(data[feat].shape[0], -1)
                w = None if weight is None else data[weight].cpu()
                ref, _ = _torch_formula(x2, list(sizes), reduce, w)
                assert _same_bits(y.cpu().numpy().reshape(3, -1), ref.numpy()), (reduce, feat)
                # the per-graph readouts, stacked
                each = torch.stack([call(g, *args) for g in gs])
                assert tuple(each.shape) == (3,) + fshape
                assert _same_bits(y.cpu().numpy(), each.cpu().numpy()), (reduce, feat)


@pytest.mark.parametrize("device", DEVICES)
def test_plain_graph_readouts(device):
    dev = _dev(device)
    gen = torch.Generator().manual_seed(9)
    n = 3000  # more than one chunk: a tolerance check, as the reference's torch.sum is no chain
    g = dgl.DGLGraph()
    g.add_nodes(n)
    g.add_edges(torch.arange(n - 1), torch.arange(1, n))
    g.ndata["h"] = (torch.randn(n, 4, 3, generator=gen)
                    * torch.exp(3 * torch.randn(n, 1, 1, generator=gen))).to(dev)
    g.edata["e"] = torch.randn(n - 1, 6, generator=gen).to(dev)
    for data, key, fns in ((g.ndata, "h", (dgl.sum_nodes, dgl.mean_nodes, dgl.max_nodes)),
                           (g.edata, "e", (dgl.sum_edges, dgl.mean_edges, dgl.max_edges))):
        x64 = data[key].cpu().double()
        bound = 1e-5 * x64.abs().sum(0)
        got = [f(g, key).cpu().double() for f in fns]
        for y in got:
            assert tuple(y.shape) == tuple(x64.shape[1:])
        assert ((got[0] - x64.sum(0)).abs() <= bound).all()
        assert ((got[1] - x64.mean(0)).abs() <= bound / x64.shape[0]).all()
        assert torch.equal(got[2], x64.max(0)[0])


# -- end to end: cycles against stars ---------------------------------------
def _cycle_or_star(n, star):
    g = dgl.DGLGraph()
    g.add_nodes(n)
    if star:
        u = torch.zeros(n - 1, dtype=torch.int64)
        v = torch.arange(1, n)
    else:
        u = torch.arange(n)
        v = (u + 1) % n
    g.add_edges(torch.cat([u, v]), torch.cat([v, u]))
    return g


def _dataset():
    rng = np.random.default_rng(4)
    gen = torch.Generator().manual_seed(4)
    graphs, labels = [], []
    for i in range(16):
        n = int(rng.integers(5, 13))
        g = _cycle_or_star(n, i % 2 == 1)
        deg = g.in_degrees().float().unsqueeze(1)
        g.ndata["x"] = torch.cat([deg, torch.ones(n, 1), torch.randn(n, 2, generator=gen)], 1)
        graphs.append(g)
        labels.append(i % 2)
    return graphs, torch.tensor(labels)


class _Classifier(torch.nn.Module):
    def __init__(self):
        super(_Classifier, self).__init__()
        self.conv1 = GraphConv(4, 16, activation=torch.relu)
        self.conv2 = GraphConv(16, 8)
        self.out = torch.nn.Linear(8, 2)

    def forward(self, bg):
        h = self.conv2(bg, self.conv1(bg, bg.ndata["x"]))
        bg.ndata["r"] = h
        return self.out(dgl.mean_nodes(bg, "r"))


def _first_step_and_training(dev):
    graphs, labels = _dataset()
    bg = dgl.batch(graphs)
    bg.ndata["x"] = bg.ndata["x"].to(dev)
    torch.manual_seed(1)
    model = _Classifier()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    labels = labels.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses, first = [], None
    for _ in range(31):
        loss = Fn.cross_entropy(model(bg), labels)
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        if first is None:
            first = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
        opt.step()
    return state, first, losses, bg


def _gradient_bounds(state, bg, labels):
    """sum|terms| of every parameter gradient of the first step: the model in
    float64 with dense matrices on |parameters| and |features|, the ReLU as the
    real step's 0/1 mask, and softmax + one-hot (the magnitudes of the
    cross-entropy gradient's subtraction) over the batch as upstream weights."""
    n, B = bg.number_of_nodes(), bg.batch_size
    src, dst = bg.all_edges()
    A = torch.zeros(n, n, dtype=torch.float64).index_put_(
        (dst, src), torch.ones(len(src), dtype=torch.float64), accumulate=True)
    din = bg.in_degrees().double().clamp(min=1).pow(-0.5)
    dout = bg.out_degrees().double().clamp(min=1).pow(-0.5)
    Ahat = din[:, None] * A * dout[None, :]
    seg = torch.arange(B).repeat_interleave(torch.tensor(bg.batch_num_nodes))
    M = torch.zeros(B, n, dtype=torch.float64)
    M[seg, torch.arange(n)] = 1.0 / torch.tensor(bg.batch_num_nodes, dtype=torch.float64)[seg]
    x = bg.ndata["x"].cpu().double()
    p = {k: v.double() for k, v in state.items()}

    def run(p, x, mask):
        pre = Ahat @ x @ p["conv1.weight"] + p["conv1.bias"]
        h1 = torch.relu(pre) if mask is None else pre * mask
        h2 = Ahat @ (h1 @ p["conv2.weight"]) + p["conv2.bias"]
        return pre, (M @ h2) @ p["out.weight"].t() + p["out.bias"]

    pre, logits = run(p, x, None)
    up = (torch.softmax(logits, 1) + Fn.one_hot(labels.cpu(), 2)) / B
    mag = {k: v.abs().requires_grad_(True) for k, v in p.items()}
    _, lm = run(mag, x.abs(), (pre > 0).double())
    (lm * up).sum().backward()
    return {k: v.grad for k, v in mag.items()}


def test_graph_classifier_trains_cpu():
    _, _, losses, _ = _first_step_and_training(torch.device("cpu"))
    assert losses[30] < losses[0]


@pytest.mark.gpu
def test_graph_classifier_trains_cuda():
    dev = _dev("cuda")
    state, g_dev, losses, _ = _first_step_and_training(dev)
    assert losses[30] < losses[0]
    state_c, g_cpu, _, bg = _first_step_and_training(torch.device("cpu"))
    _, labels = _dataset()
    bounds = _gradient_bounds(state_c, bg, labels)
    for k in g_cpu:
        err = (g_dev[k].double() - g_cpu[k].double()).abs()
        print(k, "max err / bound", float((err / (1e-5 * bounds[k])).nan_to_num().max()))
        assert (err <= 1e-5 * bounds[k]).all(), k
