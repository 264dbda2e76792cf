"""DGLSubGraph on the host: node and edge subgraphs through the native index,
feature copies to and from the parent, id maps and filters. The known answers
are the reference's (python/dgl/graph.py subgraph / edge_subgraph docstrings,
tests/graph_index/test_subgraph.py), restated. No GPU is used here."""
import pickle

import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import graph_index as gi
from dgl.base import DGLError


def cycle5():
    g = dgl.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2, 3, 4], [1, 2, 3, 4, 0])
    return g


def random_graph(n=30, m=120, seed=3, **kw):
    rng = np.random.default_rng(seed)
    g = dgl.DGLGraph(multigraph=True, **kw)
    g.add_nodes(n)
    g.add_edges(rng.integers(0, n, m), rng.integers(0, n, m))
    return g


def check_docstring_answer(sg):
    u, v = sg.edges()
    assert u.tolist() == [0, 2] and v.tolist() == [1, 0]
    assert sg.parent_nid.tolist() == [0, 1, 4]
    assert sg.parent_eid.tolist() == [0, 4]
    assert sg.number_of_nodes() == 3 and sg.number_of_edges() == 2
    assert isinstance(sg, dgl.DGLSubGraph) and isinstance(sg, dgl.DGLGraph)


def test_node_subgraph_known_answer():
    check_docstring_answer(cycle5().subgraph([0, 1, 4]))
    check_docstring_answer(cycle5().subgraph(torch.tensor([0, 1, 4])))
    check_docstring_answer(cycle5().subgraph(np.array([0, 1, 4])))


def test_edge_subgraph_known_answer():
    check_docstring_answer(cycle5().edge_subgraph([0, 4]))


def test_edge_subgraph_order_and_numbering():
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(4)
    g.add_edges([0, 0, 0, 2], [1, 1, 2, 3])
    sg = g.edge_subgraph([3, 2])
    assert sg.parent_eid.tolist() == [3, 2]
    assert sg.parent_nid.tolist() == [2, 3, 0]  # first appearance over (src, dst)
    u, v = sg.edges()
    pu, pv = g.find_edges(sg.parent_eid)
    assert torch.equal(sg.parent_nid[u], pu) and torch.equal(sg.parent_nid[v], pv)
    assert u.tolist() == [0, 2] and v.tolist() == [1, 0]


def test_node_subgraph_is_the_induced_edge_set():
    g = random_graph()
    sel = torch.tensor([17, 3, 9, 25, 0, 11, 4, 29, 8])
    sg = g.subgraph(sel)
    src, dst = g._graph.src(), g._graph.dst()
    pos = {int(v): i for i, v in enumerate(sel.tolist())}
    want = []  # the out-edges of sel[0], sel[1], ... in edge-id order
    for i, s in enumerate(sel.tolist()):
        for e in range(g.number_of_edges()):
            if int(src[e]) == s and int(dst[e]) in pos:
                want.append((i, pos[int(dst[e])], e))
    u, v = sg.edges()
    assert list(zip(u.tolist(), v.tolist(), sg.parent_eid.tolist())) == want
    assert torch.equal(sg.parent_nid, sel)


def test_copy_from_and_to_parent_round_trip():
    g = random_graph()
    n, m = g.number_of_nodes(), g.number_of_edges()
    g.ndata["h"] = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    g.edata["w"] = torch.arange(m, dtype=torch.float32).reshape(m, 1)
    sg = g.subgraph([5, 2, 20, 7, 13])
    assert len(sg.ndata) == 0 and len(sg.edata) == 0  # nothing before the copy
    sg.copy_from_parent()
    assert torch.equal(sg.ndata["h"], g.ndata["h"][sg.parent_nid])
    assert torch.equal(sg.edata["w"], g.edata["w"][sg.parent_eid])
    # a write on the subgraph is invisible to the parent ...
    before_h, before_w = g.ndata["h"].clone(), g.edata["w"].clone()
    sg.ndata["h"] = sg.ndata["h"] + 100.0
    sg.edata["w"] = sg.edata["w"] * -1.0 - 1.0
    assert torch.equal(g.ndata["h"], before_h) and torch.equal(g.edata["w"], before_w)
    # ... until copy_to_parent
    sg.copy_to_parent()
    want_h = before_h.clone()
    want_h[sg.parent_nid] += 100.0
    want_w = before_w.clone()
    want_w[sg.parent_eid] = before_w[sg.parent_eid] * -1.0 - 1.0
    assert torch.equal(g.ndata["h"], want_h) and torch.equal(g.edata["w"], want_w)


def test_copy_to_parent_inplace_keeps_storage():
    g = random_graph()
    n = g.number_of_nodes()
    g.ndata["h"] = torch.zeros(n, 2)
    col = g.ndata["h"]
    sg = g.subgraph([1, 2, 3])
    sg.copy_from_parent()
    sg.ndata["h"] = torch.ones(3, 2)
    sg.copy_to_parent(inplace=True)
    assert g.ndata["h"].data_ptr() == col.data_ptr()
    assert col[1:4].eq(1).all() and col.sum() == 6
    sg.ndata["h"] = torch.full((3, 2), 2.0)
    sg.copy_to_parent()  # out of place: a new column
    assert g.ndata["h"].data_ptr() != col.data_ptr() and g.ndata["h"].sum() == 12


def test_copy_from_parent_skips_an_empty_parent_frame():
    g = dgl.DGLGraph()
    g.add_nodes(4)  # no edges: the parent's edge frame has no rows
    g.ndata["h"] = torch.ones(4, 1)
    sg = g.subgraph([0, 2])
    sg.copy_from_parent()
    assert sg.ndata["h"].shape == (2, 1) and len(sg.edata) == 0
    sg.copy_to_parent()


def test_copy_from_parent_is_differentiable():
    g = random_graph()
    n = g.number_of_nodes()
    g.ndata["h"] = torch.arange(n * 4, dtype=torch.float32).reshape(n, 4) / 7.0
    g.ndata["h"].requires_grad_()
    sel = [4, 19, 8, 1, 22, 23, 10]
    sg = g.subgraph(sel)
    sg.copy_from_parent()
    sg.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
    weight = torch.arange(len(sel) * 4, dtype=torch.float32).reshape(len(sel), 4)
    (sg.ndata["o"] * weight).sum().backward()
    grad = g.ndata["h"].grad
    outside = torch.ones(n, dtype=torch.bool)
    outside[sel] = False
    assert grad[outside].eq(0).all() and grad[~outside].ne(0).any()
    # the same computation written with index_select
    h2 = g.ndata["h"].detach().clone().requires_grad_()
    u, v = sg.edges()
    o2 = torch.zeros(len(sel), 4).index_add(0, v, h2.index_select(0, sg.parent_nid)[u])
    (o2 * weight).sum().backward()
    assert torch.equal(sg.ndata["o"].detach(), o2.detach())
    assert torch.equal(grad, h2.grad)


def test_map_to_subgraph_nid():
    g = random_graph()
    sg = g.subgraph([9, 3, 27, 5])
    assert sg.map_to_subgraph_nid([5, 9, 27]).tolist() == [3, 0, 2]
    assert gi.map_to_subgraph_nid(sg._graph, torch.tensor([3])).tolist() == [1]
    sorted_sg = g.subgraph([3, 5, 9, 27])
    assert sorted_sg.map_to_subgraph_nid(torch.tensor([27, 3])).tolist() == [3, 0]


def test_subgraphs_equals_the_list_of_subgraph_calls():
    g = random_graph()
    sets = [[1, 2, 3, 4, 5], [20, 10, 0], []]
    many = g.subgraphs(sets)
    assert len(many) == 3
    for sg, sel in zip(many, sets):
        one = g.subgraph(sel)
        assert all(torch.equal(a, b) for a, b in zip(sg.edges(), one.edges()))
        assert torch.equal(sg.parent_nid, one.parent_nid)
        assert torch.equal(sg.parent_eid, one.parent_eid)
    idx = g._graph.node_subgraphs(sets)
    assert [i.number_of_nodes() for i in idx] == [5, 3, 0]


def test_subgraph_index_surface():
    g = random_graph()
    idx = g._graph.node_subgraph([7, 8, 9])
    assert isinstance(idx, gi.SubgraphIndex) and isinstance(idx, gi.GraphIndex)
    assert idx.has_native_index
    assert idx.induced_nodes.tolist() == [7, 8, 9]
    assert idx.induced_edges.numel() == idx.number_of_edges()
    assert idx.is_multigraph() and not idx.is_readonly()
    with pytest.raises(DGLError):
        idx.add_nodes(1)
    with pytest.raises(DGLError):
        idx.add_edges([0], [1])
    with pytest.raises(NotImplementedError):
        pickle.dumps(idx)
    eidx = g._graph.edge_subgraph([5, 1])
    assert eidx.induced_edges.tolist() == [5, 1] and eidx.number_of_edges() == 2


def test_mutation_and_shared_mode_raise():
    g = cycle5()
    sg = g.subgraph([0, 1])
    with pytest.raises(DGLError):
        sg.add_nodes(1)
    with pytest.raises(DGLError):
        sg.add_edge(0, 1)
    with pytest.raises(DGLError):
        sg.add_edges([0], [1])
    assert sg.number_of_nodes() == 2 and sg.number_of_edges() == 1
    idx = g._graph.node_subgraph([0, 1])
    with pytest.raises(DGLError):
        dgl.DGLSubGraph(g, idx.induced_nodes, idx.induced_edges, idx, shared=True)


def test_invalid_ids_raise():
    g = cycle5()
    with pytest.raises(DGLError):
        g.subgraph([0, 5])
    with pytest.raises(DGLError):
        g.subgraph([-1])
    with pytest.raises(DGLError):
        g.edge_subgraph([5])


def test_filter_nodes():
    g = cycle5()
    g.ndata["x"] = torch.tensor([[1.0], [-1.0], [1.0], [-1.0], [1.0]])

    def pred(nodes):
        assert isinstance(nodes, dgl.NodeBatch)
        return (nodes.data["x"] == 1).squeeze(1)

    assert g.filter_nodes(pred).tolist() == [0, 2, 4]
    assert g.filter_nodes(pred, [4, 3, 0, 1]).tolist() == [4, 0]
    assert g.filter_nodes(pred, torch.tensor([1, 3])).tolist() == []
    seen = []
    g.filter_nodes(lambda n: seen.append(n.nodes().tolist()) or torch.ones(len(n)).bool(), [3, 1])
    assert seen == [[3, 1]]
    sg =g.subgraph(g.filter_nodes(pred))
    assert sg.parent_nid.tolist() == [0, 2, 4] and sg.parent_eid.tolist() == [4]


def test_filter_edges():
    g = dgl.DGLGraph()
    g.add_nodes(3)
    g.ndata["x"] = torch.tensor([[1.0], [-1.0], [1.0]])
    g.add_edges([0, 1, 2], [2, 2, 1])
    g.edata["w"] = torch.tensor([0.5, 1.5, 2.5])

    def dst_one(edges):
        assert isinstance(edges, dgl.EdgeBatch)
        return (edges.dst["x"] == 1).squeeze(1)

    assert g.filter_edges(dst_one).tolist() == [0, 1]
    assert g.filter_edges(dst_one, [2, 1]).tolist() == [1]
    assert g.filter_edges(lambda e: e.data["w"] > 1).tolist() == [1, 2]
    assert g.filter_edges(lambda e: e.data["w"] > 1, [0, 2]).tolist() == [2]
    assert g.filter_edges(lambda e: e.src["x"][:, 0] < 0, ([1, 2], [2, 1])).tolist() == [1]


def test_readonly_parent_follows_the_immutable_rules():
    rng = np.random.default_rng(8)
    n, m = 25, 90
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    g = dgl.DGLGraph((src, dst), multigraph=True, readonly=True)
    assert g.number_of_nodes() <= n
    with pytest.raises(DGLError, match="has to be sorted"):
        g.subgraph([3, 1, 2])
    sel = [1, 2, 3, 8, 13]
    sg = g.subgraph(sel)
    assert sg.is_readonly and sg.parent_nid.tolist() == sel
    u, v, e = sg.all_edges("all", "eid")
    ps, pd = g.find_edges(sg.parent_eid)
    assert torch.equal(sg.parent_nid[u], ps[e]) and torch.equal(sg.parent_nid[v], pd[e])
    inside = np.isin(src, sel) & np.isin(dst, sel)
    assert sorted(sg.parent_eid.tolist()) == np.nonzero(inside)[0].tolist()
    with pytest.raises(DGLError):
        g.edge_subgraph([0])


def test_batched_graph_still_refuses_indexing():
    bg = dgl.batch([cycle5(), cycle5()])
    with pytest.raises(Exception):
        bg[0]
    assert isinstance(dgl.batch([cycle5().subgraph([0, 1, 4]), cycle5()]), dgl.BatchedDGLGraph)
