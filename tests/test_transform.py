"""dgl.transform on the host route: DGLGraph.line_graph and DGLGraph.reverse
against a checker written out in plain Python (a dict of out-edge lists walked
edge by edge, sharing no code with the package), on graphs built from explicit
edge lists so that nothing depends on another library's edge order."""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import transform
from dgl.base import DGLError
from dgl.kernel import LINE_GRAPH_TILE

N = 300
HUB = 7
NO_OUT = list(range(N - 15, N))  # 15 nodes without out-edges


def check_line_graph(src, dst, backtracking):
    """(lsrc, ldst) of the line graph of the edges (src[i], dst[i]): for every
    edge i = (u, v) in id order, the out-edges of v in id order, without those
    back to u unless backtracking."""
    out = {}
    for e, (u, v) in enumerate(zip(src, dst)):
        out.setdefault(u, []).append((e, v))
    lsrc, ldst = [], []
    for i, (u, v) in enumerate(zip(src, dst)):
        for e, w in out.get(v, ()):
            if backtracking or w != u:
                lsrc.append(i)
                ldst.append(e)
    return lsrc, ldst


def build(n, src, dst, multigraph=True):
    g = dgl.DGLGraph(multigraph=multigraph)
    g.add_nodes(n)
    if len(src):
        g.add_edges(np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64))
    return g


def edge_lists(L):
    u, v = L.edges()
    return u.tolist(), v.tolist()


def random_multigraph(tile=LINE_GRAPH_TILE):
    """(src, dst) of about 3,500 edges over N nodes in shuffled id order:
    duplicated edges, self loops, reciprocal pairs, nodes without out-edges and
    one hub whose out-edges span more than two tiles of candidates on their
    own. The properties are asserted, not assumed."""
    rng = np.random.default_rng(1313)
    hub_deg = 2 * tile + 37
    others = 3000
    sources = np.setdiff1d(np.arange(N), [HUB] + NO_OUT)
    src = rng.choice(sources, others)
    dst = rng.integers(0, N, others)
    src[:40], dst[:40] = src[40:80], dst[40:80]          # 40 duplicated edges
    dst[100:130] = src[100:130]                          # 30 self loops
    dst[300:400] = rng.choice(sources, 100)              # 100 reciprocal pairs
    src[200:300], dst[200:300] = dst[300:400], src[300:400]
    dst[400:412] = HUB                                   # the hub's in-edges
    hsrc = np.full(hub_deg, HUB)
    hdst = rng.integers(0, N, hub_deg)
    hdst[0] = HUB                                        # its self loop
    hdst[1:4] = src[400:403]                             # three reciprocal edges
    src, dst = np.concatenate([src, hsrc]), np.concatenate([dst, hdst])
    order = rng.permutation(src.size)
    src, dst = src[order], dst[order]
    outdeg, indeg = np.bincount(src, minlength=N), np.bincount(dst, minlength=N)
    pairs = set(zip(src.tolist(), dst.tolist()))
    assert src.size == others + hub_deg
    assert src.size - len(pairs) >= 40
    assert int((src == dst).sum()) >= 31
    assert sum(1 for (u, v) in pairs if u < v and (v, u) in pairs) >= 100
    assert int((outdeg == 0).sum()) >= 10 and indeg[outdeg == 0].sum() > 0
    assert outdeg[HUB] == hub_deg and indeg[HUB] >= 10 and (HUB, HUB) in pairs
    assert sum(1 for v in src[dst == HUB] if v != HUB and (HUB, int(v)) in pairs) >= 3
    assert not np.all(np.diff(src) >= 0)  # id order is not source order
    return src, dst


@pytest.fixture(scope="module")
def multigraph():
    src, dst = random_multigraph()
    want = {bt: check_line_graph(src.tolist(), dst.tolist(), bt) for bt in (True, False)}
    return src, dst, build(N, src, dst), want


def star():
    # centre 0, leaves 1..5, both directions
    src = [0] * 5 + [1, 2, 3, 4, 5]
    dst = [1, 2, 3, 4, 5] + [0] * 5
    return src, dst, build(6, src, dst, multigraph=False)


def test_star_graph_without_backtracking():
    src, dst, G = star()
    L = G.line_graph(backtracking=False)
    assert L.number_of_nodes() == 10 and not L.is_multigraph and not L.is_readonly
    linked = set(zip(*edge_lists(L)))
    for i in range(1, 6):
        out_e, in_e = int(G.edge_id(0, i)), int(G.edge_id(i, 0))
        assert (out_e, in_e) not in linked and (in_e, out_e) not in linked
    consecutive = {(i, j) for i in range(10) for j in range(10) if dst[i] == src[j]}
    reciprocal = {(i, j) for (i, j) in consecutive if dst[j] == src[i]}
    assert len(reciprocal) == 10
    assert linked == consecutive - reciprocal
    assert L.number_of_edges() == len(linked)
    assert set(zip(*edge_lists(G.line_graph()))) == consecutive


def test_shared_frames_are_one_object():
    src, dst, G = star()
    G.edata["h"] = torch.randn(10, 3)
    L = G.line_graph(backtracking=False, shared=True)
    assert L._node_frame is G._edge_frame
    assert torch.equal(L.ndata["h"], G.edata["h"])
    u, v = [0, 0, 3], [1, 4, 0]
    eids = G.edge_ids(u, v)
    L.nodes[eids].data["h"] = torch.zeros(3, 3)
    assert torch.equal(G.edges[u, v].data["h"], torch.zeros(3, 3))
    assert int((G.edata["h"] != 0).any(1).sum()) == 7
    L.ndata["w"] = torch.arange(10.0)
    assert torch.equal(G.edata["w"], torch.arange(10.0))
    G.edata["z"] = torch.ones(10, 2)
    assert torch.equal(L.ndata["z"], torch.ones(10, 2))
    assert dgl.line_graph(G)._node_frame is not G._edge_frame


@pytest.mark.parametrize("backtracking", [True, False])
def test_host_route_equals_the_checker(multigraph, backtracking):
    src, dst, g, want = multigraph
    L = g.line_graph(backtracking=backtracking)
    assert L.number_of_nodes() == src.size
    got = edge_lists(L)
    assert got[0] == want[backtracking][0] and got[1] == want[backtracking][1]
    removed = len(want[True][0]) - len(want[False][0])
    assert removed > 0
    if not backtracking:
        indeg, outdeg = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
        assert len(want[True][0]) == int((indeg * outdeg).sum())


def test_known_answers():
    # 0->1, 1->2, 1->0: edge 0 is followed by edges 1 and 2, edge 2 by edge 0
    g = build(3, [0, 1, 1], [1, 2, 0])
    assert edge_lists(g.line_graph()) == ([0, 0, 2], [1, 2, 0])
    assert edge_lists(g.line_graph(backtracking=False)) == ([0], [1])
    # the star, by brute force over its edge list
    src, dst, G = star()
    exp = [(i, j) for i in range(10) for j in range(10) if src[j] == dst[i]]
    assert list(zip(*edge_lists(transform.line_graph(G)))) == exp
    # a self loop links to every out-edge of its node, itself included; with
    # backtracking off to none of the node's self loops. Parallel edges are
    # distinct line-graph nodes
    g = build(2, [0, 0, 0, 0], [0, 0, 1, 1])
    assert edge_lists(g.line_graph()) == ([0] * 4 + [1] * 4, [0, 1, 2, 3] * 2)
    assert edge_lists(g.line_graph(backtracking=False)) == ([0, 0, 1, 1], [2, 3, 2, 3])


def test_readonly_parent_raises():
    g = dgl.DGLGraph(([0, 1], [1, 0]), readonly=True)
    with pytest.raises(DGLError, match="immutable"):
        g.line_graph()
    with pytest.raises(DGLError, match="immutable"):
        dgl.line_graph(g, backtracking=False, shared=True)


@pytest.mark.parametrize("backtracking", [True, False])
def test_batched_graph_gives_the_disjoint_union(backtracking):
    a = build(3, [0, 1, 1, 2], [1, 0, 2, 1])
    b = build(4, [0, 1, 2, 3, 3], [1, 2, 3, 0, 3])
    bg = dgl.batch([a, b])
    L = bg.line_graph(backtracking=backtracking, shared=True)
    assert L._node_frame is bg._edge_frame
    la, lb = (edge_lists(x.line_graph(backtracking=backtracking)) for x in (a, b))
    off = a.number_of_edges()
    assert L.number_of_nodes() == off + b.number_of_edges()
    assert edge_lists(L) == (la[0] + [i + off for i in lb[0]], la[1] + [i + off for i in lb[1]])


def test_result_can_be_mutated():
    g = build(3, [0, 1, 1], [1, 2, 0])
    L = g.line_graph()
    L.add_nodes(1)
    L.add_edge(3, 0)
    assert L.number_of_nodes() == 4
    assert edge_lists(L) == ([0, 0, 2, 3], [1, 2, 0, 0])


def test_reverse_structure_and_frames():
    src, dst = [0, 1, 2, 2, 2], [1, 2, 0, 0, 3]
    g = build(5, src, dst)
    g.ndata["h"] = torch.randn(5, 2)
    g.edata["w"] = torch.randn(5, 2)
    rg = g.reverse()
    assert rg.is_multigraph and not rg.is_readonly
    assert rg.number_of_nodes() == 5 and rg.number_of_edges() == 5
    assert edge_lists(rg) == (dst, src)
    assert len(rg.ndata) == 0 and len(rg.edata) == 0
    assert not build(2, [0], [1], multigraph=False).reverse().is_multigraph
    simple = build(4, [0, 1, 2, 0], [1, 2, 3, 3], multigraph=False)
    rs = dgl.reverse(simple)
    for u, v in zip([0, 1, 2, 0], [1, 2, 3, 3]):
        assert int(rs.edge_id(v, u)) == int(simple.edge_id(u, v))
    shared = g.reverse(share_ndata=True, share_edata=True)
    assert shared._node_frame is g._node_frame and shared._edge_frame is g._edge_frame
    g.ndata["h"] = g.ndata["h"] + 1
    assert torch.equal(shared.ndata["h"], g.ndata["h"])
    only_n = transform.reverse(g, share_ndata=True)
    assert only_n._node_frame is g._node_frame and len(only_n.edata) == 0


def test_reverse_transposes_the_aggregation():
    rng = np.random.default_rng(5)
    src, dst = rng.integers(0, 20, 90), rng.integers(0, 20, 90)
    g = build(20, src, dst)
    h = torch.from_numpy(rng.integers(-8, 8, (20, 3)).astype(np.float32))  # exact sums
    g.ndata["h"] = h
    rg = g.reverse(share_ndata=True)
    rg.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
    want = torch.zeros(20, 3).index_add_(0, torch.from_numpy(src), h[torch.from_numpy(dst)])
    assert torch.equal(rg.ndata["o"], want)


def test_reverse_rejects_a_batched_graph():
    bg = dgl.batch([build(2, [0], [1]), build(2, [1], [0])])
    with pytest.raises(DGLError, match="Batched"):
        bg.reverse()
