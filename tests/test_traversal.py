"""dgl.traversal and dgl.propagate on the host route (the native index,
csrc/graph_traversal.cc): known answers, exact order against a Python
restatement of the queue loops, and prop_nodes / prop_edges."""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl.base import DGLError

FORWARD, REVERSE, NONTREE = 0, 1, 2
DOC_EDGES = [(0, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5)]


# ---------------------------------------------------------------- the checker
def slot_rows(n, src, dst, reverse=False):
    """rows[u] = [(neighbour, edge id), ...] in edge-id order: the mutable
    index's slot order."""
    rows = [[] for _ in range(n)]
    for e, (u, v) in enumerate(zip(src, dst)):
        if reverse:
            u, v = v, u
        rows[int(u)].append((int(v), e))
    return rows


def csr_rows(g, reverse=False):
    """The same from the index's own CSR (a read-only index sorts each row)."""
    indptr, indices, eid = (t.tolist() for t in g._graph.get_adj(not reverse, "csr"))
    return [list(zip(indices[indptr[u]:indptr[u + 1]], eid[indptr[u]:indptr[u + 1]]))
            for u in range(len(indptr) - 1)]


def check_bfs(rows, source):
    """(node frontiers, edge frontiers) of the one-queue BFS."""
    visited, nodes, edges = set(source), [list(source)], []
    while nodes[-1]:
        nn, ee = [], []
        for u in nodes[-1]:
            for v, e in rows[u]:
                if v not in visited:
                    visited.add(v)
                    nn.append(v)
                    ee.append(e)
        nodes.append(nn)
        edges.append(ee)
    return nodes[:-1], edges[:-1]


def check_topo(rows):
    """Kahn's frontiers; the counters are the degrees in the other direction."""
    remain = [0] * len(rows)
    for row in rows:
        for v, _ in row:
            remain[v] += 1
    out = [[v for v in range(len(rows)) if remain[v] == 0]]
    while out[-1]:
        nn = []
        for u in out[-1]:
            for v, _ in rows[u]:
                remain[v] -= 1
                if remain[v] == 0:
                    nn.append(v)
        out.append(nn)
    return out[:-1]


def check_dfs(rows, sources, has_reverse_edge=False, has_nontree_edge=False):
    """(edge frontiers, label frontiers): one trace per source, zipped."""
    traces = []
    for s in sources:
        trace, visited = [], {s}
        stack = [(s, iter(rows[s]), None)]  # (node, its remaining slots, the edge that led here)
        while stack:
            u, it, via = stack[-1]
            step = next(it, None)
            if step is None:
                stack.pop()
                if via is not None and has_reverse_edge:
                    trace.append((via, REVERSE))
                continue
            v, e = step
            if v in visited:
                if has_nontree_edge:
                    trace.append((e, NONTREE))
            else:
                visited.add(v)
                trace.append((e, FORWARD))
                stack.append((v, iter(rows[v]), e))
        traces.append(trace)
    depth = max([len(t) for t in traces] + [0])
    zipped = [[t[i] for t in traces if i < len(t)] for i in range(depth)]
    return [[e for e, _ in f] for f in zipped], [[l for _, l in f] for f in zipped]


def as_lists(frontiers):
    assert isinstance(frontiers, tuple)
    for f in frontiers:
        assert f.dtype == torch.int64 and f.dim() == 1 and f.numel() > 0
    return [f.tolist() for f in frontiers]


# ---------------------------------------------------------------- known answers
def test_docstring_answers():
    g = dgl.DGLGraph(DOC_EDGES)
    assert as_lists(dgl.bfs_nodes_generator(g, 0)) == [[0], [1], [2, 3], [4, 5]]
    assert as_lists(dgl.bfs_edges_generator(g, 0)) == [[0], [1, 2], [4, 5]]
    assert as_lists(dgl.topological_nodes_generator(g)) == [[0], [1], [2], [3, 4], [5]]
    assert as_lists(dgl.dfs_edges_generator(g, 0)) == [[0], [1], [3], [5], [4]]
    edges, labels = dgl.dfs_labeled_edges_generator(g, 0, has_nontree_edge=True)
    assert as_lists(edges) == [[0], [1], [3], [5], [4], [2]]
    assert as_lists(labels) == [[0], [0], [0], [0], [0], [2]]
    assert as_lists(dgl.traversal.bfs_nodes_generator(g, torch.tensor([0]))) == \
        [[0], [1], [2, 3], [4, 5]]


def test_two_tree_labeled_dfs():
    src, dst = [0, 1, 0, 3, 3], [1, 2, 2, 4, 5]
    g = dgl.DGLGraph()
    g.add_nodes(6)
    g.add_edges(src, dst)
    edges, labels = dgl.dfs_labeled_edges_generator(g, [0, 3], has_reverse_edge=True,
                                                    has_nontree_edge=True)
    want_e, want_l = check_dfs(slot_rows(6, src, dst), [0, 3], True, True)
    assert as_lists(edges) == want_e
    assert as_lists(labels) == want_l
    # the two traces side by side: 0->1, 1->2 down and up, then 0->2 non-tree;
    # 3->4 and 3->5 down and up
    assert want_e == [[0, 3], [1, 3], [1, 4], [0, 4], [2]]
    assert want_l == [[0, 0], [0, 1], [1, 0], [1, 1], [2]]
    only = dgl.dfs_labeled_edges_generator(g, [0, 3], has_reverse_edge=True,
                                           has_nontree_edge=True, return_labels=False)
    assert as_lists(only) == want_e


# ---------------------------------------------------------------- random multigraph
N = 500
NO_OUT = list(range(470, N))  # nodes without out-edges


class Multigraph(object):
    def __init__(self):
        rng = np.random.default_rng(7)
        m = 3000
        src = rng.integers(0, 470, m)
        dst = rng.integers(0, N, m)
        dst[:60] = src[:60]                                   # self loops
        src[100:160], dst[100:160] = src[200:260], dst[200:260]  # duplicate edges
        src[-1], dst[-1] = 0, N - 1                           # the edge list names node N - 1
        self.src, self.dst = src.tolist(), dst.tolist()
        assert sum(u == v for u, v in zip(self.src, self.dst)) >= 60
        assert len(set(zip(self.src, self.dst))) <= m - 40
        assert not set(self.src) & set(NO_OUT)
        self.mutable = dgl.DGLGraph(multigraph=True)
        self.mutable.add_nodes(N)
        self.mutable.add_edges(self.src, self.dst)
        self.readonly = dgl.DGLGraph((self.src, self.dst), multigraph=True, readonly=True)
        assert self.readonly.number_of_nodes() == N
        few = rng.choice(470, 6, replace=False).tolist()
        self.sources = {"single": [few[0]], "several_with_repeat": few + [few[2]],
                        "no_out_edges": [NO_OUT[3]]}

    def graph(self, kind):
        return self.mutable if kind == "mutable" else self.readonly

    def rows(self, kind, reverse):
        if kind == "mutable":
            return slot_rows(N, self.src, self.dst, reverse)
        return csr_rows(self.readonly, reverse)


@pytest.fixture(scope="module")
def mg():
    return Multigraph()


CASES = [(k, r, s) for k in ("mutable", "readonly") for r in (False, True)
         for s in ("single", "several_with_repeat", "no_out_edges")]


@pytest.mark.parametrize("kind,reverse,name", CASES)
def test_bfs_equals_checker(mg, kind, reverse, name):
    g, source = mg.graph(kind), mg.sources[name]
    nodes, edges = check_bfs(mg.rows(kind, reverse), source)
    assert as_lists(dgl.bfs_nodes_generator(g, source, reverse)) == nodes
    assert as_lists(dgl.bfs_edges_generator(g, source, reverse)) == edges
    assert nodes[0] == source
    if name == "no_out_edges" and not reverse:
        assert nodes == [source] and edges == []
    if name == "single" and not reverse:
        assert len(nodes) >= 3


@pytest.mark.parametrize("kind,reverse,name", CASES)
def test_dfs_equals_checker(mg, kind, reverse, name):
    g, source = mg.graph(kind), mg.sources[name]
    rows = mg.rows(kind, reverse)
    assert as_lists(dgl.dfs_edges_generator(g, source, reverse)) == check_dfs(rows, source)[0]
    for rev, non in ((True, False), (False, True), (True, True)):
        want_e, want_l = check_dfs(rows, source, rev, non)
        got_e, got_l = dgl.dfs_labeled_edges_generator(g, source, reverse, rev, non)
        assert as_lists(got_e) == want_e
        assert as_lists(got_l) == want_l


@pytest.mark.parametrize("reverse", [False, True])
def test_bfs_layers_equal_networkx(mg, reverse):
    nx = pytest.importorskip("networkx")
    G = nx.MultiDiGraph()
    G.add_nodes_from(range(N))
    G.add_edges_from(zip(mg.dst, mg.src) if reverse else zip(mg.src, mg.dst))
    source = mg.sources["several_with_repeat"]
    want = [set(layer) for layer in nx.bfs_layers(G, list(dict.fromkeys(source)))]
    for kind in ("mutable", "readonly"):
        got = dgl.bfs_nodes_generator(mg.graph(kind), source, reverse)
        assert [set(f.tolist()) for f in got] == want


# ---------------------------------------------------------------- topological
def random_dag(seed=11, n=N, m=2500):
    """Edges of a DAG whose ids are not in topological order, with multi-edges
    and isolated nodes; node n - 1 has an edge, so that an index built from
    the edge list alone has n nodes."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n - 20, m), rng.integers(0, n - 20, m)  # the last 20 stay isolated
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    lo[:50], hi[:50] = lo[50:100], hi[50:100]  # multi-edges
    perm = rng.permutation(n)
    j = int(np.flatnonzero(perm == n - 1)[0])
    perm[j], perm[lo[0]] = perm[lo[0]], n - 1
    return perm[lo].tolist(), perm[hi].tolist(), sorted(perm[n - 20:].tolist())


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("readonly", [False, True])
def test_topological_equals_checker(reverse, readonly):
    src, dst, isolated = random_dag()
    assert len(set(zip(src, dst))) < len(src) and len(isolated) == 20
    if readonly:
        g = dgl.DGLGraph((src, dst), multigraph=True, readonly=True)
        rows = csr_rows(g, reverse)
    else:
        g = dgl.DGLGraph(multigraph=True)
        g.add_nodes(N)
        g.add_edges(src, dst)
        rows = slot_rows(N, src, dst, reverse)
    assert g.number_of_nodes() == N
    want = check_topo(rows)
    assert sum(len(f) for f in want) == N and len(want) > 3
    assert set(isolated) <= set(want[0]) and want[0] == sorted(want[0])
    assert any(f != sorted(f) for f in want[1:])  # later frontiers are in queue order
    assert as_lists(dgl.topological_nodes_generator(g, reverse)) == want


def test_topological_loop_and_empty():
    g = dgl.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2, 3], [1, 2, 3, 1])  # 1 -> 2 -> 3 -> 1
    with pytest.raises(DGLError, match="loop"):
        dgl.topological_nodes_generator(g)
    with pytest.raises(DGLError, match="loop"):
        dgl.topological_nodes_generator(g, reverse=True)
    assert dgl.topological_nodes_generator(dgl.DGLGraph()) == ()
    assert dgl.topological_nodes_generator(dgl.DGLGraph(), ctx=None) == ()


# ---------------------------------------------------------------- errors, registry
def test_errors_and_registry(mg):
    for g in (mg.mutable, mg.readonly):
        for bad in ([N], [-1], [3, 2 ** 40]):
            for gen in (dgl.bfs_nodes_generator, dgl.bfs_edges_generator, dgl.dfs_edges_generator,
                        dgl.dfs_labeled_edges_generator):
                with pytest.raises(DGLError):
                    gen(g, bad)
        assert dgl.bfs_nodes_generator(g, []) == ()
        assert dgl.bfs_edges_generator(g, torch.zeros(0, dtype=torch.int64)) == ()
        assert dgl.dfs_edges_generator(g, []) == ()
        assert dgl.dfs_labeled_edges_generator(g, []) == ((), ())
    names = dgl.list_global_func_names()
    for n in ("DGLBFSNodes", "DGLBFSEdges", "DGLTopologicalNodes", "DGLDFSEdges",
              "DGLDFSLabeledEdges"):
        assert "traversal._CAPI_" + n in names


def test_exports():
    for name in ("bfs_nodes_generator", "bfs_edges_generator", "topological_nodes_generator",
                 "dfs_edges_generator", "dfs_labeled_edges_generator"):
        assert getattr(dgl, name) is getattr(dgl.traversal, name)
    for name in ("prop_nodes", "prop_edges", "prop_nodes_bfs", "prop_nodes_topo",
                 "prop_edges_dfs"):
        assert getattr(dgl, name) is getattr(dgl.propagate, name)


# ---------------------------------------------------------------- propagation
def demo_graph():
    g = dgl.DGLGraph()
    g.add_nodes(4)
    g.ndata["x"] = torch.tensor([[1.], [2.], [3.], [4.]])
    g.add_edges([0, 1, 1, 2], [1, 2, 3, 3])
    g.register_message_func(lambda edges: {"m": edges.src["x"]})
    g.register_reduce_func(lambda nodes: {"x": nodes.mailbox["m"].sum(1)})
    return g


def test_prop_docstring_examples():
    g = demo_graph()
    g.prop_nodes([[1, 2], [3]])
    assert g.ndata["x"].flatten().tolist() == [1, 1, 2, 3]
    g = demo_graph()
    g.prop_edges([([0, 1], [1, 3]), ([1, 2], [2, 3])])
    assert g.ndata["x"].flatten().tolist() == [1, 1, 1, 3]
    g = demo_graph()
    dgl.prop_nodes(g, [[1, 2], [3]])
    assert g.ndata["x"].flatten().tolist() == [1, 1, 2, 3]
    g = demo_graph()
    dgl.prop_edges(g, [([0, 1], [1, 3]), ([1, 2], [2, 3])])
    assert g.ndata["x"].flatten().tolist() == [1, 1, 1, 3]


def random_trees(seed=3, count=8):
    """``count`` trees of 15 to 40 nodes, edges child -> parent, with an
    integer-valued feature 'x'; (batched graph, [(parent list, x list)])."""
    rng = np.random.default_rng(seed)
    graphs, specs = [], []
    for _ in range(count):
        n = int(rng.integers(15, 41))
        label = rng.permutation(n)  # node ids are not in tree order
        parent = [-1] * n
        for k in range(1, n):
            parent[label[k]] = int(label[rng.integers(0, k)])
        x = rng.integers(-5, 6, n).astype(np.float32)
        g = dgl.DGLGraph()
        g.add_nodes(n)
        child = [v for v in range(n) if parent[v] >= 0]
        g.add_edges(child, [parent[v] for v in child])
        g.ndata["x"] = torch.from_numpy(x).reshape(n, 1)
        graphs.append(g)
        specs.append((parent, x.tolist()))
    return dgl.batch(graphs), specs


def subtree_sums(specs):
    out = []
    for parent, x in specs:
        kids = [[] for _ in parent]
        for v, p in enumerate(parent):
            if p >= 0:
                kids[p].append(v)

        def total(v):
            return x[v] + sum(total(c) for c in kids[v])
        out.extend(total(v) for v in range(len(parent)))
    return out


def add_own(nodes):
    return {"h": nodes.data["s"] + nodes.data["x"]}


def test_prop_nodes_topo_subtree_sums():
    bg, specs = random_trees()
    n = bg.number_of_nodes()
    bg.ndata["s"] = torch.zeros(n, 1)
    bg.ndata["h"] = torch.zeros(n, 1)
    dgl.prop_nodes_topo(bg, message_func=fn.copy_src("h", "m"), reduce_func=fn.sum("m", "s"),
                        apply_node_func=add_own)
    assert bg.ndata["h"].flatten().tolist() == subtree_sums(specs)


def test_prop_nodes_bfs_equals_manual_pull(mg):
    def run(g, frontiers=None):
        g.ndata["h"] = torch.arange(N, dtype=torch.float32).reshape(N, 1) % 7
        kw = dict(message_func=fn.copy_src("h", "m"), reduce_func=fn.sum("m", "h"))
        if frontiers is None:
            dgl.prop_nodes_bfs(g, source, **kw)
        else:
            for f in frontiers:
                g.pull(f, **kw)
        return g.ndata["h"].clone()

    source = mg.sources["several_with_repeat"]
    g = mg.mutable
    want = run(g, check_bfs(slot_rows(N, mg.src, mg.dst), source)[0])
    got = run(g)
    assert torch.equal(got, want)
    assert not torch.equal(got, torch.arange(N, dtype=torch.float32).reshape(N, 1) % 7)


def test_prop_edges_dfs_equals_manual_send_and_recv(mg):
    def run(g, frontiers=None):
        g.ndata["h"] = torch.arange(N, dtype=torch.float32).reshape(N, 1) % 5
        kw = dict(message_func=fn.copy_src("h", "m"), reduce_func=fn.sum("m", "h"))
        if frontiers is None:
            dgl.prop_edges_dfs(g, source, has_reverse_edge=True, **kw)
        else:
            for f in frontiers:
                g.send_and_recv(f, **kw)
        return g.ndata["h"].clone()

    source = mg.sources["single"]
    g = mg.mutable
    want = run(g, check_dfs(slot_rows(N, mg.src, mg.dst), source, has_reverse_edge=True)[0])
    got = run(g)
    assert torch.equal(got, want)
    assert not torch.equal(got, torch.arange(N, dtype=torch.float32).reshape(N, 1) % 5)
