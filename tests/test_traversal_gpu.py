"""The device route of the BFS and topological generators (a cuda ``source`` /
``ctx``; csrc/traversal.hip) pinned against the host route of the same graph
(the native index), and both against a Python restatement of the queue loops:
the same frontiers, element for element, sections included.

Every error case here is rejected by the kernels' validation before any
dependent access: an invalid id is counted, never used as an index."""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl.base import DGLError
from dgl.kernel import TRAVERSAL_CHUNK

pytestmark = pytest.mark.gpu

N = 2000
MAIN = 1700                           # nodes [0, MAIN) carry the random edges
HUB, TARGET, PATH_FROM = 7, 11, 23
HUB_DEG = 4 * TRAVERSAL_CHUNK + 37    # more than four items, the last one partial
ISLAND = list(range(1700, 1900))      # a component no test source outside it reaches
PATH = list(range(1900, 1970))        # PATH_FROM -> 1900 -> 1901 -> ... -> 1969
NO_OUT = list(range(1970, 1995))      # 25 nodes with in-edges only; 1995.. are isolated


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


def lists(frontiers):
    assert isinstance(frontiers, tuple)
    return [f.tolist() for f in frontiers]


def on_device(frontiers):
    for f in frontiers:
        assert f.is_cuda and f.dtype == torch.int64 and f.dim() == 1 and f.numel() > 0


def same_frontiers(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.cpu(), y.cpu())


# ---------------------------------------------------------------- the graph
class Case(object):
    """The graph (built once), its sources, and the host answers (computed
    once, left as they are)."""

    def __init__(self):
        rng = np.random.default_rng(2025)
        m = 9000
        src = rng.integers(0, MAIN, m)
        dst = rng.choice(np.concatenate([np.arange(MAIN), NO_OUT]), m)
        dst[:40] = src[:40]                                       # self loops
        src[100:150], dst[100:150] = src[200:250], dst[200:250]   # duplicate edges
        hub_dst = rng.integers(0, MAIN, HUB_DEG)
        hub_dst[hub_dst == TARGET] = TARGET + 1                   # TARGET is found a level later
        racers = np.setdiff1d(hub_dst, [HUB, TARGET])[:400]       # one BFS level, all -> TARGET
        isl_src, isl_dst = rng.choice(ISLAND, 600), rng.choice(ISLAND, 600)
        path_src, path_dst = [PATH_FROM] + PATH[:-1], PATH
        src = np.concatenate([src, np.full(HUB_DEG, HUB), racers, isl_src, path_src])
        dst = np.concatenate([dst, hub_dst, np.full(racers.size, TARGET), isl_dst, path_dst])
        order = rng.permutation(src.size)  # rows' slots are not contiguous in the edge list
        self.src, self.dst = src[order].tolist(), dst[order].tolist()
        self.E = len(self.src)
        g = dgl.DGLGraph(multigraph=True)
        g.add_nodes(N)
        g.add_edges(self.src, self.dst)
        self.g = g
        self.rows = {r: slot_rows(N, self.src, self.dst, r) for r in (False, True)}
        self.sources = {
            "hub": [HUB],
            "random300": rng.choice(N, 300, replace=False).tolist(),
            "repeated": [5, HUB, 42, 5, 1200, 42],
            "no_out_edges": [NO_OUT[4]],
            "island": [ISLAND[10]],
        }
        self._host = {}
        self.check_properties(racers)

    def check_properties(self, racers):
        out_deg = np.bincount(self.src, minlength=N)
        in_deg = np.bincount(self.dst, minlength=N)
        assert 11500 <= self.E <= 12500
        assert out_deg[HUB] >= HUB_DEG > 4 * TRAVERSAL_CHUNK and HUB_DEG % TRAVERSAL_CHUNK
        assert in_deg[TARGET] >= 400 and racers.size == 400
        assert sum(u == v for u, v in zip(self.src, self.dst)) >= 30
        assert self.E - len(set(zip(self.src, self.dst))) >= 40
        assert int((out_deg[NO_OUT] == 0).sum()) == 25 and int((in_deg[NO_OUT] > 0).sum()) > 15
        nodes, _ = check_bfs(self.rows[False], [HUB])
        reached = set(v for f in nodes for v in f)
        assert not reached & set(ISLAND) and set(PATH) <= reached
        assert len(nodes) >= 70 and sum(len(f) == 1 for f in nodes) >= 60
        assert max(len(f) for f in nodes) > 256
        # the claim race: TARGET is discovered in the level in which the hub's
        # targets are expanded, by hundreds of candidates of that one level
        level = next(i for i, f in enumerate(nodes) if TARGET in f)
        assert len(set(nodes[level - 1]) & set(racers.tolist())) > 300
        back = set(v for f in check_bfs(self.rows[True], [ISLAND[10]])[0] for v in f)
        assert back <= set(ISLAND)

    def host(self, kind, name, reverse):
        key = (kind, name, reverse)
        if key not in self._host:
            gen = dgl.bfs_nodes_generator if kind == "nodes" else dgl.bfs_edges_generator
            self._host[key] = gen(self.g, self.sources[name], reverse)
        return self._host[key]

    def device_source(self, name):
        return torch.tensor(self.sources[name], dtype=torch.int64).cuda()


@pytest.fixture(scope="module")
def case():
    return Case()


# ---------------------------------------------------------------- BFS
SOURCES = ["hub", "random300", "repeated", "no_out_edges", "island"]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", SOURCES)
def test_bfs_device_equals_host_equals_checker(case, name, reverse):
    source = case.device_source(name)
    dev_nodes = dgl.bfs_nodes_generator(case.g, source, reverse)
    dev_edges = dgl.bfs_edges_generator(case.g, source, reverse)
    on_device(dev_nodes)
    on_device(dev_edges)
    want_nodes, want_edges = check_bfs(case.rows[reverse], case.sources[name])
    host_nodes, host_edges = case.host("nodes", name, reverse), case.host("edges", name, reverse)
    assert not host_nodes[0].is_cuda
    assert lists(host_nodes) == want_nodes and lists(host_edges) == want_edges
    assert lists(dev_nodes) == want_nodes and lists(dev_edges) == want_edges
    same_frontiers(dev_nodes, host_nodes)
    same_frontiers(dev_edges, host_edges)
    # edge frontier i discovered node frontier i + 1, position by position
    assert [len(f) for f in dev_edges] == [len(f) for f in dev_nodes[1:]]
    ends = torch.tensor(case.src if reverse else case.dst)
    for e, v in zip(dev_edges, dev_nodes[1:]):
        assert torch.equal(ends[e.cpu()], v.cpu())
    assert dev_nodes[0].tolist() == case.sources[name]
    if name == "hub" and not reverse:
        assert len(dev_nodes) >= 70 and len(dev_nodes[1]) > TRAVERSAL_CHUNK
    if name == "no_out_edges" and not reverse:
        assert len(dev_nodes) == 1 and dev_edges == ()
    if name == "island":
        assert set(v for f in want_nodes for v in f) <= set(ISLAND)


# ---------------------------------------------------------------- topological
def dag_part(case, seed=5):
    """The edges of the fixture graph with relabelled src < dst, multi-edges
    kept, as a graph over the new labels."""
    perm = np.random.default_rng(seed).permutation(N)
    j = int(np.flatnonzero(perm == 100)[0])
    perm[j], perm[HUB] = perm[HUB], 100  # most of the hub's edges point upwards
    src, dst = perm[np.asarray(case.src)], perm[np.asarray(case.dst)]
    keep = src < dst
    src, dst = src[keep].tolist(), dst[keep].tolist()
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(N)
    g.add_edges(src, dst)
    assert max(np.bincount(src, minlength=N)) > TRAVERSAL_CHUNK
    assert len(src) - len(set(zip(src, dst))) >= 10
    return g, src, dst


@pytest.fixture(scope="module")
def dag(case):
    return dag_part(case)


@pytest.mark.parametrize("reverse", [False, True])
def test_topological_device_equals_host_equals_checker(dag, reverse):
    g, src, dst = dag
    want = check_topo(slot_rows(N, src, dst, reverse))
    assert sum(len(f) for f in want) == N and len(want) > 5
    host = dgl.topological_nodes_generator(g, reverse)
    dev = dgl.topological_nodes_generator(g, reverse, ctx="cuda")
    on_device(dev)
    assert not host[0].is_cuda
    assert lists(host) == want
    assert lists(dev) == want
    same_frontiers(dev, host)
    again = dgl.topological_nodes_generator(g, reverse, ctx=torch.device("cuda", 0))
    same_frontiers(again, dev)


def test_topological_cycle_and_isolated_nodes():
    g = dgl.DGLGraph()
    g.add_nodes(6)
    g.add_edges([0, 1, 2, 3, 3], [1, 2, 3, 1, 4])  # 1 -> 2 -> 3 -> 1
    for reverse in (False, True):
        with pytest.raises(DGLError, match="loop"):
            dgl.topological_nodes_generator(g, reverse, ctx="cuda")
    g = dgl.DGLGraph()
    g.add_nodes(300)
    (only,) = dgl.topological_nodes_generator(g, ctx="cuda")
    assert only.is_cuda and torch.equal(only.cpu(), torch.arange(300))
    assert dgl.topological_nodes_generator(dgl.DGLGraph(), ctx="cuda") == ()


# ---------------------------------------------------------------- repeatability
def test_device_route_is_repeatable(case, dag):
    source = case.device_source("random300")
    for gen in (dgl.bfs_nodes_generator, dgl.bfs_edges_generator):
        a, b = gen(case.g, source), gen(case.g, source)
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    a = dgl.topological_nodes_generator(dag[0], ctx="cuda")
    b = dgl.topological_nodes_generator(dag[0], ctx="cuda")
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- errors
def test_invalid_and_empty_sources(case):
    for bad in ([3, N], [-1], [2 ** 40, 5], [N, -1, 2 ** 40]):
        source = torch.tensor(bad, dtype=torch.int64).cuda()
        for gen in (dgl.bfs_nodes_generator, dgl.bfs_edges_generator):
            for reverse in (False, True):
                with pytest.raises(DGLError, match="Invalid source"):
                    gen(case.g, source, reverse)
    empty = torch.zeros(0, dtype=torch.int64).cuda()
    assert dgl.bfs_nodes_generator(case.g, empty) == ()
    assert dgl.bfs_edges_generator(case.g, empty, reverse=True) == ()
    # the route still works after the refusals
    same_frontiers(dgl.bfs_nodes_generator(case.g, case.device_source("repeated")),
                   case.host("nodes", "repeated", False))


def test_capture_is_refused_before_anything_is_launched(case, dag):
    source = case.device_source("repeated")
    dgl.bfs_nodes_generator(case.g, source)  # warm: the adjacency is cached
    dgl.topological_nodes_generator(dag[0], ctx="cuda")
    x = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x.add_(1.0)
            with pytest.raises(DGLError, match="captured"):
                dgl.bfs_nodes_generator(case.g, source)
            with pytest.raises(DGLError, match="captured"):
                dgl.bfs_edges_generator(case.g, source)
            with pytest.raises(DGLError, match="captured"):
                dgl.topological_nodes_generator(dag[0], ctx="cuda")
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 4  # the capture holds the one add, nothing else
    same_frontiers(dgl.bfs_nodes_generator(case.g, source), case.host("nodes", "repeated", False))


def test_readonly_parent_takes_the_host_route(case):
    ro = dgl.DGLGraph((case.src + [0], case.dst + [N - 1]), multigraph=True, readonly=True)
    assert ro.number_of_nodes() == N
    source = case.device_source("repeated")
    for gen in (dgl.bfs_nodes_generator, dgl.bfs_edges_generator):
        host = gen(ro, case.sources["repeated"])
        dev = gen(ro, source)
        on_device(dev)
        same_frontiers(dev, host)
    assert ("adj", "cuda:0") not in ro._graph._cache  # nothing was built on the device


# ---------------------------------------------------------------- propagation
def random_trees(seed=3, count=8):
    """``count`` trees of 15 to 40 nodes, edges child -> parent, batched; the
    integer-valued feature 'x' of every node."""
    rng = np.random.default_rng(seed)
    graphs = []
    for _ in range(count):
        n = int(rng.integers(15, 41))
        label = rng.permutation(n)
        g = dgl.DGLGraph()
        g.add_nodes(n)
        g.add_edges([int(label[k]) for k in range(1, n)],
                    [int(label[rng.integers(0, k)]) for k in range(1, n)])
        g.ndata["x"] = torch.from_numpy(rng.integers(-5, 6, n).astype(np.float32)).reshape(n, 1)
        graphs.append(g)
    return dgl.batch(graphs)


def add_own(nodes):
    return {"h": nodes.data["s"] + nodes.data["x"]}


def test_prop_nodes_topo_on_device_features():
    def run(device, ctx):
        bg = random_trees()
        n = bg.number_of_nodes()
        bg.ndata["x"] = bg.ndata["x"].to(device)
        bg.ndata["s"] = torch.zeros(n, 1, device=device)
        bg.ndata["h"] = torch.zeros(n, 1, device=device)
        dgl.prop_nodes_topo(bg, message_func=fn.copy_src("h", "m"),
                            reduce_func=fn.sum("m", "s"), apply_node_func=add_own, ctx=ctx)
        return bg.ndata["h"]

    host = run("cpu", None)
    dev = run("cuda", "cuda")
    assert dev.is_cuda and torch.equal(dev.cpu(), host)
    assert float(host.abs().sum()) > 0


def test_prop_nodes_bfs_on_device_features(case):
    def run(device, source):
        g = case.g
        g.ndata["h"] = (torch.arange(N, dtype=torch.float32).reshape(N, 1) % 7).to(device)
        dgl.prop_nodes_bfs(g, source, message_func=fn.copy_src("h", "m"),
                           reduce_func=fn.sum("m", "h"))
        return g.pop_n_repr("h")

    host = run("cpu", case.sources["island"])
    dev = run("cuda", case.device_source("island"))
    assert dev.is_cuda and torch.equal(dev.cpu(), host)
    assert not torch.equal(host, torch.arange(N, dtype=torch.float32).reshape(N, 1) % 7)


# ---------------------------------------------------------------- chunk edges
def test_bfs_rows_at_exact_multiples_of_the_chunk():
    """One level whose frontier rows have out-degree 0, 1, K - 1, K, K + 1 and
    2K: a row of exactly deg / K whole items and no partial one, followed by
    rows without items; the frontier starts and ends with a row without items.
    Isolated nodes lie between the rows and at both ends of the id range."""
    K = TRAVERSAL_CHUNK
    degs = [0, 1, K - 1, K, K + 1, 2 * K]
    rows = (1 + 2 * np.arange(len(degs))).tolist()  # odd ids; the even ids between: isolated
    first = 2 * len(degs) + 1                       # the targets are first .. first + 2K - 1
    ends = [first + 2 * K + i for i in range(3)]    # reached, without out-edges
    source = ends[-1] + 1
    n = source + 2                                  # node 0 and node n - 1 are isolated
    level1 = [ends[0]] + rows[:4] + [ends[1]] + rows[4:] + [ends[2]]
    src = np.concatenate([np.full(len(level1), source)] +
                         [np.full(d, r) for r, d in zip(rows, degs)])
    dst = np.concatenate([level1] + [first + np.arange(d) for d in degs])
    assert n == 2 * K + 18 and src.size == 5 * K + 10
    src, dst = src.tolist(), dst.tolist()
    g = dgl.DGLGraph(multigraph=True)
    g.add_nodes(n)
    g.add_edges(src, dst)
    want_nodes, want_edges = check_bfs(slot_rows(n, src, dst), [source])
    assert want_nodes[1] == level1 and len(want_nodes[2]) == 2 * K and len(want_nodes) == 3
    dev_source = torch.tensor([source]).cuda()
    dev_nodes = dgl.bfs_nodes_generator(g, dev_source)
    dev_edges = dgl.bfs_edges_generator(g, dev_source)
    on_device(dev_nodes)
    on_device(dev_edges)
    assert lists(dev_nodes) == want_nodes and lists(dev_edges) == want_edges
    same_frontiers(dev_nodes, dgl.bfs_nodes_generator(g, [source]))
    same_frontiers(dev_edges, dgl.bfs_edges_generator(g, [source]))
