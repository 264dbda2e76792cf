"""The device route of dgl.contrib.sampling.NeighborSampler (seeds given as a
cuda tensor, csrc/neighbor_sample.hip) pinned against the host twin
(csrc/neighbor_sample_host.cc): the same vertices, layers, edges and edge ids,
exactly.

The error cases here are rejected before any dependent access: ns_seed_kernel
compares a seed with [0, N) first, counts it in status[1] when it is outside
and only indexes `layer` in the other branch; the Python side raises on a
non-zero count before any hop is launched."""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import kernel
from dgl.base import DGLError
from dgl.graph_index import _from_edges
from dgl.kernel import SAMPLE_REG_SLOTS

from test_neighbor_sampler import HOPS, KS, N, ROW_DEGREES, SEED_SETS, rule_graph

pytestmark = pytest.mark.gpu

NeighborSampler = dgl.contrib.sampling.NeighborSampler
HUB = len(ROW_DEGREES) - 1


class Case(object):
    """The parent graph of the host tests (about 300 nodes and 7,000 edges; a
    hub row of four register caps plus a partial stride), built once."""

    def __init__(self):
        self.src, self.dst = rule_graph()
        self.g = dgl.DGLGraph(_from_edges(N, self.src, self.dst, True, True), multigraph=True,
                              readonly=True)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self._want = {}

    def csr(self, ctx, in_dir):
        adj = self.g._graph.adjacency(ctx)
        return adj.fwd if in_dir else adj.bwd

    def host(self, name, num_hops, k, seed, in_dir):
        """The host twin's sample (computed once, left as it is)."""
        key = (name, num_hops, k, seed, in_dir)
        if key not in self._want:
            self._want[key] = kernel.neighbor_sample(
                self.csr("cpu", in_dir), torch.from_numpy(SEED_SETS[name]), num_hops, k, seed,
                in_dir=in_dir)
        return self._want[key]

    def device(self, name, num_hops, k, seed, in_dir):
        return kernel.neighbor_sample(
            self.csr(self.dev, in_dir), torch.from_numpy(SEED_SETS[name]).to(self.dev), num_hops,
            k, seed, in_dir=in_dir)


@pytest.fixture(scope="module")
def case():
    return Case()


def same_sample(got, want):
    for a, b, what in zip(got, want, ("vertices", "layers", "sub_src", "sub_dst", "parent_eid")):
        assert a.is_cuda and a.dtype == torch.int64
        assert torch.equal(a.cpu(), b), what


@pytest.mark.parametrize("in_dir", [True, False], ids=["in", "out"])
@pytest.mark.parametrize("num_hops", HOPS)
@pytest.mark.parametrize("k", KS)
def test_device_route_equals_host_twin(case, k, num_hops, in_dir):
    seed = 1000 * k + num_hops
    for name in SEED_SETS:
        same_sample(case.device(name, num_hops, k, seed, in_dir),
                    case.host(name, num_hops, k, seed, in_dir))


def test_hub_row_and_a_frontier_of_many_workgroups(case):
    """The hub alone (a row of several register caps plus a partial stride,
    selected by the recomputing passes), and all nodes as seeds: a frontier of
    300 rows, 75 workgroups of four waves."""
    deg = np.bincount(case.dst, minlength=N)
    assert deg[HUB] == 4 * SAMPLE_REG_SLOTS + 37
    csr, hcsr = case.csr(case.dev, True), case.csr("cpu", True)
    hub = torch.tensor([HUB])
    for k in (1, 5, 64, SAMPLE_REG_SLOTS, deg[HUB] - 1, deg[HUB]):
        got = kernel.neighbor_sample(csr, hub.to(case.dev), 1, k, 77)
        assert got[2].numel() == k
        same_sample(got, kernel.neighbor_sample(hcsr, hub, 1, k, 77))
    got = case.device("all", 2, 5, 8, True)
    assert got[0].numel() == N and int((got[1] == 0).sum()) == N
    same_sample(got, case.host("all", 2, 5, 8, True))


def test_device_route_is_deterministic(case):
    a, b = case.device("rows", 3, 5, 21, True), case.device("rows", 3, 5, 21, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = case.device("rows", 3, 5, 22, True)
    assert not torch.equal(a[4], c[4])


@pytest.mark.parametrize("bad", [-1, N, 2 ** 40])
def test_invalid_seeds_raise(case, bad):
    seeds = torch.tensor([3, 5, bad, 9]).to(case.dev)
    with pytest.raises(DGLError, match="1 of the 4 seeds are not in a graph of %d nodes" % N):
        kernel.neighbor_sample(case.csr(case.dev, True), seeds, 2, 5, 1)
    with pytest.raises(DGLError, match="%d nodes" % N):
        next(iter(NeighborSampler(case.g, 4, 5, seed_nodes=seeds)))
    # the next valid call is still right
    same_sample(case.device("rows", 2, 5, 1, True), case.host("rows", 2, 5, 1, True))


def test_capture_is_refused_before_anything_is_launched(case):
    seeds = torch.from_numpy(SEED_SETS["single"]).to(case.dev)
    csr = case.csr(case.dev, True)  # warm: the parent's adjacency is cached
    x = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x.add_(1.0)
            with pytest.raises(DGLError, match="captured"):
                kernel.neighbor_sample(csr, seeds, 2, 5, 1)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 4  # the capture holds the one add, nothing else
    same_sample(case.device("single", 2, 5, 1, True), case.host("single", 2, 5, 1, True))


def test_sampled_subgraph_stays_on_the_device(case):
    g = case.g
    F = 8
    E = case.src.size
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (N, F), generator=gen).to(torch.float32)  # sums are exact
    g.ndata["h"] = x.cuda()
    g.edata["w"] = torch.arange(E, dtype=torch.float32).reshape(E, 1).cuda()
    try:
        seeds = torch.arange(0, 40).cuda()
        it = NeighborSampler(g, 20, 5, num_hops=2, seed_nodes=seeds, return_seed_id=True, seed=6)
        count = 0
        for sg, aux in it:
            assert sg.parent_nid.is_cuda and sg.parent_eid.is_cuda and aux["seeds"].is_cuda
            assert torch.equal(aux["seeds"], seeds[20 * count:20 * count + 20])
            layers = sg._graph.induced_layers
            assert layers.is_cuda
            assert torch.equal(sg.parent_nid[layers == 0], aux["seeds"])
            sg.copy_from_parent()
            assert sg.ndata["h"].is_cuda and sg.edata["w"].is_cuda
            sg.update_all(fn.copy_src("h", "m"), fn.sum("m", "o"))
            out = sg.ndata["o"]
            assert not sg._graph.has_native_index
            # a dense recomputation from the downloaded edge list
            s, d = (t.cpu() for t in sg._graph._dev_coo)
            nid, eid = sg.parent_nid.cpu(), sg.parent_eid.cpu()
            want = torch.zeros(sg.number_of_nodes(), F).index_add_(0, d, x[nid][s])
            assert torch.equal(out.cpu(), want) and want.abs().sum() > 0
            assert torch.equal(sg.edata["w"].cpu().reshape(-1), eid.to(torch.float32))
            # the edges are the parent's
            assert torch.equal(nid[s], torch.from_numpy(case.src)[eid])
            assert torch.equal(nid[d], torch.from_numpy(case.dst)[eid])
            assert not sg._graph.has_native_index
            count += 1
        assert count == 2
    finally:
        g.pop_n_repr("h")
        g.pop_e_repr("w")


def test_shuffled_device_walk_is_reproducible(case):
    seeds = torch.arange(N - 20).cuda()

    def walk():
        it = NeighborSampler(case.g, 70, 5, num_hops=2, seed_nodes=seeds, shuffle=True,
                             return_seed_id=True, seed=3)
        return [(aux["seeds"], sg.parent_nid, sg.parent_eid, sg._graph._dev_coo[0])
                for sg, aux in it]

    a, b = walk(), walk()
    assert len(a) == 4
    for x, y in zip(a, b):
        assert all(p.is_cuda and torch.equal(p, q) for p, q in zip(x, y))
    order = torch.cat([x[0] for x in a]).cpu()
    assert not torch.equal(order, seeds.cpu()) and torch.equal(order.sort()[0], seeds.cpu())


def test_device_walk_equals_the_seeded_host_walk(case):
    """The same NeighborSampler arguments over host and device seeds: the same
    subgraphs, batch for batch."""
    ids = torch.from_numpy(SEED_SETS["rows"])
    kw = dict(num_hops=2, neighbor_type="out", return_seed_id=True, seed=12, num_workers=2)
    host = list(NeighborSampler(case.g, 5, 5, seed_nodes=ids, **kw))
    dev = list(NeighborSampler(case.g, 5, 5, seed_nodes=ids.cuda(), **kw))
    assert len(host) == len(dev) == 3
    for (hs, ha), (ds, da) in zip(host, dev):
        assert torch.equal(ha["seeds"], da["seeds"].cpu())
        assert torch.equal(hs.parent_nid, ds.parent_nid.cpu())
        assert torch.equal(hs.parent_eid, ds.parent_eid.cpu())
        for x, y in zip(hs._graph._dev_coo, ds._graph._dev_coo):
            assert torch.equal(x, y.cpu())
