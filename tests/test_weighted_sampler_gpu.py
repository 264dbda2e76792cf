"""The device route of weighted neighbour sampling (node_prob; the weighted
kernels of csrc/neighbor_sample.hip) pinned against the weighted host twin
(csrc/neighbor_sample_host.cc): the same vertices, layers, edges and edge ids,
exactly.

No case here can fault: a seed outside the graph is compared with [0, N)
before it indexes anything (ns_seed_kernel) and raises before any hop is
launched; a slot's neighbour id is compared with [0, N) before its weight is
gathered (WeightedKey); weights of the wrong device, dtype or shape and a
capturing stream are refused in Python, before anything is launched."""
import numpy as np
import pytest
import torch

import dgl
import dgl.function as fn
from dgl import kernel
from dgl.base import DGLError
from dgl.graph_index import _from_edges
from dgl.kernel import SAMPLE_LDS_SLOTS, SAMPLE_REG_SLOTS

from test_neighbor_sampler import HOPS, KS, N, ROW_DEGREES, SEED_SETS, rule_graph
from test_weighted_sampler import (SPECIAL_K, SPECIAL_N, SPECIAL_ROWS, SPECIAL_WEIGHTS, WEIGHTS,
                                   special_csr)

pytestmark = pytest.mark.gpu

NeighborSampler = dgl.contrib.sampling.NeighborSampler
HUB = len(ROW_DEGREES) - 1


class Case(object):
    """The parent graph and weight table of the host tests, built once."""

    def __init__(self):
        self.src, self.dst = rule_graph()
        self.g = dgl.DGLGraph(_from_edges(N, self.src, self.dst, True, True), multigraph=True,
                              readonly=True)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.w = torch.from_numpy(WEIGHTS)
        self.w_dev = self.w.to(self.dev)
        self._want = {}

    def csr(self, ctx, in_dir):
        adj = self.g._graph.adjacency(ctx)
        return adj.fwd if in_dir else adj.bwd

    def host(self, name, num_hops, k, seed, in_dir):
        """The weighted host twin's sample (computed once, left as it is)."""
        key = (name, num_hops, k, seed, in_dir)
        if key not in self._want:
            self._want[key] = kernel.neighbor_sample(
                self.csr("cpu", in_dir), torch.from_numpy(SEED_SETS[name]), num_hops, k, seed,
                in_dir=in_dir, node_weight=self.w)
        return self._want[key]

    def device(self, name, num_hops, k, seed, in_dir):
        return kernel.neighbor_sample(
            self.csr(self.dev, in_dir), torch.from_numpy(SEED_SETS[name]).to(self.dev), num_hops,
            k, seed, in_dir=in_dir, node_weight=self.w_dev)


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
def test_weighted_device_route_equals_host_twin(case, k, num_hops, in_dir):
    seed = 1000 * k + num_hops
    for name in SEED_SETS:
        same_sample(case.device(name, num_hops, k, seed, in_dir),
                    case.host(name, num_hops, k, seed, in_dir))


def test_hub_row_register_cap_and_a_frontier_of_many_workgroups(case):
    """The hub alone (longer than the LDS cap: selected by the recomputing
    passes), the rows at the register cap - 1, cap and cap + 1 alone (keys in
    registers up to the cap, staged in LDS beyond), and all nodes as seeds: a
    frontier of 300 rows, 75 workgroups of four waves."""
    deg = np.bincount(case.dst, minlength=N)
    assert deg[HUB] == 4 * SAMPLE_REG_SLOTS + 37 > SAMPLE_LDS_SLOTS
    csr, hcsr = case.csr(case.dev, True), case.csr("cpu", True)
    hub = torch.tensor([HUB])
    for k in (1, 5, 64, SAMPLE_REG_SLOTS, deg[HUB] - 1, deg[HUB]):
        got = kernel.neighbor_sample(csr, hub.to(case.dev), 1, k, 77, node_weight=case.w_dev)
        assert got[2].numel() == k
        same_sample(got, kernel.neighbor_sample(hcsr, hub, 1, k, 77, node_weight=case.w))
    for d in (SAMPLE_REG_SLOTS - 1, SAMPLE_REG_SLOTS, SAMPLE_REG_SLOTS + 1):
        row = torch.tensor([ROW_DEGREES.index(d)])
        assert deg[ROW_DEGREES.index(d)] == d
        for k in (1, 64, d - 1):
            got = kernel.neighbor_sample(csr, row.to(case.dev), 1, k, 5, node_weight=case.w_dev)
            assert got[2].numel() == k
            same_sample(got, kernel.neighbor_sample(hcsr, row, 1, k, 5, node_weight=case.w))
    got = case.device("all", 2, 5, 8, True)
    assert got[0].numel() == N and int((got[1] == 0).sum()) == N
    same_sample(got, case.host("all", 2, 5, 8, True))


def test_rows_around_the_lds_cap(case):
    """Rows of cap - 1, cap and cap + 1 slots, the cap being the longest row
    whose keys a wave stages in LDS; the longer one recomputes its keys."""
    n = SAMPLE_LDS_SLOTS + 200
    degrees = [SAMPLE_LDS_SLOTS - 1, SAMPLE_LDS_SLOTS, SAMPLE_LDS_SLOTS + 1]
    rng = np.random.default_rng(9)
    indptr = torch.tensor(np.concatenate([[0], np.cumsum(degrees + [0] * (n - 3))]))
    idx = torch.from_numpy(rng.integers(3, n, sum(degrees)).astype(np.int32))
    idx[5], idx[SAMPLE_LDS_SLOTS + 5] = -7, n  # outside the graph: weightless
    eid = torch.from_numpy(rng.permutation(sum(degrees)))
    w = torch.from_numpy((10.0 ** rng.uniform(-3, 3, n)).astype(np.float32))
    w[torch.from_numpy(rng.random(n) < 0.3)] = 0.0
    hcsr = kernel.CSR(indptr, idx, eid, n)
    csr = kernel.CSR(indptr.to(case.dev), idx.to(case.dev), eid.to(case.dev), n)
    w_dev = w.to(case.dev)
    for v, d in enumerate(degrees):
        row = torch.tensor([v])
        # (about 700 slots of each row carry weight: 900 and d - 1 take weightless ones)
        for k in (1, 64, 900, d - 1):
            got = kernel.neighbor_sample(csr, row.to(case.dev), 1, k, 31, node_weight=w_dev)
            assert got[2].numel() == k
            same_sample(got, kernel.neighbor_sample(hcsr, row, 1, k, 31, node_weight=w))
    rows = torch.arange(3)
    same_sample(kernel.neighbor_sample(csr, rows.to(case.dev), 2, 10, 2, node_weight=w_dev),
                kernel.neighbor_sample(hcsr, rows, 2, 10, 2, node_weight=w))


def test_rows_around_the_number_of_weighted_slots(case):
    """Fewer than k, k and more than k weighted slots, an all-weightless row
    (the first k positions) and parallel edges."""
    csr, hcsr = special_csr(case.dev), special_csr()
    w = torch.from_numpy(SPECIAL_WEIGHTS)
    w_dev = w.to(case.dev)
    rows = torch.arange(len(SPECIAL_ROWS))
    for seed in range(6):
        for k in (SPECIAL_K, 3, 1):
            got = kernel.neighbor_sample(csr, rows.to(case.dev), 2, k, seed, node_weight=w_dev)
            same_sample(got, kernel.neighbor_sample(hcsr, rows, 2, k, seed, node_weight=w))
    only = kernel.neighbor_sample(csr, torch.tensor([3]).to(case.dev), 1, SPECIAL_K, 0,
                                  node_weight=w_dev)
    nnz, beg = hcsr.indices.numel(), int(hcsr.indptr[3])
    assert ((nnz - 1 - only[4].cpu()) - beg).tolist() == list(range(SPECIAL_K))
    assert SPECIAL_N == w.numel()


def test_neighbour_ids_outside_the_graph_are_weightless(case):
    """The id is compared with [0, N) before it indexes the weights."""
    n = 12
    indptr = torch.tensor([0, 4] + [4] * (n - 1), dtype=torch.int64)
    idx = torch.tensor([-1, n, 10, 11], dtype=torch.int32)
    eid = torch.arange(4, dtype=torch.int64)
    csr = kernel.CSR(indptr.to(case.dev), idx.to(case.dev), eid.to(case.dev), n)
    hcsr = kernel.CSR(indptr, idx, eid, n)
    root = torch.tensor([0])
    for k in (2, 3):
        got = kernel.neighbor_sample(csr, root.to(case.dev), 1, k, 4,
                                     node_weight=torch.ones(n, device=case.dev))
        same_sample(got, kernel.neighbor_sample(hcsr, root, 1, k, 4, node_weight=torch.ones(n)))
        assert got[4].tolist() == [[2, 3], [0, 2, 3]][k - 2]


def test_weighted_device_route_is_deterministic_and_leaves_the_uniform_one_alone(case):
    a, b = case.device("rows", 3, 5, 21, True), case.device("rows", 3, 5, 21, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = case.device("rows", 3, 5, 22, True)
    assert not torch.equal(a[4], c[4])
    # the uniform route after weighted calls: still its own host twin's sample
    seeds = torch.from_numpy(SEED_SETS["rows"])
    uni = kernel.neighbor_sample(case.csr(case.dev, True), seeds.to(case.dev), 3, 5, 21)
    same_sample(uni, kernel.neighbor_sample(case.csr("cpu", True), seeds, 3, 5, 21))
    assert not torch.equal(uni[4], a[4])


@pytest.mark.parametrize("bad", [-1, N, 2 ** 40])
def test_invalid_seeds_raise(case, bad):
    seeds = torch.tensor([3, 5, bad, 9]).to(case.dev)
    with pytest.raises(DGLError, match="1 of the 4 seeds are not in a graph of %d nodes" % N):
        kernel.neighbor_sample(case.csr(case.dev, True), seeds, 2, 5, 1, node_weight=case.w_dev)
    with pytest.raises(DGLError, match="%d nodes" % N):
        next(iter(NeighborSampler(case.g, 4, 5, seed_nodes=seeds, node_prob=case.w)))
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
                kernel.neighbor_sample(csr, seeds, 2, 5, 1, node_weight=case.w_dev)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 4  # the capture holds the one add, nothing else
    same_sample(case.device("single", 2, 5, 1, True), case.host("single", 2, 5, 1, True))


def test_weights_on_the_wrong_device_raise_in_python(case):
    seeds = torch.from_numpy(SEED_SETS["single"])
    with pytest.raises(DGLError, match="node_weight is on"):
        kernel.neighbor_sample(case.csr(case.dev, True), seeds.to(case.dev), 1, 5, 1,
                               node_weight=case.w)
    with pytest.raises(DGLError, match="node_weight is on"):
        kernel.neighbor_sample(case.csr("cpu", True), seeds, 1, 5, 1, node_weight=case.w_dev)
    with pytest.raises(DGLError, match="float32"):
        kernel.neighbor_sample(case.csr(case.dev, True), seeds.to(case.dev), 1, 5, 1,
                               node_weight=case.w_dev.double())


def test_weighted_device_walk_equals_the_seeded_host_walk(case):
    """node_prob on the host and on the device, over device seeds: the same
    subgraphs, batch for batch, as the seeded host walk."""
    ids = torch.from_numpy(SEED_SETS["rows"])
    kw = dict(num_hops=2, neighbor_type="out", return_seed_id=True, seed=12, num_workers=2)
    host = list(NeighborSampler(case.g, 5, 5, seed_nodes=ids, node_prob=case.w, **kw))
    assert len(host) == 3
    for prob in (case.w, case.w_dev, case.w_dev.double()):
        dev = list(NeighborSampler(case.g, 5, 5, seed_nodes=ids.cuda(), node_prob=prob, **kw))
        assert len(dev) == 3
        for (hs, ha), (ds, da) in zip(host, dev):
            assert da["seeds"].is_cuda and ds.parent_nid.is_cuda and ds.parent_eid.is_cuda
            assert ds._graph.induced_layers.is_cuda
            assert torch.equal(ha["seeds"], da["seeds"].cpu())
            assert torch.equal(hs.parent_nid, ds.parent_nid.cpu())
            assert torch.equal(hs.parent_eid, ds.parent_eid.cpu())
            assert torch.equal(hs._graph.induced_layers, ds._graph.induced_layers.cpu())
            for x, y in zip(hs._graph._dev_coo, ds._graph._dev_coo):
                assert y.is_cuda and torch.equal(x, y.cpu())
    uniform = list(NeighborSampler(case.g, 5, 5, seed_nodes=ids.cuda(), **kw))
    assert any(not torch.equal(u[0].parent_eid, d[0].parent_eid) for u, d in zip(uniform, dev))


def test_weighted_sampled_subgraph_stays_on_the_device(case):
    g = case.g
    F = 8
    E = case.src.size
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (N, F), generator=gen).to(torch.float32)  # sums are exact
    g.ndata["h"] = x.cuda()
    g.edata["w"] = torch.arange(E, dtype=torch.float32).reshape(E, 1).cuda()
    try:
        seeds = torch.arange(0, 40).cuda()
        it = NeighborSampler(g, 20, 5, num_hops=2, seed_nodes=seeds, node_prob=case.w,
                             return_seed_id=True, seed=6)
        count = 0
        for sg, aux in it:
            assert sg.parent_nid.is_cuda and sg.parent_eid.is_cuda and aux["seeds"].is_cuda
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
            count += 1
        assert count == 2
    finally:
        g.pop_n_repr("h")
        g.pop_e_repr("w")
