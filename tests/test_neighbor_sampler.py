"""dgl.contrib.sampling.NeighborSampler on the host: the reference's sampler
tests restated on edge-list graphs, the stateless sampling rule
(csrc/sample_key.h) pinned by a numpy restatement, the seeded route pinned
against the native sampler at full fan-out, and the rule's uniformity.
No GPU."""
import numpy as np
import pytest
import torch

import dgl
from dgl import _ffi, kernel
from dgl.base import DGLError
from dgl.kernel import SAMPLE_REG_SLOTS

NeighborSampler = dgl.contrib.sampling.NeighborSampler


# ---------------------------------------------------------------------------
# the rule, restated in numpy (uint64 arithmetic wraps)
# ---------------------------------------------------------------------------
def np_mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def np_keys(seed, v, d):
    base = np_mix(np_mix(np.uint64(seed)) ^ np.uint64(v))
    return np_mix(base ^ np.arange(d, dtype=np.uint64))


def np_select(seed, v, d, k):
    """Selected positions of a row of d slots at fan-out k, ascending."""
    if k <= 0:
        return np.zeros(0, dtype=np.int64)
    if d <= k:
        return np.arange(d, dtype=np.int64)
    pos = np.arange(d, dtype=np.int64)
    order = np.lexsort((pos, np_keys(seed, v, d)))  # by key, ties by position
    return np.sort(order[:k])


def np_sample(indptr, indices, eid, seeds, num_hops, k, seed, in_dir):
    N = indptr.size - 1
    layer = np.full(N, -1, dtype=np.int64)
    front = []
    for v in seeds:
        if layer[v] < 0:
            layer[v] = 0
            front.append(int(v))
    for h in range(num_hops):
        nxt = []
        for v in front:
            beg, d = indptr[v], indptr[v + 1] - indptr[v]
            for p in np_select(seed, v, d, k):
                u = indices[beg + p]
                if layer[u] < 0:
                    layer[u] = h + 1
                    nxt.append(int(u))
        front = nxt
    vertices = np.nonzero(layer >= 0)[0].astype(np.int64)
    newid = np.full(N, -1, dtype=np.int64)
    newid[vertices] = np.arange(vertices.size)
    src, dst, pe = [], [], []
    for i, v in enumerate(vertices):
        if layer[v] >= num_hops:
            continue
        beg, d = indptr[v], indptr[v + 1] - indptr[v]
        for p in np_select(seed, v, d, k):
            u = newid[indices[beg + p]]
            src.append(u if in_dir else i)
            dst.append(i if in_dir else u)
            pe.append(eid[beg + p])
    as64 = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    return vertices, layer[vertices], as64(src), as64(dst), as64(pe)


# ---------------------------------------------------------------------------
# the graph of the rule tests: a multigraph with rows of every length the
# selection treats differently
# ---------------------------------------------------------------------------
N = 300
ROW_DEGREES = [0, 1, 4, 5, 6, 63, 64, 65, SAMPLE_REG_SLOTS - 1, SAMPLE_REG_SLOTS,
               SAMPLE_REG_SLOTS + 1, 4 * SAMPLE_REG_SLOTS + 37]
KS = [1, 5, 64]
HOPS = [0, 1, 2, 3]


def rule_graph():
    """(src, dst) of a multigraph in which node i < len(ROW_DEGREES) has
    exactly ROW_DEGREES[i] in-edges and as many out-edges: k - 1, k and k + 1
    for k = 5 and 64, the register cap and its neighbours, a hub of several
    caps plus a partial stride. Rows of four or more slots hold a pair of
    parallel edges and a self loop. The other nodes have about eleven edges
    each way among themselves, so later hops select too; nodes N - 20 .. N - 1
    have no edges at all."""
    rng = np.random.default_rng(11)
    first, live = len(ROW_DEGREES), N - 20
    src, dst = [], []
    for i, d in enumerate(ROW_DEGREES):
        loops = 1 if d >= 4 else 0
        into = rng.integers(first, live, d)
        if d >= 4:
            into[1] = into[0]  # parallel edges
            into[2] = i        # a self loop: an in-edge and an out-edge of i
        out = rng.integers(first, live, d - loops)
        if d >= 4:
            out[1] = out[0]
        src += [into, np.full(d - loops, i)]
        dst += [np.full(d, i), out]
    extra = 3000
    s = rng.integers(first, live, extra)
    t = rng.integers(first, live, extra)
    s[:20], t[:20] = s[20:40], t[20:40]
    src.append(s)
    dst.append(t)
    src, dst = np.concatenate(src), np.concatenate(dst)
    perm = rng.permutation(src.size)
    return src[perm], dst[perm]


SEED_SETS = {
    "single": np.array([11]),
    "repeated": np.array([4, 11, 4, 9, 9, 4]),
    "empty": np.zeros(0, dtype=np.int64),
    "rows": np.arange(len(ROW_DEGREES)),
    "all": np.arange(N),
}


@pytest.fixture(scope="module")
def rule_case():
    src, dst = rule_graph()
    # an edge list graph has max id + 1 nodes: anchor node N - 1 by building
    # the index from explicit sizes
    from dgl.graph_index import _from_edges
    g = dgl.DGLGraph(_from_edges(N, src, dst, True, True), multigraph=True, readonly=True)
    assert g.number_of_nodes() == N and g.is_readonly
    return g


def csr_arrays(g, in_dir):
    adj = g._graph.adjacency(torch.device("cpu"))
    c = adj.fwd if in_dir else adj.bwd
    return c, c.indptr.numpy(), c.indices.numpy().astype(np.int64), c.eid.numpy()


def test_mix_known_vector():
    assert _ffi.LIB.dglhip_sample_mix(0) == 0xE220A8397B1DCDAF
    assert kernel.sample_mix(0) == 0xE220A8397B1DCDAF
    assert int(np_mix(0)) == 0xE220A8397B1DCDAF
    assert kernel.sample_mix(-1) == int(np_mix(np.uint64(2 ** 64 - 1)))
    for seed, v, p in [(0, 0, 0), (7, 12345, 3), (2 ** 64 - 1, 2 ** 31 - 1, 10 ** 5)]:
        want = int(np_keys(seed, v, p + 1)[p])
        assert _ffi.LIB.dglhip_sample_key(seed, v, p) == want


def test_rule_graph_has_the_rows(rule_case):
    for in_dir in (True, False):
        deg = np.diff(csr_arrays(rule_case, in_dir)[1])
        assert deg[:len(ROW_DEGREES)].tolist() == ROW_DEGREES
        assert (deg[N - 20:] == 0).all()
        assert np.median(deg[len(ROW_DEGREES):N - 20]) > 5
    src, dst = rule_graph()
    assert int((src == dst).sum()) >= 8
    assert np.unique(np.stack([src, dst]), axis=1).shape[1] < src.size  # parallel edges


@pytest.mark.parametrize("in_dir", [True, False], ids=["in", "out"])
@pytest.mark.parametrize("num_hops", HOPS)
@pytest.mark.parametrize("k", KS)
def test_host_twin_equals_numpy_oracle(rule_case, k, num_hops, in_dir):
    csr, indptr, indices, eid = csr_arrays(rule_case, in_dir)
    for name, seeds in SEED_SETS.items():
        seed = 1000 * k + num_hops
        got = kernel.neighbor_sample(csr, torch.from_numpy(seeds), num_hops, k, seed,
                                     in_dir=in_dir)
        want = np_sample(indptr, indices, eid, seeds, num_hops, k, seed, in_dir)
        for a, b, what in zip(got, want, ("vertices", "layers", "sub_src", "sub_dst",
                                          "parent_eid")):
            assert a.dtype == torch.int64
            assert np.array_equal(a.numpy(), b), (name, what)
        if name == "empty":
            assert got[0].numel() == 0 and got[2].numel() == 0


def test_row_lengths_around_k_and_the_cap(rule_case):
    """One hop from every listed row alone: min(d, k) edges, the selected
    slots those of the oracle."""
    csr, indptr, indices, eid = csr_arrays(rule_case, True)
    deg = np.diff(indptr)
    for v in range(len(ROW_DEGREES)):
        for k in KS + [SAMPLE_REG_SLOTS]:
            out = kernel.neighbor_sample(csr, torch.tensor([v]), 1, k, 99)
            assert out[2].numel() == min(deg[v], k)
            want = eid[indptr[v] + np_select(99, v, deg[v], k)]
            assert np.array_equal(out[4].numpy(), want)


def test_same_seed_same_arrays_other_seed_other_arrays(rule_case):
    csr = csr_arrays(rule_case, True)[0]
    seeds = torch.from_numpy(SEED_SETS["rows"])
    a = kernel.neighbor_sample(csr, seeds, 2, 5, 3)
    b = kernel.neighbor_sample(csr, seeds, 2, 5, 3)
    c = kernel.neighbor_sample(csr, seeds, 2, 5, 4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[4], c[4])


def test_zero_fanout_and_zero_hops_give_the_distinct_seeds(rule_case):
    csr = csr_arrays(rule_case, True)[0]
    seeds = torch.from_numpy(SEED_SETS["repeated"])
    for hops, k in ((0, 5), (2, 0), (0, 0)):
        v, lay, s, d, e = kernel.neighbor_sample(csr, seeds, hops, k, 1)
        assert v.tolist() == [4, 9, 11] and lay.tolist() == [0, 0, 0]
        assert s.numel() == d.numel() == e.numel() == 0


def test_invalid_seed_raises_on_the_host(rule_case):
    csr = csr_arrays(rule_case, True)[0]
    for bad in (-1, N):
        with pytest.raises(DGLError, match="%d nodes" % N):
            kernel.neighbor_sample(csr, torch.tensor([3, bad]), 1, 5, 1)


# ---------------------------------------------------------------------------
# full fan-out against the native sampler
# ---------------------------------------------------------------------------
def simple_graph(n=120, m=900, seed=5):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, n, m), rng.integers(0, n, m)], 1), axis=0)
    pairs = pairs[rng.permutation(pairs.shape[0])]
    from dgl.graph_index import _from_edges
    return dgl.DGLGraph(_from_edges(n, pairs[:, 0], pairs[:, 1], False, True), readonly=True)


@pytest.mark.parametrize("neighbor_type", ["in", "out"])
@pytest.mark.parametrize("num_hops", [1, 2])
def test_full_fanout_equals_native_sampler(neighbor_type, num_hops):
    g = simple_graph()
    gi = g._graph
    big = int(max(gi.in_degrees().max(), gi.out_degrees().max())) + 1
    seed_sets = [torch.tensor([3]), torch.tensor([7, 50, 7, 99]), torch.arange(0, 120, 9)]
    native = gi.neighbor_sampling(seed_sets, big, num_hops, neighbor_type, None)
    seeded = gi.neighbor_sampling(seed_sets, big, num_hops, neighbor_type, None, seed=1)
    for a, b in zip(native, seeded):
        assert a.has_native_index and not b.has_native_index
        assert torch.equal(a.induced_nodes, b.induced_nodes)
        assert torch.equal(a.induced_layers, b.induced_layers)
        assert torch.equal(a.induced_edges, b.induced_edges)
        assert a.number_of_nodes() == b.number_of_nodes()
        assert a.number_of_edges() == b.number_of_edges()
        # the same structure under the same edge numbering
        for x, y in zip(a.edges("eid"), b.edges("eid")):
            assert torch.equal(x, y)


def test_native_route_pads_to_the_registered_widths():
    g = simple_graph()
    for n in (1, 2, 3, 5, 9):
        seed_sets = [torch.tensor([i, i + 1]) for i in range(n)]
        out = g._graph.neighbor_sampling(seed_sets, 3, 1, "in", None)
        assert len(out) == n
        for ids, sgi in zip(seed_sets, out):
            lay = sgi.induced_layers
            assert sorted(sgi.induced_nodes[lay == 0].tolist()) == ids.tolist()


def test_sampling_argument_checks():
    g = simple_graph()
    gi = g._graph
    s = [torch.tensor([1])]
    with pytest.raises(NotImplementedError):
        gi.neighbor_sampling(s, 3, 1, "in", torch.ones(120))
    with pytest.raises(DGLError):
        gi.neighbor_sampling(s, 3, 1, "both", None)
    with pytest.raises(DGLError):
        gi.neighbor_sampling(s, 0.5, 1, "in", None)
    assert gi.neighbor_sampling([], 3, 1, "in", None) == []
    m = dgl.DGLGraph()
    m.add_nodes(4)
    m.add_edges([0, 1], [1, 2])
    with pytest.raises(NotImplementedError):
        m._graph.neighbor_sampling(s, 3, 1, "in", None)


def test_seeded_subgraph_answers_structural_queries():
    """A seeded sample of a read-only parent builds an immutable native index
    on demand: the queries agree with the edge list the sample returned."""
    g = simple_graph()
    sgi = g._graph.neighbor_sampling([torch.arange(0, 40)], 3, 2, "in", None, seed=9)[0]
    sg = dgl.DGLSubGraph(g, sgi.induced_nodes, sgi.induced_edges, sgi)
    src, dst = sgi._dev_coo
    assert not sgi.has_native_index and sg.is_readonly
    u, v, e = sgi.edges("eid")
    assert torch.equal(u, src) and torch.equal(v, dst)
    assert torch.equal(e, torch.arange(src.numel()))
    fu, fv, _ = sgi.find_edges(torch.tensor([0, src.numel() - 1]))
    assert fu.tolist() == src[[0, -1]].tolist() and fv.tolist() == dst[[0, -1]].tolist()
    assert torch.equal(sg.in_degrees(), torch.bincount(dst, minlength=sg.number_of_nodes()))
    # the parent's edges behind the subgraph's
    ps, pd = g._graph.src(), g._graph.dst()
    nid, eid = sg.parent_nid, sg.parent_eid
    assert torch.equal(nid[src], ps[eid]) and torch.equal(nid[dst], pd[eid])


# ---------------------------------------------------------------------------
# the reference's tests/compute/test_sampler.py on edge-list graphs
# ---------------------------------------------------------------------------
def generate_rand_graph(n, seed=0):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < 0.1
    src, dst = np.nonzero(mask)
    from dgl.graph_index import _from_edges
    return dgl.DGLGraph(_from_edges(n, src, dst, False, True), readonly=True)


@pytest.fixture(scope="module")
def rand_graph():
    return generate_rand_graph(100)


def verify_subgraph(g, subg, seed_id):
    src, _, _ = g.in_edges(seed_id, form="all")
    child_id = subg.map_to_subgraph_nid(seed_id)
    child_src, _, _ = subg.in_edges(child_id, form="all")
    child_src = child_src.numpy()
    # no duplicates in the neighbour list, and it is sorted
    assert len(np.unique(child_src)) == len(child_src)
    assert np.array_equal(np.sort(child_src), child_src)
    # and a subset of the true one
    parent_src = subg.parent_nid[torch.from_numpy(child_src)].numpy()
    assert np.isin(parent_src, src.numpy()).all()


@pytest.mark.parametrize("seed", [None, 5])
def test_1neighbor_sampler_all(rand_graph, seed):
    g = rand_graph
    count = 0
    for subg, aux in NeighborSampler(g, 1, 100, neighbor_type="in", num_workers=4,
                                     return_seed_id=True, seed=seed):
        seed_ids = aux["seeds"]
        assert len(seed_ids) == 1 and int(seed_ids[0]) == count
        src, dst, _ = g.in_edges(seed_ids, form="all")
        self_loop = int((src == dst).sum()) == 1
        assert subg.number_of_nodes() == len(src) + (0 if self_loop else 1)
        assert subg.number_of_edges() == len(src)
        child_ids = subg.map_to_subgraph_nid(seed_ids)
        child_src, _, _ = subg.in_edges(child_ids, form="all")
        child_src1 = subg.map_to_subgraph_nid(src)
        assert torch.equal(torch.sort(child_src1)[0], torch.sort(child_src)[0])
        count += 1
    assert count == 100


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("seed", [None, 5])
def test_1neighbor_sampler(rand_graph, seed, prefetch):
    g = rand_graph
    count = 0
    for subg, aux in NeighborSampler(g, 1, 5, neighbor_type="in", num_workers=4,
                                     return_seed_id=True, prefetch=prefetch, seed=seed):
        seed_ids = aux["seeds"]
        assert len(seed_ids) == 1 and int(seed_ids[0]) == count
        assert subg.number_of_nodes() <= 6
        assert subg.number_of_edges() <= 5
        verify_subgraph(g, subg, seed_ids)
        count += 1
    assert count == 100


@pytest.mark.parametrize("seed", [None, 5])
def test_10neighbor_sampler_all(rand_graph, seed):
    g = rand_graph
    seen = []
    for subg, aux in NeighborSampler(g, 10, 100, neighbor_type="in", num_workers=4,
                                     return_seed_id=True, seed=seed):
        seed_ids = aux["seeds"]
        seen.append(seed_ids)
        src, _, _ = g.in_edges(seed_ids, form="all")
        child_ids = subg.map_to_subgraph_nid(seed_ids)
        child_src, _, _ = subg.in_edges(child_ids, form="all")
        child_src1 = subg.map_to_subgraph_nid(src)
        assert torch.equal(torch.sort(child_src1)[0], torch.sort(child_src)[0])
    # the batches partition the seeds in order
    assert [len(s) for s in seen] == [10] * 10
    assert torch.equal(torch.cat(seen), torch.arange(100))


@pytest.mark.parametrize("seed", [None, 5])
def test_10neighbor_sampler(rand_graph, seed):
    g = rand_graph
    picked = np.unique(np.random.default_rng(1).integers(0, 100, 25))
    for seeds in (None, picked):
        seen = []
        for subg, aux in NeighborSampler(g, 10, 5, neighbor_type="in", num_workers=4,
                                         seed_nodes=seeds, return_seed_id=True, seed=seed):
            seed_ids = aux["seeds"]
            seen.append(seed_ids)
            assert subg.number_of_nodes() <= 6 * len(seed_ids)
            assert subg.number_of_edges() <= 5 * len(seed_ids)
            for seed_id in seed_ids:
                verify_subgraph(g, subg, seed_id.reshape(1))
        want = np.arange(100) if seeds is None else picked
        assert np.array_equal(torch.cat(seen).numpy(), want)
        assert all(len(s) == 10 for s in seen[:-1]) and 1 <= len(seen[-1]) <= 10


def test_without_return_seed_id_aux_is_empty(rand_graph):
    subg, aux = next(iter(NeighborSampler(rand_graph, 10, 5)))
    assert aux == {} and subg.number_of_nodes() >= 10


def test_mutable_graph_raises():
    g = dgl.DGLGraph()
    g.add_nodes(5)
    g.add_edges([0, 1, 2], [1, 2, 3])
    with pytest.raises(NotImplementedError):
        NeighborSampler(g, 1, 5)


def test_shuffle_with_a_seed_is_reproducible(rand_graph):
    def walk(seed):
        it = NeighborSampler(rand_graph, 10, 5, num_hops=2, shuffle=True, return_seed_id=True,
                             seed=seed)
        return [(aux["seeds"], sg.parent_nid, sg.parent_eid) for sg, aux in it]

    a, b, c = walk(3), walk(3), walk(4)
    assert len(a) == 10
    for x, y in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    assert sorted(torch.cat([x[0] for x in a]).tolist()) == list(range(100))
    assert not torch.equal(torch.cat([x[0] for x in a]), torch.arange(100))
    assert not torch.equal(torch.cat([x[0] for x in a]), torch.cat([x[0] for x in c]))


def test_prefetcher_hands_over_errors(rand_graph):
    it = iter(NeighborSampler(rand_graph, 10, 5, neighbor_type="both", prefetch=True))
    with pytest.raises(DGLError):
        next(it)
    with pytest.raises(StopIteration):
        next(it)


# ---------------------------------------------------------------------------
# uniformity of the rule (deterministic: fixed seeds)
# ---------------------------------------------------------------------------
def pick_counts(d, k, keys):
    """Per position, how often it is among the k smallest of a row of keys
    (keys: R x d)."""
    pos = np.broadcast_to(np.arange(d), keys.shape)
    order = np.lexsort((pos, keys), axis=1)[:, :k]
    return np.bincount(order.reshape(-1), minlength=d)


def within_5_sigma(counts, R, d, k):
    p = k / d
    sigma = np.sqrt(R * p * (1 - p))
    return np.abs(counts - R * p).max() <= 5 * sigma


@pytest.mark.parametrize("d,k,R", [(40, 5, 4000), (700, 10, 4000), (65, 64, 2000), (3, 2, 3000)])
def test_uniform_over_seeds(d, k, R):
    for v in (0, 1, 12345):
        keys = np.stack([np_keys(seed, v, d) for seed in range(R)])
        assert within_5_sigma(pick_counts(d, k, keys), R, d, k), (d, k, v)


def test_uniform_over_vertices():
    d, k, R = 40, 5, 4000
    keys = np.stack([np_keys(7, v, d) for v in range(R)])
    assert within_5_sigma(pick_counts(d, k, keys), R, d, k)


def test_uniformity_of_the_host_twin_itself():
    """The same count through the library: one row of 40 slots, 4,000 seeds."""
    d, k, R = 40, 5, 4000
    indptr = torch.tensor([0, d] + [d] * d, dtype=torch.int64)
    csr = kernel.CSR(indptr, torch.arange(1, d + 1, dtype=torch.int32),
                     torch.arange(d, dtype=torch.int64), d + 1)
    counts = np.zeros(d, dtype=np.int64)
    root = torch.tensor([0])
    for seed in range(R):
        counts += np.bincount(kernel.neighbor_sample(csr, root, 1, k, seed)[4].numpy(),
                              minlength=d)
    assert within_5_sigma(counts, R, d, k)
