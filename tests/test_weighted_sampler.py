"""Weighted neighbour sampling (NeighborSampler's node_prob) on the host: the
weighted rule of csrc/sample_key.h pinned bit for bit by a numpy restatement
(the series for -ln u and the key E / w), the host twin pinned against the
numpy oracle, the law of the draw (successive sampling proportional to the
weights, by enumeration) and the Python surface. No GPU."""
import itertools
import math

import numpy as np
import pytest
import torch

import dgl
import test_neighbor_sampler as uniform_tests
from dgl import _ffi, kernel
from dgl.base import DGLError
from test_neighbor_sampler import (HOPS, KS, N, ROW_DEGREES, SEED_SETS, np_keys, np_mix,
                                   np_sample, rule_graph)

NeighborSampler = dgl.contrib.sampling.NeighborSampler
WEIGHTLESS = 0x7FF0000000000000


# ---------------------------------------------------------------------------
# the weighted rule, restated in numpy: every float64 operation below is one
# ufunc call, rounded on its own, in the order of sample_neglog
# ---------------------------------------------------------------------------
SQRT2 = 1.4142135623730951
LN2 = 0.6931471805599453
COEF = [0.6666666666666666, 0.4, 0.2857142857142857, 0.2222222222222222, 0.18181818181818182,
        0.15384615384615385, 0.13333333333333333, 0.11764705882352941, 0.10526315789473684]


def np_neglog(m):
    m = np.atleast_1d(np.asarray(m, dtype=np.uint64))
    mant, ex = np.frexp(m.astype(np.float64))  # exact: m <= 2^53
    f = mant * 2.0                             # m 2^-e in [1, 2), exact
    e = ex.astype(np.int64) - 1
    big = f > SQRT2
    f = np.where(big, f * 0.5, f)
    e = e + big
    s = (f - 1.0) / (f + 1.0)
    t = s * s
    r = np.full(m.shape, COEF[-1])
    for c in COEF[-2::-1]:
        r = c + t * r
    r = 2.0 + t * r
    lnf = s * r
    E = (53 - e).astype(np.float64) * LN2 - lnf
    return np.where(E < 0.0, 0.0, E)


def np_weighted_keys(seed, v, w):
    """Keys of a row whose slots' neighbours have the float32 weights w."""
    w = np.asarray(w, dtype=np.float32)
    h = np_keys(seed, v, w.size)
    E = np_neglog((h >> np.uint64(11)) + np.uint64(1))
    bits = w.view(np.uint32)
    expo = (bits >> np.uint32(23)) & np.uint32(0xFF)
    ok = ((bits >> np.uint32(31)) == 0) & (expo >= 1) & (expo <= 254)
    with np.errstate(all="ignore"):
        q = E / w.astype(np.float64)
    return np.where(ok, q.view(np.uint64), np.uint64(WEIGHTLESS))


def np_weighted_select(seed, v, w, k):
    """Selected positions of a row with the slot weights w at fan-out k."""
    d = w.size
    if k <= 0:
        return np.zeros(0, dtype=np.int64)
    if d <= k:
        return np.arange(d, dtype=np.int64)
    order = np.lexsort((np.arange(d), np_weighted_keys(seed, v, w)))
    return np.sort(order[:k])


def np_weighted_sample(monkeypatch, weights, indptr, indices, eid, seeds, num_hops, k, seed,
                       in_dir):
    """np_sample of the uniform tests with the weighted select in its place."""
    def select(seed_, v, d, k_):
        return np_weighted_select(seed_, v, weights[indices[indptr[v]:indptr[v] + d]], k_)

    monkeypatch.setattr(uniform_tests, "np_select", select)
    try:
        return np_sample(indptr, indices, eid, seeds, num_hops, k, seed, in_dir)
    finally:
        monkeypatch.undo()


def f32(x):
    return float(np.float32(x))


SMALLEST_NORMAL = float(np.finfo(np.float32).tiny)
LARGEST = float(np.finfo(np.float32).max)
DENORMAL = float(np.float32(1e-40))


# ---------------------------------------------------------------------------
# fixed inputs, shared with tests/test_weighted_sampler_gpu.py
# ---------------------------------------------------------------------------
def weight_table():
    """One float32 weight per node of the rule graph: 1e-6 .. 1e6, zero on
    about a third of the nodes, one denormal."""
    rng = np.random.default_rng(5)
    w = (10.0 ** rng.uniform(-6, 6, N)).astype(np.float32)
    w[rng.random(N) < 1 / 3] = 0.0
    w[0], w[1], w[40] = 1e-6, 1e6, DENORMAL
    return w


WEIGHTS = weight_table()

SPECIAL_K = 5
SPECIAL_N = 40
# nodes 10..24 carry weight, 25..39 none (every kind of weightless value)
SPECIAL_WEIGHTS = np.zeros(SPECIAL_N, dtype=np.float32)
SPECIAL_WEIGHTS[10:25] = [1.0, 3.5, 1e-30, SMALLEST_NORMAL, LARGEST, 2.0, 0.25, 7.0, 1e3, 1e-3,
                          5.0, 6.0, 0.5, 9.0, 11.0]
SPECIAL_WEIGHTS[25:40] = [0.0, -0.0, DENORMAL, -1.0, np.inf, np.nan, 0.0, -np.inf, 0.0, -2.5,
                          0.0, 0.0, DENORMAL, 0.0, 0.0]
SPECIAL_ROWS = [
    [25, 10, 26, 11, 27, 12, 28, 13, 29],   # d > k, k - 1 weighted slots
    [14, 30, 15, 31, 16, 32, 17, 33, 18],   # d > k, k weighted slots
    [19, 20, 34, 21, 22, 35, 23, 38, 24],   # d > k, k + 1 weighted slots
    [25, 26, 27, 28, 29, 30, 31, 32, 33],   # all weightless: the first k positions
    [11, 36, 12, 11, 37, 13, 38, 39],       # parallel edges to the weighted node 11
    [10, 25, 11],                           # d < k: kept whole whatever the weights
]


def has_weight(w):
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w >= np.float32(SMALLEST_NORMAL))


def special_csr(device="cpu"):
    """A CSR of the new rows (nodes 0..5; the others have no edges)."""
    deg = [len(r) for r in SPECIAL_ROWS] + [0] * (SPECIAL_N - len(SPECIAL_ROWS))
    indptr = torch.tensor(np.concatenate([[0], np.cumsum(deg)]), dtype=torch.int64)
    indices = torch.tensor(sum(SPECIAL_ROWS, []), dtype=torch.int32)
    eid = torch.arange(indices.numel(), dtype=torch.int64).flip(0).contiguous()
    return kernel.CSR(indptr.to(device), indices.to(device), eid.to(device), SPECIAL_N)


@pytest.fixture(scope="module")
def rule_case():
    src, dst = rule_graph()
    from dgl.graph_index import _from_edges
    return dgl.DGLGraph(_from_edges(N, src, dst, True, True), multigraph=True, readonly=True)


def csr_arrays(g, in_dir):
    adj = g._graph.adjacency(torch.device("cpu"))
    c = adj.fwd if in_dir else adj.bwd
    return c, c.indptr.numpy(), c.indices.numpy().astype(np.int64), c.eid.numpy()


# ---------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------
def lib_neglog(m):
    return np.array([_ffi.LIB.dglhip_sample_neglog(int(x)) for x in np.atleast_1d(m)],
                    dtype=np.float64)


def test_neglog_equals_the_numpy_restatement_bit_for_bit():
    at_sqrt2 = int(np.float64(SQRT2).view(np.uint64) & np.uint64(2 ** 52 - 1)) + 2 ** 52
    assert at_sqrt2 * 2.0 ** -52 == SQRT2
    ms = [1, 2, 3, 2 ** 52, 2 ** 53 - 1, 2 ** 53,
          at_sqrt2 - 1, at_sqrt2, at_sqrt2 + 1,               # f on either side of sqrt 2
          (at_sqrt2 >> 20) - 1, at_sqrt2 >> 20, (at_sqrt2 >> 20) + 1]
    hashed = (np_mix(np.arange(10000, dtype=np.uint64)) >> np.uint64(11)) + np.uint64(1)
    m = np.concatenate([np.array(ms, dtype=np.uint64), hashed])
    got, want = lib_neglog(m), np_neglog(m)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert lib_neglog(2 ** 53)[0] == 0.0 and not np.signbit(lib_neglog(2 ** 53)[0])
    assert (got >= 0).all() and got[0] == lib_neglog(1)[0] > 36.7


def test_neglog_is_the_logarithm_to_the_truncation_bound():
    hashed = (np_mix(np.arange(10000, dtype=np.uint64)) >> np.uint64(11)) + np.uint64(1)
    m = np.concatenate([np.array([1, 2, 3, 2 ** 52, 2 ** 53 - 1, 2 ** 53], dtype=np.uint64),
                        hashed])
    E = lib_neglog(m)
    exact = -np.array([math.log(int(x)) - 53 * math.log(2) for x in m])
    print("largest |neglog + ln u| / max(1, E): %.3g"
          % np.max(np.abs(E - exact) / np.maximum(1.0, E)))
    assert (np.abs(E - exact) <= 1e-12 * np.maximum(1.0, E)).all()
    # and against np.log of u itself, as stated
    u = m.astype(np.float64) * 2.0 ** -53
    assert (np.abs(E + np.log(u)) <= 1e-12 * np.maximum(1.0, E)).all()


def test_weighted_key_equals_the_numpy_key():
    weighted = [1.0, 3.5, 1e-30, SMALLEST_NORMAL, LARGEST]
    weightless = [0.0, -0.0, DENORMAL, -1.0, float("inf"), float("nan")]
    assert 0 < DENORMAL < SMALLEST_NORMAL
    for seed, v, p in [(0, 0, 0), (7, 12345, 3), (2 ** 64 - 1, 2 ** 31 - 1, 10 ** 5)]:
        for w in weighted + weightless:
            want = int(np_weighted_keys(seed, v, np.full(p + 1, w, dtype=np.float32))[p])
            got = _ffi.LIB.dglhip_sample_weighted_key(seed, v, p, w)
            assert got == want, (seed, v, p, w)
            if w in weighted:
                assert got < WEIGHTLESS
                q = np.array([got], dtype=np.uint64).view(np.float64)[0]
                E = lib_neglog((int(np_keys(seed, v, p + 1)[p]) >> 11) + 1)[0]
                assert q == E / float(np.float32(w))
            else:
                assert got == WEIGHTLESS


# ---------------------------------------------------------------------------
# host twin against the numpy oracle
# ---------------------------------------------------------------------------
def test_weight_table_is_as_described():
    w = WEIGHTS
    assert 0.25 < (w == 0).mean() < 0.42
    assert w[40] == np.float32(DENORMAL) and 0 < w[40] < SMALLEST_NORMAL
    pos = w[w >= SMALLEST_NORMAL]
    assert pos.min() == np.float32(1e-6) and pos.max() == np.float32(1e6)


@pytest.mark.parametrize("in_dir", [True, False], ids=["in", "out"])
@pytest.mark.parametrize("num_hops", HOPS)
@pytest.mark.parametrize("k", KS)
def test_weighted_host_twin_equals_numpy_oracle(rule_case, monkeypatch, k, num_hops, in_dir):
    csr, indptr, indices, eid = csr_arrays(rule_case, in_dir)
    weight = torch.from_numpy(WEIGHTS)
    for name, seeds in SEED_SETS.items():
        seed = 1000 * k + num_hops
        got = kernel.neighbor_sample(csr, torch.from_numpy(seeds), num_hops, k, seed,
                                     in_dir=in_dir, node_weight=weight)
        want = np_weighted_sample(monkeypatch, WEIGHTS, indptr, indices, eid, seeds, num_hops, k,
                                  seed, in_dir)
        for a, b, what in zip(got, want, ("vertices", "layers", "sub_src", "sub_dst",
                                          "parent_eid")):
            assert a.dtype == torch.int64
            assert np.array_equal(a.numpy(), b), (name, what)
    # the patch is gone: the uniform oracle is the uniform one again
    assert uniform_tests.np_select(1, 2, 3, 5).tolist() == [0, 1, 2]


def test_weighted_sample_differs_from_the_uniform_one(rule_case):
    csr = csr_arrays(rule_case, True)[0]
    seeds = torch.from_numpy(SEED_SETS["rows"])
    ones = torch.ones(N)
    a = kernel.neighbor_sample(csr, seeds, 1, 5, 3)
    b = kernel.neighbor_sample(csr, seeds, 1, 5, 3, node_weight=ones)
    assert a[4].numel() == b[4].numel() and not torch.equal(a[4], b[4])


def test_rows_around_the_number_of_weighted_slots(monkeypatch):
    csr = special_csr()
    indptr, indices, eid = csr.indptr.numpy(), csr.indices.numpy().astype(np.int64), csr.eid.numpy()
    weight = torch.from_numpy(SPECIAL_WEIGHTS)
    rows = np.arange(len(SPECIAL_ROWS))
    k = SPECIAL_K
    for seed in range(20):
        for hops in (1, 2):
            got = kernel.neighbor_sample(csr, torch.from_numpy(rows), hops, k, seed,
                                         node_weight=weight)
            want = np_weighted_sample(monkeypatch, SPECIAL_WEIGHTS, indptr, indices, eid, rows,
                                      hops, k, seed, True)
            for a, b in zip(got, want):
                assert np.array_equal(a.numpy(), b)
        # what each row must give, whatever the seed
        for v, row in enumerate(SPECIAL_ROWS):
            out = kernel.neighbor_sample(csr, torch.tensor([v]), 1, k, seed, node_weight=weight)
            # slot j carries the edge id nnz - 1 - j
            picked = np.sort((indices.size - 1 - out[4].numpy()) - indptr[v])
            has = has_weight(SPECIAL_WEIGHTS[row])
            assert picked.size == min(len(row), k)
            if len(row) <= k:
                assert picked.tolist() == list(range(len(row)))
            elif has.sum() <= k:
                # every weighted slot, then weightless ones, first positions first
                fill = np.nonzero(~has)[0][:k - has.sum()]
                assert picked.tolist() == sorted(np.nonzero(has)[0].tolist() + fill.tolist())
            else:
                assert has[picked].all()
    assert [int(has_weight(SPECIAL_WEIGHTS[r]).sum()) for r in SPECIAL_ROWS[:4]] == [
        k - 1, k, k + 1, 0]


def test_parallel_edges_are_separate_slots():
    """Both slots to node 11 can be taken, and over seeds each is."""
    csr = special_csr()
    weight = torch.from_numpy(SPECIAL_WEIGHTS)
    beg = int(csr.indptr[4])
    nnz = csr.indices.numel()
    seen = np.zeros(len(SPECIAL_ROWS[4]), dtype=np.int64)
    both = 0
    for seed in range(200):
        e = kernel.neighbor_sample(csr, torch.tensor([4]), 1, 3, seed, node_weight=weight)[4]
        pos = (nnz - 1 - e.numpy()) - beg
        seen[pos] += 1
        both += int(0 in pos and 3 in pos)
    assert seen[0] > 0 and seen[3] > 0 and both > 0
    assert seen[[1, 4, 6, 7]].sum() == 0  # four weighted slots, k = 3: no weightless one


def test_neighbour_ids_outside_the_graph_are_weightless():
    n = 12
    indptr = torch.tensor([0, 4] + [4] * (n - 1), dtype=torch.int64)
    csr = kernel.CSR(indptr, torch.tensor([-1, n, 10, 11], dtype=torch.int32),
                     torch.arange(4, dtype=torch.int64), n)
    for seed in range(10):
        out = kernel.neighbor_sample(csr, torch.tensor([0]), 1, 2, seed,
                                     node_weight=torch.ones(n))
        assert out[4].tolist() == [2, 3] and out[0].tolist() == [0, 10, 11]
        out = kernel.neighbor_sample(csr, torch.tensor([0]), 1, 3, seed,
                                     node_weight=torch.ones(n))
        assert out[4].tolist() == [0, 2, 3] and out[2].tolist() == [-1, 1, 2]


# ---------------------------------------------------------------------------
# the law: successive draws proportional to the weights, without replacement
# ---------------------------------------------------------------------------
def inclusion_probabilities(w, k):
    """P(slot is among k successive draws proportional to w), by enumeration."""
    w = np.asarray(w, dtype=np.float64)
    live = [i for i in range(w.size) if w[i] > 0]
    p = np.zeros(w.size)
    for seq in itertools.permutations(live, k):
        left, prob = w.sum(), 1.0
        for i in seq:
            prob *= w[i] / left
            left -= w[i]
        p[list(seq)] += prob
    return p


LAW_CASES = [([1, 2, 3, 4, 0, 6, 7, 8], 1), ([1, 2, 3, 4, 0, 6, 7, 8], 3), ([.5, .5, 4, 1, 1], 2)]


def check_law(counts, w, k, R, what):
    p = inclusion_probabilities(w, k)
    assert abs(p.sum() - k) < 1e-12
    sigma = np.sqrt(R * p * (1 - p))
    dev = np.abs(counts - R * p)
    print("%s: largest deviation %.2f sigma"
          % (what, np.max(dev[sigma > 0] / sigma[sigma > 0])))
    assert (dev <= 5 * sigma).all(), what
    assert (counts[np.asarray(w) == 0] == 0).all()


@pytest.mark.parametrize("w,k", LAW_CASES)
def test_law_of_the_weighted_keys(w, k):
    R, d = 4000, len(w)
    w32 = np.asarray(w, dtype=np.float32)
    if k == 1:
        assert np.allclose(inclusion_probabilities(w, 1), np.asarray(w) / np.sum(w))
    for v in (0, 1, 12345):
        keys = np.stack([np_weighted_keys(seed, v, w32) for seed in range(R)])
        order = np.lexsort((np.broadcast_to(np.arange(d), keys.shape), keys), axis=1)[:, :k]
        check_law(np.bincount(order.reshape(-1), minlength=d), w, k, R, (w, k, v))


def test_law_of_the_host_twin_itself():
    """The same count through the library: one row of 8 slots, 4,000 seeds."""
    w, k = LAW_CASES[1]
    d, R = len(w), 4000
    indptr = torch.tensor([0, d] + [d] * d, dtype=torch.int64)
    csr = kernel.CSR(indptr, torch.arange(1, d + 1, dtype=torch.int32),
                     torch.arange(d, dtype=torch.int64), d + 1)
    weight = torch.tensor([0.0] + list(w), dtype=torch.float32)
    counts = np.zeros(d, dtype=np.int64)
    root = torch.tensor([0])
    for seed in range(R):
        e = kernel.neighbor_sample(csr, root, 1, k, seed, node_weight=weight)[4]
        counts += np.bincount(e.numpy(), minlength=d)
    check_law(counts, w, k, R, "host twin")


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def simple_graph(n=120, m=900, seed=5):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, n, m), rng.integers(0, n, m)], 1), axis=0)
    pairs = pairs[rng.permutation(pairs.shape[0])]
    from dgl.graph_index import _from_edges
    return dgl.DGLGraph(_from_edges(n, pairs[:, 0], pairs[:, 1], False, True), readonly=True)


def test_graph_index_sampling_with_node_prob():
    g = simple_graph()
    gi = g._graph
    prob = torch.rand(120, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    prob[::3] = 0
    s = [torch.tensor([1, 5, 9]), torch.tensor([7])]
    a = gi.neighbor_sampling(s, 3, 1, "in", prob, seed=1)
    b = gi.neighbor_sampling(s, 3, 1, "in", prob.to(torch.float32), seed=1)
    adj = gi.adjacency(torch.device("cpu"))
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.induced_layers.numel() == x.induced_nodes.numel()
        assert sorted(x.induced_nodes[x.induced_layers == 0].tolist()) == s[i].tolist()
        assert torch.equal(x.induced_nodes, y.induced_nodes)
        assert torch.equal(x.induced_edges, y.induced_edges)
        want = kernel.neighbor_sample(adj.fwd, s[i], 1, 3, kernel.sample_mix(1 + i),
                                      node_weight=prob.to(torch.float32))
        assert torch.equal(x.induced_nodes, want[0]) and torch.equal(x.induced_edges, want[4])
    # a zero-weight neighbour is taken only by rows with fewer than 3 weighted ones
    src, dst = gi.src(), gi.dst()
    for x in a:
        e = x.induced_edges
        for v in dst[e].unique().tolist():
            nbrs = src[dst == v]
            if nbrs.numel() > 3 and int((prob[nbrs] > 0).sum()) >= 3:
                assert (prob[src[e[dst[e] == v]]] > 0).all()


def test_neighbor_sampler_with_node_prob_is_reproducible():
    g = simple_graph()
    prob = torch.rand(120, generator=torch.Generator().manual_seed(2))

    def walk(seed, **kw):
        it = NeighborSampler(g, 10, 5, node_prob=prob, return_seed_id=True, seed=seed, **kw)
        return [(aux["seeds"], sg.parent_nid, sg.parent_eid) for sg, aux in it]

    a, b, c = walk(3), walk(3, num_workers=3, prefetch=True), walk(4)
    assert len(a) == 12
    assert torch.equal(torch.cat([x[0] for x in a]), torch.arange(120))
    for x, y in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    assert any(not torch.equal(x[2], y[2]) for x, y in zip(a, c))
    uniform = [sg.parent_eid for sg, _ in NeighborSampler(g, 10, 5, seed=3)]
    assert any(not torch.equal(x[2], y) for x, y in zip(a, uniform))
    sh = [walk(3, shuffle=True), walk(3, shuffle=True)]
    for x, y in zip(*sh):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_bad_node_prob_raises():
    g = simple_graph()
    gi = g._graph
    s = [torch.tensor([1])]
    good = torch.ones(120)
    bad = [torch.ones(119), torch.ones(121), torch.ones(120, 1).double(),
           torch.ones(2, 60, dtype=torch.float64)]
    for value in (-1.0, float("nan"), float("inf"), -float("inf")):
        t = good.clone()
        t[17] = value
        bad.append(t)
    big = good.double()
    big[3] = 1e300  # finite, but not in float32
    bad.append(big)
    for prob in bad:
        with pytest.raises(DGLError):
            gi.neighbor_sampling(s, 3, 1, "in", prob, seed=1)
        with pytest.raises(DGLError):
            NeighborSampler(g, 10, 5, node_prob=prob, seed=1)
    # a valid one on the native route is still not implemented, and says what to do
    with pytest.raises(NotImplementedError, match="seed="):
        gi.neighbor_sampling(s, 3, 1, "in", good)
    with pytest.raises(NotImplementedError):
        next(iter(NeighborSampler(g, 10, 5, node_prob=good)))
    assert len(gi.neighbor_sampling(s, 3, 1, "in", good.numpy(), seed=1)) == 1


def test_bad_node_weight_raises():
    g = simple_graph()
    csr = g._graph.adjacency(torch.device("cpu")).fwd
    s = torch.tensor([1])
    for w in (torch.ones(120, dtype=torch.float64), torch.ones(120, dtype=torch.int64),
              torch.ones(119), torch.ones(120, 1), torch.ones(240)[::2], np.ones(120, np.float32),
              torch.ones(120, device="meta")):
        with pytest.raises(DGLError):
            kernel.neighbor_sample(csr, s, 1, 3, 1, node_weight=w)
    assert kernel.neighbor_sample(csr, s, 1, 3, 1, node_weight=torch.ones(120))[0].numel() > 1
