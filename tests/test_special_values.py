"""NaN, infinity, signed-zero and subnormal semantics of the g-SpMM reducers
(sum, mean, max, out + mean, the accumulating sum), on the host kernels and on
every device schedule: one wave per row, the short-row tiers, the heavy-row
split, the source-blocked launches (sum and max), the padded-stride gather,
the source sweep, bf16 source rows and the transposed backward.

Comparisons are by bits (int32 views, NaN masks equal; NaN payload and sign
are not compared), never by ``==``, which takes -0.0 for +0.0 and fails on
any NaN. The references are plain CPU code:

* sum: the oracle's C fma chain in edge-id order (``O.spmm_coo``), itself
  pinned here to ``torch.sparse.mm`` on the reference's uncoalesced COO;
* mean: that chain divided by float32(deg) where deg > 1;
* max: torch's rule restated in numpy (the first maximum or the first NaN in
  edge order, +0.0 for rows without messages), itself pinned here to per-row
  ``torch.max(mailbox, 0)``, values and indices; the backward is torch's CPU
  autograd of that per-row max;
* out + mean: ``base + mean`` in numpy float32;
* the accumulating sum: the chain continued from ``base`` in numpy float32
  (rows without in-edges keep ``base``, -0.0 included: the chain's definition).

One finding is pinned as it stands rather than changed: torch's dense autograd
of ``max(h[src] * w)`` multiplies the zero gradient of every message that lost
by its partner, so a losing message whose source value is NaN or infinite gets
0 * x = NaN as its edge-value gradient. The engine routes the gradient to the
winning slot only; the edge-value gradient is therefore compared with torch's
at the winning slots and with zero elsewhere.

One small graph serves every case: 300 rows over 300 sources, 3,964 edges, numbered source-major ("sorted") and at random ("random"), with rows
built so that a NaN message arrives at every place the max kernel treats
differently (test_graph_covers_the_cases asserts them from the graph alone).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dgl import kernel
from dgl._ffi import LIB, check_call, ptr
from oracle import oracle as O

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
N = 300
F_ALL = (1, 5, 41, 128, 130)  # VEC 1 and 2, several GROUP shapes, a last pass with idle lanes
NAN_SRC = (3, 150, 220)
PINF_SRC = (10, 160)
NINF_SRC = (20, 170)
NEGZERO_SRC = (30, 31, 180)
SUBNORMAL_SRC = (40, 41, 190, 191)
SPECIAL_SRC = NAN_SRC + PINF_SRC + NINF_SRC + NEGZERO_SRC + SUBNORMAL_SRC
UNROLL = 8  # slots per batch of the max kernel


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


def _same_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32 and ref.dtype == np.float32
    assert got.shape == ref.shape
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), "NaN masks differ at %s" % (np.argwhere(gn != rn)[:5],)
    gb = np.ascontiguousarray(got).view(np.int32)
    rb = np.ascontiguousarray(ref).view(np.int32)
    bad = (gb != rb) & ~gn
    assert not bad.any(), "bits differ at %s: got %s, want %s" % (
        np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5])


# ---------------------------------------------------------------------------
# The graph
# ---------------------------------------------------------------------------
class _Graph(object):
    """Edges (src[e], dst[e]) in edge-id order plus the destination-major
    grouping the engine builds from them (ORDER_EID: a row's slots in edge-id
    order): slot k holds edge order[k], row r's slots are
    [indptr[r], indptr[r+1])."""

    def __init__(self, src, dst):
        self.src, self.dst = src, dst
        self.order = np.argsort(dst, kind="stable")
        self.deg = np.bincount(dst, minlength=N)
        self.indptr = np.concatenate([[0], np.cumsum(self.deg)]).astype(np.int64)
        for a in (self.src, self.dst, self.order, self.deg, self.indptr):
            a.setflags(write=False)

    def edges_of(self, r):
        return self.order[self.indptr[r]:self.indptr[r + 1]]


def _placed(rng, plain, deg, at):
    """A row of ``deg`` distinct sources, ascending, with the special sources
    ``at`` = {slot: source} at those slots and plain sources elsewhere."""
    slots = sorted(at)
    out, lo, prev = [], -1, 0
    for s in slots + [deg]:
        hi = at[s] if s < deg else N
        pool = plain[(plain > lo) & (plain < hi)]
        out.extend(sorted(rng.choice(pool, size=s - prev, replace=False).tolist()))
        if s < deg:
            out.append(at[s])
            lo, prev = at[s], s + 1
    assert len(out) == deg and out == sorted(out)
    return out


@functools.lru_cache(maxsize=None)
def _graphs():
    """{"sorted": source-major numbering, "random": random numbering} of one
    edge multiset. The hand-built rows list their sources in ascending order
    in both numberings, so a special message sits at the same slot in both;
    the other rows' slots are shuffled in the random numbering."""
    rng = np.random.default_rng(2024)
    plain = np.setdiff1d(np.arange(N), SPECIAL_SRC)
    a, b, c = NAN_SRC
    fixed = [
        _placed(rng, plain, 12, {0: a}),            # first NaN at slot 0
        _placed(rng, plain, 12, {3: b}),            # at a slot in 1..7
        _placed(rng, plain, 30, {17: b}),           # at a slot >= 8 inside a full batch
        _placed(rng, plain, 21, {20: c}),           # in the predicated tail
        _placed(rng, plain, 20, {5: b, 13: c}),     # two NaNs
        [b],                                        # one slot, a NaN
        _placed(rng, plain, 3, {1: b}),             # a short row with a NaN
        [NEGZERO_SRC[0]],                           # only -0.0 sources: 1, 3, 12 slots
        list(NEGZERO_SRC),
        sorted(NEGZERO_SRC * 4),
        sorted(PINF_SRC * 3),                       # only +inf
        sorted(NINF_SRC * 3),                       # only -inf
        sorted(list(PINF_SRC + NINF_SRC) + rng.choice(plain, 6, replace=False).tolist()),
        sorted(SUBNORMAL_SRC + SUBNORMAL_SRC[:1]),  # only subnormal sources
        sorted(list(SUBNORMAL_SRC[:2]) + rng.choice(plain, 1).tolist()),
    ]
    rows = [(rng.permutation(N).tolist(), False)]   # the hub: every source once
    rows += [(r, True) for r in fixed]
    rows += [([], False)] * 30
    rows += [(rng.integers(0, N, 1).tolist(), False) for _ in range(30)]
    rows += [(rng.integers(0, N, rng.integers(2, 5)).tolist(), False) for _ in range(60)]
    rows += [(rng.integers(0, N, rng.integers(5, 9)).tolist(), False) for _ in range(60)]
    rows += [(rng.integers(0, N, rng.integers(9, 41)).tolist(), False)
             for _ in range(N - len(rows))]
    ids = rng.permutation(N)
    src = np.concatenate([np.asarray(r, np.int64) for r, _ in rows])
    dst = np.concatenate([np.full(len(r), ids[i], np.int64) for i, (r, _) in enumerate(rows)])
    o = np.lexsort((dst, src))
    out = {"sorted": _Graph(src[o], dst[o])}
    # random numbering: a random interleaving of the rows that keeps each
    # row's own order as listed above
    key = rng.permutation(len(src))
    p = 0
    for r, _ in rows:
        key[p:p + len(r)] = np.sort(key[p:p + len(r)])
        p += len(r)
    o = np.argsort(key)
    out["random"] = _Graph(src[o], dst[o])
    return out


def _nan_slots(g, r):
    """Row-relative slots of row r whose copy_u message is NaN (in the NaN columns)."""
    return np.nonzero(np.isin(g.src[g.edges_of(r)], NAN_SRC))[0]


def test_graph_covers_the_cases():
    for name, g in _graphs().items():
        deg = g.deg
        assert len(g.src) > 3000 and deg.max() == N
        for lo, hi in ((0, 0), (1, 1), (2, 4), (5, 8), (9, 40)):
            assert ((deg >= lo) & (deg <= hi)).sum() >= 20, (name, lo, hi)
        seen = set()
        for r in range(N):
            d, s = int(deg[r]), _nan_slots(g, r)
            if len(s) == 0 or d == N:
                continue
            k = int(s[0])
            if k == 0 and d > UNROLL:
                seen.add("slot 0")
            if 1 <= k < UNROLL and d > UNROLL:
                seen.add("first batch")
            # a full batch whether batches are counted from slot 0 or, as the
            # kernel does after seeding with slot 0, from slot 1
            if k >= UNROLL and (k // UNROLL + 1) * UNROLL <= d and \
                    1 + ((k - 1) // UNROLL + 1) * UNROLL <= d:
                seen.add("later batch")
            tail = min(d % UNROLL, (d - 1) % UNROLL)  # the tail under both countings
            if d > UNROLL and tail >= 1 and k >= d - tail:
                seen.add("tail")
            if len(s) >= 2:
                seen.add("two")
        assert seen == {"slot 0", "first batch", "later batch", "tail", "two"}, (name, seen)
        # a non-empty row with only -0.0 sources, rows that see only +inf, only -inf, both
        kinds = set()
        for r in range(N):
            s = set(g.src[g.edges_of(r)].tolist())
            if s and s <= set(NEGZERO_SRC):
                kinds.add("-0")
            p, m = bool(s & set(PINF_SRC)), bool(s & set(NINF_SRC))
            kinds.add(("+inf" if p else "") + ("-inf" if m else ""))
        assert {"-0", "+inf", "-inf", "+inf-inf"} <= kinds, (name, kinds)
    a, b = _graphs()["sorted"], _graphs()["random"]
    assert np.array_equal(a.deg, b.deg)
    assert np.all(np.diff(a.src) >= 0) and not np.all(np.diff(b.src) >= 0)


# ---------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(F, seed=0):
    """(N, F) float32 over several decades with the special rows planted.
    Columns by f % 4: 0 NaN and both infinities, 1 NaN only, 2 infinities
    only, 3 ordinary; the -0.0 and the subnormal rows fill every column."""
    rng = np.random.default_rng(1000 * seed + F)
    H = (rng.standard_normal((N, F)) * np.exp(3 * rng.standard_normal((N, 1)))).astype(np.float32)
    role = np.arange(F) % 4
    nan_cols, inf_cols = np.nonzero(role <= 1)[0], np.nonzero((role == 0) | (role == 2))[0]
    H[np.ix_(NAN_SRC, nan_cols)] = np.nan
    H[np.ix_(PINF_SRC, inf_cols)] = np.inf
    H[np.ix_(NINF_SRC, inf_cols)] = -np.inf
    H[list(NEGZERO_SRC)] = -0.0
    H[list(SUBNORMAL_SRC)] = (rng.standard_normal((len(SUBNORMAL_SRC), F)) * 1e-40).astype(np.float32)
    assert np.signbit(H[NEGZERO_SRC[0]]).all() and (np.abs(H[SUBNORMAL_SRC[0]]) < 1.2e-38).all()
    H.setflags(write=False)
    return H


@functools.lru_cache(maxsize=None)
def _weights(elen, E):
    """(E, elen) edge values by edge id: several decades, with zeros of both
    signs, an infinity, NaNs and subnormals among them."""
    rng = np.random.default_rng(77 + elen)
    w = (rng.standard_normal((E, elen)) * np.exp(rng.standard_normal((E, 1)))).astype(np.float32)
    for f in range(elen):
        w[(3 * f) % 17::17, f] = 0.0
        w[(5 + f) % 41::41, f] = -0.0
        w[(7 + f) % 97::97, f] = np.inf
        w[(11 + f) % 101::101, f] = np.nan
        w[(13 + f) % 53::53, f] = 1e-40
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _base(F):
    """(N, F) float32 whose element (r, f) is -0.0, +0.0, NaN, inf or an
    ordinary number, every kind present on rows without in-edges, on one-slot
    rows and on long rows."""
    g = _graphs()["random"]
    rng = np.random.default_rng(5 + F)
    kind = np.arange(N) % 6
    classes = [np.nonzero(g.deg == 0)[0], np.nonzero(g.deg == 1)[0], np.nonzero(g.deg > 8)[0]]
    for rows in classes:
        kind[rows] = np.arange(len(rows)) % 6
    k = (kind[:, None] + np.arange(F)[None, :]) % 6
    B = (rng.standard_normal((N, F)) * np.exp(2 * rng.standard_normal((N, 1)))).astype(np.float32)
    B[k == 0], B[k == 1], B[k == 2], B[k == 3] = -0.0, 0.0, np.nan, np.inf
    for rows in classes:
        assert all((k[rows] == v).any() for v in range(6))
    B.setflags(write=False)
    return B


# ---------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------
def _messages(g, msg, H, w):
    """(E, F) messages by edge id, each one rounding (float32 products)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if msg == "copy_u":
            return H[g.src]
        if msg == "copy_e":
            return np.ascontiguousarray(w)
        return (H[g.src] * w).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sum_ref(name, msg, F, elen=0):
    """The oracle's fma chain in edge-id order (column by column for
    per-feature edge values: the oracle takes one value per edge)."""
    g = _graphs()[name]
    H = _table(F)
    if msg == "copy_u":
        out = O.spmm_coo(N, g.dst, g.src, H)
    else:
        w = _weights(elen, len(g.src))
        if msg == "copy_e":  # fma(e, 1, acc) = acc + e
            H, col = np.ones((1, F), np.float32), np.zeros(len(g.src), np.int64)
        else:
            col = g.src
        if elen == 1:
            out = O.spmm_coo(N, g.dst, col, H, w[:, 0])
        else:
            out = np.concatenate([O.spmm_coo(N, g.dst, col, H[:, f:f + 1], w[:, f])
                                  for f in range(F)], axis=1)
    out.setflags(write=False)
    return out


def _mean_of(total, deg):
    d = np.maximum(deg, 1).astype(np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        out = np.where(deg[:, None] > 1, total / d, total).astype(np.float32)
    return out


def _max_rule(g, M):
    """torch's max over each row's mailbox M[edges in edge order], restated:
    (values, winning edge id or -1)."""
    F = M.shape[1]
    out, arg = np.zeros((N, F), np.float32), np.full((N, F), -1, np.int64)
    for r in range(N):
        es = g.edges_of(r)
        if len(es) == 0:
            continue
        val, a = M[es[0]].copy(), np.full(F, es[0], np.int64)
        for e in es[1:]:
            x = M[e]
            upd = ~np.isnan(val) & ((x > val) | np.isnan(x))
            val[upd] = x[upd]
            a[upd] = e
        out[r], arg[r] = val, a
    return out, arg


@functools.lru_cache(maxsize=None)
def _max_ref(name, msg, F, elen=0):
    g = _graphs()[name]
    w = _weights(elen, len(g.src)) if elen else None
    if w is not None and 1 < elen:
        assert elen == F
    out, arg = _max_rule(g, _messages(g, msg, _table(F), w))
    out.setflags(write=False)
    return out, arg


def _chain_from(base, g, H):
    """The copy_u chain continued from ``base``, in numpy float32."""
    out = base.copy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for e in range(len(g.src)):
            out[g.dst[e]] = out[g.dst[e]] + H[g.src[e]]
    return out


def _exact(g, H):
    """float64 sums and sums of magnitudes per row (for the chunked rows)."""
    with np.errstate(invalid="ignore", over="ignore"):
        tot, mag = np.zeros((N, H.shape[1])), np.zeros((N, H.shape[1]))
        np.add.at(tot, g.dst, H[g.src].astype(np.float64))
        np.add.at(mag, g.dst, np.abs(H[g.src].astype(np.float64)))
    return tot, mag


# ---------------------------------------------------------------------------
# The references themselves, pinned to torch on the CPU
# ---------------------------------------------------------------------------
def test_oracle_sum_chain_is_torch_sparse_mm():
    g = _graphs()["random"]
    idx = torch.from_numpy(np.stack([g.dst, g.src]))
    for F in (5, 41):
        H = _table(F)
        w = _weights(1, len(g.src))[:, 0]
        for val, ref in ((None, _sum_ref("random", "copy_u", F)),
                         (w, _sum_ref("random", "u_mul_e", F, 1))):
            v = torch.ones(len(g.src)) if val is None else torch.from_numpy(val.copy())
            A = torch.sparse_coo_tensor(idx, v, (N, N))
            _same_bits(torch.sparse.mm(A, torch.from_numpy(H.copy())).numpy(), ref)
    # what the chain does with the special values, seen in the reference
    ref = _sum_ref("random", "copy_u", 5)
    only_negzero = [r for r in range(N) if len(g.edges_of(r)) and
                    set(g.src[g.edges_of(r)].tolist()) <= set(NEGZERO_SRC)]
    assert only_negzero and not np.signbit(ref[only_negzero]).any()  # 0 + -0.0 = +0.0
    assert np.isnan(ref[:, 0]).any() and np.isinf(ref[:, 2]).any()


@pytest.mark.parametrize("msg,elen", [("copy_u", 0), ("u_mul_e", 5)])
def test_max_rule_is_torch_max(msg, elen):
    for name, g in _graphs().items():
        M = _messages(g, msg, _table(5), _weights(elen, len(g.src)) if elen else None)
        out, arg = _max_ref(name, msg, 5, elen)
        for r in range(N):
            es = g.edges_of(r)
            if len(es) == 0:
                assert not out[r].view(np.int32).any() and (arg[r] == -1).all()
                continue
            v, i = torch.max(torch.from_numpy(M[es]), 0)
            _same_bits(out[r], v.numpy())
            assert np.array_equal(arg[r], es[i.numpy()])
        late = [r for r in range(N) if len(_nan_slots(g, r)) and _nan_slots(g, r)[0] > 0]
        assert late and all(np.isnan(out[r, 1]) for r in late)


# ---------------------------------------------------------------------------
# Engine calls
# ---------------------------------------------------------------------------
def _adj(name, dev):
    g = _graphs()[name]
    return kernel.from_coo(N, N, torch.from_numpy(g.dst.copy()).to(dev),
                           torch.from_numpy(g.src.copy()).to(dev), kernel.ORDER_EID, dev)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _slot_weights(g, w):
    """Edge values laid out in the forward CSR's slot order."""
    return np.ascontiguousarray(w[g.order])


def _check_forward(adj, name, dev, F, reducers=("sum", "mean", "max"), msgs=None,
                   edge_order="eid", h=None):
    """Every message layout through ``reducers`` against the references."""
    g = _graphs()[name]
    h = _t(_table(F), dev) if h is None else h
    if msgs is None:
        msgs = [("copy_u", 0), ("u_mul_e", 1), ("copy_e", F)]
        if F in (5, 41):
            msgs.append(("u_mul_e", F))
    for msg, elen in msgs:
        e = None
        if elen:
            w = _weights(elen, len(g.src))
            e = _t(_slot_weights(g, w) if edge_order == "slot" else w, dev)
        for red in reducers:
            got = _np(kernel.gspmm(adj, msg, red, None if msg == "copy_e" else h, e,
                                   edge_order=edge_order))
            if red == "max":
                ref = _max_ref(name, msg, F, elen)[0]
            else:
                ref = _sum_ref(name, msg, F, elen)
                if red == "mean":
                    ref = _mean_of(ref, g.deg)
            try:
                _same_bits(got, ref)
            except AssertionError as err:
                raise AssertionError("%s %s F=%d elen=%d: %s" % (msg, red, F, elen, err))


def _check_mean_add(adj, name, dev, F, h=None):
    g = _graphs()[name]
    h = _t(_table(F), dev) if h is None else h
    with np.errstate(invalid="ignore"):
        ref = _base(F) + _mean_of(_sum_ref(name, "copy_u", F), g.deg)
    got = _np(kernel.gspmm_mean_add(adj, h, _t(_base(F), dev)))
    _same_bits(got, ref)
    zero = (g.deg == 0)[:, None] & (_base(F) == 0)  # rows without in-edges: -0.0 + 0.0 = +0.0
    assert np.signbit(_base(F)[zero]).any() and not np.signbit(got[zero]).any()


def _check_accumulate(adj, name, dev, F):
    g = _graphs()[name]
    H = _table(F)
    got = _np(kernel.gspmm_into(adj.fwd, _t(_base(F), dev), _t(H, dev), accumulate=True))
    ref = _chain_from(_base(F), g, H)
    _same_bits(got, ref)
    empty = g.deg == 0
    _same_bits(got[empty], _base(F)[empty])  # kept as they are, -0.0 included


def _assert_rows_path(adj, msg, red, F, ldu=0):
    """One launch, one wave per row: no blocks, no heavy-row split, no tiers."""
    path, launches = adj.fwd.plan.schedule(msg, red, F, ldu, N)
    assert (path, launches) == (kernel.PLAN_PATH_ROWS, 1)
    assert adj.fwd.plan.stats()["heavy_threshold"] == 0
    n_long, _ = adj.fwd.tiers()
    assert N - n_long < kernel.schedule_policy()["tier_min_rows"]


# ---------------------------------------------------------------------------
# One launch, one wave per row (the default at this size), and the host kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", F_ALL)
def test_sum_mean_max(device, F):
    dev = _dev(device)
    for name in ("random", "sorted"):
        adj = _adj(name, dev)
        if device == "cuda":
            for red in (kernel.RED_SUM, kernel.RED_MEAN, kernel.RED_MAX):
                _assert_rows_path(adj, kernel.MSG_COPY_U, red, F)
            assert not kernel._pad_rows(kernel.MSG_COPY_U, kernel.RED_SUM, _t(_table(F), dev), F)
        _check_forward(adj, name, dev, F)


def _torch_max_grads(g, H, W, G):
    """torch's CPU autograd of the per-row torch.max(mailbox, 0): (dH, dW at
    the winning slots, the mask of the winning (edge, feature) pairs)."""
    h = torch.from_numpy(H.copy()).requires_grad_(True)
    w = None if W is None else torch.from_numpy(W.copy()).requires_grad_(True)
    outs, won = [], np.zeros((len(g.src), H.shape[1]), bool)
    for r in range(N):
        es = g.edges_of(r)
        if len(es) == 0:
            outs.append(torch.zeros(H.shape[1]))
            continue
        m = h[torch.from_numpy(g.src[es])]
        if w is not None:
            m = m * w[torch.from_numpy(es.copy())]
        v, i = torch.max(m, 0)
        outs.append(v)
        won[es[i.numpy()], np.arange(H.shape[1])] = True
    torch.stack(outs).backward(torch.from_numpy(G.copy()))
    return h.grad.numpy(), None if w is None else w.grad.numpy(), won


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("msg", ["copy_u", "u_mul_e"])
def test_max_backward_is_torch_autograd(device, msg):
    """The gradient goes where torch sends it: to the first maximum, or to
    the first NaN. Integer upstream gradients and (u_mul_e) dyadic finite
    edge values: every scatter sum is exact, so equality is by bits."""
    dev = _dev(device)
    F = 5
    H = _table(F)
    for name, g in _graphs().items():
        rng = np.random.default_rng(9)
        G = rng.integers(-4, 5, (N, F)).astype(np.float32)
        W = None
        if msg == "u_mul_e":
            W = rng.choice(np.array([-2, -1, -0.5, 0.25, 0.5, 1, 1.5, 2], np.float32),
                           (len(g.src), F))
        dH, dW, won = _torch_max_grads(g, H, W, G)
        adj = _adj(name, dev)
        if device == "cuda":
            _assert_rows_path(adj, kernel.MSG_COPY_U if W is None else kernel.MSG_U_MUL_E,
                              kernel.RED_MAX, F)
        h = _t(H, dev).requires_grad_(True)
        w = None if W is None else _t(W, dev).requires_grad_(True)
        out = kernel.gspmm(adj, msg, "max", h, w)
        _same_bits(_np(out), _max_rule(g, _messages(g, msg, H, W))[0])
        out.backward(_t(G, dev))
        _same_bits(_np(h.grad), dH)
        if W is not None:
            # a message that lost has no gradient here; torch's dense product
            # rule gives it 0 * (its source value): NaN where that is not finite
            assert np.isnan(dW[~won]).any() and not dW[~won & ~np.isnan(dW)].any()
            _same_bits(_np(w.grad), np.where(won, dW, np.float32(0)).astype(np.float32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [1, 41, 128])
def test_mean_add_and_accumulate(device, F):
    dev = _dev(device)
    adj = _adj("random", dev)
    if device == "cuda":
        _assert_rows_path(adj, kernel.MSG_COPY_U, kernel.RED_MEAN_ACCUM, F)
        _assert_rows_path(adj, kernel.MSG_COPY_U, kernel.RED_SUM_ACCUM, F)
    _check_mean_add(adj, "random", dev, F)
    _check_accumulate(adj, "random", dev, F)


def _bf16_table(F, dev):
    """bf16 source rows, the specials planted after the cast (a bf16
    subnormal among them); and the same table widened back to float32."""
    Hb = torch.from_numpy(_table(F).copy()).to(torch.bfloat16)
    role = torch.arange(F) % 4
    Hb[torch.tensor(NAN_SRC)[:, None], torch.nonzero(role <= 1)[:, 0]] = float("nan")
    inf_cols = torch.nonzero((role == 0) | (role == 2))[:, 0]
    Hb[torch.tensor(PINF_SRC)[:, None], inf_cols] = float("inf")
    Hb[torch.tensor(NINF_SRC)[:, None], inf_cols] = float("-inf")
    Hb[list(NEGZERO_SRC)] = -0.0
    sub = torch.tensor([0x0040, 0x8001 - 0x10000], dtype=torch.int16).view(torch.bfloat16)
    Hb[list(SUBNORMAL_SRC[:2])] = sub[0]   # 2^-127
    Hb[list(SUBNORMAL_SRC[2:])] = sub[1]   # -2^-133, the smallest
    wide = Hb.to(torch.float32).numpy()
    assert (np.abs(wide[list(SUBNORMAL_SRC)]) < 1.2e-38).all() and wide[list(SUBNORMAL_SRC)].all()
    assert np.signbit(wide[SUBNORMAL_SRC[2]]).all()
    return Hb.to(dev), wide


def _check_bf16(adj, name, dev, F):
    g = _graphs()[name]
    Hb, wide = _bf16_table(F, dev)
    got = _np(kernel.gspmm_into(adj.fwd, torch.full((N, F), 7.0, device=dev), Hb))
    _same_bits(got, O.spmm_coo(N, g.dst, g.src, wide))
    got = _np(kernel.gspmm_into(adj.fwd, _t(_base(F), dev), Hb, accumulate=True))
    _same_bits(got, _chain_from(_base(F), g, wide))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [5, 128])
def test_bf16_source_rows(device, F):
    dev = _dev(device)
    adj = _adj("random", dev)
    if device == "cuda":
        _assert_rows_path(adj, kernel.MSG_COPY_U_BF16, kernel.RED_SUM, F)
    _check_bf16(adj, "random", dev, F)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [5, 128])
def test_transposed_backward(device, F):
    """dH = A^T dC with special values in dC: the oracle's chain over the
    transposed COO (per source, in edge-id order); for mean, dC / deg first."""
    dev = _dev(device)
    g = _graphs()["random"]
    adj = _adj("random", dev)
    dC = _table(F, seed=3)
    for red in ("sum", "mean"):
        h = _t(_table(F), dev).requires_grad_(True)
        kernel.gspmm(adj, "copy_u", red, h).backward(_t(dC, dev))
        d = dC
        if red == "mean":
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                d = (dC / np.maximum(g.deg, 1).astype(np.float32)[:, None]).astype(np.float32)
        _same_bits(_np(h.grad), O.spmm_coo(N, g.src, g.dst, d))


@pytest.mark.parametrize("device", DEVICES)
def test_update_all_max(device):
    import dgl
    import dgl.function as fn
    dev = _dev(device)
    g = _graphs()["random"]
    F = 41
    G = dgl.DGLGraph(multigraph=True)
    G.add_nodes(N)
    G.add_edges(g.src.copy(), g.dst.copy())
    G.ndata["h"] = _t(_table(F), dev)
    G.update_all(fn.copy_src("h", "m"), fn.max("m", "o"))
    _same_bits(_np(G.ndata["o"]), _max_ref("random", "copy_u", F)[0])


# ---------------------------------------------------------------------------
# The other device schedules
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("F", [5, 128])
def test_short_row_tiers(F):
    dev = _dev("cuda")
    old = kernel.set_short_rows(True)
    try:
        with kernel.scheduled(tier_min_rows=0):
            adj = _adj("random", dev)
            for red in (kernel.RED_SUM, kernel.RED_MEAN, kernel.RED_SUM_ACCUM,
                        kernel.RED_MEAN_ACCUM):
                assert adj.fwd.plan.schedule(kernel.MSG_COPY_U, red, F, 0, N) == \
                    (kernel.PLAN_PATH_ROWS, 1)
            assert adj.fwd.plan.stats()["heavy_threshold"] == 0
            n_long, tiers = adj.fwd.tiers()
            assert 0 < n_long < N and [t[0] for t in tiers] == [8, 4, 0]
            assert all(t[2] >= 20 for t in tiers)
            _check_forward(adj, "random", dev, F, ("sum", "mean"), [("copy_u", 0)])
            _check_accumulate(adj, "random", dev, F)
            _check_mean_add(adj, "random", dev, F)
            _check_bf16(adj, "random", dev, F)
    finally:
        kernel.set_short_rows(old)


def _check_chunked(got, exact, mag, heavy):
    """Chunked rows: NaNs and infinities where the exact sum has them, finite
    values within 1e-5 * sum|terms| of it."""
    got, exact, mag = got[heavy].astype(np.float64), exact[heavy], mag[heavy]
    assert np.array_equal(np.isnan(got), np.isnan(exact))
    inf = np.isinf(exact)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], exact[inf])
    fin = np.isfinite(exact)
    assert fin.any() and (np.abs(got[fin] - exact[fin]) <= 1e-5 * mag[fin]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [41, 128])
def test_heavy_row_split(F):
    dev = _dev("cuda")
    g = _graphs()["random"]
    H, B = _table(F), _base(F).astype(np.float64)
    old = kernel.set_row_split(64)
    try:
        adj = _adj("random", dev)
        assert adj.fwd.plan.stats()["heavy_threshold"] == 64
        heavy = g.deg > 64
        assert heavy.sum() == 1 and g.deg[~heavy].max() <= 40
        assert adj.fwd.split_plan(64, chunk=64)["num_chunks"] == -(-N // 64)
        for red in (kernel.RED_SUM, kernel.RED_MEAN, kernel.RED_SUM_ACCUM,
                    kernel.RED_MEAN_ACCUM):
            assert adj.fwd.plan.schedule(kernel.MSG_COPY_U, red, F, 0, N) == \
                (kernel.PLAN_PATH_ROWS, 1)
        tot, mag = _exact(g, H)
        d = g.deg[:, None].clip(min=1)
        h = _t(H, dev)
        with np.errstate(invalid="ignore"):
            cases = [
                (_np(kernel.gspmm(adj, "copy_u", "sum", h)), _sum_ref("random", "copy_u", F),
                 tot, mag),
                (_np(kernel.gspmm(adj, "copy_u", "mean", h)),
                 _mean_of(_sum_ref("random", "copy_u", F), g.deg), tot / d, mag / d),
                (_np(kernel.gspmm_into(adj.fwd, _t(_base(F), dev), h, accumulate=True)),
                 _chain_from(_base(F), g, H), B + tot, np.abs(B) + mag),
                (_np(kernel.gspmm_mean_add(adj, h, _t(_base(F), dev))),
                 _base(F) + _mean_of(_sum_ref("random", "copy_u", F), g.deg),
                 B + tot / d, np.abs(B) + mag / d),
            ]
        for got, chain, exact, m in cases:
            _same_bits(got[~heavy], chain[~heavy])
            _check_chunked(got, exact, m, heavy)
    finally:
        kernel.set_row_split(old)


def _blocked_policy(F, ld=None):
    """Blocks of about a fifth of the source table: several launches."""
    return dict(block_table_min=0, block_bytes=max(256, N * (ld or F) * 4 // 5),
                block_min_row_bytes=0, block_min_slots=1)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [5, 41, 128])
def test_source_blocked(F):
    dev = _dev("cuda")
    g = _graphs()["sorted"]
    old_knob = LIB.dglhip_set_blocked_mean_add(1)
    try:
        with kernel.scheduled(**_blocked_policy(F)):
            adj = _adj("sorted", dev)
            plan = adj.fwd.plan
            for msg, red, elen in ((kernel.MSG_COPY_U, kernel.RED_SUM, 0),
                                   (kernel.MSG_COPY_U, kernel.RED_MEAN, 0),
                                   (kernel.MSG_COPY_U, kernel.RED_MEAN_ACCUM, 0),
                                   (kernel.MSG_COPY_U, kernel.RED_SUM_ACCUM, 0),
                                   (kernel.MSG_U_MUL_E, kernel.RED_SUM, 1)):
                path, launches = plan.schedule(msg, red, F, 0, N, elen, 0)
                assert path == kernel.PLAN_PATH_BLOCKED and launches > 2, (msg, red)
            msgs = [("copy_u", 0), ("u_mul_e", 1)] + ([("u_mul_e", F)] if F <= 41 else [])
            _check_forward(adj, "sorted", dev, F, ("sum", "mean"), msgs, edge_order="slot")
            _check_mean_add(adj, "sorted", dev, F)
            _check_accumulate(adj, "sorted", dev, F)
            # max, continued block by block
            for msg in (kernel.MSG_COPY_U, kernel.MSG_U_MUL_E):
                path, launches = plan.schedule(msg, kernel.RED_MAX, F, 0, N,
                                               1 if msg == kernel.MSG_U_MUL_E else 0, 0)
                assert path == kernel.PLAN_PATH_MAX_BLOCKED and launches > 2
            cuts = [c.cpu().numpy() for c in kernel._block_cuts(
                adj.fwd, F * 4, kernel.schedule_policy()["block_bytes"])]
            later = 0
            for r in range(N):
                s = _nan_slots(g, r)
                if len(s) == 0:
                    continue
                k = g.indptr[r] + s[0]
                blocks = [i for i in range(len(cuts) - 1) if cuts[i + 1][r] > cuts[i][r]]
                mine = [i for i in blocks if cuts[i][r] <= k < cuts[i + 1][r]]
                later += len(mine) == 1 and mine[0] > blocks[0]
            assert later >= 3  # a first NaN in a block after the row's first
            _check_forward(adj, "sorted", dev, F, ("max",), msgs, edge_order="slot")
    finally:
        LIB.dglhip_set_blocked_mean_add(old_knob)


@pytest.mark.gpu
def test_source_blocked_max_backward():
    """The blocked max routes the gradient as the one-launch kernel does:
    to torch's winner (the first maximum or the first NaN)."""
    dev = _dev("cuda")
    F = 5
    g, H = _graphs()["sorted"], _table(5)
    G = np.random.default_rng(9).integers(-4, 5, (N, F)).astype(np.float32)
    dH, _, _ = _torch_max_grads(g, H, None, G)
    with kernel.scheduled(**_blocked_policy(F)):
        adj = _adj("sorted", dev)
        path, launches = adj.fwd.plan.schedule(kernel.MSG_COPY_U, kernel.RED_MAX, F, 0, N)
        assert path == kernel.PLAN_PATH_MAX_BLOCKED and launches > 2
        h = _t(H, dev).requires_grad_(True)
        kernel.gspmm(adj, "copy_u", "max", h).backward(_t(G, dev))
        _same_bits(_np(h.grad), dH)


@pytest.mark.gpu
def test_padded_stride_gather():
    dev = _dev("cuda")
    F, ld = 41, 48
    assert kernel.padded_width(F) == ld
    h = _t(_table(F), dev)
    with kernel.scheduled(pad_min_bytes=0):  # the plan's padded copy
        adj = _adj("random", dev)
        assert kernel._pad_rows(kernel.MSG_COPY_U, kernel.RED_SUM, h, F)
        for red in (kernel.RED_SUM, kernel.RED_MEAN, kernel.RED_MEAN_ACCUM):
            assert adj.fwd.plan.schedule(kernel.MSG_COPY_U, red, F, 0, N) == \
                (kernel.PLAN_PATH_ROWS, 1)
            assert adj.fwd.plan.workspace(kernel.MSG_COPY_U, red, F, 0, N, 0, 0, None) >= N * ld * 4
        _check_forward(adj, "random", dev, F, ("sum", "mean"), [("copy_u", 0), ("u_mul_e", 1)])
        _check_mean_add(adj, "random", dev, F)
    # a row-strided view read in place
    adj = _adj("random", dev)
    buf = torch.full((N, ld), float("nan"), device=dev)
    buf[:, :F] = h
    view = buf[:, :F]
    assert kernel._row_strided(view, F)
    assert adj.fwd.plan.schedule(kernel.MSG_COPY_U, kernel.RED_SUM, F, ld, N) == \
        (kernel.PLAN_PATH_ROWS, 1)
    _check_forward(adj, "random", dev, F, ("sum", "mean"), [("copy_u", 0)], h=view)
    _check_mean_add(adj, "random", dev, F, h=view)
    # the strided rows on the blocked schedule and in the short-row tiers
    old = kernel.set_short_rows(True)
    try:
        with kernel.scheduled(tier_min_rows=0):
            adj = _adj("random", dev)
            assert [t[0] for t in adj.fwd.tiers()[1]] == [8, 4, 0]
            _check_forward(adj, "random", dev, F, ("sum", "mean"), [("copy_u", 0)], h=view)
            _check_mean_add(adj, "random", dev, F, h=view)
    finally:
        kernel.set_short_rows(old)
    with kernel.scheduled(**_blocked_policy(F, ld)):
        adj = _adj("sorted", dev)
        path, launches = adj.fwd.plan.schedule(kernel.MSG_COPY_U, kernel.RED_SUM, F, ld, N)
        assert path == kernel.PLAN_PATH_BLOCKED and launches > 2
        _check_forward(adj, "sorted", dev, F, ("sum", "mean"), [("copy_u", 0)], h=view)


@pytest.mark.gpu
@pytest.mark.parametrize("n_blocks", [1, 3])
def test_source_sweep(n_blocks):
    dev = _dev("cuda")
    F = 128
    h = _t(_table(F), dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for name, g in _graphs().items():
        csr = _adj(name, dev).fwd
        lo, hi = int(g.src.min()), int(g.src.max()) + 1
        bs = max(1, -(-(hi - lo) // n_blocks))
        for mean in (False, True):
            out = torch.full((N, F), 7.0, device=dev)
            check_call(LIB.dglhip_gspmm_sweep_device(
                csr.num_rows, F, ptr(csr.indptr), ptr(csr.indices), ptr(h), ptr(out),
                ptr(csr.row_order), lo, bs, n_blocks, 1 if mean else 0, 10, stream))
            torch.cuda.synchronize()
            ref = _sum_ref(name, "copy_u", F)
            _same_bits(_np(out), _mean_of(ref, g.deg) if mean else ref)
