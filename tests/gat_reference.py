"""A float64 reference of the GAT aggregation and the derived error bound the
GAT tests hold the kernels to (shared by test_gat_reference.py and
test_gat_fused.py; nothing here calls the library's kernels).

The reference is plain torch float64 on the CPU over an edge list in the
forward CSR's slot order. Next to every tensor it returns the tensor's
condition scale S: the same expression with every term replaced by its
absolute value. The bound per element is

    |got - ref| <= (L + Dg + ALLOWANCE) * 2^-24 * S + 1e-30

L the element's chain length ((n - 1) u of a sequential float32 sum), Dg the
head width for d_el / d_er (their terms hold a D-term dot), ALLOWANCE = 16 the
per-term operations: the slope multiply, __expf (about 1 + |x| ulps for
|x| <= 4), the dropout scale, the product, the dz addition and the epilogue
multiplies. S == 0 must give exactly 0.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
ALLOWANCE = 16
# designated in-degrees of the hub rows and out-degrees of the hub sources: the
# edges of the 16-slot LDS batch and UNROLL, of rowsum_heads8's 64-slot step
HUB_DEGREES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)


class EdgeGraph(object):
    """src / dst (int64 numpy, edge-id order) of an R x N adjacency; hub row i
    (destination ``hub_rows[i]``) has in-degree HUB_DEGREES[i], hub source i
    (``hub_srcs[i]``) out-degree HUB_DEGREES[i]."""

    def __init__(self, R, N, src, dst, hub_rows, hub_srcs):
        self.R, self.N, self.src, self.dst = R, N, src, dst
        self.hub_rows, self.hub_srcs = hub_rows, hub_srcs


@functools.lru_cache(maxsize=None)
def edge_graph(R, N, seed, order):
    """A small graph with every batch edge in it. Rows 0..14 are the hub rows,
    sources N-15..N-1 the hub sources (neither touches the other's edges, so
    their degrees are exactly HUB_DEGREES); the other rows draw a target
    in-degree from 0..8 (the larger of two draws) and take background edges up
    to it from the other sources while those have fewer than 8 out-edges (a
    rectangular adjacency with few rows or few sources exceeds 8 on its
    ordinary ones: the hubs' edges have nowhere else to go; no degree exceeds
    129 anywhere). A few parallel edges and, on a square adjacency,
    self-loops. ``order``: "shuffled" numbers the edges at random (edge id !=
    slot order), "src" source-major."""
    rng = np.random.default_rng(seed)
    nh = len(HUB_DEGREES)
    hub_rows = np.arange(nh)
    hub_srcs = np.arange(N - nh, N)
    rows = np.arange(nh, R)           # ordinary rows
    srcs = np.arange(0, N - nh)       # ordinary sources
    src, dst = [], []
    # hub rows: sources dealt round-robin from a shuffled list (distinct
    # within a row, at most a few per source overall)
    deal = rng.permutation(srcs)
    at = 0
    for r, deg in zip(hub_rows, HUB_DEGREES):
        take = deal[(at + np.arange(deg)) % len(deal)]
        at += deg
        src.extend(take.tolist())
        dst.extend([r] * deg)
    # hub sources: destinations dealt the same way over the ordinary rows
    deal = rng.permutation(rows)
    at = 0
    for s, deg in zip(hub_srcs, HUB_DEGREES):
        take = deal[(at + np.arange(deg)) % len(deal)]
        at += deg
        src.extend([s] * deg)
        dst.extend(take.tolist())
    indeg = np.bincount(np.asarray(dst, dtype=np.int64), minlength=R)
    outdeg = np.bincount(np.asarray(src, dtype=np.int64), minlength=N)
    target = np.maximum(rng.integers(0, 9, R), rng.integers(0, 9, R))
    for r in rows:
        # self-loops on a square adjacency, a parallel edge now and then
        while indeg[r] < target[r]:
            free = srcs[outdeg[srcs] < 8]
            if free.size == 0:
                break
            s = int(rng.choice(free))
            if R == N and r < N - nh and outdeg[r] < 8 and rng.random() < 0.05:
                s = int(r)
            reps = 2 if (rng.random() < 0.03 and indeg[r] + 2 <= target[r]
                         and outdeg[s] + 2 <= 8) else 1
            for _ in range(reps):
                src.append(s)
                dst.append(int(r))
                indeg[r] += 1
                outdeg[s] += 1
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    if order == "shuffled":
        o = rng.permutation(src.size)
    elif order == "src":
        o = np.lexsort((dst, src))
    else:
        raise ValueError(order)
    return EdgeGraph(R, N, src[o], dst[o], hub_rows, hub_srcs)


def dyadic(shape, gen):
    """float32 multiples of 1/8 in [-2, 2]: sums of two are exact in float32,
    exact zeros occur, and exp(x) crosses a clamp at 10 between the grid
    points 2.25 and 2.375."""
    return torch.randint(-16, 17, shape, generator=gen).to(torch.float32) / 8.0


def _rows_add(n, index, values):
    return torch.zeros((n,) + tuple(values.shape[1:]), dtype=torch.float64).index_add(
        0, index, values)


def gat_reference64(src, dst, R, N, ft, el, er, alpha, lo, hi, apply_exp, keep, p, dout, dz,
                    shares=True):
    """The GAT aggregation and its gradients in float64 torch on the CPU.

    src / dst: int64 (E,), the edges in forward-slot order; ft (N, H, D),
    el (N, H), er (R, H): float32 values; keep: bool (E, H) or None (p == 0);
    dout (R, H, D) / dz (R, H): the gradients of fs and z, None when that
    output is unused. Returns a dict of
      fs, z, d_ft, d_el, d_er  (the gradients of (fs * dout).sum() + (z * dz).sum(),
                                leaky_relu's own backward: slope 1 for x > 0,
                                alpha for x <= 0),
      S_fs, S_z, S_dft, S_del, S_der  (each tensor's condition scale),
      L_in (R,), L_out (N,)    (in-degrees, out-degrees: the chain lengths).
    Asserts that every pair's pre-clamp value is more than 1e-3 (relative)
    away from both clamp bounds, so the clamp gate is the same set in float32
    and float64, and, when a bound is finite and ``shares``, that at least 5 %
    of the pairs are clamped and at least 5 % are not (with no finite bound
    there is no clamp to share out)."""
    src, dst = torch.as_tensor(src).long().cpu(), torch.as_tensor(dst).long().cpu()
    ft, el, er = (t.detach().cpu().double().requires_grad_(True) for t in (ft, el, er))
    H = el.shape[1]
    el2, er2 = el.reshape(-1, H), er.reshape(-1, H)
    x = el2[src] + er2[dst]
    y = F.leaky_relu(x, alpha)
    pre = torch.exp(y) if apply_exp else y
    with torch.no_grad():
        for b in (lo, hi):
            if np.isfinite(b):
                assert bool(((pre - b).abs() > 1e-3 * abs(b)).all()), \
                    "a pair within 1e-3 of the clamp bound %r" % (b,)
        inside = (pre > lo) & (pre < hi)
        share = float(inside.double().mean()) if inside.numel() else 0.0
        if shares and (np.isfinite(lo) or np.isfinite(hi)):
            assert 0.05 <= share <= 0.95, "unclamped share %.3f" % share
    a = pre.clamp(lo, hi)
    scale = 1.0 / (1.0 - p) if keep is not None else 1.0
    kf = torch.ones_like(a) if keep is None else keep.cpu().double()
    w = a * kf * scale
    fs = _rows_add(R, dst, w.unsqueeze(-1) * ft[src])
    z = _rows_add(R, dst, a)
    loss = 0.0
    if dout is not None:
        dout = dout.detach().cpu().double().reshape(R, H, -1)
        loss = loss + (fs * dout).sum()
    if dz is not None:
        dz = dz.detach().cpu().double().reshape(R, H)
        loss = loss + (z * dz).sum()
    grads = (None, None, None)
    if dout is not None or dz is not None:  # (ft is unused when only z is)
        grads = torch.autograd.grad(loss, (ft, el, er), allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, (ft, el, er))]
    with torch.no_grad():
        ftd = ft.detach()
        S_fs = _rows_add(R, dst, w.abs().unsqueeze(-1) * ftd[src].abs())
        S_z = _rows_add(R, dst, a.abs())
        slope = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, alpha))
        mag = a.abs() if apply_exp else torch.ones_like(a)
        t = torch.zeros_like(a)
        if dout is not None:
            S_dft = _rows_add(ftd.shape[0], src, w.abs().unsqueeze(-1) * dout[dst].abs())
            t = t + kf * scale * (dout[dst] * ftd[src]).abs().sum(-1)
        else:
            S_dft = torch.zeros_like(ftd)
        if dz is not None:
            t = t + dz[dst].abs()
        S_g = inside.double() * slope * mag * t
        S_del = _rows_add(el2.shape[0], src, S_g)
        S_der = _rows_add(R, dst, S_g)
    return {
        "fs": fs.detach(), "z": z.detach(), "d_ft": grads[0], "d_el": grads[1].reshape(-1, H),
        "d_er": grads[2].reshape(-1, H),
        "S_fs": S_fs, "S_z": S_z, "S_dft": S_dft, "S_del": S_del, "S_der": S_der,
        "L_in": torch.bincount(dst, minlength=R),
        "L_out": torch.bincount(src, minlength=ftd.shape[0]),
        "inside_share": share,
    }


def used_allowance(got, ref, S, L):
    """The largest err / (2^-24 * S) - L over the elements with S > 0: how
    much of the per-term allowance (plus Dg) the result uses."""
    got = got.detach().cpu().double().reshape(ref.shape)
    L = L.double().reshape((-1,) + (1,) * (ref.dim() - 1)).expand_as(ref)
    pos = S > 0
    if not bool(pos.any()):
        return 0.0
    return float((((got - ref).abs()[pos] / (U24 * S[pos])) - L[pos]).max())


# the largest used_allowance seen per tensor name since import (a measuring
# script reads it after a run; the tests themselves print nothing)
USED = {}


def assert_within(got, ref, S, L, Dg, what, rows=None):
    """got within (L + Dg + ALLOWANCE) * 2^-24 * S + 1e-30 of ref per element
    and exactly 0 where S == 0; NaN and infinity are outside any bound. ``L``:
    the chain length per leading row. ``rows``: restrict the comparison to
    these leading rows. Returns the used share of the allowance
    (used_allowance) and records its maximum per tensor name in USED."""
    got = got.detach().cpu().double().reshape(ref.shape)
    if rows is not None:
        rows = torch.as_tensor(rows).long()
        got, ref, S, L = got[rows], ref[rows], S[rows], L[rows]
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements" % (
        what, int((~torch.isfinite(got)).sum()))
    Lx = L.double().reshape((-1,) + (1,) * (ref.dim() - 1)).expand_as(ref)
    err = (got - ref).abs()
    bound = (Lx + Dg + ALLOWANCE) * U24 * S + 1e-30
    zero = S == 0
    assert bool((got[zero] == 0).all()), "%s: nonzero where the condition scale is 0" % what
    bad = ~(err <= bound)  # (a NaN compares False: outside)
    if bool(bad.any()):
        i = int(torch.argmax((err / bound).reshape(-1)))
        raise AssertionError(
            "%s: %d of %d elements outside the bound; worst err %.3e, bound %.3e (L %d, S %.3e)"
            % (what, int(bad.sum()), bad.numel(), float(err.reshape(-1)[i]),
               float(bound.reshape(-1)[i]), int(Lx.reshape(-1)[i]), float(S.reshape(-1)[i])))
    used = used_allowance(got, ref, S, L)
    name = what.split()[0] if what.split() else what
    USED[name] = max(USED.get(name, used), used)
    return used


def check_all(ref, fs=None, z=None, d_ft=None, d_el=None, d_er=None, D=0, what="", rows=None,
              srcs=None):
    """Every given tensor against the reference ``ref`` (gat_reference64's
    dict): fs, z and d_er chained along the rows (restricted to ``rows``),
    d_ft and d_el along the sources (restricted to ``srcs``)."""
    if fs is not None:
        assert_within(fs, ref["fs"], ref["S_fs"], ref["L_in"], 0, "fs " + what, rows)
    if z is not None:
        assert_within(z, ref["z"], ref["S_z"], ref["L_in"], 0, "z " + what, rows)
    if d_ft is not None:
        assert_within(d_ft, ref["d_ft"], ref["S_dft"], ref["L_out"], 0, "d_ft " + what, srcs)
    if d_el is not None:
        assert_within(d_el, ref["d_el"], ref["S_del"], ref["L_out"], D, "d_el " + what, srcs)
    if d_er is not None:
        assert_within(d_er, ref["d_er"], ref["S_der"], ref["L_in"], D, "d_er " + what, rows)
