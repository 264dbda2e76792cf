"""The fused DistMult decoder (kernel.distmult_score, csrc/typed_block.hip):
R-GCN link prediction's score (the reference's calc_score,
examples/pytorch/rgcn/link_predict.py:50-55, s = h[s] * w[r] * h[o],
score = s.sum(1)) in one kernel, and its gradients as ordered chains.

* gradients: the bits of the torch formulation the fused model used before
  (gather_rows(h, cat(s, o)) split, times gather_rows(w, r), its duplicates
  summed by gather_rows' chains) — every term and chain is the same;
* scores: within 1e-6 of that formulation's (the sum runs in the kernel's
  lane-chain + butterfly order, not torch's) and of float64;
* host = device bit for bit; out-of-range indices give NaN, not a fault.
"""
import numpy as np
import pytest
import torch

import dgl
from dgl import kernel

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


def _dev(device):
    if device == "cuda" and not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    return torch.device(device)


def _case(N=700, R=40, F=500, n=3000, seed=0, hub=True):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(N, F, generator=gen)
    w = torch.randn(R, F, generator=gen)
    s = torch.randint(0, N, (n,), generator=gen)
    o = torch.randint(0, N, (n,), generator=gen)
    r = torch.randint(0, R, (n,), generator=gen)
    if hub:  # a hub entity and relation of > DGLHIP_TYPED_CHUNK positions
        s[::7] = 3
        r[::5] = 1
    return h, w, s, r, o


def _torch_form(h, w, s, r, o):
    n = s.numel()
    ho = kernel.gather_rows(h, torch.cat([s, o]))
    return (ho[:n] * kernel.gather_rows(w, r) * ho[n:]).sum(1)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [500, 64, 37])
def test_distmult_grads_bits_of_the_torch_form(device, F):
    dev = _dev(device)
    h, w, s, r, o = (t.to(dev) for t in _case(F=F))
    h1, w1 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    h2, w2 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    sc = kernel.distmult_score(h1, w1, s, r, o)
    ref = _torch_form(h2, w2, s, r, o)
    exact = (h.double()[s] * w.double()[r] * h.double()[o]).sum(1)
    mag = (h.double()[s] * w.double()[r] * h.double()[o]).abs().sum(1)
    assert ((sc.double() - exact).abs() <= 1e-6 * mag + 1e-30).all()
    assert ((ref.double() - exact).abs() <= 1e-6 * mag + 1e-30).all()
    dsc = torch.randn(s.numel(), generator=torch.Generator().manual_seed(3)).to(dev)
    g1 = torch.autograd.grad(sc, (h1, w1), dsc)
    g2 = torch.autograd.grad(ref, (h2, w2), dsc)
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])


@pytest.mark.parametrize("device", DEVICES)
def test_distmult_only_one_grad_and_empty(device):
    dev = _dev(device)
    h, w, s, r, o = (t.to(dev) for t in _case(n=500, hub=False))
    h1 = h.clone().requires_grad_(True)
    (dh,) = torch.autograd.grad(kernel.distmult_score(h1, w, s, r, o).sum(), (h1,))
    h2 = h.clone().requires_grad_(True)
    (dh2,) = torch.autograd.grad(_torch_form(h2, w, s, r, o).sum(), (h2,))
    assert torch.equal(dh, dh2)
    e = torch.empty(0, dtype=torch.int64, device=dev)
    h3 = h.clone().requires_grad_(True)
    sc = kernel.distmult_score(h3, w, e, e, e)
    assert sc.shape == (0,)
    (dh3,) = torch.autograd.grad(sc.sum(), (h3,), allow_unused=True)
    assert dh3 is None or not dh3.any()


@pytest.mark.parametrize("device", DEVICES)
def test_distmult_out_of_range_raises(device):
    """Out-of-range subject, relation or object ids raise IndexError at the
    call, as index_select in the torch formulation does, rather
    than surfacing later as a NaN loss; the kernel itself never reads past
    its tables (NaN for such a position)."""
    dev = _dev(device)
    old = kernel.set_validate_indices(True)  # device-resident ids: checked on request
    try:
        for which, bad in ((0, "s"), (1, "r"), (2, "o"), (1, "neg")):
            h, w, s, r, o = _case(n=10, hub=False)
            t = [s, r, o][which]
            t[4] = -1 if bad == "neg" else (w.shape[0] if which == 1 else h.shape[0])
            with pytest.raises(IndexError):
                kernel.distmult_score(h.to(dev), w.to(dev), s.to(dev), r.to(dev), o.to(dev))
            # host-resident ids are checked whatever the setting
            kernel.set_validate_indices(False)
            with pytest.raises(IndexError):
                kernel.distmult_score(h.to(dev), w.to(dev), s, r, o)
            kernel.set_validate_indices(True)
    finally:
        kernel.set_validate_indices(old)
    h, w, s, r, o = _case(n=10, hub=False)
    s[4] = h.shape[0]
    r[6] = -1
    sc = kernel._DistMult.apply(h, w, s, r, o)  # the kernel without the check
    assert torch.isnan(sc[4]) and torch.isnan(sc[6])
    assert torch.isfinite(sc[[0, 1, 2, 3, 5, 7, 8, 9]]).all()


@pytest.mark.gpu
def test_distmult_host_equals_device():
    dev = _dev("cuda")
    h, w, s, r, o = _case()
    dsc = torch.randn(s.numel(), generator=torch.Generator().manual_seed(4))
    res = []
    for d in (torch.device("cpu"), dev):
        hh, ww = h.to(d).requires_grad_(True), w.to(d).requires_grad_(True)
        sc = kernel.distmult_score(hh, ww, s.to(d), r.to(d), o.to(d))
        g = torch.autograd.grad(sc, (hh, ww), dsc.to(d))
        res.append([sc.detach().cpu(), g[0].cpu(), g[1].cpu()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", [500, 37])
def test_distmult_link_loss_matches_float64(device, F):
    """kernel.distmult_link_loss (the example's get_loss: BCE-with-logits of
    the scores, mean, + reg * (mean(h^2) + mean(w^2))) — fused on a device,
    the torch expression on the host — against float64: the loss within 1e-5
    of its terms' magnitudes, the scores with distmult_score's bits, every
    gradient element within 1e-5 of its Σ|terms| (hub rows of several chunks
    and rows no triple touches included)."""
    dev = _dev(device)
    h, w, s, r, o = _case(F=F, N=900)  # rows past 700 see no triple
    s, o = s % 700, o % 700
    _check_link_loss(dev, h, w, s, r, o)


def _check_link_loss(dev, h, w, s, r, o):
    labels = (torch.arange(s.numel()) % 2).float()
    reg = 0.01
    h1, w1 = h.clone().to(dev).requires_grad_(True), w.clone().to(dev).requires_grad_(True)
    loss = kernel.distmult_link_loss(h1, w1, s.to(dev), r.to(dev), o.to(dev), labels.to(dev), reg)
    loss.backward()
    h2, w2 = h.double().requires_grad_(True), w.double().requires_grad_(True)
    score = (h2[s] * w2[r] * h2[o]).sum(1)
    ref = (torch.nn.functional.binary_cross_entropy_with_logits(score, labels.double()) +
           reg * (h2.pow(2).mean() + w2.pow(2).mean()))
    ref.backward()
    with torch.no_grad():
        mag_s = (h2[s] * w2[r] * h2[o]).abs().sum(1)
        lmag = (mag_s + 1.0).mean() + reg * (h2.pow(2).mean() + w2.pow(2).mean())
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(lmag)
    # gradient bounds: the same chains over magnitudes
    ha, wa = h.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    with torch.no_grad():
        # |sigmoid| + |label|: the Σ|terms| of the BCE gradient's subtraction
        # (saturated logits cancel it)
        ds = (torch.sigmoid(score) + labels.double()) / s.numel()
    lm = (ds * (ha[s] * wa[r] * ha[o]).sum(1)).sum() + reg * (ha.pow(2).mean() +
                                                             wa.pow(2).mean())
    lm.backward()
    for got, want, bound in ((h1.grad, h2.grad, ha.grad), (w1.grad, w2.grad, wa.grad)):
        err = (got.double().cpu() - want).abs()
        assert bool((err <= 1e-5 * bound + 1e-30).all()), float((err / (bound + 1e-30)).max())


# ---- widths and sample counts at the kernels' cuts -------------------------
# F: T = 1 up to 64 features per wave slice, T = 2 at 65..128, T = 4 at
# 193..448, T = 8 beyond, two passes past 512; a last slice with idle lanes at
# 63, 129 and 513. Samples: the score and loss kernels take 4 per workgroup, so
# 1, 2, 3, 5 and 261 leave a last workgroup with idle waves.
EDGE_F = [1, 63, 65, 128, 129, 300, 448, 512, 513, 1000]
EDGE_N = [1, 2, 3, 5, 261]
EDGE_NODES, EDGE_RELS = 40, 6


def _edge_triples(n):
    """(s, r, o) over 40 nodes and 6 relations, relation 0 never used. At 261
    samples the positions sit at the 64-position chunk: node 1 is the subject
    of exactly 64 samples, node 2 of 65, node 3 the object of 128 (none of
    them on the other side, so their gradient rows hold exactly that many
    positions), and relation 1 holds 129 samples."""
    rng = np.random.default_rng(100 + n)
    if n == 261:
        s = np.concatenate([np.full(64, 1), np.full(65, 2), rng.integers(4, EDGE_NODES, 132)])
        o = np.concatenate([np.full(128, 3), rng.integers(4, EDGE_NODES, 133)])
        r = np.concatenate([np.full(129, 1), rng.integers(2, EDGE_RELS, 132)])
        s, o, r = rng.permutation(s), rng.permutation(o), rng.permutation(r)
    else:
        s, o = rng.integers(0, EDGE_NODES, n), rng.integers(0, EDGE_NODES, n)
        r = rng.integers(1, EDGE_RELS, n)
    return tuple(torch.from_numpy(a.astype(np.int64)) for a in (s, r, o))


def test_edge_triples_have_the_intended_counts():
    s, r, o = _edge_triples(261)
    assert s.numel() == r.numel() == o.numel() == 261
    subj, obj = torch.bincount(s, minlength=EDGE_NODES), torch.bincount(o, minlength=EDGE_NODES)
    assert subj[1] == 64 and subj[2] == 65 and obj[3] == 128
    # their rows of dh hold exactly those positions of cat(s, o): 1, 2 and 3 chunks' edges
    both = subj + obj
    assert both[1] == 64 and both[2] == 65 and both[3] == 128
    assert torch.bincount(r, minlength=EDGE_RELS)[1] == 129
    ptr_, _ = kernel._position_groups(torch.cat([s, o]), EDGE_NODES)
    item_ptr, _ = kernel._typed_items(ptr_, 522)
    assert (item_ptr[1:] - item_ptr[:-1])[:4].tolist() == [1, 1, 2, 2]
    for n in EDGE_N:
        s, r, o = _edge_triples(n)
        assert s.numel() == n and int(r.min()) >= 1  # relation 0 is never used
        assert int(s.max()) < EDGE_NODES and int(o.max()) < EDGE_NODES and int(r.max()) < EDGE_RELS


def _edge_case(F, n):
    gen = torch.Generator().manual_seed(7 * F + n)
    h = torch.randn(EDGE_NODES, F, generator=gen)
    w = torch.randn(EDGE_RELS, F, generator=gen)
    dsc = torch.randn(n, generator=gen)
    return (h, w) + _edge_triples(n) + (dsc,)


def _edge_run(F, n, dev):
    h, w, s, r, o, dsc = (t.to(dev) for t in _edge_case(F, n))
    h1, w1 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    for t in (h, w):  # NaNs where the allocator is about to hand memory out again
        del_me = torch.full_like(t, float("nan"))
        del del_me
    sc = kernel.distmult_score(h1, w1, s, r, o)
    g = torch.autograd.grad(sc, (h1, w1), dsc)
    return sc.detach(), g[0], g[1]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("F", EDGE_F)
def test_distmult_widths_and_partial_blocks(device, F):
    """Every width class of distmult_grad_kernel<T> (one pass and two) and
    sample counts that leave idle waves and idle batch slots: gradients with
    the bits of the gather_rows torch form, scores within 1e-6 * Σ|terms| of
    float64, and an exactly zero gradient row for the unused relation."""
    dev = _dev(device)
    for n in EDGE_N:
        h, w, s, r, o, dsc = (t.to(dev) for t in _edge_case(F, n))
        sc, dh, dw = _edge_run(F, n, dev)
        h2, w2 = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ref = _torch_form(h2, w2, s, r, o)
        g2 = torch.autograd.grad(ref, (h2, w2), dsc)
        assert torch.equal(dh, g2[0]) and torch.equal(dw, g2[1])
        terms = h.double()[s] * w.double()[r] * h.double()[o]
        exact, mag = terms.sum(1), terms.abs().sum(1)
        err = (sc.double() - exact).abs()
        print(F, n, device, "worst score err / bound = %.3g" % float((err / (1e-6 * mag + 1e-30)).max()))
        assert (err <= 1e-6 * mag + 1e-30).all()
        assert (dw[0].view(torch.int32) == 0).all()
        untouched = torch.ones(EDGE_NODES, dtype=torch.bool)
        untouched[torch.cat([s, o]).cpu()] = False
        assert not dh.cpu()[untouched].any()


@pytest.mark.gpu
@pytest.mark.parametrize("F", EDGE_F)
def test_distmult_widths_host_equals_device(F):
    dev = _dev("cuda")
    for n in EDGE_N:
        for a, b in zip(_edge_run(F, n, torch.device("cpu")), _edge_run(F, n, dev)):
            assert torch.equal(a.view(torch.int32), b.cpu().view(torch.int32))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("F", [37, 513])
def test_distmult_link_loss_partial_blocks(device, F, n):
    """distmult_link_loss at 1 and 3 samples: a last (only) workgroup with
    idle waves, and with 40 x F and 6 x F elements over 512 h^2 / w^2 chunks,
    chunks that are empty. The bounds of test_distmult_link_loss_matches_float64."""
    dev = _dev(device)
    h, w, s, r, o, _ = _edge_case(F, n)
    _check_link_loss(dev, h, w, s, r, o)


@pytest.mark.gpu
def test_position_groups_items_of_no_ids():
    """kernel._position_groups_items over an empty id tensor (a null data
    pointer) equals the host build: every row empty, one item per row."""
    _dev("cuda")
    ids = torch.empty(0, dtype=torch.int64)
    for rows in (1, EDGE_RELS, 70):
        ph, oh = kernel._position_groups(ids, rows)
        pd, od, ipd, ird = kernel._position_groups_items(ids.cuda(), rows)
        assert torch.equal(ph, pd.cpu()) and torch.equal(oh, od.cpu()) and od.numel() == 0
        iph, irh = kernel._typed_items(ph, 0)
        assert torch.equal(iph, ipd.cpu()) and torch.equal(irh, ird.cpu())
        assert iph.tolist() == list(range(rows + 1))
