"""Modified-topology RNN-T on the GPU against the float64 references of tests/rnnt_modified_common.py.

Tolerances are the project's own for these kernels: costs 1e-5 relative, gradient and occupancy entries
test_rnnt_routes_gpu._tol(T) (the recurrence has T dependent steps here), d(logits) the bound of
test_rnnt_routes_gpu._check_dlogits, as test_rnnt_pruned_gpu.py uses it for its from-logits case.

Lengths (_lengths): utterance 0 fills the batch's frames, with U_n = min(U, T); then one with T_n = U_n (every frame emits,
the terminal label edge), one with T_n = 1 and U_n = 0, and -- `infeasible`, where U >= 2 -- one with U_n = T_n + 1, which
must cost +inf with a zero gradient while its neighbours stay within tolerance.  Batches of three drop one of the two
middle ones (by the parity of U), so every kind occurs at every lattice width.  The pruned cases keep T_n - 1 >= s_max,
without which no band of the width exists."""
import numpy as np
import pytest
import torch

import rnnt_modified_common as M
import test_rnnt_routes_gpu as R

pytestmark = pytest.mark.gpu

_cache = {}


def _d(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # (a copy: the cached references are read-only)


def _lengths(B, T, U, infeasible=False):
    m = min(T, U)
    h = max(1, (m + 1) // 2) if U else 1
    cand = [(T, m), (h, min(h, U)), (1, 0)]
    if B == 3 and U % 2:
        cand = [cand[0], cand[2], cand[1]]
    if infeasible and U >= 2:
        k = min(T, U - 1)
        cand.insert(min(B, 4) - 1, (k, k + 1))
    cand += [(max(1, T - 1), m // 3)] * B
    tl, ul = zip(*cand[:B])
    return np.array(tl, np.int32), np.array(ul, np.int32)


def _labels(B, U, V, ul, rng, blank=0):
    y = rng.integers(0, V - 1, (B, U)).astype(np.int32)
    y[y >= blank] += 1
    for n in range(B):
        y[n, ul[n]:] = V                                     # padding (never read)
    return y


def _check_costs(c, c64, what, worst):
    inf = np.isinf(c64)
    assert np.array_equal(np.isposinf(c), inf), (what, c, c64)
    if (~inf).any():
        R._check_costs(c[~inf], c64[~inf], what, worst)


# ---- the planes loss ----------------------------------------------------------------------------------------------------
PLANES = [(4, 9, 8), (3, 70, 64), (3, 300, 299), (2, 1, 1), (2, 1, 0), (4, 15, 5), (4, 16, 5), (4, 17, 5), (4, 33, 5)]


def _planes_case(B, T, U):
    key = ("planes", B, T, U)
    if key not in _cache:
        rng = np.random.default_rng(1000 * T + U)
        tl, ul = _lengths(B, T, U, infeasible=True)
        assert B < 3 or U < 2 or (ul == tl + 1).any()
        # unnormalised on purpose, and whole rows (frames) shifted by +-80
        shift = rng.choice([-80.0, 0.0, 80.0], (B, T, 1, 1))
        planes = (np.log(rng.uniform(0.05, 1.5, (B, T, U + 1, 2))) + shift).astype(np.float32)
        w = (rng.random(B) + 0.5).astype(np.float32)
        c64, ob, ol = M.planes_loss_ref(planes[..., 0], planes[..., 1], tl, ul)
        for a in (planes, tl, ul, w, c64, ob, ol):
            a.setflags(write=False)
        _cache[key] = (planes, tl, ul, w, c64, ob, ol)
    return _cache[key]


@pytest.mark.parametrize("B,T,U", PLANES, ids=["B%d-T%d-U%d" % c for c in PLANES])
def test_planes_loss_matches_fp64(hip_device, B, T, U):
    from pika_amd.rnnt import rnnt_loss_from_planes_modified
    dev = hip_device
    planes, tl, ul, w, c64, ob64, ol64 = _planes_case(B, T, U)
    pb = _d(planes[..., 0], dev).requires_grad_(True)
    pl = _d(planes[..., 1], dev).requires_grad_(True)
    costs, ob, ol = rnnt_loss_from_planes_modified(pb, pl, _d(tl, dev), _d(ul, dev), return_occupancy=True)
    assert not ob.requires_grad and not ol.requires_grad
    costs.backward(_d(w, dev))
    torch.cuda.synchronize()
    worst = {}
    _check_costs(costs.detach().cpu().numpy(), c64, "planes", worst)
    rel, abs_ = R._tol(T)
    ws = w[:, None, None].astype(np.float64)
    R._check_grads(pb.grad.cpu().numpy(), -ob64 * ws, rel, abs_, "blank plane", worst)
    R._check_grads(pl.grad.cpu().numpy(), -ol64 * ws, rel, abs_, "label plane", worst)
    R._check_grads(ob.cpu().numpy(), ob64, rel, abs_, "blank occupancy", worst)
    R._check_grads(ol.cpu().numpy(), ol64, rel, abs_, "label occupancy", worst)
    for n in np.nonzero(np.isinf(c64))[0]:                   # no path: exactly zero, no NaN
        assert not ob[n].any() and not ol[n].any() and not pb.grad[n].any() and not pl.grad[n].any()
    dead = ~R._live(tl, ul, T, U + 1)
    assert not ob.cpu().numpy()[dead].any() and not ol.cpu().numpy()[dead].any()
    only = rnnt_loss_from_planes_modified(pb, pl, _d(tl, dev), _d(ul, dev), reduction=None)
    assert torch.equal(only, costs.detach())
    R._report("modified planes B%d-T%d-U%d" % (B, T, U), worst)


# ---- the pruned loss ----------------------------------------------------------------------------------------------------
PRUNED = [(4, 9, 6, 3), (3, 40, 64, 5), (2, 300, 299, 4)]


def _band_planes(band, y, ranges, ul, U1, blank=0):
    """The two (B,T,U1) float64 planes of a band (B,T,S,V) scattered to its cells, -inf elsewhere."""
    B, T, S, V = band.shape
    s = M.clamp_ranges(ranges, ul, S)
    pb, pl = np.full((B, T, U1), -np.inf), np.full((B, T, U1), -np.inf)
    for b in range(B):
        for j in range(S):
            u = s[b] + j                                     # (T,)
            ok = u <= ul[b]
            t = np.nonzero(ok)[0]
            pb[b, t, u[t]] = band[b, t, j, blank]
            lab = ok & (u < ul[b])
            t = np.nonzero(lab)[0]
            pl[b, t, u[t]] = band[b, t, j, y[b, u[t]]]
    return pb, pl


def _band_grads(ob, ol, y, ranges, ul, S, V, w, blank=0, lam=0.0):
    """d (sum_n w_n cost_n) / d band, (B,T,S,V) float64, from the occupancies on the full lattice."""
    B, T, U1 = ob.shape
    s = M.clamp_ranges(ranges, ul, S)
    g = np.zeros((B, T, S, V))
    tt = np.arange(T)
    for b in range(B):
        for j in range(S):
            u = s[b] + j
            ok = u <= ul[b]
            t = tt[ok]
            g[b, t, j, blank] = -w[b] * ob[b, t, u[t]]
            t = tt[ok & (u < ul[b])]
            g[b, t, j, y[b, u[t]]] += -w[b] * (1.0 + lam) * ol[b, t, u[t]]
    return g


def _pruned_lengths(B, T, U, S):
    tl, ul = _lengths(B, T, U)
    return tl, np.minimum(ul, tl - 1 + S - 1).astype(np.int32)       # T_n - 1 >= U_n + 1 - S


def _searched_ranges(pb, pl, tl, ul, S, dev):
    from pika_amd.rnnt import rnnt_loss_from_planes_modified, rnnt_prune_ranges_modified
    tl_d, ul_d = _d(tl, dev), _d(ul, dev)
    fin = lambda a: _d(np.maximum(a, M.NEG).astype(np.float32), dev)   # noqa: E731
    _, ob, ol = rnnt_loss_from_planes_modified(fin(pb), fin(pl), tl_d, ul_d, return_occupancy=True)
    return rnnt_prune_ranges_modified(ob, ol, tl_d, ul_d, S).cpu().numpy()


def _pruned_case(case, V, kind, dev):
    """Raw band logits, labels, lengths, ranges, weights and the float64 reference of the band's log-softmax."""
    key = ("pruned", case, V, kind)
    if key not in _cache:
        B, T, U, S = case
        rng = np.random.default_rng(100 * T + V)
        tl, ul = _pruned_lengths(B, T, U, S)
        y = _labels(B, U, V, ul, rng)
        w = (rng.random(B) + 0.5).astype(np.float32)
        if kind == "random":
            ranges = M.random_valid_ranges_modified(tl, ul, S, rng, T=T)
        else:           # the package's own band search, on the occupancies of the planes of a full-lattice draw
            full = np.log(rng.uniform(0.05, 1.0, (2, B, T, U + 1)))
            ranges = _searched_ranges(full[0], full[1], tl, ul, S, dev)
            for n in range(B):
                assert M.is_valid_modified(ranges[n], tl[n], ul[n], S), (n, ranges[n], tl[n], ul[n])
        logits = (rng.standard_normal((B, T, S, V)) * 2).astype(np.float32)
        x64 = logits.reshape(-1, V).astype(np.float64)
        lse = R._lse(x64)
        lp64 = (x64 - lse).reshape(B, T, S, V)
        pb, pl = _band_planes(lp64, y, ranges, ul, U + 1)
        c64, ob, ol = M.planes_loss_ref(pb, pl, tl, ul)
        g = _band_grads(ob, ol, y, ranges, ul, S, V, w)
        _cache[key] = (logits, y, tl, ul, ranges, w, lp64, c64, g, (pb, pl))
    return _cache[key]


def _run(fn, dev, x, y, ranges, tl, ul, w, **kw):
    x = _d(x, dev).requires_grad_(True)
    extra = () if ranges is None else (_d(ranges, dev),)
    costs = fn(x, _d(y, dev), *extra, _d(tl, dev), _d(ul, dev), **kw)
    costs.backward(_d(w, dev))
    torch.cuda.synchronize()
    return costs.detach(), x.grad


@pytest.mark.parametrize("kind", ["random", "searched"])
@pytest.mark.parametrize("V", [8, 5000])
@pytest.mark.parametrize("case", PRUNED, ids=["B%d-T%d-U%d-S%d" % c for c in PRUNED])
def test_pruned_loss_matches_fp64(hip_device, case, V, kind):
    from pika_amd.rnnt import rnnt_loss_pruned_modified, rnnt_loss_pruned_modified_from_logits
    from rnnt_pruned_common import band_live
    dev = hip_device
    B, T, U, S = case
    logits, y, tl, ul, ranges, w, lp64, c64, g64, _ = _pruned_case(case, V, kind, dev)
    assert np.isfinite(c64).all()
    rel, abs_ = R._tol(T)
    live = band_live(ranges, tl, ul, S)
    worst = {}
    # from log-probs: the dense gradient
    costs, grad = _run(rnnt_loss_pruned_modified, dev, lp64.astype(np.float32), y, ranges, tl, ul, w)
    c, g = costs.cpu().numpy(), grad.cpu().numpy()
    _check_costs(c, c64, "pruned", worst)
    R._check_grads(g, g64, rel, abs_, "pruned", worst)
    assert np.all(g[~live] == 0)
    # from logits: d(logits)
    costs, grad = _run(rnnt_loss_pruned_modified_from_logits, dev, logits, y, ranges, tl, ul, w)
    _check_costs(costs.cpu().numpy(), c64, "pruned logits", worst)
    R._check_dlogits(grad.cpu().numpy().reshape(-1, V), V, V, g64.reshape(-1, V), np.exp(lp64.reshape(-1, V)), 1.0, rel,
                     abs_, False, live.reshape(-1), "pruned d(logits)", worst)
    R._report("modified pruned %s V=%d %s" % (case, V, kind), worst)


@pytest.mark.parametrize("case", PRUNED, ids=["B%d-T%d-U%d-S%d" % c for c in PRUNED])
def test_pruned_cost_is_at_least_the_full_lattice_cost(hip_device, case):
    """The band's rows cut out of a full-lattice tensor: dropping paths can only raise the cost."""
    from pika_amd.rnnt import rnnt_loss_modified, rnnt_loss_pruned_modified
    dev = hip_device
    B, T, U, S = case
    V = 8
    rng = np.random.default_rng(T)
    tl, ul = _pruned_lengths(B, T, U, S)
    y = _labels(B, U, V, ul, rng)
    lp = rng.standard_normal((B, T, U + 1, V)).astype(np.float64) * 2
    lp = (lp - R._lse(lp.reshape(-1, V)).reshape(B, T, U + 1, 1)).astype(np.float32)
    ranges = M.random_valid_ranges_modified(tl, ul, S, rng, T=T)
    w = np.ones(B, np.float32)
    full, g_full = _run(rnnt_loss_modified, dev, lp, y, None, tl, ul, w)
    c64, g64 = M.loss_ref(lp, y, tl, ul)
    worst = {}
    _check_costs(full.cpu().numpy(), c64, "full", worst)
    R._check_grads(g_full.cpu().numpy(), g64, *R._tol(T), "full", worst)
    band, _ = _run(rnnt_loss_pruned_modified, dev, M.gather(lp, ranges, S, ul), y, ranges, tl, ul, w)
    f = full.cpu().numpy().astype(np.float64)
    assert torch.isfinite(band).all() and np.all(band.cpu().numpy() >= f - 1e-5 * np.abs(f)), (band, full)
    R._report("modified full %s" % (case,), worst)


def test_a_pathless_band_costs_inf_and_leaves_the_neighbours_alone(hip_device):
    """A band of the REGULAR search's kind -- a jump of S - 1 columns in one frame -- holds no path here."""
    from pika_amd.rnnt import rnnt_loss_pruned_modified, rnnt_loss_pruned_modified_from_logits
    dev = hip_device
    case, V = PRUNED[0], 8
    B, T, U, S = case
    logits, y, tl, ul, ranges, w, lp64, c64, g64, _ = _pruned_case(case, V, "random", dev)
    assert tl[0] == T and ul[0] == U
    bad = np.array(ranges)
    bad[0, 1:] = np.maximum(bad[0, 1:], S - 1)               # s_0 = 0, s_1 >= 2: u_1 <= 1 is outside the band
    pb, pl = _band_planes(lp64, y, bad, ul, U + 1)
    assert M.planes_loss_ref(pb, pl, tl, ul)[0][0] == np.inf
    for fn, x in ((rnnt_loss_pruned_modified, lp64.astype(np.float32)), (rnnt_loss_pruned_modified_from_logits, logits)):
        c0, g0 = _run(fn, dev, x, y, ranges, tl, ul, w)
        c1, g1 = _run(fn, dev, x, y, bad, tl, ul, w)
        assert torch.isposinf(c1[0]) and not g1[0].any() and not torch.isnan(g1).any()
        assert torch.equal(c0[1:], c1[1:]) and torch.equal(g0[1:], g1[1:])


@pytest.mark.parametrize("V", [8, 5000])
def test_the_band_that_is_the_lattice_is_the_full_loss_bit_for_bit(hip_device, V):
    from pika_amd.rnnt import (rnnt_loss_modified, rnnt_loss_modified_from_logits, rnnt_loss_pruned_modified,
                               rnnt_loss_pruned_modified_from_logits)
    dev = hip_device
    B, T, U = 4, 9, 6
    rng = np.random.default_rng(V)
    tl, ul = _lengths(B, T, U, infeasible=True)
    y = _labels(B, U, V, ul, rng)
    logits = (rng.standard_normal((B, T, U + 1, V)) * 2).astype(np.float32)
    lp = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    w = (rng.random(B) + 0.5).astype(np.float32)
    zero = np.zeros((B, T), np.int32)
    for full, pruned, x in ((rnnt_loss_modified, rnnt_loss_pruned_modified, lp),
                            (rnnt_loss_modified_from_logits, rnnt_loss_pruned_modified_from_logits, logits)):
        a = _run(full, dev, x, y, None, tl, ul, w, fastemit_lambda=0.125)
        b = _run(pruned, dev, x, y, zero, tl, ul, w, fastemit_lambda=0.125)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.isposinf(a[0]).sum() == 1 and torch.isfinite(a[1]).all()


def test_fastemit(hip_device):
    from pika_amd.rnnt import rnnt_loss_modified
    dev = hip_device
    B, T, U, V, lam = 3, 12, 7, 8, 0.01
    rng = np.random.default_rng(12)
    tl, ul = _lengths(B, T, U)
    y = _labels(B, U, V, ul, rng)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, U + 1, V)) * 2), -1).float().numpy()
    w = (rng.random(B) + 0.5).astype(np.float32)
    c0, g0 = _run(rnnt_loss_modified, dev, lp, y, None, tl, ul, w)
    c1, g1 = _run(rnnt_loss_modified, dev, lp, y, None, tl, ul, w, fastemit_lambda=lam)
    cz, gz = _run(rnnt_loss_modified, dev, lp, y, None, tl, ul, w, fastemit_lambda=0.0)
    assert torch.equal(c0, c1) and torch.equal(c0, cz) and torch.equal(g0, gz)          # costs unchanged
    assert torch.equal(g0[..., 0], g1[..., 0])                                           # blank entries unchanged
    c64, g64 = M.loss_ref(lp, y, tl, ul, fastemit_lambda=lam)
    worst = {}
    _check_costs(c1.cpu().numpy(), c64, "fastemit", worst)
    R._check_grads(g1.cpu().numpy(), g64 * w[:, None, None, None], *R._tol(T), "fastemit", worst)
    # label entries: the one factor 1 + lambda in fp32, so one rounding of the product apart
    lab0, lab1 = g0[..., 1:].double(), g1[..., 1:].double()
    assert lab0.abs().sum() > 0
    scale = float(np.float32(1.0) + np.float32(lam))
    assert bool(((lab1 - lab0 * scale).abs() <= 2.0 ** -22 * lab0.abs()).all())


# ---- the band search ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,U,S", [(4, 7, 5, 2), (3, 70, 64, 5), (2, 300, 299, 7), (3, 1100, 9, 3)])
def test_band_search_equals_the_reference(hip_device, B, T, U, S):
    """Integer-valued occupancies: every summation order gives the same window sums, so the result is the reference's,
    integer for integer.  Few distinct values and whole flat frames: ties.  T = 1100: more than one chunk of the scans."""
    from pika_amd.rnnt import rnnt_prune_ranges_modified
    dev = hip_device
    rng = np.random.default_rng(T + U)
    tl, ul = _lengths(B, T, U, infeasible=True)
    for hi in (1025, 3):
        ob = rng.integers(0, hi, (B, T, U + 1)).astype(np.float32)
        ol = rng.integers(0, hi, (B, T, U + 1)).astype(np.float32)
        ob[:, ::3], ol[:, ::3] = 7.0, 1.0                              # flat frames: every window ties
        got = rnnt_prune_ranges_modified(_d(ob, dev), _d(ol, dev), _d(tl, dev), _d(ul, dev), S).cpu().numpy()
        want = M.prune_ranges_modified_ref(ob, ol, tl, ul, S)
        assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
        for n in range(B):
            if tl[n] - 1 >= max(0, ul[n] + 1 - S):
                assert M.is_valid_modified(got[n], tl[n], ul[n], S)
            else:
                assert got[n, 0] > 0


def test_band_search_on_real_occupancies_is_valid(hip_device):
    from pika_amd.rnnt import (rnnt_loss_from_planes_modified, rnnt_loss_pruned_modified, rnnt_prune_lm,
                               rnnt_prune_ranges_modified, rnnt_simple_planes)
    dev = hip_device
    B, T, U, S, V = 5, 40, 30, 5, 50
    tl = np.array([40, 30, 1, 17, 25], np.int32)
    ul = np.array([30, 30, 0, 3, 25], np.int32)
    rng = np.random.default_rng(2)
    y = _labels(B, U, V, ul, rng)
    g = torch.Generator().manual_seed(0)
    am = (torch.randn(B, T, V, generator=g) * 3).to(dev)
    lm = (torch.randn(B, U + 1, V, generator=g) * 3).to(dev)
    tl_d, ul_d, y_d = _d(tl, dev), _d(ul, dev), _d(y, dev)
    costs, ob, ol = rnnt_loss_from_planes_modified(*rnnt_simple_planes(am, lm, y_d), tl_d, ul_d, return_occupancy=True)
    ranges = rnnt_prune_ranges_modified(ob, ol, tl_d, ul_d, S)
    r = ranges.cpu().numpy()
    assert torch.isfinite(costs).all()
    for n in range(B):
        assert M.is_valid_modified(r[n], tl[n], ul[n], S), (n, r[n], tl[n], ul[n])
        assert (r[n, tl[n]:] == max(0, ul[n] + 1 - S)).all()
    assert rnnt_prune_lm(lm, ranges, S).shape == (B, T, S, V)
    # one symbol per frame: the occupancies of every frame of an utterance sum to one
    occ = (ob + ol).sum(2).cpu().numpy()
    for n in range(B):
        assert np.allclose(occ[n, :tl[n]], 1.0, atol=1e-3) and not occ[n, tl[n]:].any()
    # the band holds a path
    lp = torch.log_softmax(torch.randn(B, T, S, V, generator=g), -1).to(dev)
    assert torch.isfinite(rnnt_loss_pruned_modified(lp, y_d, ranges, tl_d, ul_d)).all()


# ---- the chain ----------------------------------------------------------------------------------------------------------
def _oracle_modified(J, enc, pred, y, tl, ul, layers, ranges, S):
    """test_joint_banded_gpu._oracle with the modified loss: float64 joint on the band's rows, log-softmax, the reference
    DP on the scattered band, and the gradients of the summed costs w.r.t. enc, pred and the joint's parameters."""
    fc1, fcg, fc2 = [[p.detach().double().cpu().requires_grad_(True) for p in (m.weight, m.bias)] for m in layers[:3]]
    e, p = enc.double().requires_grad_(True), pred.double().requires_grad_(True)
    H, U1 = e.shape[-1], p.shape[1]
    e1, eg = e @ fc1[0][:, :H].T + fc1[1], e @ fcg[0][:, :H].T + fcg[1]
    p1, pg = p @ fc1[0][:, H:].T, p @ fcg[0][:, H:].T
    rows = J.JB.band_rows(ranges, U1, S)
    bidx = torch.arange(e.shape[0])[:, None, None].expand(rows.shape)
    h = torch.tanh(e1[:, :, None] + p1[bidx, rows]) * torch.sigmoid(eg[:, :, None] + pg[bidx, rows])
    lp = torch.log_softmax(h @ fc2[0].T + fc2[1], -1)
    tl_n, ul_n, y_n = tl.numpy(), ul.numpy(), y.numpy()
    lp_n = lp.detach().numpy()
    pb, pl = _band_planes(lp_n, y_n, ranges, ul_n, U1)
    c64, ob, ol = M.planes_loss_ref(pb, pl, tl_n, ul_n)
    g = _band_grads(ob, ol, y_n, ranges, ul_n, S, lp_n.shape[-1], np.ones(len(tl_n)))
    lp.backward(torch.from_numpy(g))
    return c64, [e.grad, p.grad] + [t.grad for pair in (fc1, fcg, fc2) for t in pair]


@pytest.mark.parametrize("scales", [(0.0, 0.0), (0.25, 0.0)])
def test_pruned_joint_loss_modified_end_to_end(hip_device, scales):
    """(B,T,U,H,V,S) = (3,20,6,64,16,3), test_joint_banded_gpu's end-to-end shape.  The bound of the regular chain there is
    relative -- within 2x of a yardstick chain's error against its own float64 oracle, same inputs and layers -- so the
    yardstick here is the regular chain (rnnt_pruned_joint_loss_smoothed) in the same mode, measured in this test."""
    import test_joint_banded_gpu as J
    from pika_amd import gemm as G
    from pika_amd import rnnt, rnnt_pruned_joint_loss_modified, rnnt_pruned_joint_loss_smoothed
    from pika_amd.model import ops
    from oracle import rnnt as O
    dev = hip_device
    ll, la = scales
    S, H, V, B, T, U = (J.E2E[k] for k in "SHVBTU")
    assert (B, T, U, H, V, S) == (3, 20, 6, 64, 16, 3)
    enc0, pred0, y, tl, ul = J._e2e_inputs(11)
    layers = J._layers(H, H, V, dev, 2, simple=True)
    sam, slm = layers[3:]
    yd, tld, uld = y.to(dev), tl.to(dev), ul.to(dev)
    err = {}
    for name, chain in (("modified", rnnt_pruned_joint_loss_modified), ("regular", rnnt_pruned_joint_loss_smoothed)):
        enc, pred = enc0.to(dev).requires_grad_(True), pred0.to(dev).requires_grad_(True)
        simple, pruned, ranges = chain(enc, pred, yd, tld, uld, *layers, s_range=S, reduction=None, lm_only_scale=ll,
                                       am_only_scale=la)
        assert ranges.dtype == torch.int32 and ranges.shape == (B, T) and not ranges.requires_grad
        assert simple.shape == pruned.shape == (B,)
        r = ranges.cpu().numpy()
        grads = torch.autograd.grad(pruned.sum(), [enc, pred] + J._params(layers[:3]), retain_graph=True)
        assert all(g is None for g in torch.autograd.grad(pruned.sum(), J._params(layers[3:]), retain_graph=True,
                                                          allow_unused=True))
        assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
                   for g in torch.autograd.grad(simple.sum(), J._params(layers[3:])))
        # the simple loss against the float64 loss of the float64 planes on the same am / lm
        with torch.no_grad():
            am, lm = ops.linear(enc, sam.weight, sam.bias), ops.linear(pred, slm.weight, slm.bias)
            bl, lb = rnnt._smoothed_planes_torch(am.double(), lm.double(), yd, 0, ll, la)
        bl, lb = bl.cpu().numpy(), lb.cpu().numpy()
        if name == "modified":
            for n in range(B):
                assert M.is_valid_modified(r[n], int(tl[n]), int(ul[n]), S)
            want = M.planes_loss_ref(bl, lb, tl.numpy(), ul.numpy())[0]
            c64, g64 = _oracle_modified(J, enc0, pred0, y, tl, ul, layers, r, S)
        else:
            want = O.rnnt_loss(np.stack([bl, np.maximum(lb, M.NEG)], -1).astype(np.float64), np.ones((B, U), np.int32),
                               tl.numpy(), ul.numpy(), want_grads=False)[0]
            c64, g64 = J._oracle(enc0, pred0, y, tl, ul, layers, r, S)
        es = float(np.abs(simple.detach().double().cpu().numpy() - want).max() / np.abs(want).max())
        err[name] = (es, J._chain_error(name, pruned, grads, c64, g64))
    print("RNNTMODIFIED e2e mode %s scales %s: simple loss modified %.3g regular %.3g; pruned chain modified %.3g regular "
          "%.3g" % (G.PRECISION, scales, err["modified"][0], err["regular"][0], err["modified"][1], err["regular"][1]))
    assert err["modified"][0] <= 2 * err["regular"][0], err
    assert err["modified"][1] <= 2 * err["regular"][1], err


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def test_two_runs_are_bit_identical(hip_device):
    from pika_amd.rnnt import rnnt_loss_pruned_modified_from_logits
    dev = hip_device
    case = PRUNED[1]
    logits, y, tl, ul, ranges, w, _, _, _, planes = _pruned_case(case, 8, "random", dev)
    a = _run(rnnt_loss_pruned_modified_from_logits, dev, logits, y, ranges, tl, ul, w)
    b = _run(rnnt_loss_pruned_modified_from_logits, dev, logits, y, ranges, tl, ul, w)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    r1 = _searched_ranges(planes[0], planes[1], tl, ul, case[3], dev)
    r2 = _searched_ranges(planes[0], planes[1], tl, ul, case[3], dev)
    assert np.array_equal(r1, r2)


def test_the_chain_captures_into_one_graph(hip_device):
    """Forward plus backward of rnnt_pruned_joint_loss_modified in one torch.cuda.graph, replayed on new data (hence new
    ranges): losses, ranges and every gradient equal the eager call bit for bit."""
    import test_joint_banded_gpu as J
    from pika_amd import rnnt_pruned_joint_loss_modified
    dev = hip_device
    S, H, V = J.E2E["S"], J.E2E["H"], J.E2E["V"]
    layers = J._layers(H, H, V, dev, 3, simple=True)
    params = J._params(layers)

    def run(stat):
        s, p, r = rnnt_pruned_joint_loss_modified(*stat, *layers, s_range=S, fastemit_lambda=0.25, lm_only_scale=0.25)
        return s, p, r, torch.autograd.grad(0.5 * s + p, stat[:2] + params)

    stat = [t.to(dev) for t in J._e2e_inputs(20)]
    stat[0].requires_grad_(True)
    stat[1].requires_grad_(True)
    run(stat)                                                  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gs, gp, gr, gg = run(stat)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for seed in (21, 22):
        with torch.no_grad():
            for dst, src in zip(stat, J._e2e_inputs(seed)):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        es, ep, er, eg = run(stat)
        assert torch.isfinite(es).all() and torch.isfinite(ep).all()
        assert torch.equal(gs.detach(), es.detach()) and torch.equal(gp.detach(), ep.detach()) and torch.equal(gr, er)
        for a, b in zip(gg, eg):
            assert torch.equal(_bits(a), _bits(b))
        seen.append(er.clone())
    assert not torch.equal(seen[0], seen[1])                   # the replays ran on new ranges
