"""Pruned (banded) RNN-T on the GPU against the fp64 oracle on the scattered tensor (tests/rnnt_pruned_common.py).

The oracle of a banded call is oracle.rnnt.rnnt_loss on the (B,T,U+1,V) tensor that holds the band's rows at their cells
and -1e30 elsewhere, with its gradient gathered back into the band.  Tolerances are the project's existing ones for
these kernels: costs 1e-5 relative, gradient entries test_rnnt_routes_gpu._tol(T + U), d(logits) the bound of
test_rnnt_routes_gpu._check_dlogits.

CASES: lengths are ragged from helpers.make_case (one full utterance, one with T_n = 1 and U_n = 0, so some utterance
always has U_n + 1 < S).  (4,8,64,5,20,19) and (3,6,299,7,12,0) have too few frames for a band of their width to reach
their last label column ((T-1)(S-1) < U+1-S), so no valid range exists at U_n = U: there -- and for any short ragged
utterance -- U_n is clipped to what the band reaches (feasible_label_lengths); the lattice planes and the workspace are
still those of U+1 = 65 / 300.  (4,20,64,5,20,19) and (3,52,299,7,12,0) are the same widths with enough frames that a
band does reach column U, live cells on both sides of the wave edge included."""
import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import make_case
import rnnt_pruned_common as P
import test_rnnt_routes_gpu as R

pytestmark = pytest.mark.gpu

CASES = [(5, 20, 12, 4, 30, 0), (4, 8, 64, 5, 20, 19), (3, 6, 299, 7, 12, 0), (3, 9, 5, 2, 8, 0), (4, 7, 6, 5, 16, 0),
         (4, 20, 64, 5, 20, 19), (3, 52, 299, 7, 12, 0)]
_IDS = ["B%d-T%d-U%d-S%d-V%d-b%d" % c for c in CASES]
_cache = {}


def _d(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # (a copy: the cached references are read-only)


def _full_case(case):
    """The full-lattice batch of a case, its fp64 costs, and a weight per utterance (computed once)."""
    if case not in _cache:
        B, T, U, S, V, blank = case
        lp, y, tl, ul = make_case(B, T, U, V, seed=B * 1000 + T * 10 + S, ragged=True, blank=blank)
        ul = P.feasible_label_lengths(tl, ul, S)
        assert (ul + 1 < S).any()
        c_full, _ = O.rnnt_loss(lp, y, tl, ul, blank=blank, want_grads=False)
        w = (np.random.default_rng(B + T).random(B) + 0.5).astype(np.float32)
        for a in (lp, y, tl, ul, c_full, w):
            a.setflags(write=False)
        _cache[case] = (lp, y, tl, ul, c_full, w)
    return _cache[case]


def _searched_ranges(case, dev):
    """Band starts from the band search on the occupancies of the planes loss over the case's own two planes."""
    from pika_amd.rnnt import rnnt_loss_from_planes, rnnt_prune_ranges
    B, T, U, S, V, blank = case
    lp, y, tl, ul, _, _ = _full_case(case)
    yy = np.minimum(y, V - 1).astype(np.int64)
    label = np.take_along_axis(lp[:, :, :U], yy[:, None, :, None].repeat(T, 1), 3)[..., 0]
    label = np.concatenate([label, np.full((B, T, 1), P.NEG, np.float32)], 2)
    tl_d, ul_d = _d(tl, dev), _d(ul, dev)
    _, ob, ol = rnnt_loss_from_planes(_d(lp[..., blank], dev), _d(label, dev), tl_d, ul_d, return_occupancy=True)
    return rnnt_prune_ranges(ob, ol, tl_d, ul_d, S).cpu().numpy()


def _banded_ref(case, kind, dev):
    """(band, ranges, fp64 costs, fp64 band gradient scaled by w) of a case under `kind` ranges (computed once)."""
    key = (case, kind)
    if key not in _cache:
        B, T, U, S, V, blank = case
        lp, y, tl, ul, _, w = _full_case(case)
        if kind == "random":
            ranges = P.random_valid_ranges(tl, ul, S, np.random.default_rng(T + U), T=T)
        else:
            ranges = _searched_ranges(case, dev)
            for n in range(B):
                assert P.is_valid(ranges[n], tl[n], ul[n], S), (n, ranges[n], tl[n], ul[n])
        band = P.gather(lp, ranges, S, ul)
        c64, g64 = O.rnnt_loss(P.scatter(band, ranges, U + 1, ul), y, tl, ul, blank=blank)
        g = P.gather(g64, ranges, S, ul) * w[:, None, None, None]
        for a in (band, ranges, c64, g):
            a.setflags(write=False)
        _cache[key] = (band, ranges, c64, g)
    return _cache[key]


def _run_pruned(dev, band, y, ranges, tl, ul, w, blank, **kw):
    from pika_amd.rnnt import rnnt_loss_pruned
    x = _d(band, dev).requires_grad_(True)
    costs = rnnt_loss_pruned(x, _d(y, dev), _d(ranges, dev), _d(tl, dev), _d(ul, dev), blank=blank, **kw)
    costs.backward(_d(w, dev))
    torch.cuda.synchronize()
    return costs.detach(), x.grad


@pytest.mark.parametrize("kind", ["random", "searched"])
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_pruned_loss_matches_fp64_oracle(hip_device, case, kind):
    B, T, U, S, V, blank = case
    lp, y, tl, ul, c_full, w = _full_case(case)
    band, ranges, c64, g64 = _banded_ref(case, kind, hip_device)
    costs, grad = _run_pruned(hip_device, band, y, ranges, tl, ul, w, blank)
    c, g = costs.cpu().numpy(), grad.cpu().numpy()
    worst = {}
    R._check_costs(c, c64, "pruned", worst)
    rel, abs_ = R._tol(T + U)
    R._check_grads(g, g64, rel, abs_, "pruned", worst)
    assert np.all(g[~P.band_live(ranges, tl, ul, S)] == 0)          # band rows outside the lattice: exactly zero
    # dropping paths can only raise the cost
    assert np.all(c.astype(np.float64) >= c_full - 1e-5 * np.abs(c_full)), (c, c_full)
    R._report("pruned %s %s" % (_IDS[CASES.index(case)], kind), worst)


def test_fastemit(hip_device):
    case = CASES[0]
    B, T, U, S, V, blank = case
    lp, y, tl, ul, _, w = _full_case(case)
    band, ranges, c64, g64 = _banded_ref(case, "random", hip_device)
    lam = 0.5
    want = np.array(g64)
    s = P.clamp_ranges(ranges, ul, S)
    for b in range(B):
        for t in range(tl[b]):
            for j in range(S):
                u = s[b, t] + j
                if u < ul[b]:
                    want[b, t, j, y[b, u]] *= 1.0 + lam
    costs, grad = _run_pruned(hip_device, band, y, ranges, tl, ul, w, blank, fastemit_lambda=lam)
    worst = {}
    R._check_costs(costs.cpu().numpy(), c64, "fastemit", worst)
    rel, abs_ = R._tol(T + U)
    R._check_grads(grad.cpu().numpy(), want, rel, abs_, "fastemit", worst)
    c0, g0 = _run_pruned(hip_device, band, y, ranges, tl, ul, w, blank)
    cz, gz = _run_pruned(hip_device, band, y, ranges, tl, ul, w, blank, fastemit_lambda=0.0)
    assert torch.equal(c0, cz) and torch.equal(g0, gz)
    assert not torch.equal(g0, grad)


def test_the_band_that_is_the_lattice_is_rnnt_loss(hip_device):
    from pika_amd.rnnt import rnnt_loss
    dev = hip_device
    for B, T, U, V, blank in ((5, 20, 12, 30, 0), (3, 9, 70, 12, 3)):
        lp, y, tl, ul = make_case(B, T, U, V, seed=5, ragged=True, blank=blank)
        w = (np.random.default_rng(1).random(B) + 0.5).astype(np.float32)
        costs, grad = _run_pruned(dev, lp, y, np.zeros((B, T), np.int32), tl, ul, w, blank)
        x = _d(lp, dev).requires_grad_(True)
        ref = rnnt_loss(x, _d(y, dev), _d(tl, dev), _d(ul, dev), blank=blank)
        ref.backward(_d(w, dev))
        assert torch.equal(costs, ref.detach()) and torch.equal(grad, x.grad)


@pytest.mark.parametrize("V", [8, 5000])
def test_the_band_that_is_the_lattice_is_rnnt_loss_from_logits(hip_device, V):
    from pika_amd.rnnt import rnnt_loss_from_logits, rnnt_loss_pruned_from_logits
    dev = hip_device
    B, T, U = 4, 6, 5
    _, y, tl, ul = make_case(B, T, U, V, seed=9, ragged=True)
    rng = np.random.default_rng(V)
    logits = (rng.standard_normal((B, T, U + 1, V)) * 2).astype(np.float32)
    w = _d((rng.random(B) + 0.5).astype(np.float32), dev)
    y_d, tl_d, ul_d = _d(y, dev), _d(tl, dev), _d(ul, dev)
    out = []
    for fn, extra in ((rnnt_loss_pruned_from_logits, (torch.zeros((B, T), dtype=torch.int32, device=dev),)),
                      (rnnt_loss_from_logits, ())):
        x = _d(logits, dev).requires_grad_(True)
        costs = fn(x, y_d, *extra, tl_d, ul_d)
        costs.backward(w)
        out.append((costs.detach(), x.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_pruned_from_logits_matches_fp64(hip_device):
    from pika_amd.rnnt import rnnt_loss_pruned_from_logits
    dev = hip_device
    B, T, U, S, V = 4, 6, 5, 3, 5000
    _, y, tl, ul = make_case(B, T, U, V, seed=4, ragged=True)
    ul = P.feasible_label_lengths(tl, ul, S)
    rng = np.random.default_rng(17)
    ranges = P.random_valid_ranges(tl, ul, S, rng, T=T)
    logits = (rng.standard_normal((B, T, S, V)) * 2).astype(np.float32)
    w = (rng.random(B) + 0.5).astype(np.float32)
    x64 = logits.reshape(-1, V).astype(np.float64)
    lse = R._lse(x64)
    band_lp = (x64 - lse).astype(np.float32).reshape(B, T, S, V)
    c64, g64 = O.rnnt_loss(P.scatter(band_lp, ranges, U + 1, ul), y, tl, ul)
    g = (P.gather(g64, ranges, S, ul) * w[:, None, None, None]).reshape(-1, V)
    x = _d(logits, dev).requires_grad_(True)
    costs = rnnt_loss_pruned_from_logits(x, _d(y, dev), _d(ranges, dev), _d(tl, dev), _d(ul, dev))
    costs.backward(_d(w, dev))
    torch.cuda.synchronize()
    worst = {}
    R._check_costs(costs.detach().cpu().numpy(), c64, "pruned logits", worst)
    rel, abs_ = R._tol(T + U)
    live = P.band_live(ranges, tl, ul, S).reshape(-1)
    R._check_dlogits(x.grad.cpu().numpy().reshape(-1, V), V, V, g, np.exp(x64 - lse), 1.0, rel, abs_, False, live,
                     "pruned d(logits)", worst)
    R._report("pruned logits", worst)


@pytest.mark.parametrize("B,T,U", [(4, 9, 12), (3, 7, 64), (3, 6, 299)], ids=["U1=13", "U1=65", "U1=300"])
def test_planes_loss_matches_fp64(hip_device, B, T, U):
    """The oracle on a V = 2 tensor whose columns are the two planes (unnormalised on purpose), every label 1."""
    from pika_amd.rnnt import rnnt_loss_from_planes
    dev = hip_device
    rng = np.random.default_rng(U)
    _, _, tl, ul = make_case(B, T, U, 2, seed=U, ragged=True)
    planes = np.log(rng.uniform(0.05, 1.5, (B, T, U + 1, 2))).astype(np.float32)
    w = (rng.random(B) + 0.5).astype(np.float32)
    c64, g64 = O.rnnt_loss(planes, np.ones((B, U), np.int32), tl, ul, blank=0)
    pb = _d(planes[..., 0], dev).requires_grad_(True)
    pl = _d(planes[..., 1], dev).requires_grad_(True)
    costs, ob, ol = rnnt_loss_from_planes(pb, pl, _d(tl, dev), _d(ul, dev), return_occupancy=True)
    assert not ob.requires_grad and not ol.requires_grad
    costs.backward(_d(w, dev))
    torch.cuda.synchronize()
    worst = {}
    R._check_costs(costs.detach().cpu().numpy(), c64, "planes", worst)
    rel, abs_ = R._tol(T + U)
    R._check_grads(pb.grad.cpu().numpy(), g64[..., 0] * w[:, None, None], rel, abs_, "blank plane", worst)
    R._check_grads(pl.grad.cpu().numpy(), g64[..., 1] * w[:, None, None], rel, abs_, "label plane", worst)
    R._check_grads(ob.cpu().numpy(), -g64[..., 0], rel, abs_, "blank occupancy", worst)
    R._check_grads(ol.cpu().numpy(), -g64[..., 1], rel, abs_, "label occupancy", worst)
    only = rnnt_loss_from_planes(pb, pl, _d(tl, dev), _d(ul, dev), reduction="sum")
    assert torch.equal(only, costs.detach().sum())
    R._report("planes U1=%d" % (U + 1), worst)


@pytest.mark.parametrize("B,T,U,S", [(4, 7, 5, 2), (3, 33, 64, 5), (2, 130, 299, 7), (3, 1100, 9, 3)])
def test_band_search_equals_the_reference(hip_device, B, T, U, S):
    """Integer-valued occupancies in [0, 1024]: every summation order gives the same window sums, so the result is the
    reference's, integer for integer.  Few distinct values and whole flat frames: ties.  T = 1100: more than one chunk
    of the scans."""
    from pika_amd.rnnt import rnnt_prune_ranges
    dev = hip_device
    rng = np.random.default_rng(T + U)
    _, _, tl, ul = make_case(B, T, U, 2, seed=T, ragged=True)
    for hi in (1025, 3):
        ob = rng.integers(0, hi, (B, T, U + 1)).astype(np.float32)
        ol = rng.integers(0, hi, (B, T, U + 1)).astype(np.float32)
        ob[:, ::3], ol[:, ::3] = 7.0, 1.0                              # flat frames: every window ties
        got = rnnt_prune_ranges(_d(ob, dev), _d(ol, dev), _d(tl, dev), _d(ul, dev), S).cpu().numpy()
        want = P.prune_ranges_ref(ob, ol, tl, ul, S)
        assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_band_search_on_real_occupancies_is_valid(hip_device):
    from pika_amd.rnnt import rnnt_loss_from_planes, rnnt_prune_lm, rnnt_prune_ranges, rnnt_simple_planes
    dev = hip_device
    B, T, U, S, V = 5, 40, 30, 5, 50
    _, y, tl, ul = make_case(B, T, U, V, seed=2, ragged=True)
    ul = P.feasible_label_lengths(tl, ul, S)
    g = torch.Generator().manual_seed(0)
    am = (torch.randn(B, T, V, generator=g) * 3).to(dev)
    lm = (torch.randn(B, U + 1, V, generator=g) * 3).to(dev)
    tl_d, ul_d = _d(tl, dev), _d(ul, dev)
    costs, ob, ol = rnnt_loss_from_planes(*rnnt_simple_planes(am, lm, _d(y, dev)), tl_d, ul_d, return_occupancy=True)
    ranges = rnnt_prune_ranges(ob, ol, tl_d, ul_d, S)
    r = ranges.cpu().numpy()
    assert torch.isfinite(costs).all()
    for n in range(B):
        assert P.is_valid(r[n], tl[n], ul[n], S), (n, r[n], tl[n], ul[n])
        assert (r[n, tl[n]:] == max(0, ul[n] + 1 - S)).all()
    assert rnnt_prune_lm(lm, ranges, S).shape == (B, T, S, V)


def test_two_runs_are_bit_identical(hip_device):
    case = CASES[5]
    B, T, U, S, V, blank = case
    lp, y, tl, ul, _, w = _full_case(case)
    band, ranges, _, _ = _banded_ref(case, "random", hip_device)
    a = _run_pruned(hip_device, band, y, ranges, tl, ul, w, blank)
    b = _run_pruned(hip_device, band, y, ranges, tl, ul, w, blank)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    r1, r2 = _searched_ranges(case, hip_device), _searched_ranges(case, hip_device)
    assert np.array_equal(r1, r2)


def test_forward_and_backward_capture_into_one_graph(hip_device):
    from pika_amd.rnnt import rnnt_loss_pruned_from_logits
    dev = hip_device
    B, T, U, S, V = 4, 12, 9, 3, 16

    def draw(seed):
        _, y, tl, ul = make_case(B, T, U, V, seed=seed, ragged=True)
        ul = P.feasible_label_lengths(tl, ul, S)
        r = P.random_valid_ranges(tl, ul, S, np.random.default_rng(seed), T=T)
        x = (np.random.default_rng(seed + 50).standard_normal((B, T, S, V)) * 2).astype(np.float32)
        return x, y, r, tl, ul

    def eager(stat):
        x = stat[0].detach().clone().requires_grad_(True)
        c = rnnt_loss_pruned_from_logits(x, *stat[1:], fastemit_lambda=0.25)
        (g,) = torch.autograd.grad(c.sum(), x)
        return c.detach(), g

    stat = [_d(a, dev) for a in draw(0)]
    stat[0].requires_grad_(True)
    eager(stat)                                                # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gc = rnnt_loss_pruned_from_logits(*stat, fastemit_lambda=0.25)
            (gg,) = torch.autograd.grad(gc.sum(), stat[0])
    torch.cuda.current_stream().wait_stream(side)
    for seed in (1, 2):
        with torch.no_grad():
            for dst, src in zip(stat, draw(seed)):
                dst.copy_(torch.from_numpy(src))
        graph.replay()
        torch.cuda.synchronize()
        ec, eg = eager(stat)
        assert torch.equal(gc.detach(), ec) and torch.equal(gg, eg)


def test_an_invalid_range_does_not_disturb_the_other_utterances(hip_device):
    case = CASES[0]
    B, T, U, S, V, blank = case
    lp, y, tl, ul, _, w = _full_case(case)
    band, ranges, _, _ = _banded_ref(case, "random", hip_device)
    bad = np.array(ranges)
    assert tl[0] == T and ul[0] == U
    bad[0, 0] = 3                                              # s_0 = 3: cell (0, 0) of utterance 0 is dead
    bad[0, 1] = -5
    bad[0, 2] = 1 << 30
    c0, g0 = _run_pruned(hip_device, band, y, ranges, tl, ul, w, blank)
    c1, g1 = _run_pruned(hip_device, band, y, bad, tl, ul, w, blank)
    assert torch.equal(c0[1:], c1[1:]) and torch.equal(g0[1:], g1[1:])
    assert not torch.isnan(g1).any()


def test_alignment_on_a_pruned_workspace_stays_in_the_band(hip_device):
    from pika_amd import _lib
    from pika_amd.rnnt import rnnt_loss_pruned
    dev = hip_device
    L = _lib.lib()
    for case in (CASES[0], CASES[5]):
        B, T, U, S, V, blank = case
        lp, y, tl, ul, _, _ = _full_case(case)
        band, ranges, c64, _ = _banded_ref(case, "random", dev)
        tl_d, ul_d = _d(tl, dev), _d(ul, dev)
        x = _d(band, dev).requires_grad_(True)
        costs = rnnt_loss_pruned(x, _d(y, dev), _d(ranges, dev), tl_d, ul_d, blank=blank)
        ws = costs.grad_fn.saved_tensors[4]
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        frames = torch.empty((B, U), dtype=torch.int32, device=dev)
        scratch = torch.empty(L.pika_rnnt_align_scratch_bytes(B, T, U + 1), dtype=torch.uint8, device=dev)
        _lib.check(L.pika_rnnt_align(ws.data_ptr(), tl_d.data_ptr(), ul_d.data_ptr(), None, B, T, U + 1, scores.data_ptr(),
                                     frames.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "pika_rnnt_align")
        torch.cuda.synchronize()
        f, sc = frames.cpu().numpy(), scores.cpu().numpy()
        s = P.clamp_ranges(ranges, ul, S)
        for n in range(B):
            assert sc[n] <= -c64[n] + 1e-4 * abs(c64[n]) and sc[n] > -1e29
            for u in range(ul[n]):
                t = f[n, u]
                assert 0 <= t < tl[n] and s[n, t] <= u < s[n, t] + S, (n, u, t, s[n])
            assert (f[n, ul[n]:] == -1).all()
