"""The float64 references of the modified RNN-T topology (tests/rnnt_modified_common.py) against brute force, autograd and
each other; no GPU."""
import numpy as np
import pytest

import rnnt_modified_common as mc
from rnnt_pruned_common import prune_ranges_ref

TINY = [(1, 0), (1, 1), (3, 3), (4, 2), (5, 3)]


def _planes(rng, T, U):
    return rng.standard_normal((T, U + 1)) * 2 - 1.0, rng.standard_normal((T, U + 1)) * 2 - 1.0


@pytest.mark.parametrize("T,U", TINY)
def test_dp_equals_brute_force_on_the_full_lattice(T, U):
    rng = np.random.default_rng(100 * T + U)
    pb, pl = _planes(rng, T, U)
    cost, a, be, ob, ol = mc.modified_dp(pb, pl, T, U)
    assert np.isfinite(cost)
    assert abs(cost - mc.brute_force_cost(pb, pl, T, U)) <= 1e-12 * max(1.0, abs(cost))
    assert abs(-be[0, 0] - cost) <= 1e-12 * max(1.0, abs(cost))          # the beta side agrees
    # one symbol per frame: the occupancies of every frame sum to one, and U labels are emitted in all
    assert np.allclose((ob + ol).sum(1), 1.0, atol=1e-12)
    assert np.isclose(ol.sum(), U, atol=1e-10)
    assert (ol[:, U] == 0).all()


# every (T, U) of TINY with every S in {2, 3} for which a band exists: S <= U + 1 and T - 1 >= max(0, U + 1 - S)
BANDS = [(T, U, S) for T, U in TINY for S in (2, 3) if S <= U + 1 and T - 1 >= max(0, U + 1 - S)]


@pytest.mark.parametrize("T,U,S", BANDS)
def test_dp_equals_brute_force_on_random_valid_bands(T, U, S):
    assert len(BANDS) == 7
    rng = np.random.default_rng(1000 * S + 10 * T + U)
    for _ in range(4):
        pb, pl = _planes(rng, T, U)
        s = mc.random_valid_ranges_modified([T], [U], S, rng)[0]
        bb, bl = mc.band_planes(pb, pl, s, S)
        cost = mc.modified_dp(bb, bl, T, U)[0]
        want = mc.brute_force_cost(pb, pl, T, U, s, S)
        assert np.isfinite(want) and abs(cost - want) <= 1e-12 * max(1.0, abs(want))
        assert cost >= mc.modified_dp(pb, pl, T, U)[0] - 1e-12           # a band only removes paths


def test_gradient_equals_float64_autograd_of_the_torch_spelling():
    import torch
    rng = np.random.default_rng(7)
    B, T, U = 3, 6, 4
    tl, ul = np.array([6, 4, 5]), np.array([4, 4, 0])
    pb = rng.standard_normal((B, T, U + 1)) - 1.0
    pl = rng.standard_normal((B, T, U + 1)) - 1.0
    costs, ob, ol = mc.planes_loss_ref(pb, pl, tl, ul)
    tb = torch.tensor(pb, dtype=torch.float64, requires_grad=True)
    tL = torch.tensor(pl, dtype=torch.float64, requires_grad=True)
    tc = mc.torch_costs(tb, tL, tl, ul)
    assert np.allclose(tc.detach().numpy(), costs, rtol=1e-12)
    tc.sum().backward()
    assert np.allclose(tb.grad.numpy(), -ob, atol=1e-12)
    assert np.allclose(tL.grad.numpy(), -ol, atol=1e-12)
    # FastEmit on the (B,T,U1,V) form: costs unchanged, label entries times 1 + lambda
    V = 5
    lp = rng.standard_normal((B, T, U + 1, V)) - 2.0
    y = rng.integers(1, V, (B, U)).astype(np.int32)
    c0, g0 = mc.loss_ref(lp, y, tl, ul)
    c1, g1 = mc.loss_ref(lp, y, tl, ul, fastemit_lambda=0.25)
    assert np.array_equal(c0, c1)
    assert np.array_equal(g0[..., 0], g1[..., 0])
    lab = g0.copy()
    lab[..., 0] = 0
    assert np.allclose(g1 - g0, 0.25 * lab, atol=1e-15) and np.abs(lab).sum() > 0


def test_an_utterance_with_more_labels_than_frames_costs_inf():
    rng = np.random.default_rng(3)
    for T in (1, 3):
        pb, pl = _planes(rng, T, T + 1)
        cost, _, _, ob, ol = mc.modified_dp(pb, pl, T, T + 1)
        assert cost == np.inf and not ob.any() and not ol.any()
        assert mc.brute_force_cost(pb, pl, T, T + 1) == np.inf
        assert np.isfinite(mc.modified_dp(pb, pl, T, T)[0])               # U_n = T_n: every frame emits a label


def test_a_regular_band_with_a_jump_is_pathless_where_the_modified_band_is_not():
    T, U, S = 6, 4, 3
    occ = np.zeros((1, T, U + 1))
    occ[0, 0, 0] = 1.0
    occ[0, 1:, 2:] = 1.0                                                 # from frame 1 on the mass sits in columns 2..4
    zero = np.zeros_like(occ)
    reg = prune_ranges_ref(occ, zero, [T], [U], S)[0]
    mod = mc.prune_ranges_modified_ref(occ, zero, [T], [U], S)[0]
    assert list(reg) == [0, 2, 2, 2, 2, 2] and list(mod) == [0, 1, 2, 2, 2, 2]
    assert not mc.is_valid_modified(reg, T, U, S) and mc.is_valid_modified(mod, T, U, S)
    rng = np.random.default_rng(5)
    pb, pl = _planes(rng, T, U)
    assert mc.modified_dp(*mc.band_planes(pb, pl, reg, S), T, U)[0] == np.inf
    assert mc.brute_force_cost(pb, pl, T, U, reg, S) == np.inf
    cost = mc.modified_dp(*mc.band_planes(pb, pl, mod, S), T, U)[0]
    assert np.isfinite(cost) and abs(cost - mc.brute_force_cost(pb, pl, T, U, mod, S)) <= 1e-12 * abs(cost)


def test_the_band_search_reference_returns_valid_bands_with_a_path():
    rng = np.random.default_rng(11)
    for B, T, U, S in [(4, 7, 5, 2), (3, 12, 9, 3), (3, 9, 8, 1), (2, 5, 3, 4)]:
        tl = rng.integers(1, T + 1, B)
        tl[0] = T
        ul = np.minimum(rng.integers(0, U + 1, B), tl)
        ul[0] = min(U, T)
        bo, lo = rng.random((B, T, U + 1)), rng.random((B, T, U + 1))
        r = mc.prune_ranges_modified_ref(bo, lo, tl, ul, S)
        for n in range(B):
            Tn, Un = int(tl[n]), int(ul[n])
            smax = max(0, Un + 1 - S)
            assert (r[n, Tn:] == smax).all()
            if Tn - 1 >= smax:
                assert mc.is_valid_modified(r[n], Tn, Un, S)
                pb, pl = _planes(rng, T, U)
                assert np.isfinite(mc.modified_dp(*mc.band_planes(pb, pl, r[n], S), Tn, Un)[0])
            else:
                assert r[n, 0] > 0
