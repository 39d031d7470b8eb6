"""The references of tests/rnnt_pruned_common.py, pinned without a GPU: the brute-force banded cost equals the fp64
oracle on the scattered tensor (the definition of the pruned loss), and the plain-Python band search returns bands that
connect the lattice's corners whenever one of that width exists."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_pruned_common as P  # noqa: E402
from helpers import log_softmax  # noqa: E402
from oracle import rnnt as O  # noqa: E402


@pytest.mark.parametrize("T,U,S", [(4, 3, 2), (3, 4, 3), (5, 2, 3), (1, 0, 1)])
def test_brute_force_banded_cost_equals_the_oracle_on_the_scattered_tensor(T, U, S):
    rng = np.random.default_rng(100 * T + 10 * U + S)
    V = 5
    tl, ul = np.array([T], np.int32), np.array([U], np.int32)
    for _ in range(6):
        band = log_softmax(rng.standard_normal((1, T, S, V))).astype(np.float32)   # the oracle reads float32
        y = rng.integers(1, V, (1, U)).astype(np.int32)
        s = P.random_valid_ranges(tl, ul, S, rng)
        want = P.brute_force_banded_cost(band[0].astype(np.float64), s[0], y[0])
        got, _ = O.rnnt_loss(P.scatter(band, s, U + 1, ul), y, tl, ul, want_grads=False)
        assert np.isfinite(want) and abs(got[0] - want) <= 1e-9, (got, want, s)
        # gather is scatter's inverse on the band
        assert np.array_equal(P.gather(P.scatter(band, s, U + 1, ul), s, S, ul), band)


def test_brute_force_drops_the_paths_outside_the_band():
    """A band narrower than the lattice costs more than the lattice; the band that is the lattice costs the same."""
    rng = np.random.default_rng(3)
    T, U, V = 4, 3, 5
    lp = log_softmax(rng.standard_normal((T, U + 1, V)))
    y = rng.integers(1, V, U)
    full = O.brute_force_cost(lp, y)
    assert P.brute_force_banded_cost(lp, np.zeros(T, int), y) == pytest.approx(full, abs=1e-12)
    s = np.array([0, 1, 1, 2])
    band = np.stack([lp[t, s[t]:s[t] + 2] for t in range(T)])
    assert P.brute_force_banded_cost(band, s, y) > full + 1e-6


def test_band_search_reference_returns_valid_ranges():
    rng = np.random.default_rng(7)
    for i in range(200):
        B, T, U = 2, int(rng.integers(1, 12)), int(rng.integers(0, 10))
        S = int(rng.integers(1, U + 2))
        tl = rng.integers(1, T + 1, B).astype(np.int32)
        ul = P.feasible_label_lengths(tl, rng.integers(0, U + 1, B), S)
        occ = [rng.random((B, T, U + 1)).astype(np.float32) ** 4 for _ in range(2)]
        s = P.prune_ranges_ref(occ[0], occ[1], tl, ul, S)
        for n in range(B):
            smax = max(0, ul[n] + 1 - S)
            assert (tl[n] - 1) * (S - 1) >= smax                      # a band of this width exists ...
            assert P.is_valid(s[n], tl[n], ul[n], S), (i, n, s[n], tl[n], ul[n], S)    # ... and this is one
            assert (s[n, tl[n]:] == smax).all()


def test_band_search_reference_follows_the_occupancy():
    """All the mass on the cells (t, min(2t, 5)): the band of width 3 is the lowest one that holds them."""
    T = U1 = 6
    occ = np.zeros((1, T, U1), np.float32)
    occ[0, np.arange(T), np.minimum(2 * np.arange(T), U1 - 1)] = 1.0
    s = P.prune_ranges_ref(occ, np.zeros_like(occ), [T], [U1 - 1], 3)
    assert s[0].tolist() == [0, 0, 2, 3, 3, 3]
    # ties go to the smallest start: a flat plane keeps the band low for as long as it can
    flat = np.ones((1, T, U1), np.float32)
    s = P.prune_ranges_ref(flat, flat, [T], [U1 - 1], 3)
    assert s[0].tolist() == [0, 0, 0, 0, 1, 3]


def test_band_search_reference_reports_a_lattice_that_is_too_short():
    """T_n = 3 frames of width 2 reach column 3 at most: no band connects U_n = 6, and s_0 > 0 says so."""
    rng = np.random.default_rng(11)
    T, U, S = 3, 6, 2
    occ = rng.random((1, T, U + 1)).astype(np.float32)
    assert (T - 1) * (S - 1) < U + 1 - S
    s = P.prune_ranges_ref(occ, occ, [T], [U], S)
    assert s[0, 0] > 0 and not P.is_valid(s[0], T, U, S)
    assert s[0, T - 1] == U + 1 - S
