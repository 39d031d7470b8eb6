"""The float64 reference of the n-best loss (tests/ctc_nbest_loss_common.py) against central finite differences of a
brute-force sum over all C^T frame labellings, and the MWER reference's gradient against finite differences of the risk
(CPU only; no product imports)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_nbest_loss_common as NL  # noqa: E402

T, C = 4, 3
HYPS = [[[], [1], [1, 1], [2, 1], [1, 2, 1], None, [1, 1, 1], [0, 1], [3]]]     # the last four are dead
WEIGHTS = np.array([[0.7, -1.3, 0.4, 2.0, -0.6, np.nan, np.inf, 1e30, -np.inf]])


def brute_objective(lp):
    """sum_k g_k * full_k over the live entries, full_k by enumeration; lp (T,C) float64 numpy."""
    total = 0.0
    for k, seq in enumerate(HYPS[0]):
        if NL.sentinel(T, C, seq, 0, 511) is None:
            total += WEIGHTS[0, k] * -R.brute_force(lp, seq)[0]
    return total


def central(fn, x, eps=1e-5):
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        hi, lo = x.copy(), x.copy()
        hi[i] += eps
        lo[i] -= eps
        g[i] = (fn(hi) - fn(lo)) / (2 * eps)
    return g


def test_reference_against_brute_force_finite_differences():
    logits = torch.randn(T, 1, C, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    full, dx, dlp = NL.nbest_loss(logits, HYPS, [T], WEIGHTS)
    lp = torch.log_softmax(logits, -1)[:, 0].numpy()
    for k, seq in enumerate(HYPS[0]):
        dead = NL.sentinel(T, C, seq, 0, 511)
        if dead is None:
            assert abs(full[0, k] + R.brute_force(lp, seq)[0]) < 1e-12, k
        else:
            assert full[0, k] == -np.inf, k
    assert np.isnan(NL.nbest_loss(logits, HYPS, [T], WEIGHTS, max_len=2)[0][0, 4])      # longer than max_len
    assert np.isfinite(dx.numpy()).all() and np.isfinite(dlp.numpy()).all()             # the dead weights stayed out
    # d/d logits: through the log-softmax; the true d/d log_probs: the log-probs as free variables
    fd_x = central(lambda z: brute_objective(torch.log_softmax(torch.from_numpy(z), -1).numpy()), logits[:, 0].numpy())
    fd_lp = central(brute_objective, lp)
    assert np.abs(fd_x - dx[:, 0].numpy()).max() < 1e-8
    assert np.abs(fd_lp - dlp[:, 0].numpy()).max() < 1e-8
    assert np.abs(dlp.numpy()).max() > 0.1


def test_reference_zeroes_the_frames_beyond_the_length():
    logits = torch.randn(6, 2, C, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    hyps = [[[1], [2, 2]], [[1, 2], [2]]]
    w = np.array([[1.0, -2.0], [0.5, 0.25]])
    full, dx, dlp = NL.nbest_loss(logits, hyps, [6, 4], w)
    assert (dx[4:, 1] == 0).all() and (dlp[4:, 1] == 0).all() and dx[:4, 1].abs().max() > 0
    lp = torch.log_softmax(logits, -1).numpy()
    assert abs(full[1, 0] + R.dp_cost(lp[:4, 1], [1, 2])) < 1e-12
    # a duplicate pair: the gradient of both weights times one
    _, one, _ = NL.nbest_loss(logits, [[[1]], [[2]]], [6, 4], np.array([[1.0], [1.0]]))
    _, two, _ = NL.nbest_loss(logits, [[[1], [1]], [[2], [2]]], [6, 4], np.array([[0.75, -2.0], [3.0, 0.5]]))
    assert np.allclose(two[:, 0].numpy(), -1.25 * one[:, 0].numpy(), atol=1e-14)
    assert np.allclose(two[:, 1].numpy(), 3.5 * one[:, 1].numpy(), atol=1e-14)


def test_mwer_reference_against_finite_differences():
    full = np.array([[-3.1, -2.5, -np.inf, -4.0, np.nan], [-np.inf, -np.inf, np.nan, -np.inf, -np.inf],
                     [-1.0, -np.inf, -np.inf, -np.inf, -np.inf]])
    errors = np.array([[1.0, 3.0, 9.0, 0.0, 7.0], [1.0, 2.0, 3.0, 4.0, 5.0], [2.0, 0.0, 0.0, 0.0, 0.0]])
    live = np.isfinite(full)
    value, g = NL.mwer(full, errors, "none")
    p = np.exp(full[0, [0, 1, 3]])
    p /= p.sum()
    assert abs(value[0] - (p * (np.array([1.0, 3.0, 0.0]) - 4.0 / 3.0)).sum()) < 1e-14
    assert value[1] == 0.0 and value[2] == 0.0 and (g[~live] == 0).all() and (g[1] == 0).all()
    for reduction in ("none", "sum", "mean"):
        value, g = NL.mwer(full, errors, reduction)
        assert value.shape == ((3,) if reduction == "none" else ())

        def risk(z):
            return float(NL.mwer(np.where(live, z, full), errors, reduction)[0].sum())
        fd = central(risk, np.where(live, full, 0.0)) * live
        assert np.abs(fd - g).max() < 1e-8, reduction
    assert np.abs(g).max() > 0.01
