"""CPU checks of the float64 reference the long-form loss is held to (tests/ctc_common.py: torch_reference): beyond 511
labels against the plain float64 alpha recurrence (dp_cost), and its gradient at a small case against finite differences."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402


def _seq(U, C, blank, seed):
    rng = np.random.RandomState(seed)
    classes = [c for c in range(C) if c != blank]
    return [int(classes[i]) for i in rng.randint(0, len(classes), size=U)]


@pytest.mark.parametrize("U,T,C,blank", [(512, 700, 5, 0), (897, 1300, 6, 5)])
def test_reference_beyond_511_labels_equals_the_plain_recurrence(U, T, C, blank):
    g = torch.Generator().manual_seed(U)
    logits = torch.randn(T, 2, C, generator=g)
    seqs, ils = [_seq(U, C, blank, U), _seq(U - 100, C, blank, U + 1)], [T, T - 17]
    costs, dlogits, dlp = R.torch_reference(logits, seqs, ils, blank)
    lp = F.log_softmax(logits.double(), -1).numpy()
    for n in range(2):
        want = R.dp_cost(lp[:ils[n], n], seqs[n], blank)
        assert np.isfinite(want) and float(costs[n]) == pytest.approx(want, rel=1e-12)
    # rows of the true d/d log_probs sum to -1 below T_n and are zero beyond; d/d logits rows sum to 0
    assert torch.allclose(dlp[:, 0].sum(-1), torch.full((T,), -1.0, dtype=torch.float64), atol=1e-9)
    assert (dlp[T - 17:, 1] == 0).all() and (dlogits[T - 17:, 1] == 0).all()
    assert float(dlogits.sum(-1).abs().max()) < 1e-9


def test_reference_gradient_equals_finite_differences():
    g = torch.Generator().manual_seed(9)
    T, C = 7, 4
    logits = torch.randn(T, 2, C, generator=g, dtype=torch.float64)
    seqs, ils, gc = [[1, 1, 2], [3]], [7, 5], torch.tensor([0.5, -2.0], dtype=torch.float64)
    _, dlogits, dlp = R.torch_reference(logits, seqs, ils, 0, gc)

    def total(x, as_log_probs):
        lp = x if as_log_probs else F.log_softmax(x, -1)
        return sum(float(gc[n]) * R.dp_cost(lp[:ils[n], n].numpy(), seqs[n], 0) for n in range(2))
    lp = F.log_softmax(logits, -1)
    h, checked = 1e-6, 0
    for base, grad, as_lp in ((logits, dlogits, False), (lp, dlp, True)):
        for t in range(T):
            for n in range(2):
                for c in range(C):
                    up, dn = base.clone(), base.clone()
                    up[t, n, c] += h
                    dn[t, n, c] -= h
                    fd = (total(up, as_lp) - total(dn, as_lp)) / (2 * h)
                    assert float(grad[t, n, c]) == pytest.approx(fd, abs=1e-7), (as_lp, t, n, c)
                    checked += 1
    assert checked == 2 * T * 2 * C
