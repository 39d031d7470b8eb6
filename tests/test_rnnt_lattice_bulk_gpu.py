"""The one-wave alpha/beta kernel walks whole 16-diagonal renormalisation groups of the band
Un <= d <= Tn-1 in an unmasked "bulk" loop and the rest with masked code.  These shapes put the
band's edges at every place that split can go wrong, checked against the fp64 oracle: no bulk at
all (Tn-1 < Un), a lattice shorter than one group, bulks that start or end inside a group,
utterances of one batch with different (Tn, Un), the widest one-wave lattice (U1 = 64) and the
benchmark's utterance size."""

import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import make_case

pytestmark = pytest.mark.gpu


def check(dev, lp, y, tl, ul, rel=1e-4, abs_=1e-5, cost_rel=1e-5):
    from pika_amd import rnnt as R
    x = torch.from_numpy(lp).to(dev).requires_grad_(True)
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (y, tl, ul)]
    costs = R.RNNTLoss(blank=0, reduction="sum").apply(x, *args)
    costs.sum().backward()
    torch.cuda.synchronize()
    c, g = costs.detach().cpu().numpy(), x.grad.cpu().numpy()
    c64, g64 = O.rnnt_loss(lp, y, tl, ul)
    assert np.allclose(c, c64, rtol=cost_rel, atol=0), (c, c64)
    err = np.abs(g - g64)
    bad = err > rel * np.abs(g64) + abs_
    assert not bad.any(), "max excess %g" % float((err - rel * np.abs(g64)).max())


@pytest.mark.parametrize("T,U", [
    (10, 30),   # Tn-1 < Un: no bulk
    (5, 8),     # dend < 16
    (17, 0),    # U1 = 1: one bulk group, nothing to emit
    (33, 3),    # one bulk group after a short head
    (50, 7),    # bulk from d = 17, alpha's tail starts inside a group
    (64, 20),   # head of two groups, bulk ends on a group boundary
    (81, 18),   # three bulk groups per direction; alpha's tail (d = 81..98) spans two groups
    (70, 63),   # U1 = 64 with Tn-1 < 80: both directions fall back to the masked walk
    (100, 63),  # U1 = 64 in the bulk: every lane live, none reads column Un for another
])
def test_bulk_band_edges(hip_device, T, U):
    lp, y, tl, ul = make_case(2, T, U, 6, seed=T * 131 + U)
    check(hip_device, lp, y, tl, ul)


def test_mixed_lengths_in_one_batch(hip_device):
    lp, y, tl, ul = make_case(6, 90, 40, 5, seed=11)
    tl[:] = [90, 1, 40, 17, 63, 89]
    ul[:] = [40, 0, 39, 16, 5, 33]
    for n in range(6):
        y[n, ul[n]:] = 5
    check(hip_device, lp, y, tl, ul)


def test_benchmark_sized_utterance(hip_device):
    lp, y, tl, ul = make_case(1, 1000, 50, 4, seed=5)
    check(hip_device, lp, y, tl, ul, rel=1e-3, abs_=2e-5)
