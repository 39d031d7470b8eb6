"""The warp_rnnt keyword surface of pika_amd.rnnt without a GPU: `gather`, `fastemit_lambda` and `compact` exist with
warp_rnnt's defaults, RNNTLoss keeps its FastEmit factor instead of discarding it, and the new C entry points refuse a
bad lambda or packed row count before any launch."""
import ctypes
import inspect
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIKA_EINVAL, PIKA_ETOOBIG = -1, -2


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_rnnt_loss_keywords():
    from pika_amd.rnnt import rnnt_loss
    assert list(inspect.signature(rnnt_loss).parameters)[:4] == ["log_probs", "labels", "frames_lengths", "labels_lengths"]
    assert _defaults(rnnt_loss) == dict(average_frames=False, reduction=None, blank=0, gather=False, fastemit_lambda=0.0,
                                        compact=False)


def test_rnnt_loss_from_logits_keywords():
    from pika_amd.rnnt import rnnt_loss_from_logits
    assert _defaults(rnnt_loss_from_logits) == dict(blank=0, fastemit_lambda=0.0, compact=False)


def test_rnnt_loss_class_keeps_fastemit_lambda():
    from pika_amd.rnnt import RNNTLoss
    assert RNNTLoss(blank=0, reduction="sum").fastemit_lambda == 0.0
    loss = RNNTLoss(blank=0, reduction="sum", fastemit_lambda=0.01)
    assert loss.fastemit_lambda == pytest.approx(0.01) and loss.blank == 0
    sys.path.insert(0, os.path.join(ROOT, "pika_amd", "dropin"))
    try:
        from warp_rnnt import RNNTLoss as DropIn
        assert DropIn(blank=0, reduction="sum", fastemit_lambda=0.5).fastemit_lambda == 0.5
    finally:
        sys.path.pop(0)


@pytest.mark.parametrize("lam", [-1e-3, float("nan"), float("inf")])
def test_bad_fastemit_lambda_is_refused(lam):
    from pika_amd.rnnt import RNNTLoss, rnnt_loss, rnnt_loss_from_logits
    with pytest.raises(ValueError, match="fastemit_lambda"):
        RNNTLoss(blank=0, fastemit_lambda=lam)
    # refused before the tensors are looked at (these are not even tensors)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        rnnt_loss(None, None, None, None, fastemit_lambda=lam)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        rnnt_loss_from_logits(None, None, None, None, fastemit_lambda=lam)


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    L = _lib.lib()
    q = ctypes.c_void_p(256)              # never dereferenced: every call below returns before a launch
    s = None
    for lam in (-1.0, math.nan, math.inf):
        assert L.pika_rnnt_loss_backward_fe(q, q, q, 1, 2, 2, 4, 0, None, q, q, lam, s) == PIKA_EINVAL
        assert L.pika_rnnt_fused_backward_fe(q, q, q, q, q, 1, 2, 2, 4, 0, None, q, q, 0, 4, lam, s) == PIKA_EINVAL
        assert L.pika_rnnt_packed_backward(q, q, q, q, q, 1, 2, 2, 4, 4, 0, None, q, q, lam, s) == PIKA_EINVAL
        assert L.pika_rnnt_packed_fused_backward(q, q, q, q, q, q, q, 1, 2, 2, 4, 4, 0, None, q, q, 0, 4, lam, s) == PIKA_EINVAL
    # N: positive, within the B*T_max*U1_max rows of the workspace, below 2^31
    for N, want in ((0, PIKA_EINVAL), (5, PIKA_EINVAL), (1 << 31, PIKA_ETOOBIG)):
        B, T, U1 = (1, 2, 2) if N < (1 << 31) else (1 << 12, 1 << 10, 1 << 10)
        assert L.pika_rnnt_packed_forward(q, q, q, q, q, q, B, T, U1, N, 4, 0, q, q, s) == want
        assert L.pika_rnnt_packed_backward(q, q, q, q, q, B, T, U1, N, 4, 0, None, q, q, 0.0, s) == want
        assert L.pika_rnnt_packed_fused_forward(q, q, q, q, q, q, B, T, U1, N, 4, 0, q, q, q, s) == want
        assert L.pika_rnnt_packed_fused_backward(q, q, q, q, q, q, q, B, T, U1, N, 4, 0, None, q, q, 0, 4, 0.0, s) == want
    # offsets are required; U1_max > 1 needs the label offsets
    assert L.pika_rnnt_packed_forward(q, q, q, q, None, q, 1, 2, 2, 4, 4, 0, q, q, s) == PIKA_EINVAL
    assert L.pika_rnnt_packed_forward(q, q, q, q, q, None, 1, 2, 2, 4, 4, 0, q, q, s) == PIKA_EINVAL
    assert L.pika_rnnt_packed_forward(q, q, q, q, q, q, 1, 2, 1025, 4, 4, 0, q, q, s) == PIKA_ETOOBIG
