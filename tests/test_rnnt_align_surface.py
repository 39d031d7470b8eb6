"""Forced alignment without a GPU: the float64 reference of tests/align_common.py is pinned by brute force, the two
Python functions have the documented signatures, and the C entry points refuse bad arguments before any launch."""
import ctypes
import inspect
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_common as A  # noqa: E402

PIKA_EINVAL, PIKA_ETOOBIG = -1, -2


def _random_planes(rng, T, U):
    return np.log(rng.uniform(0.02, 1.0, (T, U + 1))), np.log(rng.uniform(0.02, 1.0, (T, U)))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("U", [0, 1, 2, 3, 4])
def test_fp64_viterbi_equals_brute_force(T, U):
    rng = np.random.default_rng(100 * T + U)
    for _ in range(4):
        lpb, lpe = _random_planes(rng, T, U)
        score, frames, delta = A.viterbi(lpb, lpe)
        best, arg = A.brute_force(lpb, lpe)
        assert frames.shape == (U,) and A.valid_frames(frames, T)
        assert score == pytest.approx(best, abs=1e-12)
        assert frames.tolist() == arg.tolist()
        assert A.rescore(lpb, lpe, frames) == pytest.approx(score, abs=1e-12)
        # the margin function agrees with the enumeration: best minus the best of every other path
        others = [A.rescore(lpb, lpe, np.asarray(fr)) for fr in
                  itertools.combinations_with_replacement(range(T), U) if list(fr) != arg.tolist()]
        if others:
            assert A.margin(lpb, lpe) == pytest.approx(best - max(others), abs=1e-12)
        else:
            assert A.margin(lpb, lpe) == np.inf
        assert math.comb(T - 1 + U, U) == len(others) + 1


@pytest.mark.parametrize("T,U", [(1, 3), (4, 0), (5, 4), (17, 9)])
def test_fp64_viterbi_tie_rule_gives_the_earliest_emission(T, U):
    c = math.log(0.125)
    score, frames, _ = A.viterbi(np.full((T, U + 1), c), np.full((T, U), c))
    assert frames.tolist() == [0] * U
    assert score == pytest.approx((T + U) * c, abs=1e-12)


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_python_signatures():
    from pika_amd.rnnt import rnnt_align, rnnt_align_from_logits
    assert list(inspect.signature(rnnt_align).parameters) == ["log_probs", "labels", "frames_lengths", "labels_lengths",
                                                              "blank", "compact"]
    assert list(inspect.signature(rnnt_align_from_logits).parameters) == ["logits", "labels", "frames_lengths",
                                                                          "labels_lengths", "blank", "compact"]
    assert _defaults(rnnt_align) == dict(blank=0, compact=False)
    assert _defaults(rnnt_align_from_logits) == dict(blank=0, compact=False)


def test_python_functions_refuse_cpu_tensors():
    import torch
    from pika_amd.rnnt import rnnt_align, rnnt_align_from_logits
    i32 = lambda *s: torch.ones(*s, dtype=torch.int32)   # noqa: E731
    for fn in (rnnt_align, rnnt_align_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(torch.zeros(1, 2, 2, 4), i32(1, 1), i32(1), i32(1))
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(torch.zeros(4, 4), i32(1), i32(1), i32(1), compact=True)


def test_dropin_has_no_align():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "pika_amd", "dropin"))
    try:
        import warp_rnnt
        assert not hasattr(warp_rnnt, "rnnt_align")
    finally:
        sys.path.pop(0)


def test_abi_version_is_25():
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25 and _lib.lib().pika_amd_abi_version() == 25


def test_align_scratch_bytes():
    from pika_amd import _lib
    L = _lib.lib()
    for dims in ((0, 10, 5), (1, 0, 5), (1, 10, 0), (-1, 10, 5), (1, 10, 1025)):
        assert L.pika_rnnt_align_scratch_bytes(*dims) == 0
    # one back-pointer bit per cell of the skewed lattice: [B][T+U1-1][W/64] 64-bit words
    assert L.pika_rnnt_align_scratch_bytes(32, 1000, 51) == 32 * 1050 * 8
    assert L.pika_rnnt_align_scratch_bytes(1, 10, 65) == 74 * 2 * 8
    assert L.pika_rnnt_align_scratch_bytes(3, 7, 200) == 3 * 206 * 4 * 8
    assert L.pika_rnnt_align_scratch_bytes(1, 1, 1) > 0
    assert L.pika_rnnt_align_scratch_bytes(1, 1, 1024) > 0
    # the loss workspace is not what pays for it
    assert L.pika_rnnt_workspace_bytes(32, 1000, 51) == 4 * 32 * 1050 * 64 * 4 + (2 * 32 * 1050 + 64) * 8 + 32 * 1000 * 51 * 16


def test_align_refuses_bad_arguments_without_a_launch():
    from pika_amd import _lib
    L = _lib.lib()
    q = ctypes.c_void_p(256)              # never dereferenced: every call below returns before a launch
    ok = dict(workspace=q, frames_lengths=q, labels_lengths=q, label_offsets=None, B=2, T=5, U1=3, scores=q,
              emit_frames=q, scratch=q, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.pika_rnnt_align(a["workspace"], a["frames_lengths"], a["labels_lengths"], a["label_offsets"], a["B"],
                                 a["T"], a["U1"], a["scores"], a["emit_frames"], a["scratch"], a["stream"])

    for name in ("workspace", "frames_lengths", "labels_lengths", "scores", "emit_frames", "scratch"):
        assert call(**{name: None}) == PIKA_EINVAL, name
    for name in ("B", "T", "U1"):
        assert call(**{name: 0}) == PIKA_EINVAL, name
        assert call(**{name: -3}) == PIKA_EINVAL, name
    assert call(U1=1025) == PIKA_ETOOBIG
    assert call(U1=1025, label_offsets=q) == PIKA_ETOOBIG
    assert call(B=0, U1=1025) == PIKA_EINVAL
