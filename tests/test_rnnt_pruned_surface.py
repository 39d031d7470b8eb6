"""Pruned RNN-T without a GPU: the Python functions have the documented signatures and are exported from the package,
the two torch helpers compute what they say, CPU tensors are refused, and the C entry points (include/pika_rnnt.h,
pika_prnnt_*) refuse bad arguments before any launch."""
import ctypes
import inspect

import numpy as np
import pytest

from helpers import log_softmax

PIKA_EINVAL, PIKA_ETOOBIG = -1, -2

EXPORTS = ("rnnt_loss_pruned", "rnnt_loss_pruned_from_logits", "rnnt_loss_from_planes", "rnnt_prune_ranges",
           "rnnt_simple_planes", "rnnt_prune_lm")
ENTRIES = ("pika_prnnt_forward", "pika_prnnt_backward", "pika_prnnt_fused_forward", "pika_prnnt_fused_backward",
           "pika_prnnt_planes_forward", "pika_prnnt_prune_ranges")


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_python_signatures_and_exports():
    import pika_amd
    from pika_amd import rnnt
    for name in EXPORTS:
        assert getattr(pika_amd, name) is getattr(rnnt, name) and name in dir(pika_amd)
    lossy = ["labels", "ranges", "frames_lengths", "labels_lengths", "average_frames", "reduction", "blank", "fastemit_lambda"]
    assert list(inspect.signature(rnnt.rnnt_loss_pruned).parameters) == ["log_probs"] + lossy
    assert list(inspect.signature(rnnt.rnnt_loss_pruned_from_logits).parameters) == ["logits"] + lossy
    for fn in (rnnt.rnnt_loss_pruned, rnnt.rnnt_loss_pruned_from_logits):
        assert _defaults(fn) == dict(average_frames=False, reduction=None, blank=0, fastemit_lambda=0.0)
    assert list(inspect.signature(rnnt.rnnt_loss_from_planes).parameters) == [
        "blank_lp", "label_lp", "frames_lengths", "labels_lengths", "reduction", "return_occupancy"]
    assert _defaults(rnnt.rnnt_loss_from_planes) == dict(reduction=None, return_occupancy=False)
    assert list(inspect.signature(rnnt.rnnt_prune_ranges).parameters) == [
        "blank_occ", "label_occ", "frames_lengths", "labels_lengths", "s_range"]
    assert list(inspect.signature(rnnt.rnnt_simple_planes).parameters) == ["am", "lm", "labels", "blank"]
    assert _defaults(rnnt.rnnt_simple_planes) == dict(blank=0)
    assert list(inspect.signature(rnnt.rnnt_prune_lm).parameters) == ["lm", "ranges", "s_range"]


def test_abi_version_is_25_and_the_entries_are_bound():
    from pika_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 25 and L.pika_amd_abi_version() == 25
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert _lib.SIGNATURES[name][0] is ctypes.c_int


def test_python_functions_refuse_cpu_tensors():
    import torch
    from pika_amd import rnnt
    i32 = lambda *s: torch.ones(*s, dtype=torch.int32)   # noqa: E731
    for fn in (rnnt.rnnt_loss_pruned, rnnt.rnnt_loss_pruned_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(torch.zeros(1, 2, 2, 4), i32(1, 2), torch.zeros(1, 2, dtype=torch.int32), i32(1), i32(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        rnnt.rnnt_loss_from_planes(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), i32(1), i32(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        rnnt.rnnt_prune_ranges(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), i32(1), i32(1), 2)


def test_simple_planes_are_the_log_softmax_of_am_plus_lm():
    import torch
    from pika_amd.rnnt import rnnt_simple_planes
    rng = np.random.default_rng(0)
    B, T, U, V, blank = 2, 5, 3, 7, 2
    am = rng.standard_normal((B, T, V)) * 3 + 40.0           # a large common offset: the normaliser must be max-shifted
    lm = rng.standard_normal((B, U + 1, V)) * 3 - 70.0
    y = rng.integers(0, V, (B, U)).astype(np.int32)
    y[1, 2] = V                                              # padding, clamped: the loss never reads it
    lp = log_softmax(am[:, :, None, :] + lm[:, None, :, :])
    ta = torch.tensor(am, dtype=torch.float32, requires_grad=True)
    tm = torch.tensor(lm, dtype=torch.float32, requires_grad=True)
    pb, pl = rnnt_simple_planes(ta, tm, torch.from_numpy(y), blank=blank)
    assert pb.shape == pl.shape == (B, T, U + 1) and pb.dtype == torch.float32
    assert np.allclose(pb.detach().numpy(), lp[..., blank], atol=2e-4)
    for b in range(B):
        for u in range(U):
            if y[b, u] < V:
                assert np.allclose(pl[b, :, u].detach().numpy(), lp[b, :, u, y[b, u]], atol=2e-4)
    assert (pl[:, :, U] == -1.0e30).all()
    (pb.sum() + pl[:, :, :U].sum()).backward()               # differentiable in plain torch
    assert torch.isfinite(ta.grad).all() and torch.isfinite(tm.grad).all()
    with pytest.raises(ValueError):
        rnnt_simple_planes(ta, tm, torch.from_numpy(y[:, :2]))
    with pytest.raises(ValueError):
        rnnt_simple_planes(ta, tm, torch.from_numpy(y), blank=V)


def test_prune_lm_takes_the_band_rows_with_the_clamped_index():
    import torch
    from pika_amd.rnnt import rnnt_prune_lm
    B, U1, D, S = 2, 6, 3, 3
    lm = torch.arange(B * U1 * D, dtype=torch.float32).reshape(B, U1, D)
    ranges = torch.tensor([[0, 1, 3, 3], [0, 2, 7, -4]], dtype=torch.int32)    # 7 and -4 are clamped to 3 and 0
    out = rnnt_prune_lm(lm, ranges, S)
    assert out.shape == (B, 4, S, D)
    want = np.clip(ranges.numpy(), 0, U1 - S)
    for b in range(B):
        for t in range(4):
            assert torch.equal(out[b, t], lm[b, want[b, t]:want[b, t] + S])
    assert torch.equal(rnnt_prune_lm(lm, torch.zeros(B, 2, dtype=torch.int32), U1)[:, 0], lm)
    with pytest.raises(ValueError):
        rnnt_prune_lm(lm, ranges, U1 + 1)


def _caller(L, fn, names, ok):
    def call(**kw):
        a = dict(ok, **kw)
        return getattr(L, fn)(*[a[n] for n in names])
    return call


BANDED = {
    "pika_prnnt_forward": "log_probs frames_lengths labels_lengths labels ranges B T U1 S V blank costs workspace stream",
    "pika_prnnt_backward": "frames_lengths labels_lengths labels ranges B T U1 S V blank grad_costs workspace grads "
                           "fastemit_lambda stream",
    "pika_prnnt_fused_forward": "logits frames_lengths labels_lengths labels ranges B T U1 S V blank costs lse workspace "
                                "stream",
    "pika_prnnt_fused_backward": "logits lse frames_lengths labels_lengths labels ranges B T U1 S V blank grad_costs "
                                 "workspace grad_logits out_dtype ld_out fastemit_lambda stream",
}
OPTIONAL = {"grad_costs", "grads", "stream"}


@pytest.mark.parametrize("fn", sorted(BANDED))
def test_banded_entries_refuse_bad_arguments_without_a_launch(fn):
    from pika_amd import _lib
    L = _lib.lib()
    names = BANDED[fn].split()
    assert len(names) == len(_lib.SIGNATURES[fn][1])
    q = ctypes.c_void_p(256)              # never dereferenced: every call below returns before a launch
    ints = dict(B=2, T=5, U1=4, S=2, V=8, blank=0, out_dtype=0, ld_out=8, fastemit_lambda=0.0, stream=None)
    ok = {n: ints.get(n, q) for n in names}
    call = _caller(L, fn, names, ok)
    for n in names:
        if n not in ints and n not in OPTIONAL:
            assert call(**{n: None}) == PIKA_EINVAL, n
    for n in ("B", "T", "U1", "V"):
        assert call(**{n: 0}) == PIKA_EINVAL, n
        assert call(**{n: -3}) == PIKA_EINVAL, n
    assert call(blank=8) == PIKA_EINVAL and call(blank=-1) == PIKA_EINVAL
    # the band width: 1 <= S <= U1
    assert call(S=0) == PIKA_EINVAL and call(S=-1) == PIKA_EINVAL and call(S=5) == PIKA_EINVAL
    assert call(U1=1025, S=5) == PIKA_ETOOBIG
    assert call(U1=1025, S=1026) == PIKA_EINVAL
    assert call(B=1 << 12, T=1 << 10, U1=1 << 10, S=1 << 10) == PIKA_ETOOBIG      # B*T*S = 2^32 rows
    assert call(B=1 << 12, T=1 << 10, U1=1 << 10, S=1 << 9) == PIKA_ETOOBIG       # 2^31
    if "fused" in fn:
        assert call(V=6, blank=0) == PIKA_EINVAL and call(V=8196) == PIKA_EINVAL
    if "fastemit_lambda" in names:
        assert call(fastemit_lambda=-1.0) == PIKA_EINVAL and call(fastemit_lambda=float("nan")) == PIKA_EINVAL
    if "out_dtype" in names:
        assert call(out_dtype=2) == PIKA_EINVAL and call(ld_out=4) == PIKA_EINVAL and call(ld_out=10) == PIKA_EINVAL
    # no label column: the labels may be null
    if fn == "pika_prnnt_backward":
        assert call(U1=1, S=1, labels=None, workspace=None) == PIKA_EINVAL


def test_planes_and_band_search_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    L = _lib.lib()
    q = ctypes.c_void_p(256)
    names = "blank_lp label_lp frames_lengths labels_lengths B T U1 costs blank_occ label_occ workspace stream".split()
    ok = {n: q for n in names}
    ok.update(B=2, T=5, U1=4, stream=None)
    call = _caller(L, "pika_prnnt_planes_forward", names, ok)
    for n in names:
        if ok[n] is q:
            assert call(**{n: None}) == PIKA_EINVAL, n
    for n in ("B", "T", "U1"):
        assert call(**{n: 0}) == PIKA_EINVAL and call(**{n: -2}) == PIKA_EINVAL, n
    assert call(U1=1025) == PIKA_ETOOBIG
    names = "blank_occ label_occ frames_lengths labels_lengths B T U1 S ranges stream".split()
    ok = {n: q for n in names}
    ok.update(B=2, T=5, U1=4, S=2, stream=None)
    call = _caller(L, "pika_prnnt_prune_ranges", names, ok)
    for n in names:
        if ok[n] is q:
            assert call(**{n: None}) == PIKA_EINVAL, n
    for n in ("B", "T", "U1", "S"):
        assert call(**{n: 0}) == PIKA_EINVAL and call(**{n: -2}) == PIKA_EINVAL, n
    assert call(S=5) == PIKA_EINVAL
    assert call(U1=1025, S=5) == PIKA_ETOOBIG
