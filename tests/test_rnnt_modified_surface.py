"""Modified-topology RNN-T without a GPU: the Python functions have the documented signatures and are exported from the
package, CPU tensors are refused, and the C entry points (include/pika_rnnt.h, pika_prnnt_mod_*) refuse bad arguments
before any launch."""
import ctypes
import inspect

import pytest

PIKA_EINVAL, PIKA_ETOOBIG = -1, -2

EXPORTS = ("rnnt_loss_from_planes_modified", "rnnt_prune_ranges_modified", "rnnt_loss_pruned_modified",
           "rnnt_loss_pruned_modified_from_logits", "rnnt_loss_modified", "rnnt_loss_modified_from_logits",
           "rnnt_pruned_joint_loss_modified")
ENTRIES = ("pika_prnnt_mod_forward", "pika_prnnt_mod_backward", "pika_prnnt_mod_fused_forward",
           "pika_prnnt_mod_fused_backward", "pika_prnnt_mod_planes_forward", "pika_prnnt_mod_prune_ranges")


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_python_signatures_and_exports():
    import pika_amd
    from pika_amd import rnnt
    for name in EXPORTS:
        assert getattr(pika_amd, name) is getattr(rnnt, name) and name in dir(pika_amd)
    tail = ["frames_lengths", "labels_lengths", "average_frames", "reduction", "blank", "fastemit_lambda"]
    lossy = dict(average_frames=False, reduction=None, blank=0, fastemit_lambda=0.0)
    assert _params(rnnt.rnnt_loss_pruned_modified) == ["log_probs", "labels", "ranges"] + tail
    assert _params(rnnt.rnnt_loss_pruned_modified_from_logits) == ["logits", "labels", "ranges"] + tail
    assert _params(rnnt.rnnt_loss_modified) == ["log_probs", "labels"] + tail
    assert _params(rnnt.rnnt_loss_modified_from_logits) == ["logits", "labels"] + tail
    for fn in (rnnt.rnnt_loss_pruned_modified, rnnt.rnnt_loss_pruned_modified_from_logits, rnnt.rnnt_loss_modified,
               rnnt.rnnt_loss_modified_from_logits):
        assert _defaults(fn) == lossy
    # the regular counterparts' signatures, name for name
    assert _params(rnnt.rnnt_loss_pruned_modified) == _params(rnnt.rnnt_loss_pruned)
    assert _params(rnnt.rnnt_loss_from_planes_modified) == _params(rnnt.rnnt_loss_from_planes) == [
        "blank_lp", "label_lp", "frames_lengths", "labels_lengths", "reduction", "return_occupancy"]
    assert _defaults(rnnt.rnnt_loss_from_planes_modified) == dict(reduction=None, return_occupancy=False)
    assert _params(rnnt.rnnt_prune_ranges_modified) == _params(rnnt.rnnt_prune_ranges) == [
        "blank_occ", "label_occ", "frames_lengths", "labels_lengths", "s_range"]
    assert _defaults(rnnt.rnnt_prune_ranges_modified) == {}
    chain = rnnt.rnnt_pruned_joint_loss_modified
    assert _params(chain)[:13] == ["enc", "pred", "labels", "frames_lengths", "labels_lengths", "fc1", "fc_gate", "fc2",
                                   "simple_am", "simple_lm", "s_range", "lm_only_scale", "am_only_scale"]
    assert sorted(_params(chain)) == sorted(_params(rnnt.rnnt_pruned_joint_loss_smoothed))
    assert _defaults(chain) == _defaults(rnnt.rnnt_pruned_joint_loss_smoothed) == dict(
        s_range=5, lm_only_scale=0.0, am_only_scale=0.0, blank=0, fastemit_lambda=0.0, reduction="sum")


def test_abi_version_is_25_and_the_entries_are_bound():
    from pika_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 25 and L.pika_amd_abi_version() == 25
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(L, name)
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
        assert _lib.SIGNATURES[name][1] == _lib.SIGNATURES[name.replace("_mod_", "_")][1]     # argument for argument
    assert _lib.SIGNATURES["pika_prnnt_mod_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)


def test_the_workspace_holds_the_unskewed_planes_and_the_row_metadata():
    from pika_amd import _lib
    L = _lib.lib()
    for bad in ((0, 5, 4), (2, 0, 4), (2, 5, 0), (2, 5, 1025), (-1, 5, 4)):
        assert L.pika_prnnt_mod_workspace_bytes(*bad) == 0
    for B, T, U1 in ((2, 5, 4), (3, 70, 65), (1, 1, 1), (2, 9, 1024)):
        Wp = next(64 * w for w in (1, 2, 3, 4, 6, 8, 12, 16) if 64 * w >= U1)
        # four planes, the fp64 offsets and log-likelihoods, 16 bytes of row metadata per cell, one centre per plane row
        want = 4 * B * (T + 1) * Wp * 4 + (2 * B * (T + 1) + 2 * B) * 8 + B * T * U1 * 16 + B * (T + 1) * 4
        assert L.pika_prnnt_mod_workspace_bytes(B, T, U1) == want


def test_python_functions_refuse_cpu_tensors():
    import torch
    from pika_amd import rnnt
    i32 = lambda *s: torch.ones(*s, dtype=torch.int32)   # noqa: E731
    for fn in (rnnt.rnnt_loss_pruned_modified, rnnt.rnnt_loss_pruned_modified_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(torch.zeros(1, 2, 2, 4), i32(1, 2), torch.zeros(1, 2, dtype=torch.int32), i32(1), i32(1))
    for fn in (rnnt.rnnt_loss_modified, rnnt.rnnt_loss_modified_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(torch.zeros(1, 2, 3, 4), i32(1, 2), i32(1), i32(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        rnnt.rnnt_loss_from_planes_modified(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), i32(1), i32(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        rnnt.rnnt_prune_ranges_modified(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), i32(1), i32(1), 2)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        rnnt.rnnt_loss_modified(torch.zeros(1, 2, 3, 4), i32(1, 2), i32(1), i32(1), fastemit_lambda=-1.0)


def _caller(L, fn, names, ok):
    def call(**kw):
        a = dict(ok, **kw)
        return getattr(L, fn)(*[a[n] for n in names])
    return call


BANDED = {
    "pika_prnnt_mod_forward": "log_probs frames_lengths labels_lengths labels ranges B T U1 S V blank costs workspace stream",
    "pika_prnnt_mod_backward": "frames_lengths labels_lengths labels ranges B T U1 S V blank grad_costs workspace grads "
                               "fastemit_lambda stream",
    "pika_prnnt_mod_fused_forward": "logits frames_lengths labels_lengths labels ranges B T U1 S V blank costs lse workspace "
                                    "stream",
    "pika_prnnt_mod_fused_backward": "logits lse frames_lengths labels_lengths labels ranges B T U1 S V blank grad_costs "
                                     "workspace grad_logits out_dtype ld_out fastemit_lambda stream",
}
# ranges may be null: the padded layout, which requires S == U1 (tested below)
OPTIONAL = {"grad_costs", "grads", "stream", "ranges"}


@pytest.mark.parametrize("fn", sorted(BANDED))
def test_modified_entries_refuse_bad_arguments_without_a_launch(fn):
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
    # the band width: 1 <= S <= U1; without ranges (the padded layout) S is U1
    assert call(S=0) == PIKA_EINVAL and call(S=-1) == PIKA_EINVAL and call(S=5) == PIKA_EINVAL
    assert call(ranges=None, S=2) == PIKA_EINVAL and call(ranges=None, S=3) == PIKA_EINVAL
    assert call(ranges=None, S=4, labels=None) == PIKA_EINVAL
    assert call(U1=1025, S=5) == PIKA_ETOOBIG
    assert call(U1=1025, S=1026) == PIKA_EINVAL
    assert call(B=1 << 12, T=1 << 10, U1=1 << 10, S=1 << 10) == PIKA_ETOOBIG      # B*T*S = 2^32 rows
    assert call(B=1 << 12, T=1 << 10, U1=1 << 10, S=1 << 9) == PIKA_ETOOBIG       # 2^31
    assert call(B=1 << 12, T=1 << 10, U1=1 << 10, S=1 << 10, ranges=None) == PIKA_ETOOBIG
    if "fused" in fn:
        assert call(V=6, blank=0) == PIKA_EINVAL and call(V=8196) == PIKA_EINVAL
    if "fastemit_lambda" in names:
        assert call(fastemit_lambda=-1.0) == PIKA_EINVAL and call(fastemit_lambda=float("nan")) == PIKA_EINVAL
    if "out_dtype" in names:
        assert call(out_dtype=2) == PIKA_EINVAL and call(ld_out=4) == PIKA_EINVAL and call(ld_out=10) == PIKA_EINVAL
    # no label column: the labels may be null
    if fn == "pika_prnnt_mod_backward":
        assert call(U1=1, S=1, labels=None, workspace=None) == PIKA_EINVAL


def test_planes_and_band_search_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    L = _lib.lib()
    q = ctypes.c_void_p(256)
    names = "blank_lp label_lp frames_lengths labels_lengths B T U1 costs blank_occ label_occ workspace stream".split()
    ok = {n: q for n in names}
    ok.update(B=2, T=5, U1=4, stream=None)
    call = _caller(L, "pika_prnnt_mod_planes_forward", names, ok)
    for n in names:
        if ok[n] is q:
            assert call(**{n: None}) == PIKA_EINVAL, n
    for n in ("B", "T", "U1"):
        assert call(**{n: 0}) == PIKA_EINVAL and call(**{n: -2}) == PIKA_EINVAL, n
    assert call(U1=1025) == PIKA_ETOOBIG
    names = "blank_occ label_occ frames_lengths labels_lengths B T U1 S ranges stream".split()
    ok = {n: q for n in names}
    ok.update(B=2, T=5, U1=4, S=2, stream=None)
    call = _caller(L, "pika_prnnt_mod_prune_ranges", names, ok)
    for n in names:
        if ok[n] is q:
            assert call(**{n: None}) == PIKA_EINVAL, n
    for n in ("B", "T", "U1", "S"):
        assert call(**{n: 0}) == PIKA_EINVAL and call(**{n: -2}) == PIKA_EINVAL, n
    assert call(S=5) == PIKA_EINVAL
    assert call(U1=1025, S=5) == PIKA_ETOOBIG
