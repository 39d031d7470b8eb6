"""The smoothed simple loss of pruned RNN-T without a GPU: the three Python names resolve from the package with their
signatures; the two C entry points are declared, exported and bound and refuse bad arguments before any launch; and the
plain-torch spelling (what CPU and float64 tensors run, and the GPU tests' reference) is k2's definition, checked in
float64 against a brute-force construction on the explicit (B, T, U+1, V) tensor -- values and both gradients, the path
through the batch unigram included."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIKA_EINVAL, PIKA_ETOOBIG = -1, -2
ENTRIES = {
    "pika_prnnt_smoothed_fwd": "am elm side labels B T U1 V blank lm_only_scale am_only_scale amax gathered sums blank_lp "
                               "label_lp stream",
    "pika_prnnt_smoothed_bwd": "am amax elm w sg labels B T U1 V blank lm_only_scale am_only_scale d_am m stream",
}
SCALES = [(0.0, 0.0), (0.25, 0.0), (0.0, 0.3), (0.25, 0.3)]
TINY = torch.finfo(torch.float32).tiny


def test_python_entry_points_resolve_from_the_package():
    import pika_amd
    from pika_amd import rnnt
    for name in ("rnnt_smoothed_planes", "rnnt_loss_smoothed", "rnnt_pruned_joint_loss_smoothed"):
        assert getattr(pika_amd, name) is getattr(rnnt, name) and name in dir(pika_amd)

    def defaults(fn):
        sig = inspect.signature(fn)
        return list(sig.parameters), {k: p.default for k, p in sig.parameters.items()
                                      if p.default is not inspect.Parameter.empty}
    assert defaults(rnnt.rnnt_smoothed_planes) == (
        ["am", "lm", "labels", "blank", "lm_only_scale", "am_only_scale"],
        dict(blank=0, lm_only_scale=0.0, am_only_scale=0.0))
    assert defaults(rnnt.rnnt_loss_smoothed) == (
        ["am", "lm", "labels", "frames_lengths", "labels_lengths", "blank", "lm_only_scale", "am_only_scale", "reduction",
         "return_occupancy"],
        dict(blank=0, lm_only_scale=0.0, am_only_scale=0.0, reduction=None, return_occupancy=False))
    assert defaults(rnnt.rnnt_pruned_joint_loss_smoothed) == (
        ["enc", "pred", "labels", "frames_lengths", "labels_lengths", "fc1", "fc_gate", "fc2", "simple_am", "simple_lm",
         "s_range", "blank", "fastemit_lambda", "reduction", "lm_only_scale", "am_only_scale"],
        dict(s_range=5, blank=0, fastemit_lambda=0.0, reduction="sum", lm_only_scale=0.0, am_only_scale=0.0))


def test_entries_are_declared_exported_and_bound_and_the_abi_is_25():
    from pika_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pika_rnnt.h")).read(), flags=re.S)
    L = _lib.lib()
    assert _lib.ABI_VERSION == 25 and L.pika_amd_abi_version() == 25
    for name, params in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/pika_rnnt.h" % name
        declared = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert declared == params.split()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(declared)


def test_entries_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    L = _lib.lib()
    q = ctypes.c_void_p(256)               # never dereferenced: every call below returns before a launch
    for fn, params in ENTRIES.items():
        names = params.split()
        vals = dict(B=2, T=5, U1=4, V=7, blank=0, lm_only_scale=0.25, am_only_scale=0.25, stream=None)
        ok = {n: vals.get(n, q) for n in names}

        def call(**kw):
            a = dict(ok, **kw)
            return getattr(L, fn)(*[a[n] for n in names])
        for n in names:
            if n not in vals:
                assert call(**{n: None}) == PIKA_EINVAL, (fn, n)
        for n in ("B", "T", "U1", "V"):
            assert call(**{n: 0}) == PIKA_EINVAL and call(**{n: -3}) == PIKA_EINVAL, (fn, n)
        assert call(blank=7) == PIKA_EINVAL and call(blank=-1) == PIKA_EINVAL          # blank = V
        assert call(U1=1025) == PIKA_ETOOBIG
        assert call(U1=1025, blank=7) == PIKA_EINVAL                                   # a bad argument comes before the size
        assert call(lm_only_scale=0.5, am_only_scale=0.5) == PIKA_EINVAL               # the scales sum to 1
        assert call(lm_only_scale=1.0, am_only_scale=0.0) == PIKA_EINVAL
        assert call(lm_only_scale=-0.1) == PIKA_EINVAL and call(am_only_scale=-0.1) == PIKA_EINVAL
        assert call(lm_only_scale=float("nan")) == PIKA_EINVAL and call(am_only_scale=float("inf")) == PIKA_EINVAL


def _case(blank, seed=0):
    B, T, U, V = 2, 5, 3, 7
    g = torch.Generator().manual_seed(seed)
    am = (2.0 * torch.randn(B, T, V, generator=g, dtype=torch.float64)).requires_grad_(True)
    lm = (2.0 * torch.randn(B, U + 1, V, generator=g, dtype=torch.float64)).requires_grad_(True)
    # a repeated label, a label equal to either blank, and padding labels outside [0, V) that must be clamped
    labels = torch.tensor([[3, 3, blank], [V - 1, -1, V + 4]], dtype=torch.int32)
    wb = torch.randn(B, T, U + 1, generator=g, dtype=torch.float64)
    wl = torch.randn(B, T, U + 1, generator=g, dtype=torch.float64)
    wl[:, :, U] = 0.0
    return am, lm, labels, wb, wl


def _brute_force(am, lm, labels, blank, ll, la):
    B, T, V = am.shape
    U1 = lm.shape[1]
    joint = torch.log_softmax(am[:, :, None, :] + lm[:, None, :, :], -1)                       # (B,T,U1,V)
    lm_only = torch.log_softmax(lm, -1)[:, None].expand(B, T, U1, V)
    q = torch.softmax(lm, -1).reshape(B * U1, V).mean(0) + TINY
    am_only = torch.log_softmax(am + q.log(), -1)[:, :, None, :].expand(B, T, U1, V)           # exp(am) q, normalised
    mix = (1.0 - ll - la) * joint + ll * lm_only + la * am_only
    y = labels.long().clamp(0, V - 1)
    label_lp = torch.gather(mix[:, :, :U1 - 1], 3, y[:, None, :, None].expand(B, T, U1 - 1, 1)).squeeze(3)
    label_lp = torch.cat([label_lp, label_lp.new_full((B, T, 1), -1.0e30)], 2)
    return mix[..., blank], label_lp


@pytest.mark.parametrize("blank", [0, 6])
@pytest.mark.parametrize("scales", SCALES)
def test_the_torch_spelling_is_the_definition_in_float64(scales, blank):
    from pika_amd import rnnt_smoothed_planes
    ll, la = scales
    am, lm, labels, wb, wl = _case(blank)
    got = rnnt_smoothed_planes(am, lm, labels, blank=blank, lm_only_scale=ll, am_only_scale=la)
    want = _brute_force(am, lm, labels, blank, ll, la)
    assert got[0].dtype == torch.float64 and got[0].shape == got[1].shape == (2, 5, 4)
    for a, b in zip(got, want):
        assert float((a - b).detach().abs().max()) < 1e-12
    assert (got[1][:, :, 3] == -1.0e30).all()
    g_got = torch.autograd.grad((wb * got[0]).sum() + (wl * got[1]).sum(), [am, lm])
    g_want = torch.autograd.grad((wb * want[0]).sum() + (wl * want[1]).sum(), [am, lm], retain_graph=True)
    for a, b in zip(g_got, g_want):
        assert float(b.abs().max()) > 0.1 and float((a - b).abs().max()) < 1e-10
    if la != 0.0:
        # the unigram carries gradient: holding q fixed changes d lm by far more than the bound
        q = (torch.softmax(lm, -1).reshape(-1, 7).mean(0) + TINY).detach()
        joint = torch.log_softmax(am[:, :, None, :] + lm[:, None, :, :], -1)
        mix = (1.0 - ll - la) * joint + ll * torch.log_softmax(lm, -1)[:, None] \
            + la * torch.log_softmax(am + q.log(), -1)[:, :, None, :]
        frozen = torch.autograd.grad((wb * mix[..., blank]).sum(), [lm])[0]
        through = torch.autograd.grad((wb * want[0]).sum(), [lm])[0]
        assert float((frozen - through).abs().max()) > 1e-4


def test_scales_zero_are_rnnt_simple_planes(monkeypatch):
    from pika_amd import rnnt_simple_planes, rnnt_smoothed_planes
    am, lm, labels, _, _ = _case(0, seed=1)
    got = rnnt_smoothed_planes(am, lm, labels)
    # rnnt_simple_planes casts its inputs to float32: as it stands it agrees to float32 rounding of values of order 10 ...
    f32 = rnnt_simple_planes(am, lm, labels)
    assert f32[0].dtype == torch.float32
    assert (f32[1][:, :, 3] == torch.tensor(-1.0e30)).all() and (got[1][:, :, 3] == -1.0e30).all()
    for a, b in zip(got, f32):
        a, b = a.detach()[:, :, :3], b.detach()[:, :, :3].double()
        assert float((a - b).abs().max() / a.abs().max()) < 64 * torch.finfo(torch.float32).eps
    # ... and, with that cast taken out, its own spelling in float64 agrees to 1e-12
    monkeypatch.setattr(torch.Tensor, "float", lambda self: self)
    f64 = rnnt_simple_planes(am, lm, labels)
    monkeypatch.undo()
    assert f64[0].dtype == torch.float64
    for a, b in zip(got, f64):
        assert float((a - b).detach().abs().max()) < 1e-12


def test_cpu_float32_runs_the_spelling_and_the_loss_needs_a_device():
    from pika_amd import rnnt_loss_smoothed, rnnt_smoothed_planes
    am, lm, labels, _, _ = _case(0)
    got = rnnt_smoothed_planes(am.float(), lm.float(), labels, lm_only_scale=0.25)
    want = rnnt_smoothed_planes(am, lm, labels, lm_only_scale=0.25)
    assert got[0].dtype == torch.float32 and float((got[0].double() - want[0]).detach().abs().max()) < 1e-4
    lens = torch.tensor([5, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError):      # rnnt_loss_from_planes has no CPU path
        rnnt_loss_smoothed(am.float(), lm.float(), labels, lens, torch.tensor([3, 2], dtype=torch.int32))


def test_bad_scales_shapes_and_blank_raise_value_error():
    from pika_amd import rnnt_pruned_joint_loss_smoothed, rnnt_smoothed_planes
    am, lm, labels, _, _ = _case(0)
    for ll, la in ((-0.1, 0.0), (0.0, -0.1), (0.5, 0.5), (1.0, 0.0), (0.0, 1.5), (float("nan"), 0.0), ("x", 0.0)):
        with pytest.raises(ValueError):
            rnnt_smoothed_planes(am, lm, labels, lm_only_scale=ll, am_only_scale=la)
    with pytest.raises(ValueError):
        rnnt_pruned_joint_loss_smoothed(*[None] * 10, lm_only_scale=0.75, am_only_scale=0.25)
    for blank in (-1, 7):
        with pytest.raises(ValueError):
            rnnt_smoothed_planes(am, lm, labels, blank=blank)
    for a, b, y in ((am[0], lm, labels), (am, lm[:, :, :6], labels), (am[:1], lm, labels), (am, lm, labels[:, :2]),
                    (am, lm, labels[0]), (am, lm, labels.double())):
        with pytest.raises(ValueError):
            rnnt_smoothed_planes(a, b, y)
    with pytest.raises(ValueError):
        rnnt_smoothed_planes(torch.zeros(1, 2, 3), torch.zeros(1, 1026, 3), torch.zeros(1, 1025, dtype=torch.int32))
