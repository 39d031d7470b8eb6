"""The dense RNN-T gradient written over the one returned before (pika_amd.rnnt._dense_backward,
pika_rgrad_backward_fe): when the storage of the last gradient is owned by nobody else and unwritten since, the backward
clears its old non-zeros and stores the new ones instead of streaming the tensor.

Every call here is compared bit for bit (costs and gradient) with the same call run with PIKA_RNNT_GRAD_REUSE=0, the
streaming writer, and with the fp64 oracle at the tolerance of tests/test_rnnt_loss_gpu.py (costs 1e-5, gradients
|err| <= 1e-4 |g| + 1e-5).  Both references are computed once per configuration and shared.  Shapes: a few rows, V = 8
(the per-lane vector writer on the first call), V = 5 (V % 4 != 0: the scalar writer), V = 260 (V / 4 >= 64: the
scalar-metadata writer), ragged lengths with one utterance of no labels (helpers.make_case puts T_n = 1, U_n = 0 second).
"""
import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import make_case

pytestmark = pytest.mark.gpu

_REF = {}


def _case(B, T, U, V, seed, ragged=True, blank=0, label_is_blank=False):
    lp, y, tl, ul = make_case(B, T, U, V, seed, ragged=ragged, blank=blank)
    if label_is_blank:
        y[0, 0] = blank      # utterance 0 is full size: its first label column IS the blank column
    return lp, y, tl, ul


def _fastemit(g64, y, tl, ul, lam):
    g = g64.copy()
    for n in range(g.shape[0]):
        if ul[n]:
            u = np.arange(ul[n])
            g[n, :tl[n], u, y[n, u]] *= 1.0 + lam
    return g


def _call(dev, case, blank, lam, reduction, before_drop=None):
    """One loss + backward: (costs, gradient) as numpy, the gradient's data_ptr, and which path the backward took."""
    from pika_amd import rnnt as R
    lp, y, tl, ul = case
    x = torch.from_numpy(lp).to(dev).requires_grad_(True)
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (y, tl, ul)]
    before = dict(R.GRAD_REUSE_STATS)
    costs = R._RNNTLossFn.apply(x, *args, blank, lam)
    R._reduce(costs, args[1], False, reduction).backward()
    took = [k for k in ("reused", "full") if R.GRAD_REUSE_STATS[k] != before[k]]
    assert len(took) == 1 and R.GRAD_REUSE_STATS[took[0]] == before[took[0]] + 1
    out = (costs.detach().cpu().numpy(), x.grad.cpu().numpy(), x.grad.data_ptr(), took[0])
    if before_drop is not None:
        before_drop(x.grad)
    return out


def _references(dev, key, case, blank, lam, reduction, monkeypatch):
    """(costs, gradient) of the streaming writer (the switch off), and of the fp64 oracle; once per configuration."""
    if key not in _REF:
        monkeypatch.setenv("PIKA_RNNT_GRAD_REUSE", "0")
        c, g, _, took = _call(dev, case, blank, lam, reduction)
        assert took == "full"
        lp, y, tl, ul = case
        c64, g64 = O.rnnt_loss(lp, y, tl, ul, blank=blank)
        g64 = _fastemit(g64, y, tl, ul, lam)
        if reduction == "mean":
            g64 = g64 / lp.shape[0]
        for a in (c, g, c64, g64):
            a.setflags(write=False)
        _REF[key] = (c, g, c64, g64)
    return _REF[key]


def _check(got, ref):
    c, g = got[:2]
    c_off, g_off, c64, g64 = ref
    assert np.array_equal(c.view(np.uint32), c_off.view(np.uint32))
    assert np.array_equal(g.view(np.uint32), g_off.view(np.uint32)), "differs from the streaming writer in %d words" % int(
        (g.view(np.uint32) != g_off.view(np.uint32)).sum())
    assert np.allclose(c, c64, rtol=1e-5, atol=1e-5), (c, c64)
    err = np.abs(g - g64)
    assert not (err > 1e-4 * np.abs(g64) + 1e-5).any(), "max abs err %g" % float(err.max())


def _sequence(dev, monkeypatch, specs, want, before_drop=None):
    """Run the configurations `specs` (tuples of _case arguments, then blank, lambda, reduction) one after the other with
    the reuse on, from an empty retention; each is checked against its references; the paths taken must be `want`."""
    from pika_amd import rnnt as R
    cfgs = []
    for spec in specs:
        shape, (blank, lam, reduction) = spec[:-3], spec[-3:]
        case = _case(*shape, blank=blank, label_is_blank=blank != 0)
        cfgs.append((case, blank, lam, reduction, _references(dev, spec, case, blank, lam, reduction, monkeypatch)))
    monkeypatch.setenv("PIKA_RNNT_GRAD_REUSE", "1")
    R.release_grad_buffer()
    outs = []
    for (case, blank, lam, reduction, ref), path in zip(cfgs, want):
        out = _call(dev, case, blank, lam, reduction, before_drop)
        _check(out, ref)
        assert out[3] == path, (out[3], path)
        outs.append(out)
    return outs


PLAIN = (0, 0.0, "sum")


@pytest.mark.parametrize("V", [8, 5, 260])
def test_same_shape_other_labels_and_lengths(hip_device, monkeypatch, V):
    outs = _sequence(hip_device, monkeypatch, [(2, 5, 3, V, 31, False) + PLAIN, (2, 5, 3, V, 32, True) + PLAIN,
                                               (2, 5, 3, V, 33, True) + PLAIN], ["full", "reused", "reused"])
    assert outs[0][2] == outs[1][2] == outs[2][2]


def test_fewer_rows_then_the_rows_again_leave_nothing_stale(hip_device, monkeypatch):
    from pika_amd import rnnt as R

    def scan(grad):     # the whole retained buffer: the gradient just checked, then nothing but +0.0f words
        whole = R._retained[hip_device.index].alias.view(-1).view(torch.int32)
        assert whole.numel() == 2 * 5 * 4 * 8 and grad.data_ptr() == whole.data_ptr()
        assert not whole[grad.numel():].any()

    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False) + PLAIN, (1, 4, 2, 8, 34, False) + PLAIN,
                                        (2, 5, 3, 8, 32, True) + PLAIN, (3, 3, 1, 8, 35, True) + PLAIN],
              ["full", "reused", "reused", "reused"], before_drop=scan)


def test_more_rows_or_another_vocabulary_start_over(hip_device, monkeypatch):
    from pika_amd import rnnt as R
    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False) + PLAIN, (3, 5, 3, 8, 36, True) + PLAIN,
                                        (3, 5, 3, 260, 37, True) + PLAIN, (2, 5, 3, 8, 32, True) + PLAIN],
              ["full", "full", "full", "full"])
    rec = R._retained[hip_device.index]
    assert (rec.cap_rows, rec.rows, rec.V) == (40, 40, 8) and rec.alias.numel() == 320      # the old ones are gone


@pytest.mark.parametrize("how", ["tensor", "view"])
def test_a_gradient_still_referenced_is_left_alone(hip_device, monkeypatch, how):
    kept = []
    refs =[_references(hip_device, (2, 5, 3, 8, seed, True) + PLAIN, _case(2, 5, 3, 8, seed), 0, 0.0, "sum", monkeypatch)
            for seed in (32, 33)]
    monkeypatch.setenv("PIKA_RNNT_GRAD_REUSE", "1")
    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False) + PLAIN],
              ["full"], before_drop=lambda g: kept.append((g if how == "tensor" else g[1, 2:], g.clone())))
    out = _call(hip_device, _case(2, 5, 3, 8, 32), 0, 0.0, "sum")
    _check(out, refs[0])
    assert out[3] == "full"
    held, copy = kept[0]
    assert torch.equal(held, copy if how == "tensor" else copy[1, 2:])
    assert out[2] != held.untyped_storage().data_ptr()
    del kept[:], held                    # nobody holds the second gradient: the third call reuses it
    out = _call(hip_device, _case(2, 5, 3, 8, 33), 0, 0.0, "sum")
    _check(out, refs[1])
    assert out[3] == "reused"


def test_a_gradient_modified_in_place_is_not_trusted(hip_device, monkeypatch):
    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False) + PLAIN, (2, 5, 3, 8, 32, True) + PLAIN,
                                        (2, 5, 3, 8, 33, True) + PLAIN],
              ["full", "full", "full"], before_drop=lambda g: g.add_(1))


def test_the_in_place_log_softmax_backward_of_this_package_is_seen(hip_device, monkeypatch):
    """hipops.LogSoftmaxFn.backward rewrites the incoming gradient into d(logits) with a raw kernel and hands the same
    tensor on: it must bump the version counter, or the next backward would take that dense tensor for its own zeros."""
    from pika_amd import rnnt as R
    from pika_amd.model.hipops import LogSoftmaxFn
    rng = np.random.default_rng(50)
    _, y, tl, ul = _case(2, 5, 3, 8, 32)
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(hip_device) for a in (y, tl, ul)]
    logits = torch.from_numpy(rng.standard_normal((2, 5, 4, 8)).astype(np.float32)).to(hip_device)

    def dlogits():
        x = logits.clone().requires_grad_(True)
        before = dict(R.GRAD_REUSE_STATS)
        R.rnnt_loss(LogSoftmaxFn.apply(x * 1.0, 1.0), *args, reduction="sum").backward()
        return x.grad.cpu().numpy(), {k: R.GRAD_REUSE_STATS[k] - before[k] for k in before}

    monkeypatch.setenv("PIKA_RNNT_GRAD_REUSE", "0")
    want = [dlogits()[0] for _ in range(2)]
    assert np.array_equal(want[0], want[1])
    monkeypatch.setenv("PIKA_RNNT_GRAD_REUSE", "1")
    R.release_grad_buffer()
    for _ in range(3):
        got, took = dlogits()
        assert took == {"reused": 0, "full": 1}
        assert np.array_equal(got.view(np.uint32), want[0].view(np.uint32))


def test_another_blank_and_a_label_equal_to_blank(hip_device, monkeypatch):
    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False) + PLAIN, (2, 5, 3, 8, 38, True, 3, 0.0, "sum"),
                                        (2, 5, 3, 8, 39, True, 5, 0.0, "sum"), (2, 5, 3, 8, 32, True) + PLAIN],
              ["full", "reused", "reused", "reused"])


def test_fastemit_and_mean_reduction(hip_device, monkeypatch):
    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False, 0, 0.01, "mean"), (2, 5, 3, 8, 32, True, 0, 0.01, "mean"),
                                        (2, 5, 3, 260, 40, True, 0, 0.01, "mean"), (2, 5, 3, 260, 41, True, 0, 0.01, "mean")],
              ["full", "reused", "full", "reused"])


def test_another_stream_starts_over(hip_device, monkeypatch):
    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False) + PLAIN], ["full"])
    ref = _references(hip_device, (2, 5, 3, 8, 32, True) + PLAIN, _case(2, 5, 3, 8, 32), 0, 0.0, "sum", monkeypatch)
    monkeypatch.setenv("PIKA_RNNT_GRAD_REUSE", "1")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=hip_device)
    with torch.cuda.stream(side):
        first = _call(hip_device, _case(2, 5, 3, 8, 32), 0, 0.0, "sum")
        second = _call(hip_device, _case(2, 5, 3, 8, 32), 0, 0.0, "sum")
    torch.cuda.synchronize()
    _check(first, ref)
    _check(second, ref)
    assert (first[3], second[3]) == ("full", "reused")      # the side stream's own buffer serves the side stream
    back = _call(hip_device, _case(2, 5, 3, 8, 32), 0, 0.0, "sum")
    _check(back, ref)
    assert back[3] == "full"


def test_switched_off_never_reuses(hip_device, monkeypatch):
    from pika_amd import rnnt as R
    _sequence(hip_device, monkeypatch, [(2, 5, 3, 8, 31, False) + PLAIN], ["full"])
    assert hip_device.index in R._retained
    monkeypatch.setenv("PIKA_RNNT_GRAD_REUSE", "0")
    ref = _references(hip_device, (2, 5, 3, 8, 32, True) + PLAIN, _case(2, 5, 3, 8, 32), 0, 0.0, "sum", monkeypatch)
    for _ in range(2):
        out = _call(hip_device, _case(2, 5, 3, 8, 32), 0, 0.0, "sum")
        _check(out, ref)
        assert out[3] == "full"
    assert not R._retained                                   # and nothing stays allocated
