"""The float64 oracle and the arithmetic model of the training LSTM recurrence (tests/lstm_common.py), on the CPU:

* the oracle IS nn.LSTM in float64: output, final states and, through dgates, every autograd gradient;
* for every case of the GPU table (tests/test_lstm_recurrence_gpu.py) the bound the kernels are held to,
  max(4 * e_model, floor), stays inside 2e-5 * max(1, max |oracle|) -- the GPU bound cannot hide a failure -- and the floor
  decides no case with a recurrent step;
* every mutant of the model (one cross term lost, one bf16 term of W_hh, gates in another order, cell gradient not
  carried, the wrong cell in the forget-gate gradient) is at least 10x outside that bound on some tensor the GPU test
  looks at, in every case with S >= 2: a kernel wrong in that way fails there."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_common as LC  # noqa: E402

NAMES = ("out", "gates", "cells", "dgates")


def test_oracle_is_nn_lstm_in_float64():
    B, S, E, H = 5, 9, 40, 256
    torch.manual_seed(11)
    ref = torch.nn.LSTM(E, H, 1, batch_first=True).double()
    x = torch.randn(B, S, E, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, S, H, dtype=torch.float64)
    want, (h_n, c_n) = ref(x)
    want.backward(dy)
    want = want.detach()
    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0))
    xd = x.detach()
    out, gates, cells = LC.forward(xd @ w_ih.t() + b_ih + b_hh, w_hh)
    assert out.dtype == torch.float64
    assert LC.err(out, want) < 1e-15 and LC.err(out[:, -1], h_n[0]) < 1e-15 and LC.err(cells[:, -1], c_n[0]) < 1e-14
    dg = LC.backward(dy, w_hh, gates, cells)
    d2, x2 = dg.reshape(B * S, 4 * H), xd.reshape(B * S, E)
    hprev = torch.zeros_like(out)
    hprev[:, 1:] = out[:, :-1]
    got = {"weight_ih_l0": d2.t() @ x2, "weight_hh_l0": d2.t() @ hprev.reshape(B * S, H), "bias_ih_l0": d2.sum(0),
           "bias_hh_l0": d2.sum(0)}
    for n, p in ref.named_parameters():
        e = LC.err(got[n], p.grad) / LC.scale(p.grad)
        print("%s: %.1e" % (n, e))
        assert e < 1e-13, (n, e)
    assert LC.err(dg @ w_ih, x.grad) / LC.scale(x.grad) < 1e-13


@functools.lru_cache(maxsize=None)
def _case(case):
    """Oracle and model of a case; the backward of both on the MODEL's gates and cells (the GPU test hands both the
    kernel's), and end to end."""
    B, S, H, gain, sat = LC.resolve(case)
    gx, w, dy = LC.inputs(B, S, H, gain, sat)
    want = dict(zip(NAMES, LC.forward(gx, w)))
    got = dict(zip(NAMES, LC.forward(gx, w, LC.MODEL)))
    want["dgates"] = LC.backward(dy, w, got["gates"], got["cells"])
    got["dgates"] = LC.backward(dy, w, got["gates"], got["cells"], LC.MODEL)
    want["dgates_e2e"] = LC.backward(dy, w, want["gates"], want["cells"])
    e_model = {n: LC.err(got[n], want[n]) for n in NAMES}
    e_model["dgates_e2e"] = LC.err(got["dgates"], want["dgates_e2e"])
    return (gx, w, dy), want, got, e_model


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_gpu_bound_is_inside_the_two_term_bound(case):
    B, S, H, gain, sat = LC.resolve(case)
    _, want, _, e_model = _case(case)
    for n, e in e_model.items():
        s = LC.scale(want[n])
        print("%-10s e_model %.2e  4*e_model/scale %.2e  over floor %.1f" % (n, e, LC.MARGIN * e / s, LC.MARGIN * e / (LC.FLOOR * s)))
        assert all(bool(torch.isfinite(t).all()) for t in (want[n],))
        assert LC.MARGIN * e <= LC.CEILING * s, (n, e, s)
        if S >= 2 and not sat:
            assert LC.MARGIN * e >= LC.FLOOR * s, ("the floor would decide this case", n, e, s)
    if S == 1:      # no recurrent product: the model is the oracle but for fp32 rounding
        assert max(e_model[n] / LC.scale(want[n]) for n in NAMES) < 4 * 2.0 ** -24


@pytest.mark.parametrize("mutant", LC.MUTANTS)
@pytest.mark.parametrize("case", [c for c in LC.CASES if c[1] != 1], ids=LC.case_id)
def test_every_mutant_is_ten_times_outside_the_gpu_bound(case, mutant):
    (gx, w, dy), want, got, e_model = _case(case)
    ratios = {}
    if mutant in LC.FORWARD_MUTANTS:
        bad = dict(zip(NAMES, LC.forward(gx, w, mutant)))
        for n in NAMES[:3]:
            ratios[n] = LC.err(bad[n], want[n]) / LC.bound(e_model[n], want[n])
    # the backward as the GPU test runs it: on the gates and cells a correct forward left
    bad_dg = LC.backward(dy, w, got["gates"], got["cells"], mutant)
    ratios["dgates"] = LC.err(bad_dg, want["dgates"]) / LC.bound(e_model["dgates"], want["dgates"])
    print(mutant, " ".join("%s %.0fx" % kv for kv in ratios.items()))
    assert max(ratios.values()) >= 10.0, ratios
    # every mutant changes the backward too: caught by the backward's own comparison, not only through the forward
    assert ratios["dgates"] >= 10.0, ratios
