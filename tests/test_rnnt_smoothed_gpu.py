"""The smoothed simple planes on the GPU (csrc/rnnt_simple.hip) against the plain-torch spelling in float64 on the same
inputs: planes and both gradients at the edges of the 64-wide tiles, the loss on top, determinism, guarded outputs, graph
capture and the end-to-end chain.

The bound is relative, as in tests/test_joint_banded_gpu.py: the yardstick is the same torch spelling run in float32 on the
device (at scales (0, 0) that is rnnt_simple_planes' arithmetic); errors are max-abs over the max-abs of the float64 value,
per tensor, and the kernels may be at most twice as far from float64 as the yardstick is.  Every case shifts whole rows of
am and lm by +-80, so the yardstick's float32 rounding is that of values near 80, never a few ulps of nothing."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rnnt_pruned_common as P  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = [(0.0, 0.0), (0.25, 0.0), (0.0, 0.3), (0.25, 0.3)]
# (B, T, U, V): U = 0 and one frame; odd sizes under one tile; T over a tile; U + 1 = 65 over a tile; several tiles on
# every axis, none divisible (the V chunk is 64 columns, so V = 1031 is 17 chunks)
SHAPES = [(1, 1, 0, 5), (3, 7, 1, 37), (2, 67, 5, 130), (2, 33, 64, 257), (1, 130, 129, 1031)]
BLANK_LAST = (2, 67, 5, 130)       # the case that runs with blank = V - 1
GUARD = 64


def _inputs(shape, blank, seed=0):
    B, T, U, V = shape
    g = torch.Generator().manual_seed(seed + 17 * T + V)
    am, lm = torch.randn(B, T, V, generator=g) * 2.0, torch.randn(B, U + 1, V, generator=g) * 2.0
    am += 80.0 * torch.randint(-1, 2, (B, T, 1), generator=g)
    lm += 80.0 * torch.randint(-1, 2, (B, U + 1, 1), generator=g)
    if abs(float(am[0, 0].mean())) < 40.0:                     # at least one shifted row in the smallest case
        am[0, 0] += 80.0
    y = torch.randint(0, V, (B, U), generator=g).int()
    if U >= 1:
        y[0, 0] = blank                                        # a label equal to blank
    if U >= 3:
        y[:, 2] = y[:, 1]                                      # repeated labels inside every utterance
    if U >= 5:
        y[-1, 4] = V + 3                                       # padding label, clamped to V - 1
    wb, wl = torch.randn(B, T, U + 1, generator=g), torch.randn(B, T, U + 1, generator=g)
    wl[:, :, U] = 0.0
    return am, lm, y, wb, wl


def _run(fn, am, lm, y, wb, wl, blank, ll, la):
    am, lm = am.clone().requires_grad_(True), lm.clone().requires_grad_(True)
    bl, lb = fn(am, lm, y, blank, ll, la)
    d_am, d_lm = torch.autograd.grad((wb.to(bl.dtype) * bl).sum() + (wl.to(bl.dtype) * lb).sum(), [am, lm])
    return bl.detach(), lb.detach(), d_am, d_lm


def _errors(got, want):
    U = want[0].shape[2] - 1
    assert bool((got[1][:, :, U] == torch.tensor(-1.0e30, dtype=got[1].dtype)).all())
    out = []
    for k, (a, w) in enumerate(zip(got, want)):
        if k == 1:
            a, w = a[:, :, :U], w[:, :, :U]
        if w.numel() == 0:
            out.append(0.0)
            continue
        assert bool(torch.isfinite(a).all())
        out.append(float((a.double() - w).abs().max()) / float(w.abs().max()))
    return out


def _parity(tag, shape, blank, ll, la, dev):
    from pika_amd import rnnt
    am, lm, y, wb, wl = [t.to(dev) for t in _inputs(shape, blank)]
    want = _run(rnnt._smoothed_planes_torch, am.double(), lm.double(), y, wb, wl, blank, ll, la)
    yard = _run(rnnt._smoothed_planes_torch, am, lm, y, wb, wl, blank, ll, la)
    got = _run(rnnt.rnnt_smoothed_planes, am, lm, y, wb, wl, blank, ll, la)
    assert got[0].dtype == torch.float32 and got[2].shape == am.shape and got[3].shape == lm.shape
    ek, ey = _errors(got, want), _errors(yard, want)
    for name, k, r in zip(("blank_lp", "label_lp", "d_am", "d_lm"), ek, ey):
        print("RNNTSMOOTHED %-7s (B,T,U,V)=%-18s blank %4d scales (%.2f, %.2f) %-8s kernel %.3g yardstick %.3g" % (
            tag, shape, blank, ll, la, name, k, r))
    return ek, ey


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_planes_and_gradients_against_float64(hip_device, shape, scales):
    blank = shape[3] - 1 if shape == BLANK_LAST else 0
    ek, ey = _parity("parity", shape, blank, scales[0], scales[1], hip_device)
    for k, r in zip(ek, ey):
        assert k <= 2 * r, (ek, ey)


def _loss_case(dev):
    B, T, U, V = 3, 20, 6, 16
    am, lm, y, _, _ = [t.to(dev) for t in _inputs((B, T, U, V), 0, seed=5)]
    tl = torch.tensor([20, 11, 14], dtype=torch.int32, device=dev)
    ul = torch.tensor([6, 2, 4], dtype=torch.int32, device=dev)
    return am, lm, y, tl, ul


@pytest.mark.parametrize("scales", [(0.0, 0.0), (0.25, 0.3)])
def test_loss_smoothed_is_the_planes_loss_of_the_float64_planes(hip_device, scales):
    from pika_amd import rnnt, rnnt_loss_from_planes, rnnt_loss_smoothed
    ll, la = scales
    am0, lm0, y, tl, ul = _loss_case(hip_device)

    def chain(planes, dtype):
        am, lm = am0.to(dtype).requires_grad_(True), lm0.to(dtype).requires_grad_(True)
        bl, lb = planes(am, lm)
        costs, ob, ol = rnnt_loss_from_planes(bl.float(), lb.float(), tl, ul, return_occupancy=True)
        return [costs.detach(), ob, ol] + list(torch.autograd.grad(costs.sum(), [am, lm]))
    want = chain(lambda a, b: rnnt._smoothed_planes_torch(a, b, y, 0, ll, la), torch.float64)
    yard = chain(lambda a, b: rnnt._smoothed_planes_torch(a, b, y, 0, ll, la), torch.float32)
    am, lm = am0.clone().requires_grad_(True), lm0.clone().requires_grad_(True)
    costs, ob, ol = rnnt_loss_smoothed(am, lm, y, tl, ul, lm_only_scale=ll, am_only_scale=la, return_occupancy=True)
    got = [costs.detach(), ob, ol] + list(torch.autograd.grad(costs.sum(), [am, lm]))
    assert costs.shape == (3,) and ob.shape == ol.shape == (3, 20, 7) and not ob.requires_grad
    for name, a, r, w in zip(("costs", "blank_occ", "label_occ", "d_am", "d_lm"), got, yard, want):
        scale = float(w.abs().max())
        ek, ey = float((a.double() - w.double()).abs().max()) / scale, float((r.double() - w.double()).abs().max()) / scale
        print("RNNTSMOOTHED loss    scales (%.2f, %.2f) %-9s kernel %.3g yardstick %.3g" % (ll, la, name, ek, ey))
        assert ek <= 2 * ey, (name, ek, ey)
    # reductions are rnnt_loss_from_planes'
    total = rnnt_loss_smoothed(am0, lm0, y, tl, ul, lm_only_scale=ll, am_only_scale=la, reduction="sum")
    assert torch.equal(total, costs.detach().sum())


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_two_calls_are_bit_identical(hip_device):
    from pika_amd import rnnt
    shape = (2, 67, 5, 130)
    am, lm, y, wb, wl = [t.to(hip_device) for t in _inputs(shape, 0)]
    y[:, :] = y[:, :1]                                          # every label of an utterance the same ...
    y[1, :] = 0                                                 # ... and, in one of them, equal to blank
    a = _run(rnnt.rnnt_smoothed_planes, am, lm, y, wb, wl, 0, 0.25, 0.3)
    b = _run(rnnt.rnnt_smoothed_planes, am, lm, y, wb, wl, 0, 0.25, 0.3)
    for s, t in zip(a, b):
        assert torch.equal(_bits(s), _bits(t))
    # and the repeated labels add up: d_am against float64 within the parity bound
    want = _run(rnnt._smoothed_planes_torch, am.double(), lm.double(), y, wb, wl, 0, 0.25, 0.3)
    yard = _run(rnnt._smoothed_planes_torch, am, lm, y, wb, wl, 0, 0.25, 0.3)
    for k, r in zip(_errors(a, want), _errors(yard, want)):
        assert k <= 2 * r


class _GuardedTorch(object):
    """`torch` for pika_amd.rnnt, except that every tensor it allocates uninitialised -- all the kernels' outputs -- is
    carved out of a larger buffer with GUARD sentinel elements on each side."""
    SENTINEL = 12345.0

    def __init__(self):
        self.buffers = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None):
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (shape,)
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), self.SENTINEL, dtype=dtype, device=device)
        self.buffers.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def empty_like(self, t):
        return self.empty(t.shape, dtype=t.dtype, device=t.device)


@pytest.mark.parametrize("shape", [(3, 7, 1, 37), (1, 130, 129, 1031)])
def test_outputs_stay_inside_their_buffers(hip_device, shape, monkeypatch):
    from pika_amd import rnnt
    am, lm, y, wb, wl = [t.to(hip_device) for t in _inputs(shape, 0)]
    plain = _run(rnnt.rnnt_smoothed_planes, am, lm, y, wb, wl, 0, 0.25, 0.3)
    guarded = _GuardedTorch()
    monkeypatch.setattr(rnnt, "torch", guarded)
    got = _run(rnnt.rnnt_smoothed_planes, am, lm, y, wb, wl, 0, 0.25, 0.3)
    monkeypatch.undo()
    torch.cuda.synchronize()
    # amax, gathered, sums, blank_lp, label_lp; w, d_am, m
    assert len(guarded.buffers) == 8
    for buf, n in guarded.buffers:
        assert bool((buf[:GUARD] == guarded.SENTINEL).all()) and bool((buf[GUARD + n:] == guarded.SENTINEL).all())
        assert not bool((buf[GUARD:GUARD + n] == guarded.SENTINEL).any())      # and every element was written
    for s, t in zip(plain, got):
        assert torch.equal(_bits(s), _bits(t))


# ---- the chain: tests/test_joint_banded_gpu.py's end-to-end shape ------------------------------------------------------
E2E = dict(B=3, T=20, U=6, H=64, V=16, S=3, tl=[20, 11, 14], ul=[6, 2, 4])


def _e2e_inputs(seed):
    B, T, U, H, V = (E2E[k] for k in "BTUHV")
    g = torch.Generator().manual_seed(seed)
    enc, pred = torch.randn(B, T, H, generator=g), torch.randn(B, U + 1, H, generator=g)
    y = torch.randint(1, V, (B, U), generator=g).int()
    tl, ul = torch.tensor(E2E["tl"], dtype=torch.int32), torch.tensor(E2E["ul"], dtype=torch.int32)
    for n in range(B):
        y[n, int(ul[n]):] = V
    return enc, pred, y, tl, ul


def _layers(dev, seed):
    H, V = E2E["H"], E2E["V"]
    torch.manual_seed(seed)
    layers = [torch.nn.Linear(i, o).to(dev) for i, o in [(2 * H, H), (2 * H, H), (H, V), (H, V), (H, V)]]
    with torch.no_grad():
        layers[3].bias += 80.0           # the simple joiner's logits sit near 80: the yardstick's float32 rounding is real
    return layers


def _params(layers):
    return [p for m in layers for p in (m.weight, m.bias)]


def test_pruned_joint_loss_smoothed_end_to_end(hip_device):
    from pika_amd import rnnt, rnnt_loss_from_planes, rnnt_pruned_joint_loss, rnnt_pruned_joint_loss_smoothed
    from pika_amd.model import ops
    dev = hip_device
    S = E2E["S"]
    layers = _layers(dev, 2)
    sam, slm = layers[3:]
    enc0, pred0, y, tl, ul = _e2e_inputs(11)
    yd, tld, uld = y.to(dev), tl.to(dev), ul.to(dev)
    enc, pred = enc0.to(dev).requires_grad_(True), pred0.to(dev).requires_grad_(True)
    simple, pruned, ranges = rnnt_pruned_joint_loss_smoothed(enc, pred, yd, tld, uld, *layers, s_range=S, reduction=None)
    assert ranges.dtype == torch.int32 and ranges.shape == (E2E["B"], E2E["T"]) and not ranges.requires_grad
    assert simple.shape == pruned.shape == (E2E["B"],)
    r = ranges.cpu().numpy()
    for n in range(E2E["B"]):
        assert P.is_valid(r[n], int(tl[n]), int(ul[n]), S)
    # the simple loss against the float64 planes on the same am / lm; the yardstick is rnnt_pruned_joint_loss's
    parent, _, _ = rnnt_pruned_joint_loss(enc, pred, yd, tld, uld, *layers, s_range=S, reduction=None)
    with torch.no_grad():
        am, lm = ops.linear(enc, sam.weight, sam.bias), ops.linear(pred, slm.weight, slm.bias)
        bl, lb = rnnt._smoothed_planes_torch(am.double(), lm.double(), yd, 0, 0.0, 0.0)
        want = rnnt_loss_from_planes(bl.float(), lb.float(), tld, uld).double()
    ek = float((simple.detach().double() - want).abs().max() / want.abs().max())
    ey = float((parent.detach().double() - want).abs().max() / want.abs().max())
    print("RNNTSMOOTHED e2e     simple loss: kernel %.3g yardstick %.3g" % (ek, ey))
    assert ek <= 2 * ey, (ek, ey)
    # the pruned loss does not reach the simple joiner; the simple loss does
    assert all(g is None for g in torch.autograd.grad(pruned.sum(), _params(layers[3:]), retain_graph=True, allow_unused=True))
    assert all(g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
               for g in torch.autograd.grad(simple.sum(), _params(layers[3:]), retain_graph=True))
    smooth, _, _ = rnnt_pruned_joint_loss_smoothed(enc, pred, yd, tld, uld, *layers, s_range=S, reduction=None,
                                                   lm_only_scale=0.25)
    assert float((smooth.detach() - simple.detach()).abs().min()) > 1e-3 * float(simple.detach().abs().max())


def test_pruned_joint_loss_smoothed_captures_into_one_graph(hip_device):
    """Forward plus backward at scales (0.25, 0) in one torch.cuda.graph, replayed on new data and new labels: losses,
    ranges and every gradient equal the eager call bit for bit."""
    from pika_amd import rnnt_pruned_joint_loss_smoothed
    dev = hip_device
    layers = _layers(dev, 3)
    params = _params(layers)

    def run(stat):
        s, p, r = rnnt_pruned_joint_loss_smoothed(*stat, *layers, s_range=E2E["S"], fastemit_lambda=0.25, lm_only_scale=0.25)
        return s, p, r, torch.autograd.grad(0.5 * s + p, stat[:2] + params)

    stat = [t.to(dev) for t in _e2e_inputs(20)]
    stat[0].requires_grad_(True)
    stat[1].requires_grad_(True)
    run(stat)                                                  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gs, gp, gr, gg = run(stat)
    torch.cuda.current_stream().wait_stream(side)
    for seed in (21, 22):
        with torch.no_grad():
            for dst, src in zip(stat, _e2e_inputs(seed)):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        es, ep, er, eg = run(stat)
        assert torch.equal(gs.detach(), es.detach()) and torch.equal(gp.detach(), ep.detach()) and torch.equal(gr, er)
        for a, b in zip(gg, eg):
            assert torch.equal(_bits(a), _bits(b))
