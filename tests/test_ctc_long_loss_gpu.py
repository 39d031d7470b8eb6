"""GPU checks of the long-form loss (pika_amd.ctc.ctc_long_loss*, csrc/ctc_long_loss.hip) against the float64 reference of
tests/ctc_common.py, at the smallest shapes at which the tiling can go wrong: with W = LONG_LOSS_TILE and F =
LONG_LOSS_FRAMES, state axes S = 2U+1 around W and 2W, lengths T_b around F and 2F, repeated labels on every tile and halo
boundary.

Bounds.  Costs relative, capped at 1e-3; gradients absolute; the floor is 1e-6.
* U <= 511: the yardstick is the existing `ctc_loss` on the same input and device.  The tiled path's error against float64
  is at most max((F/8) * err_existing, 1e-6): F/8 is the ratio of frames between two renormalisations, 64 against 8, and
  with it of the ulps of the fp32 state values.
* U > 511: the yardstick is torch's fp32 CPU kernel, as in tests/test_ctc_gpu.py: 4 * err_fp32.
Every figure is printed (`CTCPARITY ...`) before it is asserted, and every comparison asserts how many elements it
compared; profiles/ctc_long_loss_parity.txt keeps the output.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import test_ctc_gpu as G  # noqa: E402  (Case, bounds, rand_seq, repeats: the cases and the fp32 yardstick of the loss)

pytestmark = pytest.mark.gpu

W, F = 896, 64      # checked against the exported constants in _geometry()


def _geometry():
    from pika_amd import ctc
    assert (ctc.LONG_LOSS_TILE, ctc.LONG_LOSS_FRAMES) == (W, F)


def run(case, dev, logits_form, fn=None, x_cpu=None, targets=None, lengths_on_device=False, **kw):
    """(costs, gradient) through a public function, as float64 CPU tensors; default: the tiled path, called directly."""
    from pika_amd import ctc
    fn = fn or (ctc.ctc_long_loss_from_logits if logits_form else ctc.ctc_long_loss)
    x = (case.logits if logits_form else case.lp32()) if x_cpu is None else x_cpu
    x = x.to(dev).requires_grad_(True) if x.device.type == "cpu" else x.requires_grad_(True)
    il, tl = case.lens()
    if lengths_on_device:
        il, tl = il.to(dev), tl.to(dev)
    costs = fn(x, case.targets() if targets is None else targets, il, tl, blank=case.blank, reduction="none", **kw)
    gc = torch.ones(case.B) if case.gc is None else case.gc
    (grad,) = torch.autograd.grad((costs * gc.to(dev)).sum(), x)
    return costs.detach().double().cpu(), grad.double().cpu()


def errors(case, costs, grad, gref):
    c64 = case.ref()[0][0]
    assert costs.numel() == case.B and grad.numel() == case.T * case.B * case.C == gref.numel()
    return float(((costs - c64).abs() / c64.abs().clamp(min=1e-30)).max()), float((grad - gref).abs().max())


def bounds_for(case, dev, logits_form, tight=None):
    """(cost bound, gradient bound, what it is) for one form.  tight: held to the existing `ctc_loss` on the same input and
    device (default: whenever it can run, U <= 511); otherwise to torch's fp32 CPU kernel."""
    from pika_amd import ctc
    (c64, dx64, dl64), _ = case.ref()
    umax = max(len(s) for s in case.seqs)
    tight = umax <= 511 if tight is None else tight
    assert not tight or umax <= 511
    if not tight:
        loose = G.bounds(case)
        return loose[0], loose[1 if logits_form else 2], "4 x torch fp32"
    e_cost, e_grad = errors(case, *run(case, dev, logits_form, fn=ctc.ctc_loss_from_logits if logits_form else ctc.ctc_loss),
                            dx64 if logits_form else dl64)
    return min(max(F / 8 * e_cost, 1e-6), 1e-3), max(F / 8 * e_grad, 1e-6), "%d x ctc_loss" % (F // 8)


def check(case, dev, tight=None, **kw):
    """Both forms of the tiled path against float64."""
    _geometry()
    (c64, dx64, dl64), _ = case.ref()
    for logits_form, gref in ((False, dl64), (True, dx64)):
        b_cost, b_g, kind = bounds_for(case, dev, logits_form, tight)
        costs, grad = run(case, dev, logits_form, **kw)
        e_cost, e_grad = errors(case, costs, grad, gref)
        print("CTCPARITY long %-20s %-9s cost rel err %.3g (bound %.3g)  grad abs err %.3g (bound %.3g)  [%s]" % (
            case.name, "logits" if logits_form else "log_probs", e_cost, b_cost, e_grad, b_g, kind))
        assert torch.isfinite(grad).all()
        assert e_cost <= b_cost, (case.name, logits_form, e_cost, b_cost)
        assert e_grad <= b_g, (case.name, logits_form, e_grad, b_g)
        dead = torch.arange(case.T)[:, None] >= torch.tensor(case.ils)[None, :]
        assert int(dead.sum()) == sum(case.T - t for t in case.ils)
        assert (grad[dead] == 0).all(), "gradient beyond T_b must be exactly zero"


def tile_case(U, roomy, C=6):
    """Two utterances, the longer with S = 2U+1 on a tile edge; T = U + repeats + 3 (tight: most cells impossible) or about
    1.5 U; a ragged batch, weights that include 0 and a negative one over the two variants."""
    seqs = [G.rand_seq(U, C, 0, 7 * U + 1), G.rand_seq(max(U - 37, 0), C, 0, 7 * U + 2)]
    T = (3 * U) // 2 + 5 if roomy else max(len(s) + G.repeats(s) for s in seqs) + 3
    return G.Case("S%d_%s" % (2 * U + 1, "roomy" if roomy else "tight"), T, C, seqs, ils=[T, T - 5], seed=U + int(roomy),
                  gc=[1.5, 0.0] if roomy else [-0.75, 2.0])


TILE_EDGES = [tile_case(U, roomy) for U in ((W - 2) // 2, W // 2, 511, W - 1, W, W + 1) for roomy in (False, True)]


@pytest.mark.parametrize("case", TILE_EDGES, ids=lambda c: c.name)
def test_tile_edges_against_float64(hip_device, case):
    assert 2 * len(case.seqs[0]) + 1 in (W - 1, W + 1, 1023, 2 * W - 1, 2 * W + 1, 2 * W + 3)
    check(case, hip_device)


FRAME_EDGES = [G.Case("Tb_%d_%d_%d" % tuple(ils), max(ils), 5, [G.rand_seq(U, 5, 0, 90 + ils[0] + i) for i, U in enumerate(Us)],
                      ils=ils, seed=ils[0], gc=[1.0, -0.5, 0.0])
               for ils, Us in (([F - 1, F, F + 1], [20, 3, 0]), ([2 * F - 1, 2 * F, 2 * F + 1], [40, 1, 17]),
                               ([2 * F + 1, F, 1], [9, 30, 0]))]


@pytest.mark.parametrize("case", FRAME_EDGES, ids=lambda c: c.name)
def test_frame_block_edges_with_beta_starting_mid_block(hip_device, case):
    check(case, hip_device)


def test_skip_rule_across_tile_and_halo_boundaries(hip_device):
    # a repeated label on both sides of every tile boundary (states k W -+ 1) and of every halo boundary (k W - 2F for
    # alpha, k W + 2F for beta): whether the transition over the blank between them is allowed takes a label that the
    # neighbouring tile owns.  Everywhere else neighbours differ, so every other skip is allowed.
    U, C = W + 104, 7
    seq = [1 + (u % (C - 1)) for u in range(U)]
    edges = [k * W + d for k in (1, 2) for d in (0, -2 * F, 2 * F)]
    pairs = sorted((e - 2) // 2 for e in edges)     # labels (e-2)/2 and e/2 sit at the states e - 1 and e + 1
    assert len(pairs) == 6 and pairs == [383, 447, 511, 831, 895, 959]
    for u in pairs:
        seq[u + 1] = seq[u]
        assert seq[u + 2] != seq[u + 1] and seq[u - 1] != seq[u]
    other = [1 + (u % (C - 1)) for u in range(300)]
    T = 1200
    case = G.Case("skip_edges", T, C, [seq, other], ils=[T - 3, T], seed=77, gc=[1.0, -2.0])
    check(case, hip_device)


def test_blank_last_odd_classes_offset_pointer_and_strides(hip_device):
    dev = hip_device
    U = W // 2 + 3
    # blank = C - 1, C % 4 != 0
    seqs = [G.rand_seq(U, 7, 6, 5), G.rand_seq(11, 7, 6, 6)]
    check(G.Case("blank_last_C7", 700, 7, seqs, ils=[700, 650], blank=6, seed=31, gc=[0.5, 2.0]), dev, tight=True)
    # C % 4 == 0 with the base pointer 4 bytes off 16-byte alignment: the scalar path of every row, same values
    case = G.Case("offset_pointer_C8", 300, 8, [G.rand_seq(60, 8, 0, 7), G.rand_seq(3, 8, 0, 8)], ils=[300, 130], seed=32)
    for logits_form in (False, True):
        x = case.logits if logits_form else case.lp32()
        flat = torch.empty(x.numel() + 1, device=dev)
        flat[1:].copy_(x.reshape(-1).to(dev))
        off = flat[1:].view(x.shape)
        assert off.data_ptr() % 16 == 4
        a, b = run(case, dev, logits_form), run(case, dev, logits_form, x_cpu=off.detach())
        assert a[1].numel() == 300 * 2 * 8 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check(case, dev)
    # x read through its outer strides: batch-major storage, and rows padded to a wider class axis
    for logits_form in (False, True):
        x = (case.logits if logits_form else case.lp32()).to(dev)
        want = run(case, dev, logits_form)
        wide = torch.full((300, 2, 13), float("nan"), device=dev)
        wide[:, :, :8] = x
        for view in (x.transpose(0, 1).contiguous().transpose(0, 1), wide[:, :, :8]):
            assert not view.is_contiguous()
            got = run(case, dev, logits_form, x_cpu=view.detach())
            assert got[1].numel() == 300 * 2 * 8 and torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


def test_direct_calls_with_zero_and_one_label(hip_device):
    check(G.Case("Umax0", F + 3, 5, [[], []], ils=[F + 3, 2], seed=41, gc=[1.0, 3.0]), hip_device)
    check(G.Case("Umax1", 2 * F + 1, 5, [[2], []], ils=[2 * F + 1, F], seed=42, gc=[-1.0, 0.5]), hip_device)
    check(G.Case("Umax1_T1", 1, 4, [[3], []], seed=43), hip_device)


def test_padding_frames_and_padded_labels_change_nothing(hip_device):
    U = W // 2 + 20
    case = G.Case("padding", 760, 6, [G.rand_seq(U, 6, 0, 51), G.rand_seq(100, 6, 0, 52), []], ils=[760, 400, 70], seed=51,
                  gc=[1.0, 2.0, -1.0])
    il = torch.tensor(case.ils)
    dead = torch.arange(case.T)[:, None] >= il[None, :]
    tg = case.targets()
    for n, s in enumerate(case.seqs):       # labels beyond U_b: out of range on both sides
        tg[n, len(s):] = 2 ** 31 - 1 if n % 2 else -7
    for logits_form in (False, True):
        x = (case.logits if logits_form else case.lp32()).clone()
        clean = run(case, hip_device, logits_form)
        x[dead] = float("nan")
        dirty = run(case, hip_device, logits_form, x_cpu=x, targets=tg, lengths_on_device=True)
        assert dirty[1].numel() == 760 * 3 * 6
        assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])


def test_infeasible_utterances_beside_feasible_ones(hip_device):
    from pika_amd import ctc
    dev = hip_device
    U, C, T = W // 2 + 10, 6, 700
    good = G.rand_seq(U, C, 0, 61)
    ref_case = G.Case("infeasible_neighbour", T, C, [good], seed=61, gc=[1.5])
    (c64, dx64, dl64), _ = ref_case.ref()
    weights = torch.tensor([1.5, 2.0], device=dev)
    long_rep = [1] * 400                                     # 400 labels, 399 repeats: needs 799 frames
    bad_high, bad_low = list(good[:50]), list(good[:50])
    bad_high[20], bad_low[49] = C, -1
    for name, bad in (("too_short", long_rep), ("label_C", bad_high), ("label_-1", bad_low)):
        tg = R.pad_targets([good, bad])
        il, tl = torch.tensor([T, T]), torch.tensor([U, len(bad)])
        for logits_form, gref in ((False, dl64), (True, dx64)):
            b_cost, b_g, _ = bounds_for(ref_case, dev, logits_form)
            base = ref_case.logits if logits_form else ref_case.lp32()
            x = torch.cat([base, base.flip(0)], 1).to(dev).requires_grad_(True)
            fn = ctc.ctc_long_loss_from_logits if logits_form else ctc.ctc_long_loss
            costs = fn(x, tg, il, tl, reduction="none")
            zero = fn(x, tg, il, tl, reduction="none", zero_infinity=True)
            (grad,) = torch.autograd.grad((costs * weights).sum(), x)
            costs, zero, grad = costs.detach().double().cpu(), zero.detach().cpu(), grad.double().cpu()
            assert costs.numel() == 2 and grad.numel() == T * 2 * C
            assert costs[1] == float("inf") and float(zero[1]) == 0.0 and float(zero[0]) == float(costs[0]), name
            assert (grad[:, 1] == 0).all() and grad[:, 1].numel() == T * C, name
            e_cost = float((costs[0] - c64[0]).abs() / c64[0].abs())
            e_grad = float((grad[:, :1] - gref).abs().max())
            print("CTCPARITY long beside_%-12s %-9s cost rel err %.3g (bound %.3g)  grad abs err %.3g (bound %.3g)" % (
                name, "logits" if logits_form else "log_probs", e_cost, b_cost, e_grad, b_g))
            assert e_cost <= b_cost and e_grad <= b_g, (name, logits_form)


def test_routing_beyond_511_labels_and_not_below(hip_device):
    from pika_amd import ctc
    dev = hip_device
    g = torch.Generator().manual_seed(71)
    T, B, C = 800, 2, 6

    def batch(U):
        seqs = [G.rand_seq(U, C, 0, 71), G.rand_seq(U - 60, C, 0, 72)]
        return (torch.randn(T, B, C, generator=g).to(dev), R.pad_targets(seqs).to(dev),
                torch.tensor([T, T - 9], device=dev), torch.tensor([U, U - 60], device=dev))
    x, tg, il, tl = batch(512)
    for reduction in ("none", "mean", "sum"):
        for logits_form in (False, True):
            xin = x if logits_form else x.log_softmax(-1)
            pairs = [(ctc.ctc_loss_from_logits, ctc.ctc_long_loss_from_logits)] if logits_form else [
                (ctc.ctc_loss, ctc.ctc_long_loss), (lambda *a, **k: ctc.CTCLoss(k["blank"], k["reduction"])(*a), ctc.ctc_long_loss)]
            for routed, direct in pairs:
                outs = []
                for fn in (routed, direct):
                    xr = xin.clone().requires_grad_(True)
                    loss = fn(xr, tg, il, tl, blank=0, reduction=reduction)
                    (grad,) = torch.autograd.grad(loss.sum(), xr)
                    outs.append((loss.detach(), grad))
                assert outs[0][1].numel() == T * B * C and outs[0][0].numel() == (B if reduction == "none" else 1)
                assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (reduction, logits_form)
                assert torch.isfinite(outs[0][0]).all()
    # 1-D targets route as well, and give the padded form's bits
    xr = x.clone().requires_grad_(True)
    flat = torch.cat([tg[0, :512], tg[1, :452]]).cpu()
    a = ctc.ctc_loss_from_logits(xr, flat, il.cpu(), tl.cpu(), reduction="none")
    b = ctc.ctc_long_loss_from_logits(x, tg, il, tl, reduction="none")
    assert a.numel() == 2 and torch.equal(a, b)
    # U = 511 stays where it was: the bits of a direct call of the one-workgroup kernels
    x, tg, il, tl = batch(511)
    for logits_form in (False, True):
        xin = (x if logits_form else x.log_softmax(-1))
        xa, xb = xin.clone().requires_grad_(True), xin.clone().requires_grad_(True)
        a = (ctc.ctc_loss_from_logits if logits_form else ctc.ctc_loss)(xa, tg, il, tl, reduction="none")
        b = ctc._CTCFn.apply(xb, tg.to(torch.int32), None, il.to(torch.int32), tl.to(torch.int32), 511, 0, logits_form)
        ga, gb = torch.autograd.grad(a.sum(), xa)[0], torch.autograd.grad(b.sum(), xb)[0]
        assert a.numel() == 2 and ga.numel() == T * B * C and torch.equal(a, b) and torch.equal(ga, gb)
    with pytest.raises(ValueError, match="not supported"):
        ctc.ctc_align(x.log_softmax(-1), *batch(512)[1:])


def test_determinism_and_graph_capture(hip_device):
    from pika_amd import ctc
    _geometry()
    dev = hip_device
    T, B, C, U = 2 * F + 9, 2, 5, W // 2 + 6            # three frame blocks (beta starts mid-block), two tiles
    T = max(T, 620)
    gen = torch.Generator().manual_seed(81)
    data = []
    for i in range(3):
        seqs = [G.rand_seq(U - 4 * i, C, 0, 81 + i), G.rand_seq(30 + i, C, 0, 91 + i)]
        data.append((torch.randn(T, B, C, generator=gen), R.pad_targets(seqs, width=U), [T - 11 * i, 2 * F + 1 - i],
                     [len(s) for s in seqs]))

    def dev_args(d):
        return (d[0].to(dev).requires_grad_(True), d[1].to(dev), torch.tensor(d[2], dtype=torch.int32, device=dev),
                torch.tensor(d[3], dtype=torch.int32, device=dev))

    weights = torch.tensor([1.0, -2.0], device=dev)     # made before the capture: a host-to-device copy

    def step(x, tg, il, tl):
        out = []
        for fn, xin in ((ctc.ctc_long_loss_from_logits, x), (ctc.ctc_long_loss, x.log_softmax(-1))):
            costs = fn(xin, tg, il, tl, reduction="none")
            (g,) = torch.autograd.grad((costs * weights).sum(), x)
            out += [costs.detach(), g]
        return out
    static = dev_args(data[0])
    first, again = step(*static), step(*static)
    assert len(first) == 4 and first[1].numel() == T * B * C
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up off the default stream, then one linear capture
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*static)
    for d in data[1:]:
        with torch.no_grad():
            for s, n in zip(static, dev_args(d)):
                s.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*dev_args(d))
        for o, e in zip(outs, eager):
            assert o.numel() == e.numel() and o.cpu().numpy().tobytes() == e.cpu().numpy().tobytes()
        assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
