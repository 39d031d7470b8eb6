"""The joint network on a pruned (banded) lattice, on the GPU.

Kernels (pika_joint_gate_banded_fwd / _bwd through the C ABI) against the float64 restatements of
tests/joint_banded_common.py -- joint_common.gate_ref / gate_bwd_ref on the gathered rows, dz summed back with index_add_
in float64 -- with joint_common's tolerances GATE_H_TOL and GRAD_REL_TOL * max(1, max |ref|); every output buffer carries 64
guard elements on each side.  Then `joint_pruned` and `rnnt_pruned_joint_loss` end to end.

The end-to-end tolerance is measured, not fixed: the error of a chain is the largest, over the per-utterance costs and the
gradients of enc, pred and every joint parameter, of max |got - float64| / max |float64|; the pruned chain's error may be at
most twice that of the existing full-lattice chain (ops.joint + rnnt_loss_from_logits) at the same shape, in the arithmetic
mode the session runs in -- the band changes which rows are summed, not the arithmetic.  Both are printed
(`JOINTBANDED e2e ...`); profiles/joint_pruned_parity.txt keeps them.

Measured on the MI355X: gate h 4.1e-7 (of 2e-6), gate gradients 1.5e-6 at most (of 1e-5 * max(1, max |ref|)); end to end
in mode "mixed" 4.6e-3 on the band against 4.7e-3 for the full-lattice chain (bound 9.5e-3).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_common as J  # noqa: E402
import joint_banded_common as JB  # noqa: E402
import rnnt_pruned_common as P  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
_cache = {}


def _lib():
    from pika_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(shape, kind):
    """Inputs and float64 results of one (shape, ranges kind), computed once and never modified."""
    key = (shape, kind)
    if key not in _cache:
        B, T, U, S, H = shape
        g = torch.Generator().manual_seed(7 * T + U + H)
        e1, p1, eg, pg = (torch.randn(B, n, H, generator=g) for n in (T, U, T, U))
        dh = torch.randn(B, T, S, H, generator=g)
        dh16 = dh.bfloat16()
        ranges = JB.make_ranges(shape, kind)
        _cache[key] = dict(ins=(e1, p1, eg, pg), dh=dh, dh16=dh16, ranges=ranges,
                           h=JB.banded_gate_ref(e1, p1, eg, pg, ranges, S),
                           grads=JB.banded_gate_bwd_ref(dh, e1, p1, eg, pg, ranges, S),
                           grads16=JB.banded_gate_bwd_ref(dh16.float(), e1, p1, eg, pg, ranges, S),
                           covered=JB.covered(ranges, U, S))
    return _cache[key]


class Guarded:
    """An output of `shape` in the middle of an allocation with GUARD sentinel elements on each side."""

    def __init__(self, shape, dtype, dev):
        self.n = int(np.prod(shape))
        self.shape = shape
        self.buf = torch.full((self.n + 2 * GUARD,), -7.0, dtype=dtype, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        assert self.ptr % 16 == 0

    def result(self):
        """The output, after checking that no guard element changed."""
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.n:]
        assert bool((lo == -7.0).all()) and bool((hi == -7.0).all()), "a guard element was written"
        return self.buf[GUARD:GUARD + self.n].reshape(self.shape).clone()


def _fwd(shape, ins, ranges, dev, dtype, banded=True):
    B, T, U, S, H = shape
    d = [t.to(dev) for t in ins]
    out = Guarded((B, T, S, H), dtype, dev)
    code = J.F32 if dtype == torch.float32 else J.BF16
    if banded:
        r = torch.from_numpy(np.array(ranges)).to(dev)
        rc = _lib().pika_joint_gate_banded_fwd(*[t.data_ptr() for t in d], r.data_ptr(), out.ptr, code, B, T, U, S, H,
                                               _stream())
    else:
        assert S == U
        rc = _lib().pika_joint_gate_fwd(*[t.data_ptr() for t in d], out.ptr, code, B, T, U, H, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.result()


def _bwd(shape, ins, ranges, dh, dev, banded=True):
    B, T, U, S, H = shape
    d = [t.to(dev) for t in ins]
    dh = dh.to(dev)
    outs = [Guarded((B, n, H), torch.float32, dev) for n in (T, U, T, U)]            # de1, dp1, deg, dpg
    code = J.F32 if dh.dtype == torch.float32 else J.BF16
    if banded:
        r = torch.from_numpy(np.array(ranges)).to(dev)
        rc = _lib().pika_joint_gate_banded_bwd(dh.data_ptr(), code, *[t.data_ptr() for t in d], r.data_ptr(),
                                               *[o.ptr for o in outs], B, T, U, S, H, _stream())
    else:
        assert S == U
        rc = _lib().pika_joint_gate_bwd(dh.data_ptr(), code, *[t.data_ptr() for t in d], *[o.ptr for o in outs],
                                        B, T, U, H, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return [o.result() for o in outs]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("kind", JB.KINDS)
@pytest.mark.parametrize("shape", JB.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_banded_gate_against_float64(hip_device, shape, kind):
    dev = hip_device
    B, T, U, S, H = shape
    c = _case(shape, kind)
    name = "%s %s" % ("x".join(map(str, shape)), kind)
    # forward: fp32 within tolerance, bf16 the fp32 result rounded, bit for bit
    h32 = _fwd(shape, c["ins"], c["ranges"], dev, torch.float32)
    err = float((h32.double().cpu() - c["h"]).abs().max())
    print("JOINTBANDED gate_fwd %-28s h    err %.3g  tol %.3g" % (name, err, J.GATE_H_TOL))
    assert err < J.GATE_H_TOL
    h16 = _fwd(shape, c["ins"], c["ranges"], dev, torch.bfloat16)
    assert _same_bits(h16, h32.bfloat16())
    # backward from the fp32 dh and from the bf16 dh; the latter equals its upcast passed as fp32, bit for bit
    got32 = _bwd(shape, c["ins"], c["ranges"], c["dh"], dev)
    got16 = _bwd(shape, c["ins"], c["ranges"], c["dh16"], dev)
    up = _bwd(shape, c["ins"], c["ranges"], c["dh16"].float(), dev)
    again = _bwd(shape, c["ins"], c["ranges"], c["dh"], dev)
    for what, a32, a16, u, a2, w32, w16 in zip(("de1", "dp1", "deg", "dpg"), got32, got16, up, again, c["grads"],
                                               c["grads16"]):
        assert _same_bits(a16, u), what
        assert _same_bits(a32, a2), "%s: two runs differ" % what
        for a, w, tag in ((a32, w32, "f32"), (a16, w16, "bf16")):
            tol = J.GRAD_REL_TOL * max(1.0, float(w.abs().max()))
            err = float((a.double().cpu() - w).abs().max())
            print("JOINTBANDED gate_bwd %-28s %s dh %-4s err %.3g  tol %.3g" % (name, what, tag, err, tol))
            assert err < tol, (name, what, tag, err, tol)
    # a row no band covers: exact +0 in both prediction-side outputs
    dead = ~c["covered"]
    if shape == JB.UNCOVERED_SHAPE and kind == "nonmonotone":
        assert bool(dead[0, 4])
    for a in (got32[1], got32[3], got16[1], got16[3]):
        assert bool((_bits(a).cpu()[dead] == 0).all())


def test_entries_clamp_the_ranges(hip_device):
    """Entries -3 and U + 7 behave as 0 and U - S: the same bits as the call on the clamped ranges."""
    shape = (3, 33, 9, 4, 260)
    B, T, U, S, H = shape
    c = _case(shape, "clamped")
    clamped = np.clip(c["ranges"], 0, U - S).astype(np.int32)
    assert (clamped != c["ranges"]).any()
    assert _same_bits(_fwd(shape, c["ins"], c["ranges"], hip_device, torch.float32),
                      _fwd(shape, c["ins"], clamped, hip_device, torch.float32))
    for a, b in zip(_bwd(shape, c["ins"], c["ranges"], c["dh"], hip_device), _bwd(shape, c["ins"], clamped, c["dh"], hip_device)):
        assert _same_bits(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_band_that_is_the_lattice_is_the_full_gate(hip_device, dtype):
    """S = U and all-zero ranges: forward and all four gradients equal pika_joint_gate_fwd / _bwd bit for bit."""
    shape = (3, 33, 9, 9, 260)
    B, T, U, S, H = shape
    g = torch.Generator().manual_seed(5)
    ins = [torch.randn(B, n, H, generator=g) for n in (T, U, T, U)]
    dh = torch.randn(B, T, U, H, generator=g).to(dtype)
    zero = np.zeros((B, T), np.int32)
    assert _same_bits(_fwd(shape, ins, zero, hip_device, dtype), _fwd(shape, ins, None, hip_device, dtype, banded=False))
    for what, a, b in zip(("de1", "dp1", "deg", "dpg"), _bwd(shape, ins, zero, dh, hip_device),
                          _bwd(shape, ins, None, dh, hip_device, banded=False)):
        assert _same_bits(a, b), what


# ---- joint_pruned and rnnt_pruned_joint_loss ---------------------------------------------------------------------------
def _layers(H, Jw, V, dev, seed, simple=False):
    torch.manual_seed(seed)
    dims = [(2 * H, Jw), (2 * H, Jw), (Jw, V)] + ([(H, V), (H, V)] if simple else [])
    return [torch.nn.Linear(i, o).to(dev) for i, o in dims]


def _params(layers):
    return [p for m in layers for p in (m.weight, m.bias)]


def test_joint_pruned_on_the_whole_lattice_is_ops_joint(hip_device):
    """s_range = U + 1 with all-zero ranges: output and the gradients of enc, pred and the three layers equal
    ops.joint(log_softmax=False) bit for bit."""
    from pika_amd.model import ops
    dev = hip_device
    B, T, U1, H, V = 2, 12, 5, 64, 16
    fc1, fcg, fc2 = layers = _layers(H, H, V, dev, 0)
    g = torch.Generator().manual_seed(1)
    enc0, pred0, w = torch.randn(B, T, H, generator=g), torch.randn(B, U1, H, generator=g), torch.randn(B, T, U1, V, generator=g)
    out = []
    for banded in (True, False):
        enc, pred = enc0.to(dev).requires_grad_(True), pred0.to(dev).requires_grad_(True)
        if banded:
            y = ops.joint_pruned(enc, pred, torch.zeros(B, T, dtype=torch.int32, device=dev), U1, fc1, fcg, fc2)
        else:
            y = ops.joint(enc, pred, fc1, fcg, fc2, log_softmax=False)
        assert y.shape == (B, T, U1, V)
        grads = torch.autograd.grad((y * w.to(dev)).sum(), [enc, pred] + _params(layers))
        out.append([y.detach()] + list(grads))
    for a, b in zip(*out):
        assert _same_bits(a.contiguous(), b.contiguous())


E2E = dict(B=3, T=20, U=6, H=64, V=16, S=3, tl=[20, 11, 14], ul=[6, 2, 4])


def _e2e_inputs(seed):
    B, T, U, H, V = (E2E[k] for k in "BTUHV")
    g = torch.Generator().manual_seed(seed)
    enc, pred = torch.randn(B, T, H, generator=g), torch.randn(B, U + 1, H, generator=g)
    y = torch.randint(1, V, (B, U), generator=g).int()
    tl, ul = torch.tensor(E2E["tl"], dtype=torch.int32), torch.tensor(E2E["ul"], dtype=torch.int32)
    for n in range(B):
        y[n, int(ul[n]):] = V
        assert (int(tl[n]) - 1) * (E2E["S"] - 1) >= int(ul[n]) + 1 - E2E["S"]       # a band of this width exists
    return enc, pred, y, tl, ul


def _oracle(enc, pred, y, tl, ul, layers, ranges, S):
    """float64: the formula joint (on the band's rows when `ranges` is given, scattered into the full lattice), log-softmax,
    oracle.rnnt.rnnt_loss, and the gradients of the summed costs w.r.t. enc, pred and the joint's parameters."""
    from oracle import rnnt as O
    fc1, fcg, fc2 = [[p.detach().double().cpu().requires_grad_(True) for p in (m.weight, m.bias)] for m in layers[:3]]
    e, p = enc.double().requires_grad_(True), pred.double().requires_grad_(True)
    H, U1 = e.shape[-1], p.shape[1]
    e1, eg = e @ fc1[0][:, :H].T + fc1[1], e @ fcg[0][:, :H].T + fcg[1]
    p1, pg = p @ fc1[0][:, H:].T, p @ fcg[0][:, H:].T
    if ranges is not None:
        rows = JB.band_rows(ranges, U1, S)
        bidx = torch.arange(e.shape[0])[:, None, None].expand(rows.shape)
        p1, pg = p1[bidx, rows], pg[bidx, rows]
    else:
        p1, pg = p1[:, None], pg[:, None]
    h = torch.tanh(e1[:, :, None] + p1) * torch.sigmoid(eg[:, :, None] + pg)
    lp = torch.log_softmax(h @ fc2[0].T + fc2[1], -1)
    tl_n, ul_n, y_n = tl.numpy(), ul.numpy(), y.numpy()
    if ranges is not None:
        full = P.scatter(lp.detach().numpy(), ranges, U1, ul_n)
        c64, g64 = O.rnnt_loss(full, y_n, tl_n, ul_n)
        g = P.gather(g64, ranges, S, ul_n)
    else:
        c64, g = O.rnnt_loss(lp.detach().numpy(), y_n, tl_n, ul_n)
    lp.backward(torch.from_numpy(g))
    return c64, [e.grad, p.grad] + [t.grad for pair in (fc1, fcg, fc2) for t in pair]


def _chain_error(tag, costs, grads, c64, g64):
    names = ["costs", "enc", "pred", "fc1.w", "fc1.b", "fc_gate.w", "fc_gate.b", "fc2.w", "fc2.b"]
    got = [costs.detach().double().cpu()] + [g.double().cpu() for g in grads]
    want = [torch.from_numpy(np.asarray(c64))] + list(g64)
    worst = 0.0
    for n, a, w in zip(names, got, want):
        err = float((a - w).abs().max()) / float(w.abs().max())
        print("JOINTBANDED e2e %-6s %-9s rel err %.3g" % (tag, n, err))
        worst = max(worst, err)
    return worst


def test_pruned_joint_loss_end_to_end(hip_device):
    from pika_amd import gemm as G
    from pika_amd import rnnt_pruned_joint_loss
    from pika_amd.model import ops
    from pika_amd.rnnt import (rnnt_loss_from_logits, rnnt_loss_from_planes, rnnt_prune_ranges, rnnt_simple_planes)
    dev = hip_device
    S, H, V = E2E["S"], E2E["H"], E2E["V"]
    enc0, pred0, y, tl, ul = _e2e_inputs(11)
    layers = _layers(H, H, V, dev, 2, simple=True)
    fc1, fcg, fc2, sam, slm = layers
    yd, tld, uld = y.to(dev), tl.to(dev), ul.to(dev)
    enc, pred = enc0.to(dev).requires_grad_(True), pred0.to(dev).requires_grad_(True)
    simple, pruned, ranges = rnnt_pruned_joint_loss(enc, pred, yd, tld, uld, fc1, fcg, fc2, sam, slm, s_range=S,
                                                    reduction=None)
    assert ranges.dtype == torch.int32 and ranges.shape == (E2E["B"], E2E["T"]) and not ranges.requires_grad
    assert simple.shape == pruned.shape == (E2E["B"],)
    # the pieces, one by one, give the same band and the same simple loss
    with torch.no_grad():
        planes = rnnt_simple_planes(ops.linear(enc, sam.weight, sam.bias), ops.linear(pred, slm.weight, slm.bias), yd)
        s1, ob, ol = rnnt_loss_from_planes(*planes, tld, uld, return_occupancy=True)
        assert torch.equal(rnnt_prune_ranges(ob, ol, tld, uld, S), ranges) and torch.equal(s1, simple.detach())
    r = ranges.cpu().numpy()
    for n in range(E2E["B"]):
        assert P.is_valid(r[n], int(tl[n]), int(ul[n]), S)
    # the pruned loss does not reach the simple joiner; the simple loss does
    grads = torch.autograd.grad(pruned.sum(), [enc, pred] + _params(layers[:3]), retain_graph=True)
    assert all(g is None for g in torch.autograd.grad(pruned.sum(), _params(layers[3:]), retain_graph=True, allow_unused=True))
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in torch.autograd.grad(simple.sum(), _params(layers[3:])))
    err_pruned = _chain_error("pruned", pruned, grads, *_oracle(enc0, pred0, y, tl, ul, layers, r, S))
    # the yardstick: the existing full-lattice chain against its float64 oracle, same inputs and layers
    enc, pred = enc0.to(dev).requires_grad_(True), pred0.to(dev).requires_grad_(True)
    full = rnnt_loss_from_logits(ops.joint(enc, pred, fc1, fcg, fc2, log_softmax=False), yd, tld, uld)
    grads = torch.autograd.grad(full.sum(), [enc, pred] + _params(layers[:3]))
    err_full = _chain_error("full", full, grads, *_oracle(enc0, pred0, y, tl, ul, layers, None, S))
    print("JOINTBANDED e2e mode %s: pruned chain %.3g, full-lattice chain %.3g, bound %.3g" % (
        G.PRECISION, err_pruned, err_full, 2 * err_full))
    assert err_pruned <= 2 * err_full, (err_pruned, err_full)


def test_pruned_joint_loss_captures_into_one_graph(hip_device):
    """Forward plus backward of rnnt_pruned_joint_loss in one torch.cuda.graph, replayed on new data: losses, ranges and
    gradients equal the eager call bit for bit."""
    from pika_amd import rnnt_pruned_joint_loss
    dev = hip_device
    S, H, V = E2E["S"], E2E["H"], E2E["V"]
    layers = _layers(H, H, V, dev, 3, simple=True)
    params = _params(layers)

    def run(stat):
        s, p, r = rnnt_pruned_joint_loss(*stat, *layers, s_range=S, fastemit_lambda=0.25)
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
            assert _same_bits(a.contiguous(), b.contiguous())
