"""CTC-guided frame skipping on the device (include/pika_frame_skip.h, csrc/frame_skip.hip) against the numpy float64
definition of tests/frame_skip_common.py.

Integers (kept_lengths, frame_index, position) and moved bytes must equal the definition exactly.  blank_lp from logits is
compared with float64 within max(2 x the float32 numpy yardstick's largest error on the same rows, 1e-6): the yardstick
is the plain max / sum / log spelling with every operation rounded to float32, so the bound is what float32 itself costs
at these rows.  The keep decisions from logits must equal the float64 definition on EVERY frame; the generator keeps every
frame's float64 blank_lp at least 1e-3 from log(threshold) (asserted here before anything is compared, and on the CPU in
tests/test_frame_skip_refs.py), far more than the bound above.  Every measured error is printed (`FRAMESKIP ...`) before
it is asserted; profiles/frame_skip_parity.txt keeps those lines.

Measured on the MI355X: kernel errors 7.4e-8 .. 3.4e-7 next to yardstick errors 2.9e-7 .. 1.1e-6; the worst ratio to the
bound is 0.26 (C = 4097); 16-byte and scalar loads give the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frame_skip_common as FC  # noqa: E402
from test_frame_skip_refs import LOGIT_SHAPES, TS, same_plan  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def offset_by_one(t):
    """The same values in memory whose base is one element past a 256-byte boundary: not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


@pytest.mark.parametrize("T", TS)
def test_plan_from_log_probs_equals_the_definition(hip_device, T):
    from pika_amd import ctc_skip_plan
    dev = hip_device
    for name, x, lengths, blank, thr, mf in FC.plan_cases(T):
        want = FC.plan(x[:, :, blank], lengths, thr, mf)
        B, _, C = x.shape
        xd = torch.from_numpy(x).to(dev)
        wide = torch.zeros((B, T + 3, C + 1), device=dev)           # a non-contiguous batch (and time) stride
        wide[:, :T, :C] = xd
        inputs = [("bt", xd, False), ("tb", xd.transpose(0, 1).contiguous(), True),
                  ("strided", wide[:, :T, :C], False), ("tb_view", wide[:, :T, :C].transpose(0, 1), True)]
        for how, scores, time_major in inputs:
            for on_device in (False, True):
                ln = torch.from_numpy(lengths).to(dev if on_device else "cpu")
                m = None if mf is None else torch.from_numpy(mf).to(dev if on_device else "cpu", torch.int32)
                got = ctc_skip_plan(scores, ln, blank, thr, m, time_major=time_major)
                assert got.kept_lengths.is_cuda
                same_plan(got, want, (T, name, how, on_device))
                assert np.array_equal(got.blank_lp.cpu().numpy(), want[3], equal_nan=True), (T, name, how)


@pytest.mark.parametrize("shape", LOGIT_SHAPES, ids=lambda s: "B%d_T%d_C%d" % s)
def test_plan_from_logits(hip_device, shape):
    from pika_amd import ctc_skip_plan
    dev = hip_device
    B, T, C = shape
    rng = np.random.default_rng(C)
    lengths, blank, thr = FC.lengths_for(B, T, rng), C // 2, 0.95
    x = FC.make_logits(B, T, C, blank, thr, C)
    assert FC.margin_holds(x, blank, thr, lengths)                  # no frame is left out of the comparison below
    lp64 = FC.blank_lp_of(x, blank, True)
    yard = FC.blank_lp_of(x, blank, True, np.float32).astype(np.float64)
    valid = np.arange(T)[None, :] < lengths[:, None]
    err_y = float(np.abs(np.where(valid, yard - lp64, 0.0)).max())
    bound = max(2.0 * err_y, 1e-6)
    mf = (lengths * 9) // 10
    want = FC.plan(lp64, lengths, thr)
    assert all(k >= 1 or L <= 1 for k, L in zip(want[0], lengths))  # the top-up plays no part in `want`
    xd = torch.from_numpy(x).to(dev)
    outs = []
    for how, scores in (("aligned", xd), ("offset", offset_by_one(xd))):
        got = ctc_skip_plan(scores, lengths, blank, thr, from_logits=True)
        lp = got.blank_lp.cpu().numpy()
        assert (lp[~valid] == 0).all()
        err_k = float(np.abs(np.where(valid, lp.astype(np.float64) - lp64, 0.0)).max())
        print("FRAMESKIP logits (B,T,C)=%-14s %-8s kernel err %.3g  yardstick err %.3g  bound %.3g  ratio %.3g"
              % (shape, how, err_k, err_y, bound, err_k / bound))
        assert err_k <= bound
        same_plan(got, want, (shape, how))                          # every frame decides as float64 does
        # with a top-up, the order from logits is the order the kernel's own blank_lp gives
        own = FC.plan(lp, lengths, thr, mf)
        assert int((own[0] > want[0]).sum()) > 0                    # (frames were put back)
        same_plan(ctc_skip_plan(scores, lengths, blank, thr, mf, from_logits=True), own, (shape, how, "top-up"))
        outs.append(lp)
    assert np.array_equal(outs[0], outs[1])                         # vector and scalar loads: the same value
    tm = ctc_skip_plan(xd.transpose(0, 1).contiguous(), lengths, blank, thr, from_logits=True, time_major=True)
    same_plan(tm, want, (shape, "time_major"))
    assert np.array_equal(tm.blank_lp.cpu().numpy(), outs[0])


def guarded(shape, dtype, dev, fill):
    """A tensor inside a buffer with 64 guard elements before and after it, all set to `fill`."""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), fill, dtype=dtype, device=dev)
    return buf, buf[64:64 + n].view(shape)


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


@pytest.mark.parametrize("D", [1, 3, 4, 512, 516])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_apply_and_backward_move_the_bytes(hip_device, dtype, D):
    from pika_amd import _lib, ctc_skip_plan, frame_skip_apply
    dev = hip_device
    T = 65
    name, x, lengths, blank, thr, mf = [c for c in FC.plan_cases(T) if c[0] == "min_frames"][0]
    B = x.shape[0]
    plan = ctc_skip_plan(torch.from_numpy(x).to(dev), lengths, blank, thr, mf)
    want = FC.plan(x[:, :, blank], lengths, thr, mf)
    torch.manual_seed(D)
    feats = torch.randn(B, T, D).to(dtype)
    feats[0, 0, 0] = float("nan")                                   # bytes, not numbers: a NaN and a -0.0 travel too
    feats[0, 1, 0] = -0.0
    dout = torch.randn(B, T, D).to(dtype)
    ref = FC.apply(bits(feats), want[1])
    dref = FC.apply(bits(dout), want[2])
    assert (ref[want[1] < 0] == 0).all() and (dref[want[2] < 0] == 0).all()     # zero tails, zero dropped rows
    results = []
    for how in ("aligned", "offset"):
        xin = feats.to(dev) if how == "aligned" else offset_by_one(feats.to(dev))
        xin.requires_grad_(True)
        out = frame_skip_apply(xin, plan)
        assert np.array_equal(bits(out), ref), (how, "forward")
        g = dout.to(dev) if how == "aligned" else offset_by_one(dout.to(dev))
        grads = [torch.autograd.grad(out, xin, g, retain_graph=True)[0] for _ in range(2)]
        assert np.array_equal(bits(grads[0]), dref), (how, "backward")
        assert np.array_equal(bits(grads[0]), bits(grads[1]))       # two runs: the same bits
        results.append(bits(out))
    assert np.array_equal(results[0], results[1])                   # 16-byte and element-sized accesses: the same bytes
    # the ABI itself into a guarded output: nothing outside it is touched
    es = feats.element_size()
    for index in (plan.frame_index, plan.position):
        buf, out = guarded((B, T, D), dtype, dev, 7.0)
        xin = feats.to(dev)
        _lib.check(_lib.lib().pika_fskip_apply(xin.data_ptr(), T * D * es, D * es, index.data_ptr(), B, T, D * es, es,
                                               out.data_ptr(), torch.cuda.current_stream().cuda_stream), "apply")
        torch.cuda.synchronize()
        assert (buf[:64] == 7.0).all() and (buf[-64:] == 7.0).all()
        assert np.array_equal(bits(out), FC.apply(bits(feats), index.cpu().numpy()))


def test_plan_outputs_stay_inside_their_buffers(hip_device):
    from pika_amd import _lib
    dev, T = hip_device, 257
    name, x, lengths, blank, thr, mf = [c for c in FC.plan_cases(T) if c[0] == "min_frames"][0]
    B = x.shape[0]
    want = FC.plan(x[:, :, blank], lengths, thr, mf)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    xd = torch.from_numpy(x).to(dev)
    ln = torch.from_numpy(lengths).to(dev, torch.int32)
    m = torch.from_numpy(mf).to(dev, torch.int32)
    b_lp, lp = guarded((B, T), torch.float32, dev, 7.0)
    b_k, kept = guarded((B,), torch.int32, dev, 7)
    b_fi, fi = guarded((B, T), torch.int32, dev, 7)
    b_po, po = guarded((B, T), torch.int32, dev, 7)
    for logits in (1, 0):                                           # (the plan below reads the log-probs form's)
        _lib.check(lib.pika_fskip_rows(xd.data_ptr(), xd.stride(0), xd.stride(1), ln.data_ptr(), B, T, 3, blank, logits,
                                       lp.data_ptr(), stream), "rows")
    _lib.check(lib.pika_fskip_plan(lp.data_ptr(), ln.data_ptr(), m.data_ptr(), B, T, float(FC.log_thr(thr)),
                                   kept.data_ptr(), fi.data_ptr(), po.data_ptr(), stream), "plan")
    torch.cuda.synchronize()
    for buf in (b_lp, b_k, b_fi, b_po):
        assert (buf[:64] == 7).all() and (buf[-64:] == 7).all()
    same_plan((kept, fi, po), want, "guarded")


def test_graph_capture(hip_device):
    from pika_amd import ctc_skip_plan, frame_skip_apply
    dev = hip_device
    B, T, C, D, blank, thr = 4, 65, 37, 20, 3, 0.95
    rng = np.random.default_rng(5)
    data = [(FC.make_logits(B, T, C, blank, thr, 50 + i), FC.lengths_for(B, T, rng),
             rng.standard_normal((B, T, D)).astype(np.float32), rng.standard_normal((B, T, D)).astype(np.float32))
            for i in range(4)]

    def run(logits, lengths, feats, dout):
        plan = ctc_skip_plan(logits, lengths, blank, thr, lengths // 2, from_logits=True)
        out = frame_skip_apply(feats, plan)
        return plan, out, torch.autograd.grad(out, feats, dout)[0]

    bufs = [torch.from_numpy(a).to(dev) for a in data[0]]
    bufs[1] = bufs[1].to(torch.int32)
    bufs[2].requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(*bufs)                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan, out, dx = run(*bufs)
    for logits, lengths, feats, dout in data[1:]:
        with torch.no_grad():
            for buf, a in zip(bufs, (logits, lengths, feats, dout)):
                buf.copy_(torch.from_numpy(a).to(dev))
        graph.replay()
        eager = run(torch.from_numpy(logits).to(dev), torch.from_numpy(lengths).to(dev),
                    torch.from_numpy(feats).to(dev).requires_grad_(True), torch.from_numpy(dout).to(dev))
        for g, e in zip(tuple(plan) + (out, dx), tuple(eager[0]) + eager[1:]):
            assert torch.equal(g, e)
        same_plan(plan, FC.plan(FC.blank_lp_of(logits, blank, True), lengths, thr, lengths // 2), "replay")


def test_beyond_the_limits_and_float64_run_the_definition_in_torch(hip_device):
    from pika_amd import ctc_skip_plan, frame_skip_apply
    dev = hip_device
    name, x, lengths, blank, thr, mf = [c for c in FC.plan_cases(65) if c[0] == "min_frames"][0]
    want = FC.plan(x[:, :, blank], lengths, thr, mf)
    plan = ctc_skip_plan(torch.from_numpy(x).to(dev).double(), lengths, blank, thr, mf)
    same_plan(plan, want, "float64")
    feats = torch.randn(x.shape[0], 65, 4, dtype=torch.float64, device=dev)
    assert np.array_equal(frame_skip_apply(feats, plan).cpu().numpy(), FC.apply(feats.cpu().numpy(), want[1]))
    T = 8193                                                        # one frame past the kernels' limit
    rng = np.random.default_rng(1)
    lp = np.where(rng.uniform(size=(1, T)) < 0.5, -3.0, -0.001).astype(np.float32)
    got = ctc_skip_plan(torch.from_numpy(lp).to(dev).unsqueeze(2), [T - 7], 0, thr)
    same_plan(got, FC.plan(lp, [T - 7], thr), "long")
