"""CTC-guided frame skipping without a GPU: the plain-torch path of pika_amd/frame_skip.py (what runs on the CPU, in
float64 and beyond the kernels' limits) against the numpy definition of tests/frame_skip_common.py; a second formulation
of the min_frames top-up against the definition's stable sort; the inverse-map properties of a plan; the generator's
margin at every shape tests/test_frame_skip_gpu.py uses; the apply, its autograd and the time map; the surface."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frame_skip_common as FC  # noqa: E402

TS = [1, 63, 64, 65, 257]
LOGIT_SHAPES = [(4, 19, 2), (4, 33, 5), (4, 12, 4097), (4, 11, 8200)]      # (B, T, C) of the from-logits GPU cases


def all_cases():
    return [(T,) + c for T in TS for c in FC.plan_cases(T)]


def same_plan(got, want, name):
    for g, w, what in zip(got[:3], want[:3], ("kept_lengths", "frame_index", "position")):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, what)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_torch_path_equals_the_definition(dtype):
    from pika_amd import ctc_skip_plan
    for T, name, x, lengths, blank, thr, mf in all_cases():
        want = FC.plan(x[:, :, blank], lengths, thr, mf)
        for time_major in (False, True):
            scores = torch.from_numpy(x).to(dtype)
            if time_major:
                scores = scores.transpose(0, 1).contiguous()
            got = ctc_skip_plan(scores, torch.from_numpy(lengths), blank, thr,
                                None if mf is None else torch.from_numpy(mf), time_major=time_major)
            same_plan(got, want, (T, name, time_major))
            assert np.array_equal(got.blank_lp.numpy(), want[3].astype(got.blank_lp.numpy().dtype), equal_nan=True)


def test_torch_path_from_logits_equals_the_definition():
    from pika_amd import ctc_skip_plan
    for B, T, C in LOGIT_SHAPES:
        rng = np.random.default_rng(C)
        lengths, blank, thr = FC.lengths_for(B, T, rng), C // 2, 0.95
        x = FC.make_logits(B, T, C, blank, thr, C)
        assert FC.margin_holds(x, blank, thr, lengths), (B, T, C)      # the GPU test relies on it at these shapes
        want = FC.plan(FC.blank_lp_of(x, blank, True), lengths, thr, lengths // 2)
        got = ctc_skip_plan(torch.from_numpy(x).double(), lengths, blank, thr, lengths // 2, from_logits=True)
        same_plan(got, want, (B, T, C))
        t = np.arange(T)[None, :] < lengths[:, None]
        assert np.abs(np.where(t, got.blank_lp.numpy() - want[3], 0.0)).max() < 1e-12
        assert 0 < int(want[0].sum()) < int(lengths.sum())             # frames were dropped, frames were kept


def top_up_by_counting(lp, L, thr, m):
    """The second formulation: how many to restore, then a value threshold and a cut among the ties at it."""
    dropped = [t for t in range(L) if lp[t] >= thr]
    kept = [t for t in range(L) if not lp[t] >= thr]
    r = m - len(kept)
    if r > 0:
        vals = np.sort(np.array([lp[t] for t in dropped]))
        kth = vals[r - 1]
        below = [t for t in dropped if lp[t] < kth]
        ties = [t for t in dropped if lp[t] == kth]
        kept = sorted(kept + below + ties[:r - len(below)])
    return kept


def test_top_up_by_counting_equals_the_stable_sort():
    for T, name, x, lengths, blank, thr, mf in all_cases():
        lp = x[:, :, blank]
        kept_lengths, frame_index, _, _ = FC.plan(lp, lengths, thr, mf)
        for b in range(lp.shape[0]):
            L = min(max(int(lengths[b]), 0), T)
            m = 0 if L == 0 else min(max(1 if mf is None else int(mf[b]), 1), L)
            kept = top_up_by_counting(lp[b], L, FC.log_thr(thr), m)
            assert kept == frame_index[b, :kept_lengths[b]].tolist(), (T, name, b)


def test_a_plan_is_an_inverse_pair():
    topped_up = 0
    for T, name, x, lengths, blank, thr, mf in all_cases():
        kept_lengths, frame_index, position, _ = FC.plan(x[:, :, blank], lengths, thr, mf)
        natural = FC.plan(x[:, :, blank], lengths, thr)[0]
        for b in range(x.shape[0]):
            L, k = min(max(int(lengths[b]), 0), T), int(kept_lengths[b])
            m = 0 if L == 0 else min(max(1 if mf is None else int(mf[b]), 1), L)
            assert m <= k <= L, (T, name, b)
            row = frame_index[b, :k]
            assert (np.diff(row) > 0).all() and (row >= 0).all() and (row < L).all()
            assert (frame_index[b, k:] == -1).all()
            assert np.array_equal(position[b, row], np.arange(k))
            assert int((position[b] >= 0).sum()) == k
            topped_up += int(k > natural[b])
        if name == "everything_dropped":
            lp = x[:, :, blank]
            for b in range(x.shape[0]):
                L = min(max(int(lengths[b]), 0), T)
                if L:
                    assert kept_lengths[b] == 1 and frame_index[b, 0] == int(np.argmin(lp[b, :L]))   # earliest on ties
    assert topped_up > 20


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
def test_apply_backward_and_times_on_the_cpu(dtype):
    from pika_amd import ctc_skip_plan, frame_skip_apply, frame_skip_times
    T, name, x, lengths, blank, thr, mf = [c for c in all_cases() if c[0] == 65 and c[1] == "min_frames"][0]
    plan = ctc_skip_plan(torch.from_numpy(x), lengths, blank, thr, mf)
    want = FC.plan(x[:, :, blank], lengths, thr, mf)
    B = x.shape[0]
    torch.manual_seed(0)
    feats = torch.randn(B, T, 5).to(dtype).requires_grad_(True)
    out = frame_skip_apply(feats, plan)
    ref = FC.apply(feats.detach().float().numpy(), want[1])
    assert np.array_equal(out.detach().float().numpy(), ref)
    dout = torch.randn(B, T, 5).to(dtype)
    out.backward(dout)
    dref = FC.apply(dout.float().numpy(), want[2])
    assert np.array_equal(feats.grad.float().numpy(), dref)
    assert (feats.grad.float().numpy()[want[2] < 0] == 0).all()
    times = torch.tensor([[0, -1], [-1, -1], [0, 0], [1, 0], [2, -1], [0, T + 3]])
    back = frame_skip_times(times, plan).numpy()
    for b in range(B):
        for i in range(2):
            j = int(times[b, i])
            assert back[b, i] == (want[1][b, j] if 0 <= j < T else -1)


def test_surface():
    import pika_amd
    from pika_amd import _lib
    for name in ("FrameSkipPlan", "ctc_skip_plan", "frame_skip_apply", "frame_skip_times", "modified_beam_search_skip"):
        assert name in dir(pika_amd) and getattr(pika_amd, name) is not None
    lib = _lib.lib()
    for name in ("pika_fskip_rows", "pika_fskip_plan", "pika_fskip_apply"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    # refusals come before any launch: bad dimensions, null pointers, the stated limits, the element size
    assert lib.pika_fskip_rows(None, 0, 0, None, 1, 1, 1, 0, 0, None, None) == -1
    assert lib.pika_fskip_rows(None, 0, 0, None, 1, 8193, 1, 0, 0, None, None) == -2
    assert lib.pika_fskip_rows(None, 0, 0, None, 1 << 20, 4096, 1, 0, 0, None, None) == -2
    assert lib.pika_fskip_plan(None, None, None, 0, 1, 0.0, None, None, None, None) == -1
    assert lib.pika_fskip_plan(None, None, None, 1, 8193, 0.0, None, None, None, None) == -2
    assert lib.pika_fskip_apply(None, 0, 0, None, 1, 1, 4, 4, None, None) == -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.pika_fskip_apply(p, 0, 0, p, 1, 1, 4, 3, p, None) == -1
    assert lib.pika_fskip_apply(p, 0, 0, p, 1, 1, 6, 4, p, None) == -1
    assert lib.pika_fskip_apply(p, 0, 0, p, 1, 1, 1 << 31, 4, p, None) == -2
    with pytest.raises(ValueError):
        pika_amd.ctc_skip_plan(torch.zeros(2, 3, 4), torch.tensor([3, 3]), blank=4)
    with pytest.raises(ValueError):
        pika_amd.ctc_skip_plan(torch.zeros(2, 3, 4), torch.tensor([3, 3, 3]))
    with pytest.raises(ValueError):
        pika_amd.ctc_skip_plan(torch.zeros(2, 3, 4), torch.tensor([3, 3]), threshold=float("nan"))
