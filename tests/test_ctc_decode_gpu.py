"""CTC decoding on the MI355X against the references of tests/ctc_decode_common.py.

Greedy: tokens, lengths and frames equal the reference exactly; scores within T * 2^-23 * max|score| (the kernel sums
in fp64 and rounds once).

Search.  The reference is the float64 prefix beam search over the full vocabulary on the SAME fp32 log-probs; the
yardstick is the same function run in float32.  Per case the bound is max(4 x the yardstick's largest score error,
1e-6 * max|score|) -- the rule of tests/test_ctc_gpu.py.  A case is *separated* when its margin (the smallest gap the
reference met between the last kept and the first dropped candidate, or between neighbouring n-best entries) exceeds
2 * bound; on separated cases the token lists must equal the reference's entry by entry.  On every case the entries are
distinct and sorted and score <= -dp_cost(lp, seq) + bound (a beam sums a subset of the paths); where the beam holds
every prefix that exists the score is within the bound of -dp_cost.  tests/test_ctc_decode_surface.py checks, from the
reference alone, that at most one case in ten is unseparated and that at least three cases re-create an orphaned
prefix.  Every measured error is printed (`CTCDECODE ...`) before it is asserted; profiles/ctc_decode_parity.txt keeps
that output.

Measured on the MI355X (profiles/ctc_decode_parity.txt): worst search score error 0.12 of its bound, exhaustive cases
within 2.4e-7 of -dp_cost, greedy scores within 0.08 of their bound.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_decode_common as D  # noqa: E402

pytestmark = pytest.mark.gpu


SearchCase, SEARCH_CASES, RAGGED_CASES, ALL_SEARCH = D.SearchCase, D.SEARCH_CASES, D.RAGGED_CASES, D.ALL_SEARCH
RAGGED_T, RAGGED_C, RAGGED_BEAM, RAGGED_ILS, _RAGGED_LP = D.RAGGED_T, D.RAGGED_C, D.RAGGED_BEAM, D.RAGGED_ILS, D.RAGGED_LP


def gpu_search(lp, ils, beam, nbest, blank, dev, logits=False):
    """lp (T,B,C) numpy -> per utterance [(label tuple, score)] with missing entries as (None, -inf)."""
    from pika_amd import ctc
    fn = ctc.ctc_beam_search_from_logits if logits else ctc.ctc_beam_search
    tokens, lengths, scores = fn(torch.from_numpy(lp).to(dev), torch.tensor(ils), beam=beam, nbest=nbest, blank=blank)
    T, B = lp.shape[0], lp.shape[1]
    assert tokens.shape == (B, nbest, T) and tokens.dtype == torch.int32
    assert lengths.shape == (B, nbest) and lengths.dtype == torch.int32
    assert scores.shape == (B, nbest) and scores.dtype == torch.float32
    tokens, lengths, scores = tokens.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()
    out = []
    for n in range(B):
        hyps = []
        for k in range(nbest):
            ln = int(lengths[n, k])
            if ln < 0:
                assert scores[n, k] == -np.inf and (tokens[n, k] == -1).all()
                hyps.append((None, -np.inf))
            else:
                assert (tokens[n, k, ln:] == -1).all() and (tokens[n, k, :ln] >= 0).all()
                hyps.append((tuple(int(v) for v in tokens[n, k, :ln]), float(scores[n, k])))
        out.append(hyps)
    return out


def check_hyps(case, got, nbest):
    h64, bound, separated, _, margin, err32 = case.ref()
    want = h64[:nbest]
    real = [(l, s) for l, s in got if l is not None]
    assert len(real) == len(want) and all(l is None for l, _ in got[len(real):]), (case.name, got)
    labels = [l for l, _ in real]
    assert len(set(labels)) == len(labels), (case.name, "two entries denote the same label sequence")
    lp64 = case.lp.astype(np.float64)
    full = [-R.dp_cost(lp64, list(l), case.blank) for l in labels]
    e_ref = max([abs(s - ws) for (_, s), (_, ws) in zip(real, want)] + [0.0]) if separated else float("nan")
    over = max(s - f for (_, s), f in zip(real, full))
    e_full = max(abs(s - f) for (_, s), f in zip(real, full))
    print("CTCDECODE %-22s nbest %2d  score err %.3g  over -dp_cost %.3g  |score + dp_cost| %.3g  (bound %.3g, float32 "
          "err %.3g, margin %.3g, %s)" % (case.name, nbest, e_ref, over, e_full, bound, err32, margin,
                                          "separated" if separated else "NOT separated"))
    for (_, a), (_, b) in zip(real, real[1:]):
        assert a >= b, (case.name, "not sorted")
    assert over <= bound, (case.name, over, bound)
    if separated:
        assert labels == [l for l, _ in want], (case.name, labels, want)
        assert e_ref <= bound, (case.name, e_ref, bound)
    if case.exhaustive:
        assert e_full <= bound, (case.name, e_full, bound)


@pytest.mark.parametrize("case", SEARCH_CASES, ids=lambda c: c.name)
def test_search_against_float64(hip_device, case):
    got = gpu_search(case.lp[:, None], [case.T], case.beam, case.beam, case.blank, hip_device)[0]
    check_hyps(case, got, case.beam)
    first = gpu_search(case.lp[:, None], [case.T], case.beam, 1, case.blank, hip_device)[0]
    assert first == got[:1]                     # nbest = 1 is the head of nbest = beam
    check_hyps(case, first, 1)


def test_search_ragged_batch(hip_device):
    lp = _RAGGED_LP.copy()
    for nbest in (1, RAGGED_BEAM):
        got = gpu_search(lp, RAGGED_ILS, RAGGED_BEAM, nbest, 0, hip_device)
        for case, hyps in zip(RAGGED_CASES, got):
            check_hyps(case, hyps, nbest)
    # frames beyond T_n are never read; lengths clamp to [1,T]; int32 / int64, host / device lengths agree
    dirty = lp.copy()
    for n, il in enumerate(RAGGED_ILS):
        dirty[il:, n] = np.nan
    assert gpu_search(dirty, RAGGED_ILS, RAGGED_BEAM, RAGGED_BEAM, 0, hip_device) == got
    from pika_amd import ctc
    x = torch.from_numpy(lp).to(hip_device)
    want = ctc.ctc_beam_search(x, torch.tensor(RAGGED_ILS), beam=4, nbest=2)
    for il in (torch.tensor(RAGGED_ILS, dtype=torch.int32), torch.tensor(RAGGED_ILS).to(hip_device)):
        for a, b in zip(want, ctc.ctc_beam_search(x, il, beam=4, nbest=2)):
            assert torch.equal(a, b)
    a = ctc.ctc_beam_search(x, torch.tensor([0, 99, 11]), beam=4, nbest=2)
    b = ctc.ctc_beam_search(x, torch.tensor([1, RAGGED_T, 11]), beam=4, nbest=2)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # unbatched (T,C): utterance 0 on its own, no batch axis
    u = ctc.ctc_beam_search(x[:, 0], torch.tensor([RAGGED_ILS[0]]), beam=4, nbest=2)
    assert u[0].shape == (2, RAGGED_T) and all(torch.equal(p, q[0]) for p, q in zip(u, want))


def test_search_fewer_prefixes_than_nbest(hip_device):
    case = [c for c in SEARCH_CASES if (c.T, c.C, c.beam) == (1, 2, 4)][0]
    got = gpu_search(case.lp[:, None], [1], 4, 4, 0, hip_device)[0]
    assert [l for l, _ in got[2:]] == [None, None] and {l for l, _ in got[:2]} == {(), (1,)}
    assert sorted(s for _, s in got[:2]) == sorted(float(v) for v in case.lp[0])   # one frame: the inputs themselves


def test_search_from_logits(hip_device):
    for case in (SEARCH_CASES[4], SEARCH_CASES[8], SEARCH_CASES[7]):
        h64, bound, separated, _, _, _ = case.ref()
        logits = np.random.RandomState(1000 + case.seed).randn(case.T, case.C).astype(np.float32)
        # the same distribution up to the fp32 rounding of the logits and one of logit - lse per entry of a path
        tol = bound + case.T * 2.0 ** -22 * float(np.abs(logits).max() + np.log(case.C))
        got = gpu_search(logits[:, None], [case.T], case.beam, case.beam, case.blank, hip_device, logits=True)[0]
        lp64 = D.log_softmax64(logits)
        err = max(abs(s + R.dp_cost(lp64, list(l), case.blank)) for l, s in got[:1])
        want, margin, _ = D.beam_search(lp64, case.beam, case.beam, case.blank)
        e_ref = max(abs(s - ws) for (_, s), (_, ws) in zip(got, want))
        print("CTCDECODE %-22s from logits: score err %.3g (tol %.3g, margin %.3g)" % (case.name, e_ref, tol, margin))
        if margin > 2 * tol:
            assert [l for l, _ in got] == [l for l, _ in want]
            assert e_ref <= tol
        assert all(s <= -R.dp_cost(lp64, list(l), case.blank) + tol for l, s in got)


def test_search_agrees_with_the_loss_kernel(hip_device):
    from pika_amd import ctc
    for case in ALL_SEARCH:
        _, bound, _, _, _, _ = case.ref()
        x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
        tokens, lengths, scores = ctc.ctc_beam_search(x, torch.tensor([case.T]), beam=case.beam, nbest=1,
                                                      blank=case.blank)
        U = int(lengths[0, 0])
        tg = tokens[0, :1, :max(U, 1)].clamp(min=0)
        cost = ctc.ctc_loss(x, tg, torch.tensor([case.T]), torch.tensor([U]), blank=case.blank, reduction="none")
        cost, score = float(cost[0]), float(scores[0, 0])
        print("CTCDECODE %-22s loss(top-1) + score = %.3g (bound %.3g)" % (case.name, cost + score, bound))
        assert cost <= -score + bound, (case.name, cost, score)
        if case.exhaustive:
            assert abs(cost + score) <= bound, (case.name, cost, score)


def test_search_ties_are_pinned(hip_device):
    # one frame, a constant row: every score is the input itself, nothing rounds; the empty prefix (it was in the beam)
    # first, then the classes ascending
    for C, blank, beam in ((6, 0, 6), (6, 3, 4), (300, 0, 16), (70, 69, 64)):
        v = np.float32(np.log(1.0 / C))
        lp = np.full((1, 1, C), v, dtype=np.float32)
        got = gpu_search(lp, [1], beam, beam, blank, hip_device)[0]
        classes = [c for c in range(C) if c != blank]
        assert [l for l, _ in got] == [()] + [(c,) for c in classes[:beam - 1]], (C, blank, got)
        assert all(s == float(v) for _, s in got)
    # equal frames: at frame 1 the stays (by previous rank) come before any fresh prefix of equal tot
    lp = np.full((2, 1, 3), np.float32(np.log(1.0 / 3.0)), dtype=np.float32)
    want, _, _ = D.beam_search(lp[:, 0], 8, 8)
    got = gpu_search(lp, [2], 8, 8, 0, hip_device)[0]
    assert [l for l, _ in got if l is not None] == [l for l, _ in want]


def test_search_two_runs_are_bit_identical(hip_device):
    from pika_amd import ctc
    for case in (SEARCH_CASES[4], SEARCH_CASES[9]):
        x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
        a = ctc.ctc_beam_search(x, torch.tensor([case.T]), beam=case.beam, nbest=case.beam)
        b = ctc.ctc_beam_search(x, torch.tensor([case.T]), beam=case.beam, nbest=case.beam)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    x = torch.from_numpy(D.case_lp(9, 1028, 3, B=2)).to(hip_device)
    a, b = ctc.ctc_greedy_decode(x, torch.tensor([9, 7])), ctc.ctc_greedy_decode(x, torch.tensor([9, 7]))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------
# greedy
# ---------------------------------------------------------------------------------------------------------------
def check_greedy(x_dev, lp, ils, blank, logits=False, name=""):
    """lp (T,B,C) numpy: what x_dev holds (for logits: the float64 log-softmax of it)."""
    from pika_amd import ctc
    fn = ctc.ctc_greedy_decode_from_logits if logits else ctc.ctc_greedy_decode
    tokens, lengths, scores, frames = fn(x_dev, torch.tensor(ils), blank=blank)
    T, B, C = lp.shape
    assert tokens.shape == (B, T) and frames.shape == (B, T) and lengths.shape == (B,) and scores.shape == (B,)
    assert tokens.dtype == frames.dtype == lengths.dtype == torch.int32 and scores.dtype == torch.float32
    tokens, lengths, scores, frames = (v.cpu().numpy() for v in (tokens, lengths, scores, frames))
    worst = 0.0
    for n in range(B):
        Tn = min(max(int(ils[n]), 1), T)
        want_t, want_f, want_s = D.greedy(lp[:Tn, n], blank)
        ln = int(lengths[n])
        assert ln == len(want_t) and tokens[n, :ln].tolist() == want_t and frames[n, :ln].tolist() == want_f, (name, n)
        assert (tokens[n, ln:] == -1).all() and (frames[n, ln:] == -1).all()
        tol = Tn * 2.0 ** -23 * abs(want_s)
        if logits:      # one fp32 rounding of logit - lse per frame
            tol += Tn * 2.0 ** -22 * float(np.abs(lp[:Tn, n]).max() + np.log(C))
        worst = max(worst, abs(float(scores[n]) - want_s) / max(tol, 1e-300))
        assert abs(float(scores[n]) - want_s) <= tol, (name, n, float(scores[n]), want_s, tol)
    print("CTCDECODE greedy %-24s score err / bound %.3g" % (name, worst))


GREEDY_SHAPES = [(1, 2, 5, 0), (9, 2, 1, 0), (9, 2, 2, 0), (9, 2, 2, 1), (11, 2, 7, 6), (11, 3, 7, 3), (300, 2, 260, 0),
                 (7, 2, 1028, 0), (5, 2, 5003, 77), (5, 2, 5003, 5002), (3, 1, 9001, 0)]


@pytest.mark.parametrize("T,B,C,blank", GREEDY_SHAPES)
def test_greedy_against_reference(hip_device, T, B, C, blank):
    lp = D.case_lp(T, C, 7 * T + C, B=B)
    ils = [T] + [max(1, T - 2)] * (B - 1)
    check_greedy(torch.from_numpy(lp).to(hip_device), lp, ils, blank, name="T%d_B%d_C%d_blank%d" % (T, B, C, blank))


def test_greedy_lengths_ties_strides(hip_device):
    from pika_amd import ctc
    dev = hip_device
    T, B, C = 13, 4, 8
    lp = D.case_lp(T, C, 5, B=B)
    # ragged, one length clamped from 0 and one from above T; padding frames are never read
    ils = [13, 0, 40, 6]
    x = lp.copy()
    x[1:, 1] = np.nan
    x[6:, 3] = np.nan
    check_greedy(torch.from_numpy(x).to(dev), lp, ils, 0, name="ragged_clamped")
    # rows of equal values: the lowest class wins -- the blank when it is class 0, class 0 when the blank is elsewhere
    flat = np.full((4, 1, 12), np.float32(np.log(1.0 / 12)), dtype=np.float32)
    for blank, want in ((0, []), (5, [0]), (11, [0])):
        tokens, lengths, _, frames = ctc.ctc_greedy_decode(torch.from_numpy(flat).to(dev), torch.tensor([4]), blank=blank)
        assert tokens[0, :int(lengths[0])].tolist() == want and frames[0, :int(lengths[0])].tolist() == [0] * len(want)
    flat[2, 0, 7] = flat[2, 0, 3] = np.float32(-0.5)       # two equal maxima: class 3
    check_greedy(torch.from_numpy(flat).to(dev), flat, [4], 0, name="equal_maxima")
    # an unaligned base: rows 4 bytes off a 16-byte boundary, C % 4 == 0 -> the scalar loads; and as a slice x[..., 1:]
    want = ctc.ctc_greedy_decode(torch.from_numpy(lp).to(dev), torch.tensor(ils))
    buf = torch.zeros(lp.size + 1, device=dev)
    y = buf[1:].view(T, B, C)
    y.copy_(torch.from_numpy(lp))
    assert y.data_ptr() % 16 == 4 and y.is_contiguous()
    wide = torch.zeros(T, B, C + 1, device=dev)
    wide[..., 1:] = torch.from_numpy(lp).to(dev)
    # non-contiguous: (B,T,C) seen time-major, and a class axis with stride 2 (the one form that is copied)
    bt = torch.from_numpy(lp).to(dev).transpose(0, 1).contiguous().transpose(0, 1)
    two = torch.zeros(T, B, 2 * C, device=dev)
    two[..., ::2] = torch.from_numpy(lp).to(dev)
    assert not bt.is_contiguous() and not wide[..., 1:].is_contiguous()
    for form in (y, wide[..., 1:], bt, two[..., ::2]):
        got = ctc.ctc_greedy_decode(form, torch.tensor(ils))
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        s_want = ctc.ctc_beam_search(torch.from_numpy(lp).to(dev), torch.tensor(ils), beam=4, nbest=4)
        s_got = ctc.ctc_beam_search(form, torch.tensor(ils), beam=4, nbest=4)
        assert all(torch.equal(a, b) for a, b in zip(s_got, s_want))
    # unbatched
    u = ctc.ctc_greedy_decode(torch.from_numpy(lp[:, 0]).to(dev), torch.tensor([T]))
    assert u[0].shape == (T,) and u[2].shape == () and all(torch.equal(a, b[0]) for a, b in zip(u, want))


def test_greedy_from_logits_agrees(hip_device):
    from pika_amd import ctc
    for T, B, C, blank in ((11, 3, 7, 3), (7, 2, 1028, 0), (5, 2, 5003, 77), (300, 2, 260, 0)):
        logits = np.random.RandomState(T + C).randn(T, B, C).astype(np.float32)
        lp64 = D.log_softmax64(logits)
        ils = [T, max(1, T - 3), T][:B]
        x = torch.from_numpy(logits).to(hip_device)
        check_greedy(x, lp64, ils, blank, logits=True, name="logits_T%d_C%d" % (T, C))
        a = ctc.ctc_greedy_decode_from_logits(x, torch.tensor(ils), blank=blank)
        b = ctc.ctc_greedy_decode(torch.log_softmax(x, -1), torch.tensor(ils), blank=blank)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
        assert torch.allclose(a[2], b[2], rtol=0, atol=T * 2 ** -21 * float(np.abs(logits).max() + np.log(C)))


def test_row_pass_many_equal_values(hip_device):
    # more candidates tie at the K-th value than the row pass's pool holds (1024): the exact selection and its
    # lowest-class-first rule, through the search's first frame
    C, beam = 3000, 16
    lp = np.full((1, 1, C), np.float32(-9.0), dtype=np.float32)
    lp[0, 0, 2000:2005] = np.float32(-1.0)
    lp[0, 0, 0] = np.float32(-2.0)                           # the blank
    got = gpu_search(lp, [1], beam, beam, 0, hip_device)[0]
    want = [(c,) for c in range(2000, 2005)] + [()] + [(c,) for c in range(1, 11)]
    assert [l for l, _ in got] == want


def test_graph_capture_equals_eager(hip_device):
    from pika_amd import ctc
    dev = hip_device
    T, B, C = 12, 3, 9
    data = [(D.case_lp(T, C, 60 + i, B=B), il) for i, il in enumerate(([12, 9, 10], [5, 12, 12], [12, 1, 7]))]

    def step(x, il):
        return (ctc.ctc_greedy_decode(x, il) + ctc.ctc_beam_search(x, il, beam=4, nbest=3)
                + ctc.ctc_greedy_decode_from_logits(x, il) + ctc.ctc_beam_search_from_logits(x, il, beam=4, nbest=3))

    sx = torch.from_numpy(data[0][0]).to(dev)
    sil = torch.tensor(data[0][1], dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up off the default stream, then one linear capture
        step(sx, sil)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sx, sil)
    for lp, il in data[1:]:
        sx.copy_(torch.from_numpy(lp))
        sil.copy_(torch.tensor(il, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = step(torch.from_numpy(lp).to(dev), torch.tensor(il, dtype=torch.int32, device=dev))
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)


def test_adjacent_buffers_keep_their_guards(hip_device):
    from pika_amd import _lib, ctc
    lib, dev = _lib.lib(), hip_device
    T, B, C, beam, nbest, GUARD = 10, 2, 37, 8, 5, 256
    K = 2 * beam
    lp = D.case_lp(T, C, 70, B=B)
    x = torch.from_numpy(lp).to(dev)
    il = torch.tensor([10, 8], dtype=torch.int32, device=dev)
    sizes = dict(blank_lp=4 * T * B, top_val=4 * T * B * K, top_idx=4 * T * B * K, blank1=4 * T * B, val1=4 * T * B,
                 idx1=4 * T * B, g_tokens=4 * B * T, g_lengths=4 * B, g_scores=4 * B, g_frames=4 * B * T,
                 tokens=4 * B * nbest * T, lengths=4 * B * nbest, scores=4 * B * nbest,
                 scratch=lib.pika_ctc_beam_scratch_bytes(B, T, beam))
    assert sizes["scratch"] > 0
    offs, total = {}, GUARD
    for name, nbytes in sizes.items():
        offs[name] = total
        total += (nbytes + 15) // 16 * 16 + GUARD
    arena = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    p = {name: arena.data_ptr() + o for name, o in offs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    st, sb = x.stride(0), x.stride(1)
    assert lib.pika_ctc_decode_rows(x.data_ptr(), st, sb, il.data_ptr(), B, T, C, 0, 1, 0, p["blank1"], p["val1"],
                                    p["idx1"], None, stream) == 0
    assert lib.pika_ctc_greedy(p["blank1"], p["val1"], p["idx1"], il.data_ptr(), B, T, C, 0, p["g_tokens"],
                               p["g_lengths"], p["g_scores"], p["g_frames"], stream) == 0
    assert lib.pika_ctc_decode_rows(x.data_ptr(), st, sb, il.data_ptr(), B, T, C, 0, K, 0, p["blank_lp"], p["top_val"],
                                    p["top_idx"], None, stream) == 0
    assert lib.pika_ctc_beam_search(x.data_ptr(), st, sb, None, p["blank_lp"], p["top_val"], p["top_idx"], il.data_ptr(),
                                    B, T, C, 0, beam, nbest, p["tokens"], p["lengths"], p["scores"], p["scratch"],
                                    stream) == 0
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    keep = np.ones(total, dtype=bool)
    for name, nbytes in sizes.items():
        keep[offs[name]:offs[name] + nbytes] = False
    assert (host[keep] == 0xA5).all(), "a kernel wrote outside its buffer"

    def view(name, dtype, shape):
        return np.frombuffer(host[offs[name]:offs[name] + sizes[name]].tobytes(), dtype=dtype).reshape(shape)
    g = ctc.ctc_greedy_decode(x, il)
    s = ctc.ctc_beam_search(x, il, beam=beam, nbest=nbest)
    assert (view("g_tokens", np.int32, (B, T)) == g[0].cpu().numpy()).all()
    assert (view("g_frames", np.int32, (B, T)) == g[3].cpu().numpy()).all()
    assert (view("g_scores", np.float32, (B,)) == g[2].cpu().numpy()).all()
    assert (view("tokens", np.int32, (B, nbest, T)) == s[0].cpu().numpy()).all()
    assert (view("lengths", np.int32, (B, nbest)) == s[1].cpu().numpy()).all()
    assert (view("scores", np.float32, (B, nbest)) == s[2].cpu().numpy()).all()
