"""CTC beam search with an LM and a second automaton (hotwords, or a second LM) on the MI355X against the reference of
tests/ctc_bias_common.py.

The reference is the float64 search with two automata on the SAME fp32 log-probs and the same two FSTs; the yardstick
is the same function in float32.  Per case bound = max(4 x the yardstick's largest error of a fused or acoustic score,
1e-6 * max|score|), and a case is *separated* when its margin exceeds 2 * bound -- the rule of the LM suite.  On
separated cases the token lists equal the reference's entry by entry and both scores lie within the bound; on every
case the entries are distinct and sorted, am_scores <= -dp_cost + bound, and scores - am_scores is within the bound of
lm_weight * LM + bias_weight * BIAS + length_bonus * length (+ the final terms) recomputed in float64 from the two FSTs.
Streaming: any chunking gives the one-shot call's bits.  Every measured error is printed (`CTCBIAS ...`) before it is
asserted.  tests/test_ctc_bias_surface.py checks the properties of the case list from the reference alone.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_bias_common as Bc  # noqa: E402
import ctc_lm_common as L  # noqa: E402
from test_ctc_lm_gpu import unpack  # noqa: E402

pytestmark = pytest.mark.gpu

_DEVICE = {}


def device_lm(ref, dev):
    """One upload per reference automaton."""
    from pika_amd import ctc
    if id(ref) not in _DEVICE:
        _DEVICE[id(ref)] = (ref, ctc.CtcNgramLm(ref.fst, ref.backoff_id, ref.label_offset, device=dev))
    return _DEVICE[id(ref)][1]


def device_bias(case, dev):
    """The case's second automaton on the device: hotword cases go through `CtcHotwords` itself."""
    from pika_amd import ctc
    key = ("bias", id(case.bias))
    if key not in _DEVICE:
        if case.phrases is None:
            return device_lm(case.bias, dev)
        hot = ctc.CtcHotwords(case.phrases, case.C, boost=case.boost, blank=case.blank, device=dev)
        assert hot.num_states == case.bias.fst.num_states and hot.backoff_id == case.C + 1
        assert np.array_equal(hot.weight.cpu().numpy(), case.bias.fst.weight)
        _DEVICE[key] = (case.bias, hot)
    return _DEVICE[key][1]


def pair(case, dev, bias_weight=None):
    from pika_amd import ctc
    return ctc.CtcBiasedLm(device_lm(case.lm, dev), device_bias(case, dev),
                           case.bias_weight if bias_weight is None else bias_weight)


def search_kw(case, nbest, use_final=None):
    return dict(beam=case.beam, nbest=nbest, blank=case.blank, lm_weight=case.lm_weight, length_bonus=case.length_bonus,
                candidates=case.candidates, use_final=case.use_final if use_final is None else use_final)


def gpu_search(case, lp, ils, nbest, dev, logits=False):
    """lp (T,B,C) numpy -> per utterance [(label tuple, score, am_score)], missing entries as (None, -inf, -inf)."""
    from pika_amd import ctc
    fn = ctc.ctc_beam_search_lm_from_logits if logits else ctc.ctc_beam_search_lm
    out = fn(torch.from_numpy(lp).to(dev), torch.tensor(ils), pair(case, dev), **search_kw(case, nbest))
    return unpack(out, lp.shape[0], lp.shape[1], nbest)


def check_hyps(case, got, nbest, what=""):
    h64, bound, separated, _, margin, err32 = case.ref()
    want = h64[:nbest]
    real = [h for h in got if h[0] is not None]
    assert len(real) == len(want) and all(h[0] is None for h in got[len(real):]), (case.name, got)
    labels = [h[0] for h in real]
    assert len(set(labels)) == len(labels), (case.name, "two entries denote the same label sequence")
    lp64 = case.lp.astype(np.float64)
    over, e_t = -np.inf, 0.0
    for l, s, am in real:
        over = max(over, am + R.dp_cost(lp64, list(l), case.blank))
        term = case.terms(l)
        assert term is not None, (case.name, l, "an automaton cannot produce this prefix")
        e_t = max(e_t, abs(s - am - term))
    e_f = max([abs(g[1] - w[1]) for g, w in zip(real, want)] + [0.0]) if separated else float("nan")
    e_a = max([abs(g[2] - w[2]) for g, w in zip(real, want)] + [0.0]) if separated else float("nan")
    print("CTCBIAS %-32s %s nbest %2d  fused err %.3g  am err %.3g  am over -dp_cost %.3g  |fused - am - LM64 - BIAS64 "
          "terms| %.3g  (bound %.3g, float32 err %.3g, margin %.3g, %s)" % (
              case.name, what, nbest, e_f, e_a, over, e_t, bound, err32, margin,
              "separated" if separated else "NOT separated"))
    for x, y in zip(real, real[1:]):
        assert x[1] >= y[1], (case.name, "not sorted")
    assert over <= bound, (case.name, over, bound)
    assert e_t <= bound, (case.name, e_t, bound)
    if separated:
        assert labels == [w[0] for w in want], (case.name, labels, want)
        assert e_f <= bound and e_a <= bound, (case.name, e_f, e_a, bound)


@pytest.mark.parametrize("case", Bc.BIAS_CASES, ids=lambda c: c.name)
def test_search_against_float64(hip_device, case):
    got = gpu_search(case, case.lp[:, None], [case.T], case.beam, hip_device)[0]
    check_hyps(case, got, case.beam)
    first = gpu_search(case, case.lp[:, None], [case.T], 1, hip_device)[0]
    assert first == got[:1]                     # nbest = 1 is the head of nbest = beam


def test_search_from_logits(hip_device):
    for case in (Bc.BIAS_CASES[1], Bc.BIAS_CASES[4]):
        # the logits whose float64 log-softmax, rounded to fp32, is the case's lp (tests/ctc_decode_common.case_lp)
        logits = np.random.RandomState(1000 + case.seed).randn(case.T, case.C).astype(np.float32)
        _, bound, separated, _, _, _ = case.ref()
        got = gpu_search(case, logits[:, None], [case.T], case.beam, hip_device, logits=True)[0]
        plain = gpu_search(case, case.lp[:, None], [case.T], case.beam, hip_device)[0]
        same = [g[0] for g in got] == [p[0] for p in plain]
        e_form = max(max(abs(g[1] - p[1]), abs(g[2] - p[2])) for g, p in zip(got, plain)) if same else float("nan")
        print("CTCBIAS %-32s from logits against the log-prob form: %.3g (bound %.3g)" % (case.name, e_form, bound))
        if separated:
            assert same, case.name
            assert e_form <= bound, (case.name, e_form, bound)


def test_search_ragged_batch(hip_device):
    from pika_amd import ctc
    dev = hip_device
    lp, ils, c0 = Bc.RAGGED_LP.copy(), Bc.RAGGED_ILS, Bc.RAGGED_CASES[0]
    for nbest in (1, Bc.RAGGED_BEAM):
        got = gpu_search(c0, lp, ils, nbest, dev)
        for case, hyps in zip(Bc.RAGGED_CASES, got):
            check_hyps(case, hyps, nbest)
    # host / device lengths, int32 / int64
    both = pair(c0, dev)
    x = torch.from_numpy(lp).to(dev)
    kw = search_kw(c0, 2)
    want = ctc.ctc_beam_search_lm(x, torch.tensor(ils), both, **kw)
    for il in (torch.tensor(ils, dtype=torch.int32), torch.tensor(ils).to(dev),
               torch.tensor(ils, dtype=torch.int32).to(dev)):
        for u, v in zip(want, ctc.ctc_beam_search_lm(x, il, both, **kw)):
            assert torch.equal(u, v)
    # a (B,T,C) tensor seen time-major
    bt = x.transpose(0, 1).contiguous().transpose(0, 1)
    assert not bt.is_contiguous()
    for p, q in zip(want, ctc.ctc_beam_search_lm(bt, torch.tensor(ils), both, **kw)):
        assert torch.equal(p, q)


def test_bad_second_automaton_is_refused(hip_device):
    from pika_amd import ctc
    case = Bc.BIAS_CASES[0]
    lm = device_lm(case.lm, hip_device)
    x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
    # hotwords compiled for fewer classes than the input has: their back-off label is a class of the input
    small = ctc.CtcHotwords([(1,)], case.C - 1, device=hip_device)
    with pytest.raises(ValueError, match="backoff_id"):
        ctc.ctc_beam_search_lm(x, torch.tensor([case.T]), ctc.CtcBiasedLm(lm, small), beam=2)
    stream = ctc.CtcBeamStream(1, case.T, beam=2, lm=ctc.CtcBiasedLm(lm, small), device=hip_device)
    with pytest.raises(ValueError, match="backoff_id"):
        stream.advance(x)


# ---------------------------------------------------------------------------------------------------------------
# the one-automaton paths are what they were
# ---------------------------------------------------------------------------------------------------------------
def direct_one_fst(case, x, lm, nbest):
    """pika_ctc_lm_beam_search through the C ABI, as the parent commit's Python called it."""
    from pika_amd import _lib
    lib = _lib.lib()
    T, B, C = x.shape
    dev, K = x.device, case.candidates
    il = torch.tensor([case.T], dtype=torch.int32, device=dev)
    blank_lp = torch.empty((T, B), device=dev)
    top_val = torch.empty((T, B, K), device=dev)
    top_idx = torch.empty((T, B, K), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pika_ctc_decode_rows(x.data_ptr(), x.stride(0), x.stride(1), il.data_ptr(), B, T, C, case.blank, K, 0,
                                    blank_lp.data_ptr(), top_val.data_ptr(), top_idx.data_ptr(), None, stream) == 0
    tokens = torch.empty((B, nbest, T), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, nbest), dtype=torch.int32, device=dev)
    scores, am = torch.empty((B, nbest), device=dev), torch.empty((B, nbest), device=dev)
    scratch = torch.empty(lib.pika_ctc_lm_scratch_bytes(B, T, case.beam, K), dtype=torch.uint8, device=dev)
    assert lib.pika_ctc_lm_beam_search(
        x.data_ptr(), x.stride(0), x.stride(1), None, blank_lp.data_ptr(), top_val.data_ptr(), top_idx.data_ptr(),
        il.data_ptr(), B, T, C, case.blank, case.beam, nbest, *L.fst_args(lm), K, case.lm_weight, case.length_bonus,
        int(case.use_final), tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), am.data_ptr(), scratch.data_ptr(),
        stream) == 0
    return tokens, lengths, scores, am


def test_without_a_second_automaton_nothing_changed(hip_device):
    from pika_amd import ctc
    dev = hip_device
    for case in (Bc.BIAS_CASES[2], Bc.BIAS_CASES[6]):          # the small and the large cells
        lm = device_lm(case.lm, dev)
        x = torch.from_numpy(case.lp[:, None].copy()).to(dev)
        kw = search_kw(case, case.beam)
        want = direct_one_fst(case, x, lm, case.beam)
        got = ctc.ctc_beam_search_lm(x, torch.tensor([case.T]), lm, **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), case.name
        stream = ctc.CtcBeamStream(1, case.T, beam=case.beam, blank=case.blank, lm=lm, lm_weight=case.lm_weight,
                                   length_bonus=case.length_bonus, candidates=case.candidates, device=dev)
        assert stream._hdr.shape[1] * 4 == 2592                # the LM record, not the wider one
        for s in range(0, case.T, 3):
            stream.advance(x[s:s + 3])
        got = stream.results(nbest=case.beam, use_final=case.use_final)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), case.name
        # hotwords with weight 0 reach every class and add 0.0 to every bonus: the same bits out of the two-FST kernel
        got = ctc.ctc_beam_search_lm(x, torch.tensor([case.T]), pair(case, dev, bias_weight=0.0), **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), case.name
    # hotwords alone are an LM: the one-FST search, boost per matched token
    case = Bc.BIAS_CASES[0]
    hot = device_bias(case, dev)
    x = torch.from_numpy(case.lp[:, None].copy()).to(dev)
    tokens, lengths, scores, am = ctc.ctc_beam_search_lm(x, torch.tensor([case.T]), hot, beam=case.beam,
                                                         nbest=case.beam, lm_weight=1.0, candidates=case.candidates)
    for k in range(case.beam):
        if int(lengths[0, k]) >= 0:
            l = tuple(int(v) for v in tokens[0, k, :int(lengths[0, k])])
            want = Bc.hot_bias(case.phrases, l, case.boost, final=True)
            assert abs(float(scores[0, k]) - float(am[0, k]) - want) <= 1e-5 * max(1.0, abs(float(scores[0, k])))


# ---------------------------------------------------------------------------------------------------------------
# streaming
# ---------------------------------------------------------------------------------------------------------------
def bias_stream(case, dev, batch=1, max_frames=None):
    from pika_amd import ctc
    return ctc.CtcBeamStream(batch, case.T if max_frames is None else max_frames, beam=case.beam, blank=case.blank,
                             lm=pair(case, dev), lm_weight=case.lm_weight, length_bonus=case.length_bonus,
                             candidates=case.candidates, device=dev)


def one_shot(case, x, ils, nbest, use_final, dev):
    from pika_amd import ctc
    return ctc.ctc_beam_search_lm(x, torch.tensor(ils), pair(case, dev), **search_kw(case, nbest, use_final))


def assert_same(got, want, T):
    assert torch.equal(got[0][..., :T], want[0]) and bool((got[0][..., T:] == -1).all())
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and torch.equal(g, w)


STREAM_CASES = [Bc.BIAS_CASES[i] for i in (1, 2, 6, 7, 9, 10, 13)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_chunked_equals_one_shot(hip_device, case):
    x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
    want = {uf: one_shot(case, x, [case.T], case.beam, uf, hip_device) for uf in (True, False)}
    stream = bias_stream(case, hip_device)
    assert stream._hdr.shape[1] * 4 == 2592 + 256
    for k in (1, 3, 8, case.T):
        if case.T >= 600 and k == 1:
            continue                            # 600 launches: chunks of 3 cross every renormalisation phase as well
        stream.reset()
        for s in range(0, case.T, k):
            stream.advance(x[s:s + k])
            if s == (case.T // (2 * k)) * k and s + k < case.T:           # a look in the middle, both settings
                part = {uf: stream.results(nbest=case.beam, use_final=uf) for uf in (True, False)}
                if k in (8, case.T):
                    for uf in (True, False):
                        assert_same(part[uf], one_shot(case, x[:s + k], [s + k], case.beam, uf, hip_device), s + k)
        got = {uf: stream.results(nbest=case.beam, use_final=uf) for uf in (True, False)}
        for uf in (True, False):
            assert_same(got[uf], want[uf], case.T)
        assert_same(stream.results(nbest=case.beam, use_final=True), want[True], case.T)      # nothing stuck
        assert stream.frames.tolist() == [case.T] and stream.overflowed.tolist() == [False]


def test_stream_ragged_idle_and_reset(hip_device):
    dev, ils, T, beam = hip_device, Bc.RAGGED_ILS, Bc.RAGGED_T, Bc.RAGGED_BEAM
    c0 = Bc.RAGGED_CASES[0]
    x = torch.from_numpy(Bc.RAGGED_LP).to(dev)
    want = one_shot(c0, x, ils, beam, True, dev)
    stream = bias_stream(c0, dev, batch=3, max_frames=24)
    sizes = [4, 4, 4, 2]
    assert [int(min(max(ils[1] - s, 0), 4)) for s in (0, 4, 8, 12)] == [4, 4, 1, 0]           # stream 1 idles at the end
    for form in (lambda v: v, lambda v: torch.tensor(v, dtype=torch.int32, device=dev)):
        stream.reset()
        s = 0
        for k in sizes:
            stream.advance(x[s:s + k], form([int(min(max(il - s, 0), k)) for il in ils]))
            s += k
        got = stream.results(nbest=beam)
        assert_same(got, want, T)
        assert stream.frames.tolist() == ils
    for n, case in enumerate(Bc.RAGGED_CASES):
        check_hyps(case, unpack(tuple(o[n:n + 1, :, :case.T] if i == 0 else o[n:n + 1] for i, o in enumerate(got)),
                                case.T, 1, beam)[0], beam, what="stream")
    # reset(which) in the middle: stream 1 starts utterance 2's frames anew -- in BOTH start states -- while 0 goes on
    stream.reset()
    stream.advance(x[0:6], [6, 6, 0])
    stream.reset(which=[False, True, False])
    assert stream.frames.tolist() == [6, 0, 0]
    y = x.clone()
    y[:, 1] = x[:, 2]
    stream.advance(y[0:6], [0, 6, 6])
    stream.advance(torch.cat([x[6:14, 0:1], y[6:14, 1:2], x[6:14, 2:3]], 1), [8, 5, 5])
    got = stream.results(nbest=beam)
    want2 = one_shot(c0, torch.stack([x[:, 0], x[:, 2], x[:, 2]], 1), [14, 11, 11], beam, True, dev)
    assert_same(got, want2, T)


def test_stream_overflow_and_graph_capture(hip_device):
    dev, beam = hip_device, Bc.RAGGED_BEAM
    c0 = Bc.RAGGED_CASES[0]
    x = torch.from_numpy(Bc.RAGGED_LP).to(dev)
    stream = bias_stream(c0, dev, batch=3, max_frames=8)
    buf = x[0:4].clone()
    lens = torch.full((3,), 4, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):               # warm-up off the default stream, then one linear capture
        stream.advance(buf, lens)
        stream.results(nbest=beam)
    torch.cuda.current_stream().wait_stream(side)
    stream.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream.advance(buf, lens)
        outs = stream.results(nbest=beam)
    stream.reset()
    for i in range(2):                          # two replays fill the stream
        buf.copy_(x[4 * i:4 * i + 4])
        graph.replay()
    torch.cuda.synchronize()
    assert_same(outs, one_shot(c0, x[:8], [8, 8, 8], beam, True, dev), 8)
    assert stream.frames.tolist() == [8, 8, 8] and stream.overflowed.tolist() == [False] * 3
    lens.copy_(torch.tensor([4, 0, 4], dtype=torch.int32))
    graph.replay()                              # the host cannot see a replay: the device drops the frames
    torch.cuda.synchronize()
    assert stream.frames.tolist() == [8, 8, 8] and stream.overflowed.tolist() == [True, False, True]
    assert_same(outs, one_shot(c0, x[:8], [8, 8, 8], beam, True, dev), 8)
    # what the host can see it refuses before any launch
    fresh = bias_stream(c0, dev, batch=3, max_frames=8)
    fresh.advance(x[0:4])
    fresh.advance(x[4:8])
    with pytest.raises(ValueError, match="max_frames"):
        fresh.advance(x[8:12])
    assert_same(fresh.results(nbest=beam), one_shot(c0, x[:8], [8, 8, 8], beam, True, dev), 8)
