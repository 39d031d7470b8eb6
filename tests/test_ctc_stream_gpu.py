"""Streaming CTC beam search on the MI355X: `CtcBeamStream` against the one-shot searches and the float64 references.

The acceptance criterion is exact: ANY chunking of the frames gives bit for bit (`torch.equal`) what `ctc_beam_search`
/ `ctc_beam_search_lm` give on the whole tensor -- the streaming kernels run the one-shot kernels' per-frame code on a
state that rests in device memory between launches.  So that the test does not rest on the two code paths sharing a bug,
every chunked result also goes through the float64 checks of tests/test_ctc_decode_gpu.py and tests/test_ctc_lm_gpu.py,
restated here: per case the bound is max(4 x the float32 yardstick's largest score error, 1e-6 * max|score|); a case is
*separated* when the reference's margin exceeds 2 * bound.  Plain search: on separated cases the label lists equal the
reference's entry by entry and the scores lie within the bound; on every case the entries are distinct and sorted and
score <= -dp_cost + bound; on exhaustive cases |score + dp_cost| <= bound.  LM search: the same with the fused and the
acoustic score, am_score <= -dp_cost + bound, and scores - am_scores within the bound of lm_weight * LM + length_bonus *
length (+ the final term), the LM part recomputed in float64 from the FST.  One `CTCSTREAM` line is printed per case
and chunking before anything is asserted; profiles/ctc_stream_parity.txt keeps that output.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_decode_common as D  # noqa: E402
import ctc_lm_common as L  # noqa: E402

pytestmark = pytest.mark.gpu

_DEVICE_LMS = {}
_CHECKED = {}


def device_lm(lm, dev):
    """One upload per reference LM."""
    from pika_amd import ctc
    if id(lm) not in _DEVICE_LMS:
        _DEVICE_LMS[id(lm)] = (lm, ctc.CtcNgramLm(lm.fst, lm.backoff_id, lm.label_offset, device=dev))
    return _DEVICE_LMS[id(lm)][1]


def chunkings(T, seed):
    """name -> chunk sizes: frame by frame; 3 (does not divide 8: boundaries at every renormalisation phase); 8; 5; one
    chunk; one uneven seeded split."""
    def fixed(k):
        return [min(k, T - s) for s in range(0, T, k)]
    rng = np.random.RandomState(500 + seed)
    uneven, left = [], T
    while left:
        uneven.append(int(rng.randint(1, min(left, 11) + 1)))
        left -= uneven[-1]
    return [("1", fixed(1)), ("3", fixed(3)), ("8", fixed(8)), ("5", fixed(5)), ("T", [T]), ("uneven", uneven)]


def feed(stream, x, sizes, ils=None, logits=False, lengths_as=None):
    """The frames of x (T,B,C) in chunks of `sizes`; ils: per-utterance lengths -> per-chunk lengths clip(il - start)."""
    start = 0
    fn = stream.advance_from_logits if logits else stream.advance
    for k in sizes:
        lengths = None
        if ils is not None:
            lengths = [int(min(max(il - start, 0), k)) for il in ils]
            if lengths_as is not None:
                lengths = lengths_as(lengths)
        fn(x[start:start + k], lengths)
        start += k


def assert_same(got, want, T):
    """The stream's outputs (token width = max_frames >= T) against the one-shot's (width T), bit for bit."""
    assert torch.equal(got[0][..., :T], want[0]) and bool((got[0][..., T:] == -1).all())
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and torch.equal(g, w)


def hyps_of(out, n=0):
    """Outputs -> [(labels or None, scores...)] of utterance n."""
    tokens, lengths = out[0].cpu().numpy(), out[1].cpu().numpy()
    rest = [o.cpu().numpy() for o in out[2:]]
    res = []
    for k in range(tokens.shape[1]):
        ln = int(lengths[n, k])
        labels = None if ln < 0 else tuple(int(v) for v in tokens[n, k, :ln])
        res.append((labels,) + tuple(float(r[n, k]) for r in rest))
    return tuple(res)


def check_plain(case, got, what):
    """The float64 check of the one-shot test on got = [(labels, score)] (nbest = beam)."""
    key = (case.name, got)
    if key not in _CHECKED:
        h64, bound, separated, _, margin, _ = case.ref()
        real = [(l, s) for l, s in got if l is not None]
        assert len(real) == len(h64) and all(l is None for l, _ in got[len(real):]), (case.name, got)
        labels = [l for l, _ in real]
        assert len(set(labels)) == len(labels), (case.name, "two entries denote the same label sequence")
        lp64 = case.lp.astype(np.float64)
        full = [-R.dp_cost(lp64, list(l), case.blank) for l in labels]
        e_ref = max([abs(s - ws) for (_, s), (_, ws) in zip(real, h64)] + [0.0]) if separated else float("nan")
        over = max(s - f for (_, s), f in zip(real, full))
        e_full = max(abs(s - f) for (_, s), f in zip(real, full))
        _CHECKED[key] = (e_ref, over, e_full, labels, real)
    e_ref, over, e_full, labels, real = _CHECKED[key]
    h64, bound, separated, _, margin, _ = case.ref()
    print("CTCSTREAM %-22s chunks %-6s score err %.3g  over -dp_cost %.3g  |score + dp_cost| %.3g  (bound %.3g, margin "
          "%.3g, %s)  == one-shot" % (case.name, what, e_ref, over, e_full, bound, margin,
                                     "separated" if separated else "NOT separated"))
    for (_, a), (_, b) in zip(real, real[1:]):
        assert a >= b, (case.name, "not sorted")
    assert over <= bound, (case.name, over, bound)
    if separated:
        assert labels == [l for l, _ in h64], (case.name, labels, h64)
        assert e_ref <= bound, (case.name, e_ref, bound)
    if case.exhaustive:
        assert e_full <= bound, (case.name, e_full, bound)


def check_lm(case, got, what):
    """The float64 check of the one-shot LM test on got = [(labels, score, am_score)] (nbest = beam, the case's own
    use_final)."""
    h64, bound, separated, _, margin, _ = case.ref()
    key = (case.name, got)
    if key not in _CHECKED:
        real = [h for h in got if h[0] is not None]
        assert len(real) == len(h64[:case.beam]) and all(h[0] is None for h in got[len(real):]), (case.name, got)
        labels = [h[0] for h in real]
        assert len(set(labels)) == len(labels), (case.name, "two entries denote the same label sequence")
        lp64 = case.lp.astype(np.float64)
        over, e_lm = -np.inf, 0.0
        for l, s, am in real:
            over = max(over, am + R.dp_cost(lp64, list(l), case.blank))
            lm64 = case.lm.score(l)
            assert lm64 is not None, (case.name, l, "the LM cannot produce this prefix")
            term = case.lm_weight * lm64[0] + case.length_bonus * len(l)
            if case.use_final:
                fin = case.lm.final(lm64[1])
                assert fin is not None, (case.name, l, "no final state")
                term += case.lm_weight * float(fin)
            e_lm = max(e_lm, abs(s - am - term))
        want = h64[:case.beam]
        e_f = max([abs(g[1] - w[1]) for g, w in zip(real, want)] + [0.0]) if separated else float("nan")
        e_a = max([abs(g[2] - w[2]) for g, w in zip(real, want)] + [0.0]) if separated else float("nan")
        _CHECKED[key] = (over, e_lm, e_f, e_a, labels, real)
    over, e_lm, e_f, e_a, labels, real = _CHECKED[key]
    print("CTCSTREAM %-28s chunks %-6s fused err %.3g  am err %.3g  am over -dp_cost %.3g  |fused - am - LM64 terms| "
          "%.3g  (bound %.3g, margin %.3g, %s)  == one-shot" % (case.name, what, e_f, e_a, over, e_lm, bound, margin,
                                                               "separated" if separated else "NOT separated"))
    for x, y in zip(real, real[1:]):
        assert x[1] >= y[1], (case.name, "not sorted")
    assert over <= bound, (case.name, over, bound)
    assert e_lm <= bound, (case.name, e_lm, bound)
    if separated:
        assert labels == [w[0] for w in h64[:case.beam]], (case.name, labels)
        assert e_f <= bound and e_a <= bound, (case.name, e_f, e_a, bound)


def lm_stream(case, dev, batch=1, max_frames=None):
    from pika_amd import ctc
    return ctc.CtcBeamStream(batch, case.T if max_frames is None else max_frames, beam=case.beam, blank=case.blank,
                             lm=device_lm(case.lm, dev), lm_weight=case.lm_weight, length_bonus=case.length_bonus,
                             candidates=case.candidates, device=dev)


def lm_one_shot(case, x, ils, nbest, use_final, dev, logits=False):
    from pika_amd import ctc
    fn = ctc.ctc_beam_search_lm_from_logits if logits else ctc.ctc_beam_search_lm
    return fn(x, torch.tensor(ils), device_lm(case.lm, dev), beam=case.beam, nbest=nbest, blank=case.blank,
              lm_weight=case.lm_weight, length_bonus=case.length_bonus, candidates=case.candidates, use_final=use_final)


# ---------------------------------------------------------------------------------------------------------------
# 1. chunked equals one-shot, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.ALL_SEARCH, ids=lambda c: c.name)
def test_chunked_equals_one_shot(hip_device, case):
    from pika_amd import ctc
    x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
    want = ctc.ctc_beam_search(x, torch.tensor([case.T]), beam=case.beam, nbest=case.beam, blank=case.blank)
    stream = ctc.CtcBeamStream(1, case.T, beam=case.beam, blank=case.blank, device=hip_device)
    for name, sizes in chunkings(case.T, case.seed):
        stream.reset()
        feed(stream, x, sizes)
        got = stream.results(nbest=case.beam)
        assert len(got) == 3 and got[0].shape == (1, case.beam, case.T)
        check_plain(case, hyps_of(got), name)          # prints before the bitwise assertion
        assert_same(got, want, case.T)
        assert stream.frames.tolist() == [case.T] and stream.overflowed.tolist() == [False]


# ---------------------------------------------------------------------------------------------------------------
# 2. ragged batch
# ---------------------------------------------------------------------------------------------------------------
def test_ragged_batch(hip_device):
    from pika_amd import ctc
    dev, ils, T = hip_device, D.RAGGED_ILS, D.RAGGED_T
    lp = D.RAGGED_LP.copy()
    x = torch.from_numpy(lp).to(dev)
    want = ctc.ctc_beam_search(x, torch.tensor(ils), beam=D.RAGGED_BEAM, nbest=D.RAGGED_BEAM)
    sizes = [4, 4, 4, 2]
    assert [int(min(max(ils[1] - s, 0), 4)) for s in (0, 4, 8, 12)] == [4, 4, 1, 0]
    dirty = lp.copy()
    for n, il in enumerate(ils):
        dirty[il:, n] = np.nan                         # frames beyond each length are never used
    stream = ctc.CtcBeamStream(3, T, beam=D.RAGGED_BEAM, device=dev)
    forms = [None, lambda v: torch.tensor(v, dtype=torch.int32), lambda v: torch.tensor(v, dtype=torch.int64),
             lambda v: torch.tensor(v, dtype=torch.int32, device=dev), lambda v: torch.tensor(v, device=dev)]
    for data in (x, torch.from_numpy(dirty).to(dev)):
        for form in forms:
            stream.reset()
            feed(stream, data, sizes, ils, lengths_as=form)
            got = stream.results(nbest=D.RAGGED_BEAM)
            assert_same(got, want, T)
            assert stream.frames.tolist() == ils
    for n, case in enumerate(D.RAGGED_CASES):
        check_plain(case, hyps_of(got, n), "4")


# ---------------------------------------------------------------------------------------------------------------
# 3. capacity does not matter
# ---------------------------------------------------------------------------------------------------------------
def test_capacity_does_not_matter(hip_device):
    from pika_amd import ctc
    for case in (D.SEARCH_CASES[4], D.SEARCH_CASES[7]):
        x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
        outs = []
        for cap in (case.T, 4 * case.T):               # another table size: every node id differs
            stream = ctc.CtcBeamStream(1, cap, beam=case.beam, blank=case.blank, device=hip_device)
            feed(stream, x, [min(5, case.T - s) for s in range(0, case.T, 5)])
            outs.append(stream.results(nbest=case.beam))
            assert outs[-1][0].shape[-1] == cap
        assert_same(outs[1], tuple(o[..., :case.T] if i == 0 else o for i, o in enumerate(outs[0])), case.T)


# ---------------------------------------------------------------------------------------------------------------
# 4. partial results are non-destructive
# ---------------------------------------------------------------------------------------------------------------
def test_partial_results_are_non_destructive(hip_device):
    from pika_amd import ctc
    for case in (D.SearchCase(24, 4, 4, 2), D.SearchCase(30, 4, 3, 3)):
        x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
        watched = ctc.CtcBeamStream(1, case.T, beam=case.beam, device=hip_device)
        quiet = ctc.CtcBeamStream(1, case.T, beam=case.beam, device=hip_device)
        for s in range(0, case.T, 5):
            k = min(s + 5, case.T)
            watched.advance(x[s:k])
            quiet.advance(x[s:k])
            part = watched.results(nbest=case.beam)
            assert_same(part, ctc.ctc_beam_search(x[:k], torch.tensor([k]), beam=case.beam, nbest=case.beam), k)
        for a, b in zip(watched.results(nbest=case.beam), quiet.results(nbest=case.beam)):
            assert torch.equal(a, b)
    # with an LM: the final term is applied on the side at every look
    case = L.LM_CASES[2]
    x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
    watched, quiet = lm_stream(case, hip_device), lm_stream(case, hip_device)
    for s in range(0, case.T, 5):
        k = min(s + 5, case.T)
        watched.advance(x[s:k])
        quiet.advance(x[s:k])
        for uf in (True, False):
            assert_same(watched.results(nbest=case.beam, use_final=uf),
                        lm_one_shot(case, x[:k], [k], case.beam, uf, hip_device), k)
    for a, b in zip(watched.results(nbest=case.beam), quiet.results(nbest=case.beam)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# 5. reset of one stream
# ---------------------------------------------------------------------------------------------------------------
def test_reset_of_one_stream(hip_device):
    from pika_amd import ctc
    dev, C, beam = hip_device, 6, 4
    X, Y, Z = D.case_lp(22, C, 81), D.case_lp(16, C, 82), D.case_lp(13, C, 83)
    stream = ctc.CtcBeamStream(2, 24, beam=beam, device=dev)

    def chunk(a, sa, b, sb):
        """Four frames of a from sa next to four of b from sb, with the lengths either side has left."""
        buf = np.zeros((4, 2, C), dtype=np.float32)
        la, lb = min(max(len(a) - sa, 0), 4), min(max(len(b) - sb, 0), 4)
        buf[:la, 0], buf[:lb, 1] = a[sa:sa + la], b[sb:sb + lb]
        return torch.from_numpy(buf).to(dev), [la, lb]

    for s in (0, 4):                                   # X and Y side by side, until Y is cut off half-way
        stream.advance(*chunk(X, s, Y, s))
    assert stream.frames.tolist() == [8, 8]
    stream.reset(which=[False, True])
    assert stream.frames.tolist() == [8, 0]
    for s in (8, 12, 16, 20):                          # X goes on; Z from its start; lengths 0 where a side has run out
        stream.advance(*chunk(X, s, Z, s - 8))
    assert stream.frames.tolist() == [22, 13]
    got = stream.results(nbest=beam)
    for n, lp in ((0, X), (1, Z)):
        x = torch.from_numpy(lp[:, None].copy()).to(dev)
        want = ctc.ctc_beam_search(x, torch.tensor([len(lp)]), beam=beam, nbest=beam)
        assert_same(tuple(o[n:n + 1] for o in got), want, len(lp))
    # the selection as a device tensor of another dtype
    stream.reset(which=torch.tensor([1, 0], device=dev))
    assert stream.frames.tolist() == [0, 13]


# ---------------------------------------------------------------------------------------------------------------
# 6. from logits
# ---------------------------------------------------------------------------------------------------------------
def test_from_logits(hip_device):
    from pika_amd import ctc
    case = D.SEARCH_CASES[4]
    logits = torch.from_numpy(np.random.RandomState(1000 + case.seed).randn(case.T, 1, case.C).astype(np.float32))
    logits = logits.to(hip_device)
    sizes = [min(3, case.T - s) for s in range(0, case.T, 3)]
    stream = ctc.CtcBeamStream(1, case.T, beam=case.beam, blank=case.blank, device=hip_device)
    feed(stream, logits, sizes, logits=True)
    assert_same(stream.results(nbest=case.beam),
                ctc.ctc_beam_search_from_logits(logits, torch.tensor([case.T]), beam=case.beam, nbest=case.beam), case.T)
    case = L.LM_CASES[3]
    logits = torch.from_numpy(np.random.RandomState(1000 + case.seed).randn(case.T, 1, case.C).astype(np.float32))
    logits = logits.to(hip_device)
    stream = lm_stream(case, hip_device)
    feed(stream, logits, sizes, logits=True)
    assert_same(stream.results(nbest=case.beam, use_final=case.use_final),
                lm_one_shot(case, logits, [case.T], case.beam, case.use_final, hip_device, logits=True), case.T)


# ---------------------------------------------------------------------------------------------------------------
# 7. LM-fused
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.ALL_CASES, ids=lambda c: c.name)
def test_lm_chunked_equals_one_shot(hip_device, case):
    x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
    want = {uf: lm_one_shot(case, x, [case.T], case.beam, uf, hip_device) for uf in (True, False)}
    stream = lm_stream(case, hip_device)
    for name, k in (("1", 1), ("3", 3), ("T", case.T)):
        stream.reset()
        feed(stream, x, [min(k, case.T - s) for s in range(0, case.T, k)])
        got = {uf: stream.results(nbest=case.beam, use_final=uf) for uf in (True, False)}
        again = stream.results(nbest=case.beam, use_final=True)       # the final term did not stick
        assert len(again) == 4
        check_lm(case, hyps_of(got[case.use_final]), name)
        for uf in (True, False):
            assert_same(got[uf], want[uf], case.T)
        assert_same(again, want[True], case.T)


# ---------------------------------------------------------------------------------------------------------------
# 8. / 9. graph capture and overflow
# ---------------------------------------------------------------------------------------------------------------
def captured_stream(dev, max_frames, lm_case=None):
    """A stream over the ragged batch with one captured advance of 4 frames (static chunk buffer, device lengths) and one
    captured results; freshly reset."""
    from pika_amd import ctc
    if lm_case is None:
        stream = ctc.CtcBeamStream(3, max_frames, beam=D.RAGGED_BEAM, device=dev)
    else:
        stream = lm_stream(lm_case, dev, batch=3, max_frames=max_frames)
    buf = torch.zeros(4, 3, D.RAGGED_C, device=dev)
    buf[:] = torch.from_numpy(D.RAGGED_LP[:4]).to(dev)
    lens = torch.full((3,), 4, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up off the default stream, then one linear capture
        stream.advance(buf, lens)
        stream.results(nbest=D.RAGGED_BEAM)
    torch.cuda.current_stream().wait_stream(side)
    stream.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream.advance(buf, lens)
        outs = stream.results(nbest=D.RAGGED_BEAM)
    stream.reset()
    return stream, graph, buf, lens, outs


@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
def test_graph_capture_equals_eager(hip_device, with_lm):
    from pika_amd import ctc
    dev, ils, T = hip_device, D.RAGGED_ILS, D.RAGGED_T
    case = L.RAGGED_CASES[0] if with_lm else None
    x = torch.from_numpy(D.RAGGED_LP).to(dev)
    stream, graph, buf, lens, outs = captured_stream(dev, 16, case)
    eager = lm_stream(case, dev, batch=3, max_frames=16) if with_lm else ctc.CtcBeamStream(3, 16, beam=4, device=dev)
    for s in range(0, T, 4):
        k = min(4, T - s)
        chunk_lens = [int(min(max(il - s, 0), k)) for il in ils]
        buf.zero_()
        buf[:k] = x[s:s + k]
        lens.copy_(torch.tensor(chunk_lens, dtype=torch.int32))
        graph.replay()
        eager.advance(x[s:s + k], torch.tensor(chunk_lens, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    if with_lm:
        want = lm_one_shot(case, x, ils, D.RAGGED_BEAM, True, dev)
    else:
        want = ctc.ctc_beam_search(x, torch.tensor(ils), beam=D.RAGGED_BEAM, nbest=D.RAGGED_BEAM)
    assert_same(outs, want, T)
    assert_same(eager.results(nbest=D.RAGGED_BEAM), want, T)
    assert stream.frames.tolist() == ils and stream.overflowed.tolist() == [False] * 3


def test_overflow(hip_device):
    from pika_amd import ctc
    dev = hip_device
    x = torch.from_numpy(D.RAGGED_LP).to(dev)
    # host: the third chunk of 4 frames does not fit into max_frames = 8, and nothing is launched
    stream = ctc.CtcBeamStream(3, 8, beam=D.RAGGED_BEAM, device=dev)
    stream.advance(x[0:4])
    stream.advance(x[4:8])
    before = stream._state.clone()
    with pytest.raises(ValueError, match="max_frames"):
        stream.advance(x[8:12])
    assert torch.equal(stream._state, before) and stream.frames.tolist() == [8, 8, 8]
    assert stream.overflowed.tolist() == [False] * 3
    stream.reset(which=[True, False, False])           # a partial reset does not lower the host's bound
    with pytest.raises(ValueError, match="max_frames"):
        stream.advance(x[8:12])
    # device: three replays of a captured advance of 4 frames; the third is cut
    stream, graph, buf, lens, outs = captured_stream(dev, 8)
    for i, chunk_lens in enumerate(([4, 4, 4], [4, 4, 2], [4, 0, 1])):
        buf[:] = x[4 * i:4 * i + 4]
        lens.copy_(torch.tensor(chunk_lens, dtype=torch.int32))
        graph.replay()
    torch.cuda.synchronize()
    assert stream.frames.tolist() == [8, 8, 7]
    assert stream.overflowed.tolist() == [True, False, False]   # only stream 0 was offered frames it could not take
    # stream 2 took frames 0..5 and then frame 8
    lp2 = np.concatenate([D.RAGGED_LP[:6, 2], D.RAGGED_LP[8:9, 2]])
    y = x[:8].clone()
    y[:7, 2] = torch.from_numpy(lp2).to(dev)
    want = ctc.ctc_beam_search(y, torch.tensor([8, 8, 7]), beam=D.RAGGED_BEAM, nbest=D.RAGGED_BEAM)
    assert_same(outs, want, 8)
    stream.reset()
    assert stream.overflowed.tolist() == [False] * 3 and stream.frames.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------
# 9b. the bytes reset writes, for the three record types
# ---------------------------------------------------------------------------------------------------------------
def test_reset_writes_the_documented_bytes_and_nothing_else(hip_device):
    """One reset kernel serves the plain, the LM and the two-FST record.  A blob filled with 0xA5, reset(which=[1, 0, 1]):
    stream 1 keeps every byte; streams 0 and 2 have an empty table (all 0xFF), the header (1, 0, 0, 0, 0.0, 0.0) and
    the empty prefix in slot 0, in the start state of each automaton.  Offsets from the record layouts of
    include/pika_ctc_decode.h and include/pika_ctc_lm.h: the header in 32 bytes, then arrays of 64 -- i32 node, last,
    parent node, len, f32 p_b, p_nb, tot (1824 bytes); f64 bonus, i32 LM state (2592); i32 second state (2848).  The
    root's values are root_slot()'s of csrc/ctc_search_core.h and csrc/ctc_lm.hip."""
    from pika_amd import ctc
    from pika_amd.decoder.ngram_fst import NgramFst
    dev = hip_device
    B, max_frames, beam, K, slots = 3, 4, 2, 2, 64          # C = 3; 64 = max(64, 2 * max_frames * beam) table slots
    arcs = [(0, 2, 1.0, 0), (1, 2, 1.0, 0), (1, 9, 0.5, 0)]
    lm = ctc.CtcNgramLm(NgramFst.from_arcs(2, arcs, {0: 0.0}, start=1), 9, device=dev)
    bias = ctc.CtcNgramLm(NgramFst.from_arcs(2, arcs, {0: 0.5}, start=1), 9, device=dev)
    assert (lm.num_states, lm.start, bias.num_states, bias.start) == (2, 1, 2, 1)
    i32, f32, f64 = np.dtype("<i4"), np.dtype("<f4"), np.dtype("<f8")
    header = [(0, i32, 1), (4, i32, 0), (8, i32, 0), (12, i32, 0), (16, f64, 0.0), (24, f64, 0.0)]
    root = [(32, i32, 0x7ffffffe), (288, i32, -1), (544, i32, 0x7ffffffd), (800, i32, 0), (1056, f32, 0.0),
            (1312, f32, np.float32(-1.0e30)), (1568, f32, 0.0)]
    lm_root = root + [(1824, f64, 0.0), (2336, i32, lm.start)]
    for name, given, rec, fields in (("plain", None, 1824, header + root), ("LM", lm, 2592, header + lm_root),
                                     ("LM + bias", ctc.CtcBiasedLm(lm, bias), 2848,
                                      header + lm_root + [(2592, i32, bias.start)])):
        stream = ctc.CtcBeamStream(B, max_frames, beam=beam, lm=given, candidates=K, device=dev)
        assert stream._state.numel() == B * (8 * slots + rec), name
        stream._state.fill_(0xA5)
        stream.reset(which=[1, 0, 1])
        blob = stream._state.cpu().numpy()
        tables = blob[:B * 8 * slots].reshape(B, 8 * slots)
        recs = blob[B * 8 * slots:].reshape(B, rec)
        assert (tables[1] == 0xA5).all() and (recs[1] == 0xA5).all(), (name, "a stream that was not selected changed")
        written = np.zeros(rec, dtype=bool)
        for b in (0, 2):
            assert (tables[b] == 0xFF).all(), (name, b)
            for off, dtype, want in fields:
                got = recs[b, off:off + dtype.itemsize].copy().view(dtype)[0]
                assert got == want and type(got) is dtype.type, (name, b, off, got, want)
                written[off:off + dtype.itemsize] = True
            assert (recs[b][~written] == 0xA5).all(), (name, b, "reset wrote beyond the header and slot 0")
        assert stream.frames.tolist()[::2] == [0, 0] and stream.overflowed.tolist()[::2] == [False, False]
        stream.reset()
        blob = stream._state.cpu().numpy()
        tables = blob[:B * 8 * slots].reshape(B, 8 * slots)
        recs = blob[B * 8 * slots:].reshape(B, rec)
        assert (tables[1] == tables[0]).all() and (recs[1][written] == recs[0][written]).all(), name
        assert (recs[1][~written] == 0xA5).all(), name


# ---------------------------------------------------------------------------------------------------------------
# 10. two runs are bit-identical
# ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(hip_device):
    from pika_amd import ctc
    case, lcase = D.SEARCH_CASES[4], L.LM_CASES[3]
    for c, stream in ((case, ctc.CtcBeamStream(1, case.T, beam=case.beam, device=hip_device)),
                      (lcase, lm_stream(lcase, hip_device))):
        x = torch.from_numpy(c.lp[:, None].copy()).to(hip_device)
        runs = []
        for _ in range(2):
            stream.reset()
            feed(stream, x, [min(3, c.T - s) for s in range(0, c.T, 3)])
            runs.append(stream.results(nbest=c.beam))
        assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---------------------------------------------------------------------------------------------------------------
# 11. guards
# ---------------------------------------------------------------------------------------------------------------
def test_adjacent_buffers_keep_their_guards(hip_device):
    from pika_amd import _lib, ctc
    lib, dev = _lib.lib(), hip_device
    T, Tc, B, C, beam, nbest, K, GUARD = 10, 5, 2, 37, 8, 5, 12, 256
    ref_lm = L.make_lm(C, 0, 71, order=3)
    lm = device_lm(ref_lm, dev)
    x = torch.from_numpy(D.case_lp(T, C, 70, B=B)).to(dev)
    lens = [torch.tensor(v, dtype=torch.int32, device=dev) for v in ([5, 5], [5, 3])]
    which = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    sizes = dict(blank_lp=4 * Tc * B, top_val=4 * Tc * B * 2 * beam, top_idx=4 * Tc * B * 2 * beam,
                 state=lib.pika_ctc_stream_state_bytes(B, T, beam), tokens=4 * B * nbest * T, lengths=4 * B * nbest,
                 scores=4 * B * nbest,
                 lm_val=4 * Tc * B * K, lm_idx=4 * Tc * B * K, lm_state=lib.pika_ctc_lm_stream_state_bytes(B, T, beam, K),
                 lm_tokens=4 * B * nbest * T, lm_lengths=4 * B * nbest, lm_scores=4 * B * nbest, lm_am=4 * B * nbest)
    assert sizes["state"] > 0 and sizes["lm_state"] > 0
    offs, total = {}, GUARD
    for name, nbytes in sizes.items():
        offs[name] = total
        total += (nbytes + 15) // 16 * 16 + GUARD
    arena = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    p = {name: arena.data_ptr() + o for name, o in offs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    fst = L.fst_args(lm, start=False)
    assert lib.pika_ctc_stream_reset(p["state"], B, T, beam, which.data_ptr(), stream) == 0
    assert lib.pika_ctc_lm_stream_reset(p["lm_state"], B, T, beam, K, lm.num_states, lm.start, None, stream) == 0
    for i in range(2):
        xc = x[i * Tc:(i + 1) * Tc]
        st, sb = xc.stride(0), xc.stride(1)
        assert lib.pika_ctc_decode_rows(xc.data_ptr(), st, sb, lens[i].data_ptr(), B, Tc, C, 0, 2 * beam, 0,
                                        p["blank_lp"], p["top_val"], p["top_idx"], None, stream) == 0
        assert lib.pika_ctc_stream_advance(xc.data_ptr(), st, sb, None, p["blank_lp"], p["top_val"], p["top_idx"],
                                           lens[i].data_ptr(), B, Tc, C, 0, beam, p["state"], T, stream) == 0
        assert lib.pika_ctc_decode_rows(xc.data_ptr(), st, sb, lens[i].data_ptr(), B, Tc, C, 0, K, 0, p["blank_lp"],
                                        p["lm_val"], p["lm_idx"], None, stream) == 0
        assert lib.pika_ctc_lm_stream_advance(xc.data_ptr(), st, sb, None, p["blank_lp"], p["lm_val"], p["lm_idx"],
                                              lens[i].data_ptr(), B, Tc, C, 0, beam, *fst, K, 0.5, 0.25,
                                              p["lm_state"], T, stream) == 0
    assert lib.pika_ctc_stream_results(p["state"], B, T, beam, nbest, T, p["tokens"], p["lengths"], p["scores"],
                                       stream) == 0
    assert lib.pika_ctc_lm_stream_results(p["lm_state"], B, T, beam, K, *fst, 0.5, 1, nbest, T, p["lm_tokens"],
                                          p["lm_lengths"], p["lm_scores"], p["lm_am"], stream) == 0
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    keep = np.ones(total, dtype=bool)
    for name, nbytes in sizes.items():
        keep[offs[name]:offs[name] + nbytes] = False
    assert (host[keep] == 0xA5).all(), "a kernel wrote outside its buffer"

    def view(name, dtype, shape):
        return np.frombuffer(host[offs[name]:offs[name] + sizes[name]].tobytes(), dtype=dtype).reshape(shape)
    il = torch.tensor([10, 8])
    s = ctc.ctc_beam_search(x, il, beam=beam, nbest=nbest)
    assert (view("tokens", np.int32, (B, nbest, T)) == s[0].cpu().numpy()).all()
    assert (view("lengths", np.int32, (B, nbest)) == s[1].cpu().numpy()).all()
    assert (view("scores", np.float32, (B, nbest)) == s[2].cpu().numpy()).all()
    s = ctc.ctc_beam_search_lm(x, il, lm, beam=beam, nbest=nbest, lm_weight=0.5, length_bonus=0.25, candidates=K)
    assert (view("lm_tokens", np.int32, (B, nbest, T)) == s[0].cpu().numpy()).all()
    assert (view("lm_scores", np.float32, (B, nbest)) == s[2].cpu().numpy()).all()
    assert (view("lm_am", np.float32, (B, nbest)) == s[3].cpu().numpy()).all()
    # the documented header of a record: frames at +4, overflow at +8
    rec = np.frombuffer(host[offs["state"] + lib.pika_ctc_beam_scratch_bytes(B, T, beam):
                             offs["state"] + sizes["state"]].tobytes(), dtype=np.int32).reshape(B, 1824 // 4)
    assert rec[:, 1].tolist() == [10, 8] and rec[:, 2].tolist() == [0, 0]
