"""CPU-side checks of the streaming CTC beam search: the Python surface, the size functions of the state blob, the
argument checks of the C entry points (refused before any launch, so no GPU is needed), and the meaning of "partial
results after k frames", pinned to the float64 reference alone."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_decode_common as D  # noqa: E402


def test_class_is_exported_with_the_documented_signatures():
    import pika_amd
    from pika_amd import ctc
    assert pika_amd.CtcBeamStream is ctc.CtcBeamStream and "CtcBeamStream" in dir(pika_amd)

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][1:]
    E = inspect.Parameter.empty
    S = ctc.CtcBeamStream
    assert sig(S.__init__) == [("batch", E), ("max_frames", E), ("beam", 16), ("blank", 0), ("lm", None),
                               ("lm_weight", 0.5), ("length_bonus", 0.0), ("candidates", None), ("device", None)]
    assert sig(S.reset) == [("which", None)]
    assert sig(S.advance) == [("log_probs", E), ("lengths", None)]
    assert sig(S.advance_from_logits) == [("logits", E), ("lengths", None)]
    assert sig(S.results) == [("nbest", 1), ("use_final", True)]
    assert isinstance(S.frames, property) and isinstance(S.overflowed, property)


def test_abi_version_is_unchanged():
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25 and _lib.lib().pika_amd_abi_version() == 25


def test_state_bytes():
    from pika_amd import _lib
    lib = _lib.lib()
    plain = lib.pika_ctc_stream_state_bytes

    def fused(B, F, beam):
        return lib.pika_ctc_lm_stream_state_bytes(B, F, beam, 32)
    for fn in (plain, fused):
        for bad in ((0, 10, 4), (2, 0, 4), (2, 10, 0), (-1, 10, 4), (2, 10, 65), (65536, 10, 4), (1, 2 ** 21 + 1, 64)):
            assert fn(*bad) == 0, bad
        assert fn(1, 2 ** 21, 64) > 0                       # 2 max_frames beam == 2^28: the limit itself
        for B, beam in ((1, 4), (3, 16), (32, 64)):
            c = {(fn(B, F, beam) - lib.pika_ctc_beam_scratch_bytes(B, F, beam)) for F in (1, 24, 600)}
            assert len(c) == 1 and c.pop() % B == 0
    # the table part is the one-shot's scratch; the records are the constants of the headers
    assert plain(3, 24, 4) == lib.pika_ctc_beam_scratch_bytes(3, 24, 4) + 3 * 1824
    assert fused(3, 24, 4) == lib.pika_ctc_lm_scratch_bytes(3, 24, 4, 32) + 3 * 2592
    assert lib.pika_ctc_lm_stream_state_bytes(2, 10, 4, 0) == 0 and lib.pika_ctc_lm_stream_state_bytes(2, 10, 4, 129) == 0
    for h, name, value in (("pika_ctc_decode.h", "PIKA_CTC_STREAM_RECORD_BYTES", 1824),
                           ("pika_ctc_lm.h", "PIKA_CTC_LM_STREAM_RECORD_BYTES", 2592),
                           ("pika_ctc_decode.h", "PIKA_CTC_STREAM_FRAMES_OFFSET", 4),
                           ("pika_ctc_decode.h", "PIKA_CTC_STREAM_OVERFLOW_OFFSET", 8)):
        text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", h)).read()
        assert "#define %s %d\n" % (name, value) in text


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    N = None
    # reset(state, B, max_frames, beam, which, stream)
    assert lib.pika_ctc_stream_reset(N, 1, 8, 4, N, N) == -1
    assert lib.pika_ctc_stream_reset(N, 0, 8, 4, N, N) == -1
    assert lib.pika_ctc_stream_reset(N, 1, 8, 65, N, N) == -2
    assert lib.pika_ctc_stream_reset(N, 65536, 8, 4, N, N) == -2
    # advance(x, st, sb, lse, blank_lp, top_val, top_idx, chunk_lengths, B, Tc, C, blank, beam, state, max_frames, stream)
    assert lib.pika_ctc_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 0, 4, N, 8, N) == -1
    assert lib.pika_ctc_stream_advance(N, 0, 0, N, N, N, N, N, 1, 0, 5, 0, 4, N, 8, N) == -1
    assert lib.pika_ctc_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 5, 4, N, 8, N) == -1
    assert lib.pika_ctc_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 0, 4, N, 0, N) == -1
    assert lib.pika_ctc_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 0, 65, N, 8, N) == -2
    assert lib.pika_ctc_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 0, 64, N, 2 ** 21 + 1, N) == -2
    # results(state, B, max_frames, beam, nbest, L, tokens, lengths, scores, stream)
    assert lib.pika_ctc_stream_results(N, 1, 8, 4, 1, 8, N, N, N, N) == -1
    assert lib.pika_ctc_stream_results(N, 1, 8, 4, 0, 8, N, N, N, N) == -1
    assert lib.pika_ctc_stream_results(N, 1, 8, 4, 1, 0, N, N, N, N) == -1
    assert lib.pika_ctc_stream_results(N, 1, 8, 4, 5, 8, N, N, N, N) == -2
    # the LM forms
    assert lib.pika_ctc_lm_stream_reset(N, 1, 8, 4, 8, 3, 0, N, N) == -1
    assert lib.pika_ctc_lm_stream_reset(N, 1, 8, 4, 8, 3, 3, N, N) == -1            # start outside [0, S)
    assert lib.pika_ctc_lm_stream_reset(N, 1, 8, 4, 129, 3, 0, N, N) == -2
    fst = (N, N, N, N, N, 3, 0)
    assert lib.pika_ctc_lm_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 0, 4, *fst, 9, 1, 8, 0.5, 0.0, N, 8, N) == -1
    assert lib.pika_ctc_lm_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 0, 4, N, N, N, N, N, 0, 0, 9, 1, 8, 0.5, 0.0,
                                          N, 8, N) == -1
    assert lib.pika_ctc_lm_stream_advance(N, 0, 0, N, N, N, N, N, 1, 4, 5, 0, 4, *fst, 9, 1, 129, 0.5, 0.0, N, 8,
                                          N) == -2
    assert lib.pika_ctc_lm_stream_results(N, 1, 8, 4, 8, *fst, 9, 1, 0.5, 1, 1, 8, N, N, N, N, N) == -1
    assert lib.pika_ctc_lm_stream_results(N, 1, 8, 4, 8, *fst, 9, 1, 0.5, 1, 5, 8, N, N, N, N, N) == -2
    assert lib.pika_ctc_lm_stream_results(N, 1, 8, 65, 8, *fst, 9, 1, 0.5, 1, 1, 8, N, N, N, N, N) == -2


def test_constructor_checks():
    from pika_amd import ctc
    for kw in (dict(beam=0), dict(beam=65), dict(batch=0), dict(max_frames=0)):
        args = dict(batch=2, max_frames=8)
        args.update(kw)
        with pytest.raises(ValueError):
            ctc.CtcBeamStream(**args)
    with pytest.raises(TypeError):
        ctc.CtcBeamStream(2, 8, lm="not an LM")
    # candidates and nbest are checked before anything touches the device
    lm = object.__new__(ctc.CtcNgramLm)
    for candidates in (0, 129):
        with pytest.raises(ValueError, match="candidates"):
            ctc.CtcBeamStream(2, 8, lm=lm, candidates=candidates)
    stream = object.__new__(ctc.CtcBeamStream)
    stream.beam = 4
    for nbest in (0, 5):
        with pytest.raises(ValueError, match="nbest"):
            stream.results(nbest=nbest)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            ctc.CtcBeamStream(2, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ctc.CtcBeamStream(2, 8, device="cpu") if torch.cuda.is_available() else ctc.CtcBeamStream(2, 8)


def test_partial_results_mean_the_reference_on_the_prefix():
    case = D.SearchCase(24, 4, 4, 2)
    for k in (1, 7, 8, 9, 24):
        hyps, margin, _ = D.beam_search(case.lp[:k], case.beam, case.beam, case.blank)
        assert 1 <= len(hyps) <= case.beam and margin >= 0.0
        labels = [l for l, _ in hyps]
        assert len(set(labels)) == len(labels) and all(len(l) <= k for l in labels)
        assert all(a >= b for (_, a), (_, b) in zip(hyps, hyps[1:])) and all(s <= 0.0 for _, s in hyps)
        assert all(s > -float("inf") for _, s in hyps)
    # the whole utterance is its own prefix
    assert D.beam_search(case.lp[:24], 4, 4)[0] == case.ref()[0]
