"""The host path of the CTC searches before it touches a device (pika_amd/ctc.py: `_Search`, `_hip_device`).

`_Search` is the one description of the variant -- plain, one FST, two FSTs -- that `ctc_beam_search_lm` and
`CtcBeamStream` build from their `lm` argument and make every C call through.  This file pins what it hands to the C
ABI, group by group, and the exact text and order of the errors on the way.  The expected tuples are written down from
the call sites of the commit before the variants had one home (fe38a5a), in the order of include/pika_ctc_decode.h and
include/pika_ctc_lm.h; the expected messages are what that commit's module raised, recorded from a run of it.  Nothing
here needs a device: the LMs are stand-ins with a distinct small integer in every field.
"""
import pytest
import torch

from pika_amd import ctc

D0, D1 = torch.device("cuda", 0), torch.device("cuda", 1)


class Ptr(object):
    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def standin(base, device=D0, backoff_id=None, label_offset=None):
    """A `CtcNgramLm` that was never uploaded: arrays at base + 1 .. base + 5, num_states base + 6, num_arcs base + 7,
    start base + 8, backoff_id base + 9, label_offset base + 10 (class -1: no clash with any C)."""
    lm = object.__new__(ctc.CtcNgramLm)
    lm.offsets, lm.ilabel, lm.weight, lm.nextstate, lm.final = (Ptr(base + i) for i in range(1, 6))
    lm.num_states, lm.num_arcs, lm.start = base + 6, base + 7, base + 8
    lm.backoff_id = base + 9 if backoff_id is None else backoff_id
    lm.label_offset = base + 10 if label_offset is None else label_offset
    lm.device = device
    return lm


LM, BIAS = standin(10), standin(30)
LM_FST, LM_FST_START = (11, 12, 13, 14, 15, 16, 17, 19, 20), (11, 12, 13, 14, 15, 16, 17, 18, 19, 20)
BIAS_FST, BIAS_FST_START = (31, 32, 33, 34, 35, 36, 37, 39, 40), (31, 32, 33, 34, 35, 36, 37, 38, 39, 40)


def search(lm, lm_weight, length_bonus, beam, candidates, need_lm=False):
    return ctc._Search(lm, lm_weight, length_bonus, need_lm).sized(beam, candidates)


def groups(v):
    return dict(prefix=v.prefix, tables=v.prefix + v.scratch_bytes, candidates=v.candidates, dims=v.dims,
                fsts=v.fsts(False), fsts_start=v.fsts(True),
                starts=v.starts(), weights=v.weights, results_weights=v.results_weights, fused=v.fused)


def test_argument_groups_of_the_three_variants():
    # plain: only a stream has it; the row pass's K is 2 * beam whatever `candidates` says
    v = search(None, 0.5, 0.25, 3, 7)
    assert groups(v) == dict(prefix="pika_ctc_", tables="pika_ctc_beam_scratch_bytes", candidates=6, dims=(), fsts=(),
                             fsts_start=(), starts=(), weights=(),
                             results_weights=(), fused=False)
    assert (v.lm, v.bias, v.bias_weight, v.lm_weight, v.length_bonus) == (None, None, 1.0, 0.5, 0.25)
    # one FST
    for need_lm in (False, True):
        v = search(LM, 0.5, 0.25, 3, 5, need_lm)
        assert groups(v) == dict(prefix="pika_ctc_lm_", tables="pika_ctc_lm_scratch_bytes", candidates=5, dims=(5,),
                                 fsts=LM_FST, fsts_start=LM_FST_START,
                                 starts=(16, 18), weights=(5, 0.5, 0.25), results_weights=(0.5,), fused=True)
        assert (v.lm, v.bias, v.bias_weight) == (LM, None, 1.0)
    # two FSTs
    for need_lm in (False, True):
        v = search(ctc.CtcBiasedLm(LM, BIAS, 0.75), 0.5, 0.25, 3, 5, need_lm)
        assert groups(v) == dict(prefix="pika_ctc_lm2_", tables="pika_ctc_lm2_scratch_bytes", candidates=5, dims=(5,),
                                 fsts=LM_FST + BIAS_FST,
                                 fsts_start=LM_FST_START + BIAS_FST_START, starts=(16, 18, 36, 38),
                                 weights=(5, 0.5, 0.75, 0.25), results_weights=(0.5, 0.75), fused=True)
        assert (v.lm, v.bias, v.bias_weight) == (LM, BIAS, 0.75)
    # every weight reaches ctypes as a Python float
    v = search(ctc.CtcBiasedLm(LM, BIAS, 2), 1, 0, 3, 5)
    assert all(type(w) is float for w in v.weights[1:] + v.results_weights) and v.weights == (5, 1.0, 2.0, 0.0)


def test_candidates_default_is_twice_the_beam_capped_at_128():
    for beam, want in ((1, 2), (16, 32), (63, 126), (64, 128)):
        assert search(LM, 0.5, 0.0, beam, None).candidates == want
        assert search(ctc.CtcBiasedLm(LM, BIAS), 0.5, 0.0, beam, None, True).dims == (want,)
        assert search(None, 0.5, 0.0, beam, None).candidates == 2 * beam
    assert search(LM, 0.5, 0.0, 64, "7").candidates == 7      # int() of what was given
    assert search(None, 0.5, 0.0, 64, 3).candidates == 128    # the plain search keeps 2 * beam: exact


def raised(kind, fn):
    with pytest.raises(kind) as e:
        fn()
    assert type(e.value) is kind
    return str(e.value)


def test_messages_of_the_checks_before_any_device():
    one_shot, stream = ctc.ctc_beam_search_lm, ctc.CtcBeamStream
    assert raised(TypeError, lambda: one_shot(None, None, "nope")) == "lm must be a CtcNgramLm, got str"
    assert raised(TypeError, lambda: one_shot(None, None, None)) == "lm must be a CtcNgramLm, got NoneType"
    assert raised(TypeError, lambda: ctc.ctc_beam_search_lm_from_logits(None, None, 3)) == \
        "lm must be a CtcNgramLm, got int"
    assert raised(TypeError, lambda: stream(1, 4, lm="nope")) == "lm must be a CtcNgramLm or None, got str"
    for c in (0, 129):
        want = "need 1 <= candidates <= 128, got %d" % c
        assert raised(ValueError, lambda: one_shot(None, None, LM, candidates=c)) == want
        assert raised(ValueError, lambda: one_shot(None, None, ctc.CtcBiasedLm(LM, BIAS), candidates=c)) == want
        assert raised(ValueError, lambda: stream(1, 4, lm=LM, candidates=c)) == want
    for b in (0, 65):
        assert raised(ValueError, lambda: one_shot(None, None, LM, beam=b)) == \
            "need 1 <= nbest <= beam <= 64, got beam=%d nbest=1" % b
        assert raised(ValueError, lambda: stream(1, 4, beam=b, lm=LM)) == "need 1 <= beam <= 64, got beam=%d" % b
        assert raised(ValueError, lambda: stream(1, 4, beam=b)) == "need 1 <= beam <= 64, got beam=%d" % b
    assert raised(ValueError, lambda: one_shot(None, None, LM, beam=3, nbest=4)) == \
        "need 1 <= nbest <= beam <= 64, got beam=3 nbest=4"
    assert raised(ValueError, lambda: ctc.ctc_beam_search(None, None, beam=3, nbest=4)) == \
        "need 1 <= nbest <= beam <= 64, got beam=3 nbest=4"


def test_the_order_in_which_the_checks_fire():
    one_shot, stream = ctc.ctc_beam_search_lm, ctc.CtcBeamStream
    # one-shot: the type of lm, then beam / nbest, then candidates
    assert raised(TypeError, lambda: one_shot(None, None, "nope", beam=0, candidates=0)) == \
        "lm must be a CtcNgramLm, got str"
    assert raised(ValueError, lambda: one_shot(None, None, LM, beam=0, candidates=0)) == \
        "need 1 <= nbest <= beam <= 64, got beam=0 nbest=1"
    # stream: beam, then the type of lm, then candidates, then batch / max_frames / blank
    assert raised(ValueError, lambda: stream(1, 4, beam=0, lm="nope", candidates=0)) == "need 1 <= beam <= 64, got beam=0"
    assert raised(TypeError, lambda: stream(1, 4, lm="nope", candidates=0)) == "lm must be a CtcNgramLm or None, got str"
    assert raised(ValueError, lambda: stream(0, 4, lm=LM, candidates=0)) == "need 1 <= candidates <= 128, got 0"
    assert raised(ValueError, lambda: stream(0, 4, lm=LM)) == "need batch >= 1, max_frames >= 1 and blank >= 0, got 0, 4, 0"


def test_check_against_classes_and_device():
    lm_clash, bias_clash = standin(10, backoff_id=7, label_offset=1), standin(30, backoff_id=5, label_offset=2)
    far = standin(30, device=D1)
    one = search(lm_clash, 0.5, 0.0, 3, None)
    assert raised(ValueError, lambda: one.check_against(7, D0, "log_probs")) == \
        "the LM's backoff_id 7 is the label of class 6"
    one.check_against(6, D0, "log_probs")                   # class 6 is no class of a 6-class input
    two = search(ctc.CtcBiasedLm(LM, bias_clash), 0.5, 0.0, 3, None)
    for where in ("log_probs", "the stream"):
        assert raised(ValueError, lambda: two.check_against(7, D0, where)) == \
            "the backoff_id 5 of bias is the label of class 3"
    two.check_against(3, D0, "logits")
    # devices: against an input, against a stream
    one = search(LM, 0.5, 0.0, 3, None)
    assert raised(ValueError, lambda: one.check_against(7, D1, "log_probs")) == \
        "the LM lives on cuda:0, log_probs on cuda:1"
    assert raised(ValueError, lambda: one.check_against(7, D1, "logits")) == "the LM lives on cuda:0, logits on cuda:1"
    assert raised(ValueError, lambda: one.check_against(0, D1, "the stream")) == \
        "the LM lives on cuda:0, the stream on cuda:1"
    pair = ctc.CtcBiasedLm(LM, standin(30))
    pair.bias.device = D1                                   # (CtcBiasedLm itself refuses such a pair)
    two = search(pair, 0.5, 0.0, 3, None)
    assert raised(ValueError, lambda: two.check_against(7, D0, "log_probs")) == \
        "bias lives on cuda:1, log_probs on cuda:0"
    assert raised(ValueError, lambda: two.check_against(7, D0, "the stream")) == \
        "bias lives on cuda:1, the stream on cuda:0"
    assert raised(ValueError, lambda: ctc.CtcBiasedLm(LM, far)) == "the LM lives on cuda:0, bias on cuda:1"
    # the LM's checks before the second automaton's; of one automaton, the backoff_id before the device
    both = search(ctc.CtcBiasedLm(lm_clash, bias_clash), 0.5, 0.0, 3, None)
    assert raised(ValueError, lambda: both.check_against(7, D1, "log_probs")) == \
        "the LM's backoff_id 7 is the label of class 6"
    assert raised(ValueError, lambda: both.check_against(4, D1, "log_probs")) == \
        "the LM lives on cuda:0, log_probs on cuda:1"
    assert raised(ValueError, lambda: both.check_against(4, D0, "log_probs")) == \
        "the backoff_id 5 of bias is the label of class 3"


def test_hip_device_serves_both_classes(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for who in ("CtcNgramLm", "CtcBeamStream"):
        assert raised(RuntimeError, lambda: ctc._hip_device(None, "cuda", who)) == \
            "pika_amd %s: needs a HIP device (there is no CPU path)" % who
    assert raised(RuntimeError, lambda: ctc.CtcBeamStream(1, 4)) == \
        "pika_amd CtcBeamStream: needs a HIP device (there is no CPU path)"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 2)
    for who in ("CtcNgramLm", "CtcBeamStream"):
        assert raised(RuntimeError, lambda: ctc._hip_device("cpu", "cuda", who)) == \
            "pika_amd %s: device cpu is not a HIP device (there is no CPU path)" % who
    assert raised(RuntimeError, lambda: ctc.CtcBeamStream(1, 4, lm=LM, device="cpu")) == \
        "pika_amd CtcBeamStream: device cpu is not a HIP device (there is no CPU path)"
    # always an indexed device; the default is the LM's for a stream with an LM
    assert ctc._hip_device(None, "cuda", "x") == torch.device("cuda", 2)
    assert ctc._hip_device("cuda:1", "cuda", "x") == D1 and ctc._hip_device(None, D0, "x") == D0
    assert raised(ValueError, lambda: ctc.CtcBeamStream(1, 4, lm=LM, device="cuda:1")) == \
        "the LM lives on cuda:0, the stream on cuda:1"
