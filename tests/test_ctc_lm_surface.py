"""CPU-side checks of the CTC search with LM fusion: the reference of tests/ctc_lm_common.py against brute force, its
LM primitives by hand, the Python signatures and exports, the C ABI's size formula and argument refusals (no launch, no
GPU), `CtcNgramLm`'s validation, and the properties the GPU test's case list must have -- from the reference alone."""
import ctypes
import inspect
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_decode_common as D  # noqa: E402
import ctc_lm_common as L  # noqa: E402
from pika_amd.decoder.ngram_fst import NgramFst  # noqa: E402

# (T, C, blank, LM order, lm_weight, length_bonus, use_final): a beam of 64 holds every prefix that can exist
EXHAUSTIVE = [(3, 3, 0, 2, 0.5, 0.0, True), (3, 3, 2, 3, 1.0, 0.5, False), (2, 4, 1, 2, 0.3, -0.5, True),
              (4, 2, 0, 2, 2.0, 1.0, True), (1, 4, 3, 2, 0.7, 0.0, True), (4, 3, 1, 3, 0.0, 0.25, True),
              (3, 4, 0, 3, 1.5, -0.25, True)]


@pytest.mark.parametrize("T,C,blank,order,lmw,lb,use_final", EXHAUSTIVE)
def test_reference_equals_brute_force_when_the_beam_holds_everything(T, C, blank, order, lmw, lb, use_final):
    lp = D.case_lp(T, C, 10 * T + C)
    lm = L.make_lm(C, blank, 100 + T + C, order)
    every = {tuple(R.collapse(fl, blank)) for fl in itertools.product(range(C), repeat=T)}
    assert len(every) <= 64
    hyps, _, reent = L.search(lp, lm, 64, C - 1, blank, lmw, lb, use_final)
    want = {}
    for l in every:
        sc = lm.score(l)
        if sc is None:
            continue
        bonus = lmw * sc[0] + lb * len(l)
        if use_final:
            fin = lm.final(sc[1])
            if fin is None:
                continue
            bonus += lmw * float(fin)
        want[l] = (-R.dp_cost(lp.astype(np.float64), list(l), blank) + bonus, bonus)
    assert {l for l, _, _ in hyps} == set(want) and reent == 0
    for l, fused, am in hyps:
        assert fused == pytest.approx(want[l][0], abs=1e-12)
        assert am == pytest.approx(want[l][0] - want[l][1], abs=1e-12)
    assert [f for _, f, _ in hyps] == sorted((f for _, f, _ in hyps), reverse=True)


def hand_lm():
    """Labels: class c is c + 1, back-off 9.  State 0: unigrams of classes 1, 2 (not 3), final 0.5.  State 1 (start):
    class 1 -> 2, back-off 0.25 -> 0.  State 2: back-off 1.0 -> 0.  State 3: class 2 -> 3, back-off 0.75 -> 1.
    State 4: nothing at all."""
    arcs = [(0, 2, 1.5, 2), (0, 3, 2.5, 3), (1, 2, 0.5, 2), (1, 9, 0.25, 0), (2, 9, 1.0, 0), (3, 3, 0.125, 3),
            (3, 9, 0.75, 1)]
    return L.RefLm(NgramFst.from_arcs(5, arcs, {0: 0.5}, start=1), 9, 1)


def test_lm_primitives_by_hand():
    lm = hand_lm()
    assert lm.step(1, 1) == (-0.5, 2)                       # a direct arc
    assert lm.step(1, 2) == (-(0.25 + 2.5), 3)              # one back-off hop
    assert lm.step(3, 1) == (-(0.75 + 0.5), 2)              # the first match along the chain wins: state 1's arc
    assert lm.step(3, 2) == (-0.125, 3)
    assert lm.step(3, 3) is None and lm.step(1, 3) is None  # two hops down to the unigram state: class 3 is nowhere
    assert lm.step(4, 1) is None                            # neither arc
    assert lm.final(0) == -0.5
    assert lm.final(3) == -(0.75 + 0.25 + 0.5)              # a final reached through two back-off hops
    assert lm.final(4) is None
    assert lm.score((1, 2, 2)) == (-(0.5 + 1.0 + 2.5 + 0.125), 3)
    assert lm.score((1, 3)) is None
    # a class the LM cannot reach is excluded whatever the weight, 0 included
    lp = np.log(np.array([[0.1, 0.1, 0.1, 0.7], [0.1, 0.1, 0.1, 0.7]]))
    for lmw in (0.0, 1.0):
        hyps, _, _ = L.search(lp, lm, 8, 3, 0, lmw, 0.0, False)
        assert hyps and all(3 not in l for l, _, _ in hyps)
    # the hop bound: a chain of 9 back-off arcs is not walked to its end, one of 8 is
    for hops, found in ((8, True), (9, False)):
        arcs = [(s, 9, 0.5, s + 1) for s in range(hops)] + [(hops, 2, 1.0, 0)]
        chain = L.RefLm(NgramFst.from_arcs(hops + 1, arcs, {hops: 0.25}), 9, 1)
        assert (chain.step(0, 1) is not None) == found and (chain.final(0) is not None) == found
    assert chain.step(1, 1) == (-(8 * 0.5 + 1.0), 0)


def test_signatures_and_exports():
    import pika_amd
    from pika_amd import _lib, ctc

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    tail = [("beam", 16), ("nbest", 1), ("blank", 0), ("lm_weight", 0.5), ("length_bonus", 0.0), ("candidates", None),
            ("use_final", True)]
    assert sig(ctc.ctc_beam_search_lm) == [("log_probs", E), ("input_lengths", E), ("lm", E)] + tail
    assert sig(ctc.ctc_beam_search_lm_from_logits) == [("logits", E), ("input_lengths", E), ("lm", E)] + tail
    assert sig(ctc.CtcNgramLm.__init__)[1:] == [("fst", E), ("backoff_id", E), ("label_offset", 1), ("device", None)]
    for name in ("CtcNgramLm", "ctc_beam_search_lm", "ctc_beam_search_lm_from_logits"):
        assert getattr(pika_amd, name) is getattr(ctc, name) and name in dir(pika_amd)
    # the plain search is as it was
    assert sig(ctc.ctc_beam_search) == [("log_probs", E), ("input_lengths", E), ("beam", 16), ("nbest", 1), ("blank", 0)]
    assert _lib.ABI_VERSION == 25               # new symbols only: no signature changed
    for name in ("pika_ctc_lm_scratch_bytes", "pika_ctc_lm_beam_search"):
        assert name in _lib.SIGNATURES
    doc = ctc.ctc_beam_search_lm.__doc__
    assert "candidates >= C - 1" in doc and "PRUNING" in doc


def test_cpu_tensors_and_bad_limits_are_refused():
    import torch
    from pika_amd import ctc
    lp, il = torch.zeros(3, 1, 4), torch.tensor([3])
    lm = object.__new__(ctc.CtcNgramLm)        # never reached beyond the type check: the limits come first
    for fn in (ctc.ctc_beam_search_lm, ctc.ctc_beam_search_lm_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp, il, lm)
        with pytest.raises(TypeError):
            fn(lp, il, None)
        for kw in (dict(beam=65), dict(beam=4, nbest=5), dict(beam=0), dict(beam=4, nbest=0), dict(candidates=0),
                   dict(candidates=129), dict(beam=64, candidates=-1)):
            with pytest.raises(ValueError):
                fn(lp, il, lm, **kw)


def test_scratch_size_follows_the_header():
    from pika_amd import _lib
    lib = _lib.lib()

    def want(B, T, beam):
        n = 64
        while n < 2 * T * beam:
            n *= 2
        return 8 * B * n
    for dims in [(32, 240, 16, 32), (1, 1, 1, 1), (3, 9, 64, 128), (2, 1000, 16, 32), (1, 600, 4, 5), (5, 1, 33, 7),
                 (1, 2 ** 21, 64, 128)]:
        assert lib.pika_ctc_lm_scratch_bytes(*dims) == want(*dims[:3]), dims
        assert lib.pika_ctc_lm_scratch_bytes(*dims) == lib.pika_ctc_beam_scratch_bytes(*dims[:3])
    for dims in [(0, 5, 4, 8), (1, 0, 4, 8), (1, 5, 0, 8), (1, 5, 4, 0), (-1, 5, 4, 8), (1, 5, 4, -2), (1, 5, 65, 8),
                 (1, 5, 4, 129), (65536, 5, 4, 8), (1, 2 ** 21 + 1, 64, 8)]:
        assert lib.pika_ctc_lm_scratch_bytes(*dims) == 0, dims


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2
    p = ctypes.c_void_p(0x1000)     # never dereferenced: EVERY call below is refused before any launch
    good = dict(B=2, T=5, C=4, blank=0, beam=4, nbest=2, S=3, A=6, start=1, cand=8)

    # q: x, lse, blank_lp, top_val, top_idx, input_lengths, offsets, ilabel, weight, nextstate, final, tokens, lengths,
    #    scores, am_scores, scratch
    def call(q, B, T, C, blank, beam, nbest, S, A, start, cand):
        return lib.pika_ctc_lm_beam_search(q[0], C * B, C, q[1], q[2], q[3], q[4], q[5], B, T, C, blank, beam, nbest,
                                           q[6], q[7], q[8], q[9], q[10], S, A, start, 9, 1, cand, 0.5, 0.0, 1, q[11],
                                           q[12], q[13], q[14], q[15], None)
    full = [p] * 16
    for kw in (dict(B=0), dict(T=0), dict(C=0), dict(B=-1), dict(T=-3), dict(C=-2), dict(blank=-1), dict(blank=4),
               dict(beam=0), dict(nbest=0), dict(cand=0), dict(cand=-1), dict(S=0), dict(S=-1), dict(A=-1),
               dict(start=-1), dict(start=3)):
        assert call(full, **dict(good, **kw)) == EINVAL, kw
    for kw in (dict(beam=65, nbest=1), dict(beam=4, nbest=5), dict(beam=64, nbest=65), dict(cand=129), dict(B=65536),
               dict(T=2 ** 21 + 1, beam=64)):
        assert call(full, **dict(good, **kw)) == ETOOBIG, kw
    for i in range(16):
        if i == 1:                              # lse alone may be NULL (log-probs): that call would launch
            continue
        q = [None if j == i else p for j in range(16)]
        assert call(q, **good) == EINVAL, i
    # an LM without arcs needs no arc arrays (still refused here: another required pointer is missing)
    q = [p] * 16
    q[7] = q[8] = q[9] = q[11] = None
    assert call(q, **dict(good, A=0)) == EINVAL
    q[7] = p
    q[11] = p
    assert call(q, **good) == EINVAL            # A > 0: weight and nextstate are required


def chain_fst(hops):
    arcs = [(s, 9, 0.5, s + 1) for s in range(hops)] + [(hops, 2, 1.0, 0), (hops, 3, 1.0, 0)]
    return NgramFst.from_arcs(hops + 1, arcs, {hops: 0.25})


def test_ngram_lm_validation():
    from pika_amd import ctc

    def refused(fst, backoff_id=9, label_offset=1, match=None):
        with pytest.raises(ValueError, match=match):
            ctc.CtcNgramLm(fst, backoff_id, label_offset)
    # a back-off cycle
    refused(NgramFst.from_arcs(3, [(0, 2, 1.0, 1), (0, 9, 0.5, 1), (1, 9, 0.5, 2), (2, 9, 0.5, 0)], {0: 0.0}), match="hops")
    refused(NgramFst.from_arcs(1, [(0, 9, 0.5, 0)], {0: 0.0}), match="hops")
    # a chain of 9 hops; 8 pass the check (and then need a device)
    refused(chain_fst(9), match="hops")
    try:
        ctc.CtcNgramLm(chain_fst(8), 9)
    except RuntimeError as e:
        assert "HIP device" in str(e)
    # nextstate / start out of range
    good = hand_lm().fst
    bad = NgramFst(good.offsets, good.ilabel, good.weight, np.where(np.arange(len(good.ilabel)) == 2, 5, good.nextstate),
                   good.final, good.start)
    refused(bad, match="nextstate")
    refused(NgramFst(good.offsets, good.ilabel, good.weight, good.nextstate, good.final, start=5), match="start")
    refused(NgramFst(good.offsets, good.ilabel, good.weight, -np.ones(len(good.ilabel), np.int32), good.final, 1),
            match="nextstate")
    # backoff_id is a class label: 3 = class 2 (labels 2..3 and the back-off 9 are in the table)
    refused(good, backoff_id=3, match="collides")
    refused(good, backoff_id=2, match="collides")
    # two back-off arcs out of one state
    refused(NgramFst.from_arcs(2, [(0, 2, 1.0, 1), (1, 9, 0.5, 0), (1, 9, 0.7, 0)], {0: 0.0}), match="more than one")
    # offsets that do not describe the arcs
    refused(NgramFst(np.array([0, 2, 4, 5, 7, 6]), good.ilabel, good.weight, good.nextstate, good.final, 1),
            match="offsets")


def test_gpu_case_list_has_the_required_properties():
    # properties of tests/test_ctc_lm_gpu.py's cases (kept in ctc_lm_common), from the float64 reference and the
    # float32 yardstick
    refs = [(c,) + c.ref() for c in L.ALL_CASES]
    lm_matters = pruned = 0
    for c, h64, bound, separated, reent, margin, err32 in refs:
        plain, _, _ = D.beam_search(c.lp, c.beam, 1, c.blank)
        differs = bool(h64) and h64[0][0] != plain[0][0]
        lm_matters += differs
        narrow = ""
        if c.candidates < c.C - 1:
            full, _, _ = c.run(candidates=c.C - 1)
            moved = [(l, round(f, 9)) for l, f, _ in full] != [(l, round(f, 9)) for l, f, _ in h64]
            pruned += moved
            narrow = "  candidates < C - 1: the result %s" % ("differs from the unpruned one" if moved else "is the same")
        print("CTCLM %-28s bound %.3g margin %.3g float32 err %.3g re-entries %d top-1 %s the plain search's%s %s" % (
            c.name, bound, margin, err32, reent, "differs from" if differs else "equals", narrow,
            "" if separated else "NOT separated"))
        assert bound >= 4 * err32 and bound >= 1e-6 * max(max(abs(f), abs(a)) for _, f, a in h64)
        assert h64 == sorted(h64, key=lambda h: -h[1])
    unseparated = [r[0].name for r in refs if not r[3]]
    assert len(refs) >= 20 and len(unseparated) <= 0.1 * len(refs), unseparated
    assert lm_matters >= 15
    assert sum(1 for r in refs if r[4] > 0) >= 3                     # orphan re-entries
    assert pruned >= 2
    assert any(any(not c.lm.reaches(k) for k in range(c.C) if k != c.blank) for c in L.ALL_CASES)
    # the shapes, the mixes
    have = {(c.T, c.C, c.beam, c.candidates) for c in L.LM_CASES}
    for want in ((12, 3, 2, 2), (30, 4, 3, 3), (24, 4, 4, 3), (60, 8, 8, 7), (20, 6, 1, 5), (16, 8, 16, 7),
                 (10, 40, 16, 32), (10, 40, 16, 8), (6, 260, 16, 32), (8, 70, 64, 128), (8, 70, 64, 20),
                 (5, 1028, 16, 32), (4, 5003, 4, 8), (40, 12, 8, 4), (40, 12, 8, 11), (600, 6, 4, 5), (3, 3, 16, 2),
                 (2, 4, 16, 3), (1, 2, 4, 1), (4, 2, 16, 1)):
        assert want in have, want
    assert sum(1 for c in L.LM_CASES if (c.T, c.C) == (600, 6)) == 2
    assert any(c.blank == 100 for c in L.LM_CASES) and len(L.RAGGED_CASES) == 3
    assert {c.use_final for c in L.ALL_CASES} == {True, False} and {c.order for c in L.ALL_CASES} == {2, 3}
    weights = {c.lm_weight for c in L.ALL_CASES}
    assert 0.0 in weights and max(weights) == 2.0 and L.f32(0.3) in weights
    bonuses = {c.length_bonus for c in L.ALL_CASES}
    assert min(bonuses) == -0.5 and max(bonuses) == 1.0 and 0.0 in bonuses
