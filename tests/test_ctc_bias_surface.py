"""CPU-side checks of hotword biasing beside the LM: the graph `CtcHotwords.compile` builds, walked with the reference's
`RefLm` and compared EXACTLY with the string simulator of tests/ctc_bias_common.py (the weights are fp32 multiples of
a dyadic boost); its refusals; the new C symbols, the record size and the unchanged ABI version; the argument refusals
of the new entry points (no launch, no GPU); and the properties the GPU test's case list must have -- from the
reference alone."""
import ctypes
import inspect
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_bias_common as Bc  # noqa: E402
import ctc_lm_common as L  # noqa: E402

NINE = (1,) * 9                 # prefixes 1, 11, ..., 1^8: a fail chain of exactly 8 hops from the deepest state
# over C = 4 (classes 1..3): overlapping phrases, a one-token phrase, a phrase inside another
LISTS_C4 = [[(1, 2, 3), (2, 3, 1)], [(3,), (1, 2, 3), (2, 3, 1)], [(2, 3), (1, 2, 3, 2)], [(1, 1, 2), (1, 2, 1), (2, 2)],
            [NINE, (1, 2)], [(1, 2, 1, 2, 3), (2, 1, 3), (3, 3)]]


def compile_ref(phrases, C, boost=1.0, blank=0):
    from pika_amd.ctc import CtcHotwords
    fst = CtcHotwords.compile(phrases, C, boost, blank)
    return fst, L.RefLm(fst, C + 1, 1)


def check_sequence(ref, phrases, boost, labels):
    got = ref.score(labels)
    assert got is not None, (phrases, labels, "the graph reaches every non-blank class")
    done, m, _ = Bc.hot_walk(phrases, labels)
    assert got[0] == boost * (done + len(m)), (phrases, labels, got[0], done, m)
    fin = ref.final(got[1])
    assert fin is not None and got[0] + float(fin) == boost * done, (phrases, labels, fin)
    return got[1]


@pytest.mark.parametrize("phrases", LISTS_C4, ids=lambda p: "-".join("".join(map(str, q)) for q in p))
@pytest.mark.parametrize("boost", [1.0, 1.5])
def test_compiled_graph_equals_the_string_rules_on_every_short_sequence(phrases, boost):
    fst, ref = compile_ref(phrases, 4, boost)
    # the contract of the graph: the states, the root's arcs, no back-off arc at the root
    prefixes = {p[:k] for p in phrases for k in range(1, len(p))}
    assert fst.num_states == 1 + len(prefixes) and fst.start == 0
    root = {int(fst.ilabel[a]): a for a in range(int(fst.offsets[0]), int(fst.offsets[1]))}
    assert sorted(root) == [2, 3, 4] and fst.final[0] == 0.0
    assert fst.weight.dtype == np.float32 and set(np.unique(fst.weight / np.float32(boost))) <= set(range(-1, 10))
    ends = set()
    for n in range(7):
        for labels in itertools.product((1, 2, 3), repeat=n):
            ends.add(check_sequence(ref, phrases, boost, labels))
    if NINE not in phrases:
        assert ends == set(range(fst.num_states))           # every state was visited
    # the final cost of a state is its credit: boost * depth
    assert sorted(float(v) for v in fst.final) == sorted(boost * len(p) for p in prefixes | {()})


def test_compiled_graph_equals_the_string_rules_on_seeded_sequences():
    C = 12
    for seed in range(6):
        phrases = Bc.seeded_phrases(C, 5, seed, 8, lo=1 if seed % 2 else 2, hi=6)
        if seed == 0:
            phrases = [p for p in phrases if p[0] != 7] + [(7,) * 9, (7, 7, 3)]     # with a chain of 8 hops
        fst, ref = compile_ref(phrases, C, 0.75, blank=5)
        assert 5 + 1 not in set(int(v) for v in fst.ilabel)     # blank has no arc
        rng = np.random.RandomState(seed)
        pool = sorted({c for p in phrases for c in p}) + [0, 11]
        for _ in range(300):
            n = int(rng.randint(0, 25))
            # mostly tokens the phrases use, so that matches start, overlap, fail and complete
            labels = tuple(int(rng.choice(pool)) for _ in range(n))
            check_sequence(ref, phrases, 0.75, labels)
        labels = (7,) * 20
        check_sequence(ref, phrases, 0.75, labels) if seed == 0 else None


def test_duplicates_merge_and_blank_moves():
    a, _ = compile_ref([(1, 2), (1, 2), (3,)], 5)
    b, _ = compile_ref([(3,), (1, 2)], 5)
    for x, y in zip((a.offsets, a.ilabel, a.weight, a.nextstate, a.final), (b.offsets, b.ilabel, b.weight, b.nextstate, b.final)):
        assert np.array_equal(x, y)
    fst, ref = compile_ref([(0, 1)], 3, 2.0, blank=2)
    assert ref.score((0, 1)) == (4.0, 0) and ref.score((0, 0)) == (2.0, 1) and ref.score((2,)) is None
    assert ref.step(1, 0) == (0.0, 1)          # refund 2, then the root's arc earns 2 again


def test_refusals():
    from pika_amd import ctc

    def refused(phrases, C=4, match=None, **kw):
        with pytest.raises(ValueError, match=match):
            ctc.CtcHotwords.compile(phrases, C, **kw)
        with pytest.raises(ValueError, match=match):
            ctc.CtcHotwords(phrases, C, **kw)      # the constructor compiles first: no device is needed to refuse
    refused([(1, 2), ()], match="empty")
    refused([(1, 0)], match="blank")
    refused([(1, 2)], blank=2, match="blank")
    refused([(1, 4)], match="outside")
    refused([(-1,)], match="outside")
    refused([(1, 2, 3), (1, 2)], match="proper prefix")
    refused([(1,), (1, 2, 3)], match="proper prefix")
    for boost in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        refused([(1, 2)], boost=boost, match="boost")
    # a fail chain of 9 hops is refused by CtcNgramLm's own check; 8 hops pass it (and then need a device)
    fst = ctc.CtcHotwords.compile([(1,) * 10], 4)
    assert fst.num_states == 10
    with pytest.raises(ValueError, match="hops"):
        ctc.CtcHotwords([(1,) * 10], 4)
    try:
        ctc.CtcHotwords([NINE], 4)
    except RuntimeError as e:
        assert "HIP device" in str(e)
    # the pair: types first
    lm = object.__new__(ctc.CtcNgramLm)
    for args in ((lm, None), (None, lm), (lm, "x"), (3, lm)):
        with pytest.raises(TypeError):
            ctc.CtcBiasedLm(*args)


def test_exports_symbols_and_record_size():
    import pika_amd
    from pika_amd import _lib, ctc
    for name in ("CtcHotwords", "CtcBiasedLm"):
        assert getattr(pika_amd, name) is getattr(ctc, name) and name in dir(pika_amd)
    assert issubclass(ctc.CtcHotwords, ctc.CtcNgramLm)
    E = inspect.Parameter.empty
    sig = [(p.name, p.default) for p in inspect.signature(ctc.CtcHotwords.__init__).parameters.values()][1:]
    assert sig == [("phrases", E), ("num_classes", E), ("boost", 1.0), ("blank", 0), ("device", None)]
    sig = [(p.name, p.default) for p in inspect.signature(ctc.CtcBiasedLm.__init__).parameters.values()][1:]
    assert sig == [("lm", E), ("bias", E), ("bias_weight", 1.0)]
    assert "lm=hotwords, lm_weight=1.0" in ctc.CtcHotwords.__doc__ and "8 hops" in ctc.CtcHotwords.__doc__
    assert _lib.ABI_VERSION == 25               # new symbols only
    lib = _lib.lib()
    assert lib.pika_amd_abi_version() == 25
    # the counterparts' arguments plus the second FST's (header): 5 arrays, S, A, (start,) backoff, label_offset, weight
    counts = dict(scratch_bytes=0, beam_search=11, stream_state_bytes=0, stream_reset=2, stream_advance=10,
                  stream_results=10)
    for name, more in counts.items():
        one, two = _lib.SIGNATURES["pika_ctc_lm_" + name], _lib.SIGNATURES["pika_ctc_lm2_" + name]
        assert len(two[1]) == len(one[1]) + more and two[0] == one[0], name
        assert getattr(lib, "pika_ctc_lm2_" + name) is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "pika_ctc_lm.h")).read()
    assert "#define PIKA_CTC_LM_STREAM_RECORD_BYTES 2592" in header
    assert "#define PIKA_CTC_LM2_STREAM_RECORD_BYTES (PIKA_CTC_LM_STREAM_RECORD_BYTES + 256)" in header
    rec2 = 2592 + 64 * 4
    assert rec2 % 8 == 0
    for dims in [(1, 1, 1, 1), (3, 9, 64, 128), (32, 240, 16, 32), (5, 1000, 33, 7)]:
        tables = lib.pika_ctc_lm2_scratch_bytes(*dims)
        assert tables == lib.pika_ctc_lm_scratch_bytes(*dims) > 0
        assert lib.pika_ctc_lm2_stream_state_bytes(*dims) == tables + dims[0] * rec2
        assert lib.pika_ctc_lm_stream_state_bytes(*dims) == tables + dims[0] * 2592        # as it was
    for dims in [(0, 5, 4, 8), (1, 0, 4, 8), (1, 5, 65, 8), (1, 5, 4, 129), (65536, 5, 4, 8)]:
        assert lib.pika_ctc_lm2_scratch_bytes(*dims) == 0 and lib.pika_ctc_lm2_stream_state_bytes(*dims) == 0


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2
    p = ctypes.c_void_p(0x1000)     # never dereferenced: EVERY call below is refused before any launch
    good = dict(B=2, T=5, C=4, blank=0, beam=4, nbest=2, S=3, A=6, start=1, S2=2, A2=4, start2=0, cand=8)

    # q: x, lse, blank_lp, top_val, top_idx, lengths | 5 arrays of the LM | 5 of the second FST | tokens, lengths, scores,
    #    am_scores, scratch
    def one_shot(q, B, T, C, blank, beam, nbest, S, A, start, S2, A2, start2, cand):
        return lib.pika_ctc_lm2_beam_search(q[0], C * B, C, q[1], q[2], q[3], q[4], q[5], B, T, C, blank, beam, nbest,
                                            q[6], q[7], q[8], q[9], q[10], S, A, start, 9, 1,
                                            q[11], q[12], q[13], q[14], q[15], S2, A2, start2, 9, 1,
                                            cand, 0.5, 1.0, 0.0, 1, q[16], q[17], q[18], q[19], q[20], None)
    full = [p] * 21
    for kw in (dict(B=0), dict(T=0), dict(C=0), dict(blank=4), dict(beam=0), dict(nbest=0), dict(cand=0), dict(S=0),
               dict(A=-1), dict(start=3), dict(S2=0), dict(S2=-1), dict(A2=-1), dict(start2=-1), dict(start2=2)):
        assert one_shot(full, **dict(good, **kw)) == EINVAL, kw
    for kw in (dict(beam=65, nbest=1), dict(beam=4, nbest=5), dict(cand=129), dict(B=65536)):
        assert one_shot(full, **dict(good, **kw)) == ETOOBIG, kw
    for i in range(21):
        if i == 1:                              # lse alone may be NULL: that call would launch
            continue
        q = [None if j == i else p for j in range(21)]
        assert one_shot(q, **good) == EINVAL, i
    # the streaming forms
    assert lib.pika_ctc_lm2_stream_reset(p, 2, 8, 4, 8, 3, 1, 0, 0, None, None) == EINVAL      # num_states2
    assert lib.pika_ctc_lm2_stream_reset(p, 2, 8, 4, 8, 3, 1, 2, 2, None, None) == EINVAL      # start2
    assert lib.pika_ctc_lm2_stream_reset(p, 2, 8, 4, 8, 3, 3, 2, 0, None, None) == EINVAL      # start
    assert lib.pika_ctc_lm2_stream_reset(None, 2, 8, 4, 8, 3, 1, 2, 0, None, None) == EINVAL
    assert lib.pika_ctc_lm2_stream_reset(p, 2, 8, 65, 8, 3, 1, 2, 0, None, None) == ETOOBIG

    def advance(q, S2=2, A2=4, Tc=4, beam=4):
        return lib.pika_ctc_lm2_stream_advance(q[0], 8, 4, None, q[1], q[2], q[3], q[4], 2, Tc, 4, 0, beam,
                                               q[5], q[6], q[7], q[8], q[9], 3, 6, 9, 1,
                                               q[10], q[11], q[12], q[13], q[14], S2, A2, 9, 1, 8, 0.5, 1.0, 0.0,
                                               q[15], 8, None)

    def results(q, S2=2, A2=4, nbest=2, L=8):
        return lib.pika_ctc_lm2_stream_results(q[0], 2, 8, 4, 8, q[1], q[2], q[3], q[4], q[5], 3, 6, 9, 1,
                                               q[6], q[7], q[8], q[9], q[10], S2, A2, 9, 1, 0.5, 1.0, 1, nbest, L,
                                               q[11], q[12], q[13], q[14], None)
    for fn, n in ((advance, 16), (results, 15)):
        assert fn([p] * n, S2=0) == EINVAL and fn([p] * n, A2=-1) == EINVAL
        for i in range(n):
            assert fn([None if j == i else p for j in range(n)]) == EINVAL, (fn.__name__, i)
    assert advance([p] * 16, Tc=0) == EINVAL and advance([p] * 16, beam=65) == ETOOBIG
    assert results([p] * 15, nbest=0) == EINVAL and results([p] * 15, nbest=5) == ETOOBIG


def test_reference_equals_brute_force_when_the_beam_holds_everything():
    # search2 against the sum over all paths, the bonus from the two automata and the string rules
    import ctc_common as R
    import ctc_decode_common as D
    for T, C, blank, lmw, bw, lb, use_final, phrases in ((3, 3, 0, 0.5, 1.0, 0.0, True, [(1, 2), (2, 2, 1)]),
                                                        (4, 3, 1, 1.0, 1.5, 0.5, False, [(0, 2), (2,)]),
                                                        (2, 4, 0, 0.3, 2.0, -0.5, True, [(3, 1), (1, 1)])):
        lp = D.case_lp(T, C, 10 * T + C)
        lm = L.make_lm(C, blank, 100 + T + C, 3)
        bias = Bc.hot_lm(phrases, C, 1.5, blank)
        every = {tuple(R.collapse(fl, blank)) for fl in itertools.product(range(C), repeat=T)}
        hyps, _, _ = Bc.search2(lp, lm, bias, 64, C - 1, blank, lmw, bw, lb, use_final)
        want = {}
        for l in every:
            sc = lm.score(l)
            fin = lm.final(sc[1]) if sc is not None else None
            if sc is None or (use_final and fin is None):
                continue
            bonus = lmw * sc[0] + bw * Bc.hot_bias(phrases, l, 1.5, use_final) + lb * len(l)
            bonus += lmw * float(fin) if use_final else 0.0
            want[l] = (-R.dp_cost(lp.astype(np.float64), list(l), blank) + bonus, bonus)
        assert {l for l, _, _ in hyps} == set(want)
        for l, fused, am in hyps:
            assert fused == pytest.approx(want[l][0], abs=1e-12) and am == pytest.approx(want[l][0] - want[l][1], abs=1e-12)


def test_gpu_case_list_has_the_required_properties():
    refs = [(c,) + c.ref() for c in Bc.ALL_CASES]
    matters = refunded = 0
    for c, h64, bound, separated, reent, margin, err32 in refs:
        alone = c.without_bias()
        differs = bool(h64) and bool(alone) and h64[0][0] != alone[0][0]
        matters += differs
        refunds = Bc.hot_walk(c.phrases, h64[0][0])[2] if (c.phrases and h64) else 0
        refunded += refunds > 0
        print("CTCBIAS %-32s bound %.3g margin %.3g float32 err %.3g top-1 %s the LM-only search's, %d refunds on the "
              "winning path %s" % (c.name, bound, margin, err32, "differs from" if differs else "equals", refunds,
                                   "" if separated else "NOT separated"))
        assert bound >= 4 * err32 and bound >= 1e-6 * max(max(abs(f), abs(a)) for _, f, a in h64)
        assert h64 == sorted(h64, key=lambda h: -h[1])
        for l, f, a in h64:                     # the reference's bonus is what the two FSTs and the string rules give
            assert f - a == pytest.approx(c.terms(l), abs=1e-9)
    assert 3 * sum(1 for r in refs if r[3]) >= 2 * len(refs), [r[0].name for r in refs if not r[3]]
    assert matters >= 3 and refunded >= 1
    have = {(c.T, c.C, c.beam, c.candidates) for c in Bc.BIAS_CASES}
    for want in ((12, 3, 2, 2), (30, 4, 3, 3), (60, 8, 8, 7), (20, 6, 1, 5), (10, 40, 16, 32), (6, 260, 16, 32),
                 (8, 70, 64, 128), (8, 70, 64, 20), (4, 5003, 4, 8), (600, 6, 4, 5), (1, 2, 4, 1)):
        assert want in have, want
    assert any(c.blank == 100 for c in Bc.BIAS_CASES) and len(Bc.RAGGED_CASES) == 3
    assert {c.use_final for c in Bc.ALL_CASES} == {True, False}
    assert any(c.bias_weight == 0.0 for c in Bc.ALL_CASES) and any(c.length_bonus < 0 for c in Bc.ALL_CASES)
    second = [c for c in Bc.ALL_CASES if c.phrases is None]
    assert second and any(not c.bias.reaches(k) for c in second for k in range(c.C) if k != c.blank)
    assert all(c.bias is Bc.RAGGED_BIAS and c.lm is Bc.RAGGED_LM for c in Bc.RAGGED_CASES)
