"""The reference of the fused one-symbol-per-frame search (tests/msearch_lm_common.py) against brute force, on cases so
small that nothing is pruned: V = 4, T <= 4, K = C = 64.  Brute force: every alignment (one symbol per frame) of the
table model is enumerated, the alignments that spell one token sequence are summed in float64, and the LM term comes
from `RefLm.score`, which knows nothing of the search."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_bias_common as CB  # noqa: E402
import ctc_lm_common as CL  # noqa: E402
import msearch_common as M  # noqa: E402
import msearch_lm_common as ML  # noqa: E402

V, K, C = 4, 64, 64


def brute_force(model, T, sm_scale, penalty):
    """{tokens: float64 log of the summed probability of its alignments}"""
    total = {}
    for align in itertools.product(range(V), repeat=T):
        tok, lp = (), 0.0
        for t, v in enumerate(align):
            lp += M.log_probs(np.asarray(model(tok, t))[None], 0, sm_scale, penalty)[0][v]
            if v != 0:
                tok = tok + (v,)
        total[tok] = np.logaddexp(total[tok], lp) if tok in total else lp
    return total


# (T, the automaton, the classes it cannot reach): 4 frames fit into 64 candidates only with a class out of reach
CASES = [(3, "hot", ()), (3, "lm", ()), (4, "lm", (3,)), (4, "lm3", (2,))]


@pytest.mark.parametrize("T,kind,unreachable", CASES)
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_brute_force(T, kind, unreachable, seed):
    if kind == "hot":
        lm = CB.hot_lm([(1, 2), (3,)], V, 1.5)
    else:
        lm = CL.make_lm(V, 0, 10 + seed, order=3 if kind == "lm3" else 2, unreachable=unreachable)
    lmw, lb, sm, pen = ML.f32(0.7), ML.f32(0.25), 0.9, 0.1
    model = M.TableModel(T, V, 50 + seed)
    beam, infos = ML.search(model, T, V, K, C, [lm], [lmw], lb, 0, sm, pen)
    for info in infos:                                  # nothing was pruned: every finite candidate was selected
        assert len(info["selected"]) == int((info["cand"] > ML.NINF).sum()) and len(info["groups"]) <= K
    want = brute_force(model, T, sm, pen)
    live = [e for e in beam if e[0] > ML.NINF]
    got = {e[3]: e for e in live}
    assert len(got) == len(live)
    reachable = {tok for tok in want if lm.score(tok) is not None}
    assert set(got) == reachable                        # a class the LM cannot reach never appears; the rest all do
    assert not any(c in tok for tok in got for c in unreachable) and (not unreachable or len(reachable) < len(want))
    for tok, (F, am, bonus, _, states) in got.items():
        assert abs(float(am) - want[tok]) <= 1e-12
        score, state = lm.score(tok)
        assert states == (state,)
        # the reference rounds every increment to fp32 once, as the device's walk does: <= 2^-24 * 10 per label
        assert abs(float(F) - (want[tok] + lmw * score + lb * len(tok))) <= 1e-5
    assert [float(e[0]) for e in live] == sorted((float(e[0]) for e in live), reverse=True)


def test_two_automata_and_final_costs():
    """The pair: both bonuses add up, a class either automaton misses is gone, and `results` adds both final terms,
    drops the entries without a final state and sorts again."""
    T, seed = 4, 3
    lm = CL.make_lm(V, 0, 21, order=3, unreachable=(3,))
    phrases = [(1, 2, 1), (2, 2)]
    hot = CB.hot_lm(phrases, V, 2.0)
    lmw, bw, lb = ML.f32(0.5), ML.f32(1.25), ML.f32(-0.1)
    model = M.TableModel(T, V, 60 + seed)
    beam, infos = ML.search(model, T, V, K, C, [lm, hot], [lmw, bw], lb)
    want = brute_force(model, T, 1.0, 0.0)
    live = {e[3]: e for e in beam if e[0] > ML.NINF}
    assert set(live) == {tok for tok in want if lm.score(tok) is not None and hot.score(tok) is not None}
    assert not any(3 in tok for tok in live)
    for tok, (F, am, bonus, _, states) in live.items():
        fused = want[tok] + lmw * lm.score(tok)[0] + bw * CB.hot_bias(phrases, tok, 2.0) + lb * len(tok)
        assert abs(float(am) - want[tok]) <= 1e-12 and abs(float(F) - fused) <= 1e-5
        assert ML.bonus_of([lm, hot], [lmw, bw], lb, tok)[0] == bonus
    final = ML.results(beam, [lm, hot], [lmw, bw], True)
    plain = ML.results(beam, [lm, hot], [lmw, bw], False)
    assert [f[0] for f in plain] == [e[3] for e in beam if e[0] > ML.NINF]
    assert [float(f[1]) for f in final] == sorted((float(f[1]) for f in final), reverse=True)
    have_final = {tok for tok in live if lm.final(lm.score(tok)[1]) is not None}
    assert {f[0] for f in final} == have_final and 0 < len(have_final)
    for tok, score, am in final:
        s = lm.score(tok)
        fused = want[tok] + lmw * (s[0] + float(lm.final(s[1]))) + bw * CB.hot_bias(phrases, tok, 2.0, final=True) \
            + lb * len(tok)
        assert abs(float(score) - fused) <= 1e-5 and abs(float(am) - want[tok]) <= 1e-12


def test_zero_weights_are_the_plain_reference():
    """With zero weights, C = K and an automaton that reaches every class, the fused reference is `msearch_common.step`
    value for value, in float64 and in float32."""
    T, Vv, Kk = 8, 9, 4
    hot = CB.hot_lm([(1, 2), (3,)], Vv, 1.0)
    model = M.TableModel(T, Vv, 5)
    for dtype in (np.float64, np.float32):
        beam, _ = ML.search(model, T, Vv, Kk, Kk, [hot], [0.0], 0.0, 0, 0.9, 0.1, dtype)
        ref, _ = M.search(model, T, Vv, Kk, 0, 0.9, 0.1, dtype)
        assert [(e[0], e[3]) for e in beam] == [(s, tok) for s, tok in ref]
        assert all(e[0] == e[1] for e in beam)
