"""The reference of the one-symbol-per-frame search with a neural LM (tests/msearch_nn_common.py) against brute force,
on cases so small that nothing is pruned: V = 4, T <= 4, K = C = 64.  Brute force: every alignment (one symbol per frame)
of the table model is enumerated, the alignments that spell one token sequence are summed in float64; the LM terms come
from a log-softmax of the table LM's rows written here and from `RefLm.score`, which know nothing of the search."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_lm_common as CL  # noqa: E402
import msearch_common as M  # noqa: E402
import msearch_lm_common as ML  # noqa: E402
import msearch_nn_common as MN  # noqa: E402
from test_msearch_lm_refs import brute_force, V, K, C  # noqa: E402


def table_score(table, scale, offset, tok):
    """sum_i log_softmax(scale * table[row of tok[:i]])[tok[i] + offset], float64; None: a class outside the table."""
    total, last = 0.0, -1
    for v in tok:
        y = scale * table[last].astype(np.float64)
        if not 0 <= v + offset < len(y):
            return None
        total += y[v + offset] - np.log(np.exp(y - y.max()).sum()) - y.max()
        last = v
    return total


# (T, V_lm, nn_label_offset, with an n-gram, the class it cannot reach): 4 frames fit into 64 candidates only with a
# class out of reach -- of the n-gram, or of the LM's rows (V_lm = 3: label 3 falls outside; with offset -1 every label is inside again)
CASES = [(3, 4, 0, False, ()), (3, 6, 2, True, ()), (4, 3, 0, False, (3,)), (4, 4, 0, True, (2,)), (3, 3, -1, False, ())]


@pytest.mark.parametrize("T,VL,off,ngram,unreachable", CASES)
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_brute_force(T, VL, off, ngram, unreachable, seed):
    nnw, nns, lmw, lb, sm, pen = ML.f32(0.4), ML.f32(0.8), ML.f32(0.7), ML.f32(0.25), 0.9, 0.1
    table = MN.make_table(V, VL, 70 + seed)
    lm = CL.make_lm(V, 0, 10 + seed, order=3, unreachable=unreachable) if ngram else None
    lms = ([lm] if ngram else []) + [MN.table_lm(table, nns, off)]
    weights = ([lmw] if ngram else []) + [nnw]
    model = M.TableModel(T, V, 50 + seed)
    beam, infos = ML.search(model, T, V, K, C, lms, weights, lb, 0, sm, pen)
    for info in infos:                                  # nothing was pruned: every finite candidate was selected
        assert len(info["selected"]) == int((info["cand"] > ML.NINF).sum()) and len(info["groups"]) <= K
    want = brute_force(model, T, sm, pen)
    live = [e for e in beam if e[0] > ML.NINF]
    got = {e[3]: e for e in live}
    assert len(got) == len(live)
    exists = {tok for tok in want if table_score(table, nns, off, tok) is not None
              and (lm is None or lm.score(tok) is not None)}
    assert set(got) == exists                           # a class outside [0, V_lm) never appears; the rest all do
    outside = [v for v in range(1, V) if not 0 <= v + off < VL]
    assert not any(v in tok for tok in got for v in outside + list(unreachable))
    assert len(exists) < len(want) or not (outside or unreachable)
    for tok, (F, am, bonus, _, states) in got.items():
        assert abs(float(am) - want[tok]) <= 1e-12
        fused = want[tok] + nnw * table_score(table, nns, off, tok) + lb * len(tok)
        if ngram:
            fused += lmw * lm.score(tok)[0]
        # the reference rounds every increment to fp32 once, as the device does: <= 2^-24 * 10 per label and term
        assert abs(float(F) - fused) <= 1e-5
        assert abs(MN.table_lm(table, nns, off).score(tok) - table_score(table, nns, off, tok)) <= 1e-12
    assert [float(e[0]) for e in live] == sorted((float(e[0]) for e in live), reverse=True)


def test_rows_that_cannot_be_scored():
    """-inf and NaN columns take no part in the row's statistics and their labels do not exist; a row without a finite
    maximum kills every label; the float32 yardstick follows the float64 reference."""
    inf, nan = np.inf, np.nan
    for dtype in (np.float64, np.float32):
        lp, ok = MN.log_softmax_row(np.float32([0.0, 0.5, -inf, nan]), 1.0, dtype)
        assert ok and lp.dtype == dtype and abs(lp[1] - (0.5 - np.log(1 + np.exp(0.5)))) <= 1e-6
        lm = MN.DenseLm(lambda p: np.float32([0.0, 0.5, -inf, nan]), 1.0, 0, dtype)
        assert lm.step((), 0) is not None and lm.step((), 2) is None and lm.step((), 3) is None and lm.step((), 4) is None
        assert lm.step((1,), 1)[1] == (1, 1) and lm.final((1,)) == 0.0
        for row in ([-inf, -inf], [inf, 0.0], [nan, nan]):
            dead = MN.DenseLm(lambda p, row=row: np.float32(row), 1.0, 0, dtype)
            assert dead.step((), 0) is None and dead.step((), 1) is None
    rows = MN.lm_rows(MN.make_table(4, 3, 0), [(), (2,), (1, 3)], [True, False, True])
    assert np.isnan(rows[1]).all() and (rows[0] == MN.make_table(4, 3, 0)[-1]).all() and (rows[2] == MN.make_table(4, 3, 0)[3]).all()


def test_zero_nn_weight_is_the_fused_reference():
    """With nn_weight = 0 and every class in range the dense term changes nothing: `ML.search` value for value."""
    T, Vv, Kk, Cc = 8, 9, 4, 8
    lm = CL.make_lm(Vv, 0, 4, order=3)
    model = M.TableModel(T, Vv, 5)
    dense = MN.table_lm(MN.make_table(Vv, Vv, 1), 0.8, 0)
    for dtype in (np.float64, np.float32):
        a, _ = ML.search(model, T, Vv, Kk, Cc, [lm], [0.5], 0.25, 0, 0.9, 0.1, dtype)
        b, _ = ML.search(model, T, Vv, Kk, Cc, [lm, dense], [0.5, 0.0], 0.25, 0, 0.9, 0.1, dtype)
        assert [e[:4] for e in a] == [e[:4] for e in b]
