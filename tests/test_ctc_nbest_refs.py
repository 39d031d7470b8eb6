"""The float64 reference of the n-best alignment (tests/ctc_nbest_common.py) against brute force, and the margin census
of the inputs on which tests/test_ctc_nbest_gpu.py compares paths exactly (CPU only; no product imports)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_nbest_common as NB  # noqa: E402

# (T, C = 3, hypotheses, blank): empty, single, repeats, the skip rule, blank not at 0, an infeasible one among feasible
BRUTE = [(1, [[], [1], [2]], 0), (4, [[1, 2], [2], [1, 1]], 0), (5, [[2, 1, 2], [1, 1], [1, 1, 1]], 0),
         (6, [[1, 2, 1], [2, 2, 1], []], 0), (5, [[0, 1], [1, 1, 0]], 2), (3, [[1, 1], [1, 2, 1], [2, 2, 2]], 0)]


@pytest.mark.parametrize("T,hyps,blank", BRUTE)
def test_reference_equals_brute_force(T, hyps, blank):
    lp = NB.randn_lp(T, 3, 10 * T + len(hyps))       # continuous values: the optimum is unique
    for seq, ref in zip(hyps, NB.nbest_align(lp, hyps, blank)):
        cost, best, arg = R.brute_force(lp, seq, blank)
        if np.isinf(cost):
            assert not ref.feasible and ref.full == -np.inf and ref.best == -np.inf
            continue
        assert ref.feasible
        assert ref.full == pytest.approx(-cost, abs=1e-12)
        assert ref.best == pytest.approx(best, abs=1e-12)
        assert ref.labels.tolist() == arg.tolist()
        # the runs are the path: they give its labelling back, and their scores sum with the blanks' to the best score
        fl = NB.labelling(T, ref.starts, ref.ends, seq, blank)
        assert fl.tolist() == arg.tolist()
        blanks = R.rescore(lp[fl == blank], [blank] * int((fl == blank).sum()))
        assert ref.token_scores.sum() + blanks == pytest.approx(best, abs=1e-12)


def test_missing_entries_stay_missing():
    lp = NB.randn_lp(4, 3, 0)
    refs = NB.nbest_align(lp, [[1], None, [3], [0]])
    assert refs[1] is None and refs[0].feasible and not refs[2].feasible and not refs[3].feasible


@pytest.mark.parametrize("T,C,beam", NB.RANDN_SHAPES)
def test_margin_census_of_the_exact_path_inputs(T, C, beam):
    flags = []
    for seed in NB.SEEDS:
        lp, hyps = NB.randn_case(T, C, beam, seed)
        assert len(hyps) == beam
        flags += [r.unique for r in NB.nbest_align(lp, hyps)]
    print("n-best margin census (%d, %d, %d): %d of %d unique by margin" % (T, C, beam, sum(flags), len(flags)))
    assert sum(flags) >= 0.9 * len(flags)
