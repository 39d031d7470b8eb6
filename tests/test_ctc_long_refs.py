"""CPU checks of the long-form alignment's fp32 reference (tests/ctc_long_common.py) -- against brute-force enumeration
with constructed ties, against ctc_common's float64 Viterbi, and with / without the row-maximum shift on dyadic inputs --
and of `ctc_segment_scores` on CPU tensors against a loop."""
import itertools
import math

import numpy as np
import torch

import ctc_common as R
import ctc_long_common as L


def _check_against_brute(x, seq):
    ref = L.reference(x, seq, 0, shift=False)
    best, path = L.brute_force(x, seq, 0)
    if path is None:
        assert ref.path is None and ref.score64 == -np.inf
        return ref
    assert ref.score64 == best, (seq, ref.score64, best)
    assert ref.path.tolist() == path.tolist(), (seq, ref.path, path)
    shifted = L.reference(x, seq, 0)
    assert shifted.path.tolist() == path.tolist() and abs(shifted.score64 - best) < 1e-9
    # the outputs follow from the path
    for j, c in enumerate(seq):
        ts = np.nonzero(path == 2 * j + 1)[0]
        assert (ref.starts[j], ref.ends[j]) == (ts[0], ts[-1])
        assert ref.token_scores[j] == np.float32(sum(float(x[t, c]) for t in ts))
    return ref


def test_reference_against_brute_force_with_constructed_ties():
    C = 3
    kinds, end_ties, cases = np.zeros(3, dtype=np.int64), 0, 0
    seqs = [[], [1], [2], [1, 2], [1, 1], [2, 1, 2], [1, 1, 2], [1, 2, 2], [2, 2, 2]]
    # all-equal inputs: every comparison in the lattice is a tie, so the path is the tie rule alone
    for T, seq in itertools.product(range(1, 7), seqs):
        ref = _check_against_brute(np.zeros((T, C), dtype=np.float32), seq)
        if ref.path is not None:
            kinds += ref.kinds
            end_ties += ref.end_tie
            cases += 1
    # two-valued and few-valued dyadic inputs: ties between SOME predecessors, a strict winner elsewhere
    rng = np.random.default_rng(11)
    for trial in range(300):
        T, seq = int(rng.integers(1, 7)), seqs[int(rng.integers(len(seqs)))]
        x = L.dyadic(rng, (T, C), kmax=128, step=64 if trial % 2 else 32)
        ref = _check_against_brute(x, seq)
        if ref.path is not None:
            kinds += ref.kinds
            end_ties += ref.end_tie
            cases += 1
    assert cases > 200 and (kinds >= 3).all() and end_ties > 20, (cases, kinds, end_ties)


def test_each_preference_on_a_hand_built_lattice():
    # seq (1, 2), states (b, 1, b, 2, b), T = 3, all values equal: every complete path scores the same.
    # End rule: state 4 over state 3.  Backwards from (t=2, s=4): stay (4) is impossible at t=1 (not reachable in one step),
    # so the rule falls to s-1 = 3, which at t=1 is reachable only by the skip from 1: path (1, 3, 4).
    z = np.zeros((3, 3), dtype=np.float32)
    assert L.reference(z, [1, 2]).path.tolist() == [1, 3, 4]
    # one more frame: (t=3, s=4) prefers the stay; then as above
    assert L.reference(np.zeros((4, 3), dtype=np.float32), [1, 2]).path.tolist() == [1, 3, 4, 4]
    # a repeat forbids the skip: seq (1, 1) needs the blank between, T = 3 has the single path (1, 2, 3)
    assert L.reference(z, [1, 1]).path.tolist() == [1, 2, 3]
    # s-1 over s-2: make the stay strictly worse at (t=2, s=3) and let 2 -> 3 and 1 -> 3 tie
    x = np.zeros((3, 3), dtype=np.float32)
    x[1, 2] = -1.0      # being in state 3 (class 2) at t=1 costs 1: the stay loses to both others
    # the end is then state 3 (0) rather than state 4 (-1, it can only come through state 3 at t=1); at (t=2, s=3) the stay
    # holds -1 while s-1 (the blank, state 2) and s-2 (state 1) both hold 0: s-1 wins, and state 2 at t=1 comes from 1
    r = L.reference(x, [1, 2], shift=False)
    assert r.path.tolist() == [1, 2, 3] and r.kinds[1] == 1 and r.score64 == 0.0
    # U = 0: state 0 alone
    r = L.reference(x, [])
    assert r.path.tolist() == [0, 0, 0] and r.starts.shape == (0,)
    # infeasible: too short, a bad token, the blank as a token
    for seq, T in (([1, 1], 2), ([3], 3), ([-1], 3), ([0], 3)):
        r = L.reference(np.zeros((T, 3), dtype=np.float32), seq)
        assert r.score64 == -np.inf and (r.starts == -1).all() and (r.ends == -1).all() and np.isneginf(r.token_scores).all()


def test_reference_against_float64_viterbi_on_random_inputs():
    rng = np.random.default_rng(5)
    decided = 0
    for trial in range(40):
        T, C = int(rng.integers(20, 120)), int(rng.integers(3, 8))
        U = int(rng.integers(0, T // 2))
        seq = [int(c) for c in rng.integers(1, C, size=U)]
        x = torch.log_softmax(torch.from_numpy(rng.normal(size=(T, C)) * 3), -1).float().numpy()
        ref = L.reference(x, seq, 0)
        score, labels, path, delta = R.viterbi(x, seq, 0)
        if not np.isfinite(score):
            assert ref.path is None
            continue
        b = R.bound(delta, T)
        assert abs(ref.score64 - score) <= b + 1e-12
        assert R.collapse(ref.labels, 0) == seq
        if R.margin(x, seq, 0) > 2 * b:     # the optimum is decided beyond fp32's reach: the paths must be the same
            decided += 1
            assert ref.path.tolist() == path.tolist() and ref.labels.tolist() == labels.tolist()
        assert abs(R.rescore(x, ref.labels) - ref.score64) <= b + 1e-12
    assert decided >= 20


def test_row_maximum_shift_changes_nothing_on_dyadic_inputs():
    rng = np.random.default_rng(7)
    ties = 0
    for trial in range(25):
        T, C = int(rng.integers(30, 200)), int(rng.integers(3, 6))
        U = int(rng.integers(0, T // 2))
        seq = [int(c) for c in rng.integers(1, C, size=U)]
        x = L.dyadic(rng, (T, C))           # -k/64, k in [0, 640]: every sum below is exact in fp32
        a, b = L.reference(x, seq, 0, shift=True), L.reference(x, seq, 0, shift=False)
        if a.path is None:
            assert b.path is None
            continue
        assert a.path.tolist() == b.path.tolist() and a.score64 == b.score64
        assert (a.starts == b.starts).all() and (a.ends == b.ends).all()
        assert a.token_scores.tobytes() == b.token_scores.tobytes()
        assert a.score64 == R.rescore(x, a.labels)
        ties += a.ties
    assert ties > 0


def test_segment_scores_on_cpu_against_a_loop():
    from pika_amd import ctc
    rng = np.random.default_rng(3)
    B, U = 3, 9
    starts = np.full((B, U), -1, dtype=np.int32)
    ends = np.full((B, U), -1, dtype=np.int32)
    ts = np.full((B, U), -np.inf, dtype=np.float32)
    for b, n in enumerate((9, 6, 0)):       # a full row, a shorter one, an infeasible one
        edges = np.sort(rng.choice(60, size=2 * n, replace=False))
        starts[b, :n], ends[b, :n] = edges[0::2], edges[1::2]
        ts[b, :n] = -rng.random(n).astype(np.float32) * (ends[b, :n] - starts[b, :n] + 1)
    shared = [0, 2, 2, 5, 9]                 # an empty segment among them
    per_row = [[0, 3, 6, 9, 9], [0, 1, 6, 6, 8], [0, 4, 9, 9, 9]]
    for off in (shared, per_row):
        got = ctc.ctc_segment_scores(torch.from_numpy(starts), torch.from_numpy(ends), torch.from_numpy(ts),
                                     torch.tensor(off))
        assert [tuple(g.shape) for g in got] == [(B, 4)] * 3 and got[2].dtype == torch.float32
        for b in range(B):
            want = L.segment_loop(starts[b], ends[b], ts[b], off if off is shared else off[b])
            assert got[0][b].tolist() == want[0] and got[1][b].tolist() == want[1]
            for g, w in zip(got[2][b].tolist(), want[2]):
                assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-6 * abs(w), (b, g, w)
    # unbatched, int64 offsets, and no token at all
    one = ctc.ctc_segment_scores(torch.from_numpy(starts[0]), torch.from_numpy(ends[0]), torch.from_numpy(ts[0]),
                                 torch.tensor(shared, dtype=torch.int64))
    assert one[0].tolist() == L.segment_loop(starts[0], ends[0], ts[0], shared)[0] and one[0].shape == (4,)
    none = ctc.ctc_segment_scores(torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32),
                                  torch.zeros((2, 0)), torch.tensor([0, 0, 0]))
    assert none[0].tolist() == [[-1, -1]] * 2 and torch.isnan(none[2]).all()
