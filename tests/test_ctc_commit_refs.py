"""CPU-side checks of the references behind tests/test_ctc_commit_gpu.py (tests/ctc_commit_common.py): the recharge rule,
the exact and the forced hook, and the conditions the chosen inputs must meet so that the GPU tests show something."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_commit_common as M  # noqa: E402
import ctc_decode_common as D  # noqa: E402
import ctc_lm_common as L  # noqa: E402


def test_recharge_never_raises_frames_and_keeps_the_phase():
    rng = np.random.RandomState(0)
    for _ in range(300):
        beam = int(rng.randint(1, 17))
        frames = int(rng.randint(0, 60))
        # a beam that `frames` frames can have produced: at most `beam` tuples of at most `frames` labels over 3 classes,
        # their trie within frames * beam keys
        labels = sorted({tuple(int(v) for v in rng.randint(1, 4, size=rng.randint(0, frames + 1)))
                         for _ in range(int(rng.randint(1, beam + 1)))})
        _, _, tails = M.apply_commit(labels)
        live, tail, new = M.recharge(tails, beam, frames)
        if live > frames * beam:
            continue
        assert new <= frames and new % M.RENORM == frames % M.RENORM, (labels, beam, frames, new)
        assert new >= tail and new * beam >= live and new - M.RENORM < max(-(-live // beam), tail)
    assert M.recharge([()], 4, 13) == (0, 0, 5)
    assert M.recharge([(1, 2), (1, 3), (2,)], 2, 21) == (4, 2, 5)       # keys 1, 12, 13, 2: two frames' worth
    assert M.recharge([(1, 2, 3)], 4, 3) == (3, 3, 3)


def test_hooks_on_a_hand_made_beam():
    beam = [(5, 1, 2, 7), (5, 1, 2), (5, 1, 3, 3), (5, 1), (5, 1, 2, 7, 4), (6,)]
    assert M.common_prefix(beam[:5]) == (5, 1) and M.common_prefix(beam) == () and M.common_prefix([(3, 4)]) == (3, 4)
    assert M.apply_commit(beam[:5]) == ((5, 1), [0, 1, 2, 3, 4], [(2, 7), (2,), (3, 3), (), (2, 7, 4)])
    # forced: the best entry keeps 1 label; entries 2, 3 and 5 do not start with 5 1 2 and go; entry 1, the new root
    # itself, stays with no label left
    assert M.apply_commit(beam, 1) == ((5, 1, 2), [0, 1, 4], [(7,), (), (7, 4)])
    assert M.apply_commit(beam, 0) == ((5, 1, 2, 7), [0, 4], [(), (4,)])
    assert M.apply_commit(beam[:5], 2) == M.apply_commit(beam[:5])          # the tail is short enough: exact
    assert M.apply_commit(beam, 4) == ((), [0, 1, 2, 3, 4, 5], beam)


def test_exact_hook_leaves_the_final_nbest_unchanged():
    for n, il in enumerate(M.ILS1):
        lp = M.LP1[:il, n]
        for beam in M.BEAMS:
            want, margin, _ = D.beam_search(lp, beam, beam)
            for _, sizes in M.CHUNKINGS1:
                done, hyps, m = M.beam_search(lp, beam, beam, commits=M.commit_points(sizes, il))
                assert [(done + l, s) for l, s in hyps] == want and m == margin
    # without a hook it is the reference it restates
    assert M.beam_search(M.LP1[:, 0], 4, 4)[:2] == ((), D.beam_search(M.LP1[:, 0], 4, 4)[0])


def test_case_1_inputs_commit_before_the_last_chunk():
    pairs = early = 0
    for n, il in enumerate(M.ILS1):
        for beam in M.BEAMS:
            for _, sizes in M.CHUNKINGS1:
                log = []
                M.beam_search(M.LP1[:il, n], beam, beam, commits=M.commit_points(sizes, il), log=log)
                pairs += 1
                early += sum(c for t, c, _, _ in log if t < il) > 0
    assert 2 * early >= pairs, (early, pairs)


def test_case_2_inputs_fit_and_commit():
    assert M.MAXF2 < M.T2
    for n in range(M.B):
        for beam in M.BEAMS:
            log = []
            done, _, _ = M.beam_search(M.LP2[:, n], beam, beam, commits=range(M.CHUNK2, M.T2 + 1, M.CHUNK2), log=log)
            peak = max(before for _, _, before, _ in log)
            assert peak <= M.MAXF2 and len(done) > 0, (n, beam, peak, len(done))
            assert all(after <= before and after % 8 == before % 8 for _, _, before, after in log)


def test_case_2_inputs_fit_and_commit_with_the_lm():
    """The LM search has no hook of its own and needs none: an exact commit does not change the search, so the charge
    follows from the reference's beams on the prefixes of the utterance."""
    lm = L.make_lm(M.C, 0, M.LM_SEED, order=3)
    kw = M.LM_KW
    for n in range(M.B):
        for beam in M.BEAMS:
            frames = peak = done = 0
            for t in range(M.CHUNK2, M.T2 + 1, M.CHUNK2):
                hyps, _, _ = L.search(M.LP2[:t, n], lm, beam, kw["candidates"], 0, L.f32(kw["lm_weight"]),
                                      L.f32(kw["length_bonus"]), False)
                prefix = M.common_prefix([h[0] for h in hyps])
                assert len(prefix) >= done                    # what was committed stays a prefix of every entry
                done = len(prefix)
                peak = max(peak, frames + M.CHUNK2)
                frames = M.recharge([h[0][done:] for h in hyps], beam, frames + M.CHUNK2)[2]
            assert peak <= M.MAXF2 and done > 0, (n, beam, peak, done)


def test_forced_inputs_force():
    """Cases 5 and 6: at frame 24 the forced commit goes beyond the exact one and drops entries for some (stream, beam,
    max_tail), so the forced path is exercised."""
    dropped = deeper = 0
    for n in range(M.B):
        for beam in M.BEAMS:
            _, hyps, _ = M.beam_search(M.LP5[:M.T5, n], beam, beam)
            labels = [l for l, _ in hyps]
            exact = M.apply_commit(labels)
            for m in M.TAILS:
                forced = M.apply_commit(labels, m)
                assert forced[0][:len(exact[0])] == exact[0] and len(labels[0]) - len(forced[0]) <= m
                deeper += len(forced[0]) > len(exact[0])
                dropped += len(forced[1]) < len(labels)
    assert deeper >= 6 and dropped >= 6, (deeper, dropped)
