"""float64 reference of the n-best alignment (numpy + torch on the CPU; no product imports), assembled from
tests/ctc_common.py: per hypothesis the full-sum score (`dp_cost`), the Viterbi path by the tie rule of include/pika_ctc.h
(`forward_sweep`, `backtrace` -- what `viterbi` runs), from it the first and last frame of every token's run and the
run's summed log-probability (`rescore`), the rounding bound of an fp32 path score (`bound`) and whether the optimum is
unique by `margin` > 2 * bound -- only then can an fp32 path be compared frame by frame.

Inputs: `randn_lp`, log_softmax64(scale * randn) rounded once to fp32 -- at scale 3 the hypotheses of a beam search stay
unique by margin (tests/test_ctc_nbest_refs.py counts them) -- and `ctc_commit_common.commit_lp`, speech-like and
blank-heavy, whose optima do NOT stay unique: used for the rescore criterion only, never for path identity.  n-best
lists come from `ctc_decode_common.beam_search`.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ctc_common as R
import ctc_commit_common as K
import ctc_decode_common as D

# (T, C, beam = nbest): the inputs whose paths the GPU test compares exactly, each at seeds 0-2
RANDN_SHAPES = [(12, 5, 4), (40, 8, 8), (70, 8, 16), (150, 40, 16)]
SEEDS = (0, 1, 2)


def randn_lp(T, C, seed, scale=3.0):
    """RandomState(1000 + seed), the seeding of `ctc_decode_common.case_lp`."""
    return D.log_softmax64(scale * np.random.RandomState(1000 + seed).randn(T, C)).astype(np.float32)


def commit_lp(T, C, seed, blank=0):
    return K.commit_lp(T, C, seed, blank=blank)


def beam_hyps(lp, beam, nbest, blank=0):
    """The label lists of the float64 prefix beam search, best first."""
    return [list(l) for l, _ in D.beam_search(lp, beam, nbest, blank)[0]]


@functools.lru_cache(maxsize=None)
def randn_case(T, C, beam, seed):
    lp = randn_lp(T, C, seed)
    return lp, beam_hyps(lp, beam, beam)


def repeats(seq):
    return sum(1 for a, b in zip(seq, seq[1:]) if a == b)


def feasible(T, C, seq, blank):
    return all(0 <= c < C and c != blank for c in seq) and T >= len(seq) + repeats(seq)


class Ref(object):
    """One hypothesis against lp (T,C): full, best, starts, ends, token_scores, labels (T,), bound, unique; an
    infeasible one has full = best = -inf and nothing else."""

    def __init__(self, lp, seq, blank=0):
        lp = np.asarray(lp, dtype=np.float64)
        T, C = lp.shape
        self.seq, self.feasible = list(seq), feasible(T, C, seq, blank)
        if not self.feasible:
            self.full = self.best = -np.inf
            return
        self.cost = R.dp_cost(lp, seq, blank)
        self.full = -self.cost
        self.best, self.labels, path, delta = R.viterbi(lp, seq, blank)
        assert np.array_equal(path, R.backtrace(*R.forward_sweep(lp, seq, blank)))
        self.bound = R.bound(delta, T)
        self.unique = R.margin(lp, seq, blank) > 2 * self.bound
        self.starts = np.array([np.flatnonzero(path == 2 * j + 1)[0] for j in range(len(seq))], dtype=np.int64)
        self.ends = np.array([np.flatnonzero(path == 2 * j + 1)[-1] for j in range(len(seq))], dtype=np.int64)
        self.token_scores = np.array([run_score(lp, s, e, c) for s, e, c in zip(self.starts, self.ends, seq)])


def run_score(lp, start, end, c):
    """Sum of lp[t, c] over t = start .. end in float64."""
    return R.rescore(np.asarray(lp, dtype=np.float64)[start:end + 1], [c] * (end - start + 1))


def nbest_align(lp, hyps, blank=0):
    """lp (T,C) of one utterance (its own T_b frames), hyps a list of label lists (None: a missing entry) ->
    [Ref or None]."""
    return [None if h is None else Ref(lp, h, blank) for h in hyps]


def labelling(T, starts, ends, seq, blank):
    """The frame labels that the runs [starts[j], ends[j]] of seq imply, blank elsewhere."""
    fl = np.full(T, blank, dtype=np.int64)
    for s, e, c in zip(starts, ends, seq):
        fl[s:e + 1] = c
    return fl


def cost_bound(lp, seqs, blank=0):
    """The relative bound tests/test_ctc_gpu.py uses for costs, min(max(4 * e32, 1e-6), 1e-3): e32 is the relative error
    of torch's fp32 CPU ctc_loss against float64 on the same (feasible) hypotheses of lp (T,C)."""
    seqs = [s for s in seqs if len(s) > 0]
    if not seqs:
        return 1e-6
    T, C = lp.shape
    x = torch.from_numpy(np.asarray(lp, dtype=np.float64))[:, None, :].expand(T, len(seqs), C).contiguous()
    tg, il = R.pad_targets(seqs), torch.full((len(seqs),), T, dtype=torch.int64)
    tl = torch.tensor([len(s) for s in seqs], dtype=torch.int64)
    c64 = F.ctc_loss(x, tg, il, tl, blank=blank, reduction="none")
    c32 = F.ctc_loss(x.float(), tg, il, tl, blank=blank, reduction="none").double()
    e32 = float(((c32 - c64).abs() / c64.abs().clamp(min=1e-30)).max())
    return min(max(4 * e32, 1e-6), 1e-3)
