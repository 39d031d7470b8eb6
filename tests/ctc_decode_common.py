"""References of CTC decoding (numpy on the CPU; no product imports).

`beam_search(lp, beam, nbest, blank, dtype)` is the usual prefix beam search over the FULL vocabulary, keyed by label
tuples: every prefix l of the beam carries (p_b, p_nb), tot = p_b (+) p_nb; at each frame blank adds lp[blank] + tot to
p_b(l); a class c == last(l) adds lp[c] + p_nb to p_nb(l) and lp[c] + p_b to p_nb(l+c); any other class adds
lp[c] + tot to p_nb(l+c); contributions to one label sequence are summed whichever parent they come from; the `beam`
best by tot survive.  Tie order: higher tot, then prefixes that were in the beam (by their previous rank) before fresh
ones (by parent rank, then class index).  Candidates of probability zero (tot = -inf) do not exist.

In float64 it is the reference; run in float32 it is the yardstick of the tolerances.  It also returns
  margin    the smallest gap met at any frame between the last kept and the first dropped candidate, or between
            neighbouring entries of the final n-best (inf when nothing was ever dropped and one entry is returned)
  reentries the number of orphan re-entries: a prefix that was not in the beam enters it while a descendant of it is
            still there (in the beam the frame started with)
"""
import numpy as np


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def case_lp(T, C, seed, B=None):
    """The seeded inputs of the decode tests: RandomState(1000+seed).randn, float64 log-softmax, rounded to fp32."""
    shape = (T, C) if B is None else (T, B, C)
    return log_softmax64(np.random.RandomState(1000 + seed).randn(*shape)).astype(np.float32)


def greedy(lp, blank=0):
    """(tokens, first frames, score) of one utterance lp (T, C): per-frame argmax (lowest index on equal values),
    repeats merged, blanks dropped; score = the sum of the chosen values in float64."""
    lp = np.asarray(lp)
    best = lp.argmax(-1)                       # numpy: the first maximum
    score = float(lp[np.arange(len(best)), best].astype(np.float64).sum())
    tokens, frames, prev = [], [], -1
    for t, c in enumerate(int(v) for v in best):
        if c != prev and c != blank:
            tokens.append(c)
            frames.append(t)
        prev = c
    return tokens, frames, score


def beam_search(lp, beam, nbest=1, blank=0, dtype=np.float64):
    """-> (hyps, margin, reentries); hyps = [(label tuple, score)] * min(nbest, prefixes alive), best first."""
    lp = np.asarray(lp).astype(dtype)
    T, C = lp.shape
    ninf = dtype(-np.inf)
    lae = np.logaddexp
    cur = [((), dtype(0.0), ninf)]             # rank order
    margin, reentries = np.inf, 0
    for t in range(T):
        row = lp[t]
        old = {l: r for r, (l, _, _) in enumerate(cur)}
        acc, order = {}, {}

        def add(l, key, b, nb):
            if l in acc:
                pb, pnb = acc[l]
                acc[l] = (lae(pb, b), lae(pnb, nb))
            else:
                acc[l] = (b, nb)
                order[l] = key
            if l in old:
                order[l] = (0, old[l], 0)
        for r, (l, pb, pnb) in enumerate(cur):
            tot = lae(pb, pnb)
            add(l, (0, r, 0), row[blank] + tot, (row[l[-1]] + pnb) if l else ninf)
            for c in range(C):
                if c == blank:
                    continue
                add(l + (c,), (1, r, c), ninf, row[c] + (pb if (l and c == l[-1]) else tot))
        cand = [(lae(b, nb), order[l], l, b, nb) for l, (b, nb) in acc.items()]
        cand = [x for x in cand if x[0] > ninf]
        cand.sort(key=lambda x: (-x[0], x[1]))
        if len(cand) > beam:
            margin = min(margin, float(cand[beam - 1][0] - cand[beam][0]))
        cand = cand[:beam]
        kept = [x[2] for x in cand]
        for l in kept:
            if l not in old and any(len(d) > len(l) and d[:len(l)] == l for d in old):
                reentries += 1
        cur = [(l, b, nb) for (_, _, l, b, nb) in cand]
    hyps = [(l, float(lae(b, nb))) for (l, b, nb) in cur[:nbest]]
    for (_, a), (_, b) in zip(hyps, hyps[1:]):
        margin = min(margin, a - b)
    return hyps, float(margin), reentries


class SearchCase(object):
    """One utterance: seeded fp32 log-probs (T,C); float64 reference, float32 yardstick, bound -- computed once."""

    def __init__(self, T, C, beam, seed=0, blank=0, exhaustive=False, lp=None):
        self.T, self.C, self.beam, self.seed, self.blank, self.exhaustive = T, C, beam, seed, blank, exhaustive
        self.name = "T%d_C%d_beam%d_s%d" % (T, C, beam, seed)
        self.lp = case_lp(T, C, seed) if lp is None else lp
        self._ref = None

    def ref(self):
        """(hyps64 (nbest = beam), bound, separated, re-entries)"""
        if self._ref is None:
            h64, margin, reent = beam_search(self.lp, self.beam, self.beam, self.blank)
            h32, _, _ = beam_search(self.lp, self.beam, self.beam, self.blank, dtype=np.float32)
            s64 = dict(h64)
            err = max([abs(s - s64[l]) for l, s in h32 if l in s64] + [0.0])
            bound = max(4 * err, 1e-6 * max(abs(s) for _, s in h64))
            self._ref = (h64, bound, margin > 2 * bound, reent, margin, err)
        return self._ref


# The search cases of tests/test_ctc_decode_gpu.py; tests/test_ctc_decode_surface.py checks their properties on the CPU.
SEARCH_CASES = [
    SearchCase(12, 3, 2, 1), SearchCase(30, 4, 3, 3), SearchCase(24, 4, 4, 2), SearchCase(24, 4, 4, 3),
    SearchCase(60, 8, 8, 0),                                     # the re-entry cases
    SearchCase(20, 6, 1, 0),                                     # beam = 1
    SearchCase(16, 8, 16, 0), SearchCase(10, 40, 16, 0),
    SearchCase(6, 260, 16, 4, blank=100),
    SearchCase(8, 70, 64, 0), SearchCase(8, 70, 64, 2),           # the wave-wide beam; K = 128 > C - 1: padded class list
    SearchCase(5, 1028, 16, 0), SearchCase(4, 5003, 4, 0),
    SearchCase(600, 6, 4, 23), SearchCase(600, 6, 4, 0),          # drift; seed 23 is separated, seed 0 is not
    SearchCase(3, 3, 16, 0, exhaustive=True), SearchCase(3, 3, 16, 1, blank=2, exhaustive=True),
    SearchCase(2, 4, 16, 0, exhaustive=True), SearchCase(1, 2, 4, 0, exhaustive=True),
    SearchCase(4, 2, 16, 0, exhaustive=True),
]
# the ragged batch: three utterances of one (T,B,C) tensor
RAGGED_T, RAGGED_C, RAGGED_BEAM, RAGGED_ILS = 14, 5, 4, [14, 9, 11]
RAGGED_LP = case_lp(RAGGED_T, RAGGED_C, 40, B=3)
RAGGED_CASES = [SearchCase(il, RAGGED_C, RAGGED_BEAM, 40 + n, lp=RAGGED_LP[:il, n]) for n, il in enumerate(RAGGED_ILS)]
ALL_SEARCH = SEARCH_CASES + RAGGED_CASES
