"""Reference of the CTC prefix beam search with n-gram LM shallow fusion (numpy on the CPU; the only product import
is `NgramFst`, the container of the LM's arrays).

The LM is an ilabel-sorted CSR back-off FST; class c is label c + label_offset, back-off arcs carry backoff_id.
`RefLm.step(s, c)`: the arc c + label_offset out of s if s has it -- increment -(back-off cost so far + weight), new
state its nextstate; otherwise s's back-off arc (add its weight, move on), at most 8 hops; a state with neither arc:
None, the child does not exist.  The first match along the chain wins.  `RefLm.final(s)`: the same walk to the first
state with a finite final cost.

`search(lp, lm, beam, candidates, blank, lm_weight, length_bonus, use_final, dtype)` is keyed by label tuples.  A prefix
l carries (p_b, p_nb), tot = p_b (+) p_nb, and bonus(l) = lm_weight * LM(l) + length_bonus * |l|, LM(l) the sum of the
step increments along l from the start state; it is ranked by F = tot + bonus.  The acoustic recursion is
`ctc_decode_common.beam_search`'s; contributions to one label sequence are summed whichever parent they come from.
Candidates of a parent l at a frame: the `candidates` best non-blank classes of the row (higher value, then lower
class), plus last(l), plus every class whose child is in the beam.  Tie order: higher F, then prefixes that were in the
beam (by previous rank), then fresh ones by parent rank, then class.  At the end, with use_final, every prefix adds
lm_weight * final(state), prefixes without a final state drop out, and the list is sorted again (ties: the rank
before).  It returns ([(labels, fused score, tot)], margin, re-entries), margin and re-entries as in
`ctc_decode_common`: the smallest gap between the last kept and the first dropped candidate at any frame or between
neighbours of the final list; the number of prefixes that re-enter the beam while a descendant is still in it.

In float64 it is the reference; in float32 (LM sums, bonus and F included) the yardstick of the tolerances.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_decode_common as D  # noqa: E402
from pika_amd.decoder.ngram_fst import NgramFst  # noqa: E402

MAX_HOPS = 8


class RefLm(object):
    def __init__(self, fst, backoff_id, label_offset=1):
        self.fst, self.backoff_id, self.label_offset = fst, int(backoff_id), int(label_offset)
        self.off = [int(v) for v in fst.offsets]
        self.il = [int(v) for v in fst.ilabel]
        self.w = [float(v) for v in fst.weight]         # fp32 values, exact in float64
        self.ns = [int(v) for v in fst.nextstate]
        self.fin = [float(v) for v in fst.final]
        self.start = int(fst.start)
        self.arcs = [{self.il[a]: a for a in range(self.off[s], self.off[s + 1])} for s in range(fst.num_states)]

    def step(self, s, c, dtype=np.float64):
        """(increment, next state) or None."""
        cost = dtype(0.0)
        for _ in range(MAX_HOPS + 1):
            a = self.arcs[s].get(c + self.label_offset)
            if a is not None:
                return -(cost + dtype(self.w[a])), self.ns[a]
            b = self.arcs[s].get(self.backoff_id)
            if b is None:
                return None
            cost = cost + dtype(self.w[b])
            s = self.ns[b]
        return None

    def final(self, s, dtype=np.float64):
        """The increment of the final cost, or None."""
        cost = dtype(0.0)
        for _ in range(MAX_HOPS + 1):
            if np.isfinite(self.fin[s]):
                return -(cost + dtype(self.fin[s]))
            b = self.arcs[s].get(self.backoff_id)
            if b is None:
                return None
            cost = cost + dtype(self.w[b])
            s = self.ns[b]
        return None

    def score(self, labels):
        """float64 (LM(l), state) of a label sequence, or None when the LM cannot produce it."""
        s, total = self.start, 0.0
        for c in labels:
            st = self.step(s, c)
            if st is None:
                return None
            total += float(st[0])
            s = st[1]
        return total, s

    def reaches(self, c):
        return any(c + self.label_offset in arcs for arcs in self.arcs)


def make_lm(C, blank, seed, order=2, unreachable=(), arcs_per_state=4):
    """A seeded back-off LM over the non-blank classes: state 0 the unigram state (an arc for every class but the
    `unreachable` ones, a final cost, no back-off arc), state 1 the start state, one bigram state per class and, with
    order = 3, trigram states under a random subset of the bigram arcs; each of them holds a random subset of arcs and
    one back-off arc; random final costs; costs in [0.3, 5] rounded to fp32.  Labels are class + 1, the back-off label
    is C + 1."""
    rng = np.random.RandomState(7000 + seed)
    classes = [c for c in range(C) if c != blank and c not in unreachable]
    backoff_id = C + 1

    def cost():
        return float(np.float32(rng.uniform(0.3, 5.0)))

    def subset():
        k = int(rng.randint(0, min(len(classes), arcs_per_state) + 1))
        return sorted(int(v) for v in rng.choice(classes, size=k, replace=False)) if k else []
    bigram = {c: 2 + i for i, c in enumerate(classes)}
    n = 2 + len(classes)
    arcs, finals = [], {0: cost()}
    for c in classes:
        arcs.append((0, c + 1, cost(), bigram[c]))
    bi_arcs = {h: subset() for h in classes}
    trigram = {}
    if order >= 3:
        for h in classes:
            for c in bi_arcs[h]:
                if rng.rand() < 0.6:
                    trigram[(h, c)] = n
                    n += 1
    for c in subset():                                    # the start state
        arcs.append((1, c + 1, cost(), bigram[c]))
    arcs.append((1, backoff_id, cost(), 0))
    for h in classes:
        s = bigram[h]
        for c in bi_arcs[h]:
            arcs.append((s, c + 1, cost(), trigram.get((h, c), bigram[c])))
        arcs.append((s, backoff_id, cost(), 0))
        if rng.rand() < 0.5:
            finals[s] = cost()
    for (h, c), s in trigram.items():
        for d in subset():
            arcs.append((s, d + 1, cost(), trigram.get((c, d), bigram[d])))
        arcs.append((s, backoff_id, cost(), bigram[c]))
        if rng.rand() < 0.3:
            finals[s] = cost()
    return RefLm(NgramFst.from_arcs(n, arcs, finals, start=1), backoff_id, 1)


def fst_args(lm, start=True):
    """A device LM (the attributes of a `CtcNgramLm`) in the order the headers give an automaton's arguments: the five
    arrays, num_states, num_arcs, start where the call has one, backoff_id, label_offset.  Written out here, not taken
    from the package, so that the tests that call the C ABI check this order from outside."""
    arrays = [getattr(lm, name).data_ptr() for name in ("offsets", "ilabel", "weight", "nextstate", "final")]
    return tuple(arrays + [lm.num_states, lm.num_arcs] + ([lm.start] if start else []) + [lm.backoff_id, lm.label_offset])


def search(lp, lm, beam, candidates, blank=0, lm_weight=0.5, length_bonus=0.0, use_final=True, dtype=np.float64):
    """-> (hyps, margin, reentries); hyps = [(label tuple, fused score, tot)] of the whole final beam, best first."""
    lp = np.asarray(lp).astype(dtype)
    T, C = lp.shape
    ninf = dtype(-np.inf)
    lae = np.logaddexp
    lmw, lb = dtype(lm_weight), dtype(length_bonus)
    nonblank = [c for c in range(C) if c != blank]
    cur = [((), dtype(0.0), ninf, dtype(0.0), lm.start)]          # (labels, p_b, p_nb, bonus, LM state), rank order
    margin, reentries = np.inf, 0
    for t in range(T):
        row = lp[t]
        if candidates >= len(nonblank):
            top = nonblank
        else:
            idx = np.lexsort((np.asarray(nonblank), -row[nonblank]))[:candidates]
            top = [nonblank[i] for i in idx]
        old = {l: r for r, (l, _, _, _, _) in enumerate(cur)}
        acc, info = {}, {}

        def add(l, key, b, nb, bonus, state):
            if l in acc:
                pb, pnb = acc[l]
                acc[l] = (lae(pb, b), lae(pnb, nb))
            else:
                acc[l] = (b, nb)
            if key is not None:                 # a contribution to a prefix of the beam brings neither key nor bonus
                info[l] = (key, bonus, state)
        for r, (l, pb, pnb, bonus, state) in enumerate(cur):
            tot = lae(pb, pnb)
            add(l, (0, r, 0), row[blank] + tot, (row[l[-1]] + pnb) if l else ninf, bonus, state)
            cands = set(top)
            if l:
                cands.add(l[-1])
            cands.update(d[-1] for d in old if len(d) == len(l) + 1 and d[:-1] == l)
            for c in sorted(cands):
                child = l + (c,)
                am = row[c] + (pb if (l and c == l[-1]) else tot)
                if child in old:
                    add(child, None, ninf, am, None, None)
                    continue
                st = lm.step(state, c, dtype)
                if st is None:
                    continue
                add(child, (1, r, c), ninf, am, bonus + lmw * st[0] + lb, st[1])
        cand = []
        for l, (b, nb) in acc.items():
            tot = lae(b, nb)
            if tot > ninf:
                key, bonus, state = info[l]
                cand.append((dtype(tot + bonus), key, l, b, nb, bonus, state))
        cand.sort(key=lambda x: (-x[0], x[1]))
        if len(cand) > beam:
            margin = min(margin, float(cand[beam - 1][0] - cand[beam][0]))
        cand = cand[:beam]
        for x in cand:
            l = x[2]
            if l not in old and any(len(d) > len(l) and d[:len(l)] == l for d in old):
                reentries += 1
        cur = [(l, b, nb, bonus, state) for (_, _, l, b, nb, bonus, state) in cand]
    hyps = []
    for rank, (l, b, nb, bonus, state) in enumerate(cur):
        tot = lae(b, nb)
        fused = dtype(tot + bonus)
        if use_final:
            fin = lm.final(state, dtype)
            if fin is None:
                continue
            fused = dtype(fused + lmw * fin)
        hyps.append((-fused, rank, l, float(fused), float(tot)))
    hyps.sort(key=lambda x: (x[0], x[1]))
    hyps = [(l, f, a) for (_, _, l, f, a) in hyps]
    for (_, a, _), (_, b, _) in zip(hyps, hyps[1:]):
        margin = min(margin, a - b)
    return hyps, float(margin), reentries


def sharp_lp(T, C, seed, scale):
    """Sharpened posteriors: the float64 log-softmax of scale * randn, rounded to fp32."""
    return D.log_softmax64(scale * np.random.RandomState(1000 + seed).randn(T, C)).astype(np.float32)


def f32(v):
    """A Python float that fp32 holds exactly: what the device gets is what the reference gets."""
    return float(np.float32(v))


class LmCase(object):
    """One utterance: seeded fp32 log-probs (T,C) and a seeded LM; float64 reference, float32 yardstick, bound --
    computed once.  Bound and "separated" are `ctc_decode_common.SearchCase`'s."""

    def __init__(self, T, C, beam, candidates, seed=0, blank=0, lm_weight=0.5, length_bonus=0.0, use_final=True,
                 order=2, unreachable=(), sharpen=None, lp=None, lm=None, lm_seed=None):
        self.T, self.C, self.beam, self.candidates, self.seed, self.blank = T, C, beam, candidates, seed, blank
        self.lm_weight, self.length_bonus, self.use_final = f32(lm_weight), f32(length_bonus), use_final
        self.order, self.unreachable = order, tuple(unreachable)
        self.name = "T%d_C%d_beam%d_cand%d_s%d" % (T, C, beam, candidates, seed)
        if lp is None:
            lp = D.case_lp(T, C, seed) if sharpen is None else sharp_lp(T, C, seed, sharpen)
        self.lp = lp
        self.lm = lm if lm is not None else make_lm(C, blank, seed if lm_seed is None else lm_seed, order, unreachable)
        self._ref = None

    def run(self, candidates=None, dtype=np.float64):
        return search(self.lp, self.lm, self.beam, self.candidates if candidates is None else candidates, self.blank,
                      self.lm_weight, self.length_bonus, self.use_final, dtype)

    def ref(self):
        """(hyps64 (the whole beam), bound, separated, re-entries, margin, float32 error)"""
        if self._ref is None:
            h64, margin, reent = self.run()
            h32, _, _ = self.run(dtype=np.float32)
            s64 = {l: (f, a) for l, f, a in h64}
            err = max([max(abs(f - s64[l][0]), abs(a - s64[l][1])) for l, f, a in h32 if l in s64] + [0.0])
            top = max([max(abs(f), abs(a)) for _, f, a in h64] + [0.0])
            bound = max(4 * err, 1e-6 * top)
            self._ref = (h64, bound, margin > 2 * bound, reent, margin, err)
        return self._ref


# The cases of tests/test_ctc_lm_gpu.py; tests/test_ctc_lm_surface.py checks their properties on the CPU.
LM_CASES = [
    LmCase(12, 3, 2, 2, 1, lm_weight=0.5), LmCase(30, 4, 3, 3, 3, lm_weight=0.3, length_bonus=0.5),
    LmCase(24, 4, 4, 3, 2, lm_weight=1.0, order=3), LmCase(60, 8, 8, 7, 0, lm_weight=0.7, length_bonus=-0.5, order=3),
    LmCase(20, 6, 1, 5, 0, lm_weight=2.0),                                         # beam = 1
    LmCase(16, 8, 16, 7, 0, lm_weight=0.5, use_final=False, order=3),
    LmCase(10, 40, 16, 32, 0, lm_weight=1.0, length_bonus=1.0), LmCase(10, 40, 16, 8, 0, lm_weight=1.0, order=3),
    LmCase(6, 260, 16, 32, 4, blank=100, lm_weight=0.5, unreachable=(7, 101, 200)),
    LmCase(8, 70, 64, 128, 0, lm_weight=0.3, use_final=False),                     # the widest beam and class list
    LmCase(8, 70, 64, 20, 2, lm_weight=1.5, length_bonus=0.25, order=3),
    LmCase(5, 1028, 16, 32, 0, lm_weight=0.5), LmCase(4, 5003, 4, 8, 0, lm_weight=0.3, length_bonus=0.5),
    LmCase(40, 12, 8, 4, 0, lm_weight=1.0, order=3), LmCase(40, 12, 8, 11, 0, lm_weight=1.0, order=3),
    # drift, on sharpened posteriors (flat ones never separate at T = 600); seed 23 is separated, seed 0 is not
    LmCase(600, 6, 4, 5, 23, lm_weight=0.5, sharpen=5.0), LmCase(600, 6, 4, 5, 0, lm_weight=0.3, sharpen=3.0, order=3),
    LmCase(3, 3, 16, 2, 0, lm_weight=0.0), LmCase(2, 4, 16, 3, 0, lm_weight=1.0, length_bonus=-0.5),
    LmCase(1, 2, 4, 1, 0, lm_weight=0.5), LmCase(4, 2, 16, 1, 0, lm_weight=2.0, use_final=False),
]
# the ragged batch: three utterances of one (T,B,C) tensor, one LM
RAGGED_T, RAGGED_C, RAGGED_BEAM, RAGGED_CAND, RAGGED_ILS = 14, 5, 4, 3, [14, 9, 11]
RAGGED_LP = D.case_lp(RAGGED_T, RAGGED_C, 40, B=3)
RAGGED_LM = make_lm(RAGGED_C, 0, 40, order=3)
RAGGED_CASES = [LmCase(il, RAGGED_C, RAGGED_BEAM, RAGGED_CAND, 40 + n, lm_weight=0.5, length_bonus=0.25,
                       lp=RAGGED_LP[:il, n], lm=RAGGED_LM) for n, il in enumerate(RAGGED_ILS)]
ALL_CASES = LM_CASES + RAGGED_CASES
