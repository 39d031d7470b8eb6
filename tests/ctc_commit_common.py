"""References of `CtcBeamStream.commit` (numpy on the CPU; no product imports).

`beam_search(lp, beam, nbest, blank, dtype, commits, max_tail)` is the prefix beam search of `ctc_decode_common`,
restated so that a prefix carries its last label beside its label tuple: after a commit the tuple holds the
UNCOMMITTED labels only, and a prefix whose tuple is empty still has the last label the repeat rule needs.  After the
frames listed in `commits` (counted from 1: "after t frames") the hook runs:

  exact   (max_tail None)  the longest common prefix of the beam's label tuples -- the path to the common ancestor of
          their trie nodes -- moves to the committed list and is cut from every tuple.  Nothing else changes, so the
          final n-best (committed + tuple) is `ctc_decode_common.beam_search`'s.
  forced  (max_tail = m)   if the best entry would keep more than m labels beyond that prefix, the prefix becomes the
          best entry's labels less its last m, and the entries that do not start with it are dropped; the others keep
          their order.

`recharge(labels, beam, frames_old)` simulates what a commit leaves in the stream's header: `live` -- the keys of the
rebuilt trie, one per distinct non-empty prefix of the uncommitted tuples --, `tail`, the longest of them, and
frames_new, the smallest value >= max(ceil(live / beam), tail) congruent to frames_old modulo 8.

`commit_lp(T, C, seed, boost)` generates inputs on which a beam converges: randn, with runs of 1-3 frames in which one
random non-blank class is boosted, each followed by 0-2 frames in which the blank is.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_decode_common as D  # noqa: E402

RENORM = 8


def common_prefix(labels):
    """The longest common prefix of a list of label tuples (the empty list shares nothing)."""
    if not labels:
        return ()
    first = labels[0]
    d = min(len(l) for l in labels)
    for l in labels[1:]:
        k = 0
        while k < d and l[k] == first[k]:
            k += 1
        d = k
    return tuple(first[:d])


def apply_commit(labels, max_tail=None):
    """labels: the beam's tuples in rank order -> (committed prefix, [index kept], [tuple after the commit])."""
    prefix = common_prefix(labels)
    if max_tail is not None and labels and len(labels[0]) - len(prefix) > max_tail:
        prefix = tuple(labels[0][:len(labels[0]) - max_tail])
    d = len(prefix)
    keep = [i for i, l in enumerate(labels) if tuple(l[:d]) == prefix]
    return prefix, keep, [tuple(labels[i][d:]) for i in keep]


def recharge(labels, beam, frames_old):
    """labels: the tuples AFTER the commit -> (live, tail, frames_new)."""
    live = len({l[:k] for l in labels for k in range(1, len(l) + 1)})
    tail = max([len(l) for l in labels] + [0])
    need = max(-(-live // beam), tail)
    frames_new = need + (frames_old - need) % RENORM
    return live, tail, frames_new


def beam_search(lp, beam, nbest=1, blank=0, dtype=np.float64, commits=(), max_tail=None, log=None):
    """-> (committed labels, hyps, margin); hyps = [(uncommitted label tuple, score)], best first.  `log`, a list, gets
    one (frame count, labels committed by that hook, frames before, frames after) per hook: the simulated charge."""
    lp = np.asarray(lp).astype(dtype)
    T, C = lp.shape
    ninf = dtype(-np.inf)
    lae = np.logaddexp
    cur = [((), -1, dtype(0.0), ninf)]         # (uncommitted labels, last label, p_b, p_nb), rank order
    committed, margin, frames = [], np.inf, 0
    commits = set(commits)
    for t in range(T):
        row = lp[t]
        old = {l: r for r, (l, _, _, _) in enumerate(cur)}
        acc, order, last_of = {}, {}, {}

        def add(l, last, key, b, nb):
            if l in acc:
                pb, pnb = acc[l]
                acc[l] = (lae(pb, b), lae(pnb, nb))
            else:
                acc[l] = (b, nb)
                order[l] = key
                last_of[l] = last
            if l in old:
                order[l] = (0, old[l], 0)
        for r, (l, last, pb, pnb) in enumerate(cur):
            tot = lae(pb, pnb)
            add(l, last, (0, r, 0), row[blank] + tot, (row[last] + pnb) if last >= 0 else ninf)
            for c in range(C):
                if c == blank:
                    continue
                add(l + (c,), c, (1, r, c), ninf, row[c] + (pb if c == last else tot))
        cand = [(lae(b, nb), order[l], l, b, nb) for l, (b, nb) in acc.items()]
        cand = [x for x in cand if x[0] > ninf]
        cand.sort(key=lambda x: (-x[0], x[1]))
        if len(cand) > beam:
            margin = min(margin, float(cand[beam - 1][0] - cand[beam][0]))
        cur = [(l, last_of[l], b, nb) for (_, _, l, b, nb) in cand[:beam]]
        frames += 1
        if t + 1 in commits:
            if max_tail is not None and len(cur) > 1:   # the forced hook follows the best entry: its lead counts
                margin = min(margin, float(lae(cur[0][2], cur[0][3]) - lae(cur[1][2], cur[1][3])))
            prefix, keep, tails = apply_commit([l for l, _, _, _ in cur], max_tail)
            cur = [(tl,) + cur[i][1:] for i, tl in zip(keep, tails)]
            committed.extend(prefix)
            before = frames
            frames = recharge(tails, beam, frames)[2]
            if log is not None:
                log.append((t + 1, len(prefix), before, frames))
    hyps = [(l, float(lae(b, nb))) for (l, _, b, nb) in cur[:nbest]]
    for (_, a), (_, b) in zip(hyps, hyps[1:]):
        margin = min(margin, a - b)
    return tuple(committed), hyps, float(margin)


def commit_lp(T, C, seed, boost=3.0, blank=0):
    """Seeded fp32 log-probs (T,C) on which a beam converges (the module's docstring)."""
    rng = np.random.RandomState(3000 + seed)
    x = rng.randn(T, C)
    classes = [c for c in range(C) if c != blank]
    t = 0
    while t < T:
        c = classes[int(rng.randint(len(classes)))]
        k = int(rng.randint(1, 4))
        x[t:t + k, c] += boost
        t += k
        k = int(rng.randint(0, 3))
        x[t:t + k, blank] += boost
        t += k
    return D.log_softmax64(x).astype(np.float32)


def fixed(k, T):
    return [min(k, T - s) for s in range(0, T, k)]


def uneven(T, seed):
    rng = np.random.RandomState(500 + seed)
    sizes, left = [], T
    while left:
        sizes.append(int(rng.randint(1, min(left, 11) + 1)))
        left -= sizes[-1]
    return sizes


# ---- the inputs of tests/test_ctc_commit_gpu.py; tests/test_ctc_commit_refs.py asserts their properties on the CPU ----
C, B = 12, 3
BEAMS = (4, 16)
# the LM variant: ctc_lm_common.make_lm(C, 0, LM_SEED, order=3) with these arguments of the search
LM_SEED, LM_KW = 90, dict(lm_weight=0.5, length_bonus=0.25, candidates=8)
# case 1: max_frames = T = 40, ragged, commit after every chunk
T1, ILS1 = 40, [40, 29, 35]
LP1 = np.stack([commit_lp(T1, C, 10 + n) for n in range(B)], axis=1)         # (T,B,C)
CHUNKINGS1 = [("1", fixed(1, T1)), ("3", fixed(3, T1)), ("8", fixed(8, T1)), ("uneven", uneven(T1, 1))]
# case 2: T = 160 through max_frames = 80, chunks of 8
T2, MAXF2, CHUNK2 = 160, 80, 8
LP2 = np.stack([commit_lp(T2, C, seed) for seed in (20, 22, 24)], axis=1)
# cases 5 and 6: 24 frames, a forced commit, 16 more
T5, T6, TAILS = 24, 40, (0, 4)
LP5 = np.stack([commit_lp(T6, C, 30 + n, boost=1.5) for n in range(B)], axis=1)


def commit_points(sizes, il):
    """The frame counts at which an utterance of `il` frames is committed when a commit follows every chunk."""
    return sorted(set(int(min(s, il)) for s in np.cumsum(sizes)))
