"""A numpy **fp32** reference of the long-form alignment contract (include/pika_ctc.h: pika_ctc_long_align), operation for
operation: one rounded fp32 subtraction per emission, one rounded fp32 addition per cell, max picks an operand.  Vectorised
over states, one loop over frames.  No product imports.

For one recording (its own T_b rows of x, its own U_b labels):
  value_t(c)  x (log-probs) or fl32(logit - lse); anything below -1e30, -inf and NaN included, reads as -1e30
  m_t         max_c value_t(c); for logits also maxlogit_t, and m_t = fl32(maxlogit_t - lse_t)
  e_t(s)      fl32(value_t(class(s)) - m_t), for logits fl32(logit_t(class(s)) - maxlogit_t)
  v_0(0) = e_0(0), v_0(1) = e_0(1), -1e30 elsewhere; v_t(s) = fl32(e_t(s) + max(stay, s-1, s-2 where allowed))
  back-pointer: the first maximal predecessor in the order stay, s-1, s-2; end: S-1 preferred over S-2
  score       fp64(v_end) + sum_t fp64(m_t)
A cell is TIED when two or more of its existing predecessors hold the maximum.
"""
import numpy as np

NEG = np.float32(-1.0e30)
F32 = np.float32


def dyadic(rng, shape, kmax=640, step=1):
    """-k/64 with integer k in [0, kmax], k a multiple of `step`: every sum of a few thousand of them is exact in fp32."""
    k = rng.integers(0, kmax // step + 1, size=shape) * step
    return (-k / 64.0).astype(np.float32)


def clamp(v):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(v >= NEG, v, NEG).astype(np.float32)


def states(seq, blank):
    ext = np.full(2 * len(seq) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(seq, dtype=np.int64)
    skip = np.zeros(len(ext), dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    return ext, skip


def _up(v, k):
    out = np.full(len(v), -np.inf, dtype=np.float32)    # a predecessor that does not exist never wins
    out[k:] = v[:len(v) - k]
    return out


class Result(object):
    """score64 (fp64; -inf: infeasible), score (f32), path (T,) states or None, starts / ends (U,) i32, token_scores (U,) f32,
    labels (T,) the class per frame, ties: number of tied cells, tied: (T,S) bool map (when asked for), live: (T,S) bool map
    of the cells some path reaches, kinds: on-path cells tied [stay = s-1, s-1 = s-2 above stay, stay = s-2], end_tie."""


def reference(x, seq, blank=0, lse=None, shift=True, maps=False):
    """The contract on one recording.  x (T,C) f32: log-probs, or logits when lse (T,) f32 is given.  shift=False: the
    same recurrence on value_t itself (log-probs only): what the row-maximum normalisation must not change."""
    x = np.asarray(x, dtype=np.float32)
    T, C = x.shape
    U = len(seq)
    R = Result()
    R.ties, R.tied, R.live, R.kinds, R.end_tie = 0, None, None, [0, 0, 0], False
    bad = any((c < 0 or c >= C or c == blank) for c in seq)
    raw = clamp(x)
    if lse is None:
        val = raw
        m = val.max(1)
    else:
        lse = np.asarray(lse, dtype=np.float32)
        val = clamp((x - lse[:, None]).astype(np.float32))
        m = clamp((raw.max(1) - lse).astype(np.float32))
    R.m = m

    def refuse():
        R.score64, R.score, R.path, R.labels = -np.inf, F32(-np.inf), None, None
        R.starts = np.full(U, -1, dtype=np.int32)
        R.ends = np.full(U, -1, dtype=np.int32)
        R.token_scores = np.full(U, -np.inf, dtype=np.float32)
        return R
    if bad:
        return refuse()
    ext, skip = states(seq, blank)
    S = len(ext)
    if lse is None:
        e = (val[:, ext] - m[:, None]).astype(np.float32) if shift else val[:, ext]
    else:
        assert shift
        e = (raw[:, ext] - raw.max(1)[:, None]).astype(np.float32)
    v = np.full(S, NEG, dtype=np.float32)
    v[:2] = e[0, :2]
    bp = np.zeros((T, S), dtype=np.int8)
    tied = np.zeros((T, S), dtype=bool) if maps else None
    live = np.zeros((T, S), dtype=bool) if maps else None
    if maps:
        live[0] = v > F32(-1e29)
    eq = np.zeros((T, S, 3), dtype=bool)
    for t in range(1, T):
        p0, p1 = v, _up(v, 1)
        p2 = np.where(skip, _up(v, 2), F32(-np.inf)).astype(np.float32)
        best, k = p0.copy(), np.zeros(S, dtype=np.int8)
        w = p1 > best
        best[w], k[w] = p1[w], 1
        w = p2 > best
        best[w], k[w] = p2[w], 2
        eq[t, :, 0], eq[t, :, 1], eq[t, :, 2] = p0 == best, p1 == best, p2 == best
        n = eq[t].sum(1)
        R.ties += int((n >= 2).sum())
        v = (e[t] + best).astype(np.float32)
        bp[t] = k
        if maps:
            tied[t] = n >= 2
            live[t] = v > F32(-1e29)
    R.tied, R.live = tied, live
    second = S >= 2 and v[S - 2] > v[S - 1]
    R.end_tie = bool(S >= 2 and v[S - 2] == v[S - 1])
    s = S - 2 if second else S - 1
    vend = v[s]
    if not vend > F32(-1e29):
        return refuse()
    R.score64 = float(np.float64(vend) + (m.astype(np.float64).sum() if shift else 0.0))
    R.score = F32(R.score64)
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        q = eq[t, s]
        if q[0] and q[1]:
            R.kinds[0] += 1
        if q[1] and q[2] and not q[0]:
            R.kinds[1] += 1
        if q[0] and q[2]:
            R.kinds[2] += 1
        s -= int(bp[t, s])
    R.path, R.labels = path, ext[path]
    R.starts = np.zeros(U, dtype=np.int32)
    R.ends = np.zeros(U, dtype=np.int32)
    R.token_scores = np.zeros(U, dtype=np.float32)
    for j in range(U):
        ts = np.nonzero(path == 2 * j + 1)[0]
        R.starts[j], R.ends[j] = ts[0], ts[-1]
        R.token_scores[j] = np.cumsum(val[ts[0]:ts[-1] + 1, seq[j]], dtype=np.float32)[-1]     # sequential fp32 adds
    return R


def batch_reference(x, targets, input_lengths, target_lengths, blank=0, lse=None, **kw):
    """x (T,B,C), targets (B,U_max), lengths as lists: ([Result per recording], scores (B,) f32, starts, ends (B,U_max) i32,
    token_scores (B,U_max) f32) with the padding the calls write beyond a length (-1, -1, -inf)."""
    x = np.asarray(x, dtype=np.float32)
    T, B, C = x.shape
    targets = np.asarray(targets).reshape(B, -1)
    U_max = targets.shape[1]
    scores = np.zeros(B, dtype=np.float32)
    starts = np.full((B, U_max), -1, dtype=np.int32)
    ends = np.full((B, U_max), -1, dtype=np.int32)
    tscores = np.full((B, U_max), -np.inf, dtype=np.float32)
    results = []
    for b in range(B):
        Tb = min(max(int(input_lengths[b]), 1), T)
        Ub = min(max(int(target_lengths[b]), 0), U_max)
        r = reference(x[:Tb, b], [int(c) for c in targets[b, :Ub]], blank,
                      None if lse is None else np.asarray(lse)[:Tb, b], **kw)
        results.append(r)
        scores[b] = r.score
        starts[b, :Ub], ends[b, :Ub], tscores[b, :Ub] = r.starts, r.ends, r.token_scores
    return results, scores, starts, ends, tscores


def frame_labels(starts, ends, seq, T, blank=0):
    """The frame labelling the token runs imply: token j on [starts[j], ends[j]], blank elsewhere."""
    out = np.full(T, blank, dtype=np.int64)
    for j, c in enumerate(seq):
        out[starts[j]:ends[j] + 1] = c
    return out


def state_paths(T, S, skip):
    """Every state path a CTC lattice of S states allows over T frames (tiny T, S only)."""
    for first in range(min(2, S)):
        stack = [(first,)]
        while stack:
            p = stack.pop()
            if len(p) == T:
                if p[-1] >= S - 2:
                    yield p
                continue
            s = p[-1]
            for d in (0, 1, 2):
                n = s + d
                if n < S and (d < 2 or skip[n]):
                    stack.append(p + (n,))


def brute_force(x, seq, blank=0):
    """(best score in fp64, the state path the tie rule selects) by enumerating every state path: among the paths of
    maximal score the rule picks the one whose REVERSED state sequence is lexicographically largest (the higher end
    state; then, frame by frame backwards, the nearest predecessor).  Exact on dyadic inputs.  (-inf, None): no path."""
    x = np.asarray(x, dtype=np.float64)
    ext, skip = states(seq, blank)
    T, S = x.shape[0], len(ext)
    best, arg = -np.inf, None
    for p in state_paths(T, S, skip):
        sc = float(x[np.arange(T), ext[list(p)]].sum())
        key = tuple(reversed(p))
        if sc > best or (sc == best and key > arg):
            best, arg = sc, key
    return best, (None if arg is None else np.asarray(tuple(reversed(arg)), dtype=np.int64))


def segment_loop(starts, ends, token_scores, offsets):
    """ctc_segment_scores by a loop, one row: (seg_start, seg_end, seg_confidence) lists."""
    U = len(starts)
    out = ([], [], [])
    for g in range(len(offsets) - 1):
        a, b = min(max(int(offsets[g]), 0), U), min(max(int(offsets[g + 1]), 0), U)
        toks = range(a, b)
        if b <= a or any(starts[j] < 0 for j in toks):
            row = (-1, -1, float("nan"))
        else:
            total = sum(float(token_scores[j]) for j in toks)
            frames = sum(int(ends[j]) - int(starts[j]) + 1 for j in toks)
            row = (int(starts[a]), int(ends[b - 1]), float(np.exp(total / frames)))
        for o, r in zip(out, row):
            o.append(r)
    return out

