"""float64 reference of the RNN-T forced alignment (numpy only; no product imports).

One utterance is two planes over its own (T, U+1) sub-lattice: lpb (T, U+1), the blank log-prob of cell (t, u), and
lpe (T, U), the log-prob of emitting label u+1 from cell (t, u).

    delta(0,0) = 0
    delta(t,u) = max(delta(t-1,u) + lpb(t-1,u), delta(t,u-1) + lpe(t,u-1))
    score      = delta(T-1,U) + lpb(T-1,U)

frames[u] is the frame at which the best path leaves cell (t, u) over the emission edge.  Ties go to the blank
predecessor in the back-trace from (T-1, U), i.e. to the earliest emission.
"""
import itertools

import numpy as np


def planes(lp, labels, n, Tn, Un, blank=0):
    """The two planes of utterance n of a dense (B,T,U1,V) array, in float64."""
    Tn, Un = int(Tn), int(Un)
    x = np.asarray(lp[n, :Tn, :Un + 1], dtype=np.float64)
    lpb = x[:, :, blank]
    lpe = x[:, np.arange(Un), np.asarray(labels[n, :Un], dtype=np.int64)] if Un else np.zeros((Tn, 0))
    return np.ascontiguousarray(lpb), np.ascontiguousarray(lpe)


def forward_sweep(lpb, lpe):
    """delta (T, U+1) and the decision of every cell (True: it was reached over the emission edge; a tie is False),
    one anti-diagonal at a time with exactly the two additions of the recurrence."""
    T, U1 = lpb.shape
    delta = np.full((T, U1), -np.inf)
    emit = np.zeros((T, U1), dtype=bool)
    delta[0, 0] = 0.0
    for d in range(1, T + U1 - 1):
        u = np.arange(max(0, d - T + 1), min(U1 - 1, d) + 1)
        t = d - u
        x = np.full(u.shape, -np.inf)
        y = np.full(u.shape, -np.inf)
        m = t >= 1
        x[m] = delta[t[m] - 1, u[m]] + lpb[t[m] - 1, u[m]]
        m = u >= 1
        y[m] = delta[t[m], u[m] - 1] + lpe[t[m], u[m] - 1]
        delta[t, u] = np.maximum(x, y)
        emit[t, u] = y > x
    return delta, emit


def backward_sweep(lpb, lpe):
    """gamma (T, U+1): the best score from cell (t, u) to the end, terminal blank included."""
    T, U1 = lpb.shape
    gamma = np.full((T, U1), -np.inf)
    gamma[T - 1, U1 - 1] = lpb[T - 1, U1 - 1]
    for d in range(T + U1 - 3, -1, -1):
        u = np.arange(max(0, d - T + 1), min(U1 - 1, d) + 1)
        t = d - u
        x = np.full(u.shape, -np.inf)
        y = np.full(u.shape, -np.inf)
        m = t + 1 < T
        x[m] = lpb[t[m], u[m]] + gamma[t[m] + 1, u[m]]
        m = u + 1 < U1
        y[m] = lpe[t[m], u[m]] + gamma[t[m], u[m] + 1]
        gamma[t, u] = np.maximum(x, y)
    return gamma


def backtrace(emit):
    T, U1 = emit.shape
    frames = np.zeros(U1 - 1, dtype=np.int64)
    t, u = T - 1, U1 - 1
    while t > 0 or u > 0:
        if u > 0 and (t == 0 or emit[t, u]):
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    return frames


def viterbi(lpb, lpe):
    """(score, frames (U,), delta)."""
    delta, emit = forward_sweep(lpb, lpe)
    return float(delta[-1, -1] + lpb[-1, -1]), backtrace(emit), delta


def rescore(lpb, lpe, frames):
    """Sum of the edges of the path that emits label u at frames[u], in float64."""
    T, U1 = lpb.shape
    frames = np.asarray(frames, dtype=np.int64)
    assert frames.shape == (U1 - 1,)
    ts = np.arange(T)
    col = np.searchsorted(frames, ts, side="right")     # labels emitted up to and including frame t
    return float(lpe[frames, np.arange(U1 - 1)].sum() + lpb[ts, col].sum())


def path_cells(frames, T):
    """Boolean (T, U+1) mask of the cells the path visits."""
    frames = np.asarray(frames, dtype=np.int64)
    U = frames.shape[0]
    on = np.zeros((T, U + 1), dtype=bool)
    lo = np.concatenate([[0], frames])                   # column u is entered at frame lo[u] ...
    hi = np.concatenate([frames, [T - 1]])               # ... and left at frame hi[u]
    for u in range(U + 1):
        on[lo[u]:hi[u] + 1, u] = True
    return on


def margin(lpb, lpe, frames=None):
    """Best score minus the best score of any path through a cell off the optimal path (inf if there is none)."""
    delta, emit = forward_sweep(lpb, lpe)
    gamma = backward_sweep(lpb, lpe)
    if frames is None:
        frames = backtrace(emit)
    best = delta[-1, -1] + lpb[-1, -1]
    off = ~path_cells(frames, lpb.shape[0])
    if not off.any():
        return np.inf
    return float(best - (delta + gamma)[off].max())


def bound(delta, T, U):
    """(T+U) * 2^-23 * max|delta|: T+U rounded fp32 additions on values no larger than the fp64 lattice's own."""
    return (int(T) + int(U)) * 2.0 ** -23 * float(np.abs(delta[np.isfinite(delta)]).max())


def brute_force(lpb, lpe):
    """(score, frames) by enumerating all C(T-1+U, U) monotone paths; the first maximum in lexicographic order of the
    frames is the earliest-emission one."""
    T, U1 = lpb.shape
    best, arg = -np.inf, None
    for fr in itertools.combinations_with_replacement(range(T), U1 - 1):
        s = rescore(lpb, lpe, np.asarray(fr, dtype=np.int64))
        if s > best:
            best, arg = s, np.asarray(fr, dtype=np.int64)
    return best, arg


def valid_frames(frames, T):
    """Non-decreasing and inside [0, T-1]."""
    frames = np.asarray(frames)
    return bool((np.diff(frames) >= 0).all() and (frames >= 0).all() and (frames <= T - 1).all())
