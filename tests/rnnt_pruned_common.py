"""Numpy / plain-Python references of the pruned (banded) RNN-T lattice (include/pika_rnnt.h "Pruned RNN-T"); no product
imports.  `ranges` (B, T) holds the band starts s_t; everything here clamps them as the device does, to
[0, max(0, U_n + 1 - S)]."""
import numpy as np

NEG = -1.0e30


def clamp_ranges(ranges, ul, S):
    smax = np.maximum(0, np.asarray(ul, np.int64) + 1 - S)
    return np.clip(np.asarray(ranges, np.int64), 0, smax[:, None])


def scatter(band, ranges, U1, ul):
    """band (B,T,S,V) -> (B,T,U1,V) float32: row j of frame t at cell (t, s_t + j), -1e30 everywhere else."""
    B, T, S, V = band.shape
    s = clamp_ranges(ranges, ul, S)
    full = np.full((B, T, U1, V), NEG, np.float32)
    for b in range(B):
        for t in range(T):
            hi = min(S, U1 - s[b, t])
            full[b, t, s[b, t]:s[b, t] + hi] = band[b, t, :hi]
    return full


def gather(full, ranges, S, ul):
    """The inverse: (B,T,U1,V) -> (B,T,S,V), rows that fall beyond column U1 - 1 zero."""
    B, T, U1, V = full.shape
    s = clamp_ranges(ranges, ul, S)
    band = np.zeros((B, T, S, V), full.dtype)
    for b in range(B):
        for t in range(T):
            hi = min(S, U1 - s[b, t])
            band[b, t, :hi] = full[b, t, s[b, t]:s[b, t] + hi]
    return band


def band_live(ranges, tl, ul, S):
    """(B,T,S) bool: band row j of frame t is a cell of the utterance's lattice (t < T_n and s_t + j <= U_n)."""
    s = clamp_ranges(ranges, ul, S)
    B, T = s.shape
    u = s[:, :, None] + np.arange(S)[None, None, :]
    return (np.arange(T)[None, :, None] < np.asarray(tl)[:, None, None]) & (u <= np.asarray(ul)[:, None, None])


def feasible_label_lengths(tl, ul, S):
    """U_n clipped to what a band of width S can reach in T_n frames: (T_n - 1)(S - 1) >= max(0, U_n + 1 - S)."""
    tl, ul = np.asarray(tl, np.int64), np.asarray(ul, np.int64)
    return np.minimum(ul, (tl - 1) * (S - 1) + S - 1).astype(np.int32)


def is_valid(s, Tn, Un, S):
    """The four conditions of a band that connects (0, 0) with (T_n - 1, U_n)."""
    s = np.asarray(s[:Tn], np.int64)
    d = np.diff(s)
    return bool(s[0] == 0 and s[-1] == max(0, Un + 1 - S) and (d >= 0).all() and (d <= S - 1).all())


def random_valid_ranges(tl, ul, S, rng, T=None):
    """(B,T) int32: a random valid band per utterance (frames t >= T_n hold s_max)."""
    B = len(tl)
    T = int(max(tl)) if T is None else T
    out = np.zeros((B, T), np.int32)
    for n in range(B):
        Tn, smax = int(tl[n]), max(0, int(ul[n]) + 1 - S)
        assert (Tn - 1) * (S - 1) >= smax, "no band of width %d connects T_n=%d, U_n=%d" % (S, Tn, ul[n])
        s = [0]
        for t in range(1, Tn):
            lo = max(s[-1], smax - (Tn - 1 - t) * (S - 1))
            hi = min(s[-1] + S - 1, smax)
            s.append(smax if t == Tn - 1 else int(rng.integers(lo, hi + 1)))
        out[n, :Tn] = s
        out[n, Tn:] = smax
        assert is_valid(out[n], Tn, int(ul[n]), S)
    return out


def prune_ranges_ref(blank_occ, label_occ, tl, ul, S):
    """The band search of include/pika_rnnt.h in plain loops over float64."""
    B, T, U1 = blank_occ.shape
    out = np.zeros((B, T), np.int32)
    for n in range(B):
        Tn, Un = int(tl[n]), int(ul[n])
        smax = max(0, Un + 1 - S)
        occ = blank_occ[n].astype(np.float64) + label_occ[n].astype(np.float64)
        raw = []
        for t in range(Tn):
            best, arg = -np.inf, 0
            for s in range(smax + 1):
                w = 0.0
                for u in range(s, min(s + S - 1, Un) + 1):
                    w += occ[t, u]
                if w > best:
                    best, arg = w, s
            raw.append(arg)
        raw[Tn - 1] = smax
        m = list(raw)
        for t in range(Tn - 2, -1, -1):
            m[t] = min(m[t], m[t + 1])
        f = [0]
        for t in range(1, Tn):
            f.append(min(m[t], f[t - 1] + S - 1))
        for t in range(Tn):
            out[n, t] = max(f[t], smax - (Tn - 1 - t) * (S - 1))
        out[n, Tn:] = smax
    return out


def brute_force_banded_cost(band, s, y, blank=0):
    """-log of the sum over the alignment paths that visit live cells only; tiny lattices.

    band (T,S,V) float64 log-probs of ONE utterance with T_n = T, U_n = len(y); s (T,) its band starts."""
    T, S, _ = band.shape
    U = len(y)
    total = []

    def walk(t, u, acc):
        if not s[t] <= u < s[t] + S:
            return
        row = band[t, u - s[t]]
        if t == T - 1 and u == U:
            total.append(acc + row[blank])
            return
        if t < T - 1:
            walk(t + 1, u, acc + row[blank])
        if u < U:
            walk(t, u + 1, acc + row[y[u]])

    walk(0, 0, 0.0)
    return -float(np.logaddexp.reduce(np.array(total, dtype=np.float64))) if total else np.inf
