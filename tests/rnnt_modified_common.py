"""Numpy / plain-Python float64 references of the modified RNN-T topology (include/pika_rnnt.h "Modified topology"); no
product imports.  Every frame emits exactly one symbol: the blank edge is (t, u) -> (t+1, u), the label edge
(t, u) -> (t+1, u+1), row T_n is terminal and ll = alpha(T_n, U_n)."""
import numpy as np

from rnnt_pruned_common import NEG, clamp_ranges, gather, scatter  # noqa: F401  (re-exported for the tests)


def planes_of(lp, y, ul, blank=0):
    """(B,T,U1,V) log-probs -> the two (B,T,U1) float64 planes; label_lp is -inf from column U_n on."""
    B, T, U1, V = lp.shape
    pb = lp[..., blank].astype(np.float64)
    pl = np.full((B, T, U1), -np.inf)
    for b in range(B):
        for u in range(min(int(ul[b]), U1 - 1)):
            if 0 <= y[b, u] < V:
                pl[b, :, u] = lp[b, :, u, y[b, u]]
    return pb, pl


def modified_dp(pb, pl, Tn, Un):
    """One utterance: planes (T,U1) float64 -> (cost, alpha (Tn+1,Un+1), beta, occ_blank (T,U1), occ_label (T,U1)).

    Values <= -1e29 in the planes count as log zero.  No path: cost +inf, zero occupancies."""
    T, U1 = pb.shape
    pb = np.where(pb <= -1e29, -np.inf, pb.astype(np.float64))[:Tn, :Un + 1]
    pl = np.where(pl <= -1e29, -np.inf, pl.astype(np.float64))[:Tn, :Un + 1].copy()
    pl[:, Un] = -np.inf
    a = np.full((Tn + 1, Un + 1), -np.inf)
    a[0, 0] = 0.0
    for t in range(Tn):
        a[t + 1] = a[t] + pb[t]
        a[t + 1, 1:] = np.logaddexp(a[t + 1, 1:], a[t, :-1] + pl[t, :-1])
    be = np.full((Tn + 1, Un + 2), -np.inf)
    be[Tn, Un] = 0.0
    for t in range(Tn - 1, -1, -1):
        be[t, :Un + 1] = np.logaddexp(be[t + 1, :Un + 1] + pb[t], be[t + 1, 1:] + pl[t])
    ll = a[Tn, Un]
    ob, ol = np.zeros((T, U1)), np.zeros((T, U1))
    if np.isfinite(ll):
        with np.errstate(invalid="ignore"):
            eb = a[:Tn] + pb + be[1:, :Un + 1] - ll
            el = a[:Tn] + pl + be[1:, 1:] - ll
        ob[:Tn, :Un + 1] = np.exp(np.where(np.isnan(eb), -np.inf, eb))
        ol[:Tn, :Un + 1] = np.exp(np.where(np.isnan(el), -np.inf, el))
    return (-ll if np.isfinite(ll) else np.inf), a, be[:, :Un + 1], ob, ol


def planes_loss_ref(pb, pl, tl, ul):
    """Batch: (costs (B,), occ_blank (B,T,U1), occ_label (B,T,U1)), float64; d cost / d lp = -occ.  Lengths are clamped
    as on the device: T_n into [1, T], U_n into [0, U1 - 1]."""
    B, T, U1 = pb.shape
    costs, ob, ol = np.zeros(B), np.zeros((B, T, U1)), np.zeros((B, T, U1))
    for b in range(B):
        Tn, Un = int(np.clip(tl[b], 1, T)), int(np.clip(ul[b], 0, U1 - 1))
        costs[b], _, _, ob[b], ol[b] = modified_dp(pb[b], pl[b], Tn, Un)
    return costs, ob, ol


def loss_ref(lp, y, tl, ul, blank=0, fastemit_lambda=0.0):
    """(B,T,U1,V) log-probs (float32 or float64; <= -1e29 is log zero) -> (costs (B,), grads (B,T,U1,V)) float64, the
    label entries of the gradient times 1 + lambda."""
    B, T, U1, V = lp.shape
    pb, pl = planes_of(lp, y, ul, blank)
    costs, ob, ol = planes_loss_ref(pb, pl, tl, ul)
    g = np.zeros((B, T, U1, V))
    g[..., blank] = -ob
    for b in range(B):
        for u in range(min(int(ul[b]), U1 - 1)):
            if 0 <= y[b, u] < V:
                g[b, :, u, y[b, u]] += -(1.0 + fastemit_lambda) * ol[b, :, u]
    return costs, g


def brute_force_cost(pb, pl, Tn, Un, s=None, S=None):
    """-log of the sum over all paths of (T_n, U_n) in the modified topology, optionally through band cells only
    (s_t <= u < s_t + S for every visited cell (t, u), t < T_n); tiny lattices.  inf when there is no path."""
    total = []

    def walk(t, u, acc):
        if t == Tn:
            if u == Un:
                total.append(acc)
            return
        if s is not None and not s[t] <= u < s[t] + S:
            return
        walk(t + 1, u, acc + pb[t, u])
        if u < Un:
            walk(t + 1, u + 1, acc + pl[t, u])

    walk(0, 0, 0.0)
    total = [v for v in total if np.isfinite(v)]
    return -float(np.logaddexp.reduce(np.array(total, dtype=np.float64))) if total else np.inf


def band_planes(pb, pl, s, S):
    """One utterance's planes with everything outside the band at -inf."""
    T, U1 = pb.shape
    u = np.arange(U1)[None, :]
    inside = (u >= np.asarray(s)[:T, None]) & (u < np.asarray(s)[:T, None] + S)
    return np.where(inside, pb, -np.inf), np.where(inside, pl, -np.inf)


def is_valid_modified(s, Tn, Un, S):
    """s_0 = 0, s_{T_n-1} = s_max, steps in [0, 1]: a band that holds a path whenever U_n <= T_n."""
    s = np.asarray(s[:Tn], np.int64)
    d = np.diff(s)
    return bool(s[0] == 0 and s[-1] == max(0, Un + 1 - S) and (d >= 0).all() and (d <= 1).all())


def random_valid_ranges_modified(tl, ul, S, rng, T=None):
    """(B,T) int32: a random valid modified band per utterance (frames t >= T_n hold s_max); needs T_n - 1 >= s_max."""
    B = len(tl)
    T = int(max(tl)) if T is None else T
    out = np.zeros((B, T), np.int32)
    for n in range(B):
        Tn, smax = int(tl[n]), max(0, int(ul[n]) + 1 - S)
        assert Tn - 1 >= smax, "no modified band of width %d connects T_n=%d, U_n=%d" % (S, Tn, ul[n])
        s = [0]
        for t in range(1, Tn):
            lo = max(s[-1], smax - (Tn - 1 - t))
            hi = min(s[-1] + 1, smax)
            s.append(smax if t == Tn - 1 else int(rng.integers(lo, hi + 1)))
        out[n, :Tn] = s
        out[n, Tn:] = smax
        assert is_valid_modified(out[n], Tn, int(ul[n]), S)
    return out


def prune_ranges_modified_ref(blank_occ, label_occ, tl, ul, S):
    """The band search with step bound 1 (include/pika_rnnt.h) in plain loops over float64."""
    B, T, U1 = blank_occ.shape
    out = np.zeros((B, T), np.int32)
    for n in range(B):
        Tn, Un = int(np.clip(tl[n], 1, T)), int(np.clip(ul[n], 0, U1 - 1))
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
            f.append(min(m[t], f[t - 1] + 1))
        for t in range(Tn):
            out[n, t] = max(f[t], smax - (Tn - 1 - t))
        out[n, Tn:] = smax
    return out


def torch_costs(pb, pl, tl, ul):
    """The same DP in torch (any float dtype), differentiable: (B,) costs from (B,T,U1) planes."""
    import torch
    B, T, U1 = pb.shape
    ninf = NEG          # finite: logaddexp(-inf, -inf) has a NaN gradient, and exp(-1e30 - x) is exactly zero
    costs = []
    for b in range(B):
        Tn, Un = int(tl[b]), int(ul[b])
        a = torch.full((Un + 1,), ninf, dtype=pb.dtype)
        a = torch.cat([a.new_zeros(1), a[1:]])
        for t in range(Tn):
            stay = a + pb[b, t, :Un + 1]
            if Un > 0:
                move = torch.cat([a.new_full((1,), ninf), a[:-1] + pl[b, t, :Un]])
                a = torch.logaddexp(stay, move)
            else:
                a = stay
        costs.append(-a[Un])
    return torch.stack(costs)
