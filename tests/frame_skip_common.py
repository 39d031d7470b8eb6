"""CTC-guided frame skipping (include/pika_frame_skip.h): the definition in numpy float64 -- a
plain loop per utterance, the min_frames top-up by an explicit stable sort --, the float32 yardstick of blank_lp, and the
input generators of tests/test_frame_skip_refs.py and tests/test_frame_skip_gpu.py."""
import math

import numpy as np

MARGIN = 1e-3       # every generated from-logits frame's float64 blank_lp is at least this far from log(threshold)


def log_thr(threshold):
    """float32(log(threshold)): what every implementation compares against."""
    if threshold <= 0:
        return np.float32(-np.inf)
    return np.float32(math.log(threshold)) if threshold != np.inf else np.float32(np.inf)


def blank_lp_of(scores, blank, from_logits, dtype=np.float64):
    """(B,T) blank log-prob of scores (B,T,C) computed in `dtype`: float64 is the definition, float32 the yardstick (the
    plain max / sum / log spelling, every operation rounded to float32)."""
    x = np.asarray(scores).astype(dtype)
    if not from_logits:
        return x[:, :, blank]
    with np.errstate(all="ignore"):
        m = x.max(axis=2)
        lse = m + np.log(np.exp(x - m[:, :, None]).sum(axis=2, dtype=dtype)).astype(dtype)
        return (x[:, :, blank] - lse).astype(dtype)


def plan(blank_lp, lengths, threshold, min_frames=None):
    """The definition.  blank_lp (B,T) -> (kept_lengths (B,), frame_index (B,T), position (B,T), blank_lp (B,T) with 0
    beyond L), integers as int32."""
    lp = np.asarray(blank_lp)
    B, T = lp.shape
    thr = log_thr(threshold)
    kept_lengths = np.zeros(B, np.int32)
    frame_index = np.full((B, T), -1, np.int32)
    position = np.full((B, T), -1, np.int32)
    out_lp = np.zeros((B, T), lp.dtype)
    for b in range(B):
        L = min(max(int(lengths[b]), 0), T)
        out_lp[b, :L] = lp[b, :L]
        dropped = [t for t in range(L) if lp[b, t] >= thr]              # a NaN compares false: kept
        kept = [t for t in range(L) if not lp[b, t] >= thr]
        m = 0 if L == 0 else min(max(1 if min_frames is None else int(min_frames[b]), 1), L)
        if len(kept) < m:
            order = np.argsort(np.array([lp[b, t] for t in dropped]), kind="stable")    # (value, then t: stable)
            kept = sorted(kept + [dropped[i] for i in order[:m - len(kept)]])
        kept_lengths[b] = len(kept)
        for j, t in enumerate(kept):
            frame_index[b, j] = t
            position[b, t] = j
    return kept_lengths, frame_index, position, out_lp


def apply(x, frame_index):
    """out[b,j] = x[b, frame_index[b,j]] where frame_index >= 0, zeros elsewhere (any dtype: rows are copied)."""
    out = np.zeros_like(x)
    for b in range(x.shape[0]):
        for j in range(x.shape[1]):
            if frame_index[b, j] >= 0:
                out[b, j] = x[b, frame_index[b, j]]
    return out


def lengths_for(B, T, rng):
    """Ragged lengths that always hold 0, 1 and T when B allows it."""
    fixed = [T, 0, 1][:B]
    return np.array(fixed + [int(v) for v in rng.integers(1, T + 1, B - len(fixed))], np.int64)


def make_log_probs(B, T, C, blank, threshold, seed, keep_share=0.4):
    """(B,T,C) float32 'log-probs' (the plan reads the blank's column alone): about keep_share of the frames below the
    threshold, a few exactly AT float32(log thr) (dropped)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    thr = log_thr(threshold)
    base = np.float32(thr) if np.isfinite(thr) else np.float32(0.0)
    col = base + rng.uniform(0.0, 0.04, (B, T)).astype(np.float32)
    low = rng.uniform(size=(B, T)) < keep_share
    col = np.where(low, base - rng.uniform(0.01, 3.0, (B, T)).astype(np.float32), col)
    at = rng.uniform(size=(B, T)) < 0.05
    x[:, :, blank] = np.where(at, base, col)
    return x


def make_logits(B, T, C, blank, threshold, seed):
    """(B,T,C) float32 logits with blank posteriors on both sides of the threshold; the blank logit of any frame whose
    float64 blank_lp is within MARGIN of log(threshold) is nudged until it is not, so float32 and float64 decide alike."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((B, T, C))).astype(np.float32)
    odds = rng.uniform(-1.0, 7.0, (B, T))                    # log(p / (1 - p)) of the blank posterior p: 0.27 .. 0.999
    rest = x.astype(np.float64)
    rest[:, :, blank] = -np.inf
    m = rest.max(axis=2)
    lse_rest = m + np.log(np.exp(rest - m[:, :, None]).sum(axis=2))
    x[:, :, blank] = (lse_rest + odds).astype(np.float32)
    thr = float(log_thr(threshold))
    for _ in range(8):
        near = np.abs(blank_lp_of(x, blank, True) - thr) < 2 * MARGIN
        if not near.any():
            break
        x[:, :, blank] = np.where(near, x[:, :, blank] + np.float32(0.05), x[:, :, blank])
    return x


def margin_holds(x, blank, threshold, lengths):
    lp = blank_lp_of(x, blank, True)
    ok = np.abs(lp - float(log_thr(threshold))) >= MARGIN
    t = np.arange(x.shape[1])[None, :]
    return bool((ok | (t >= np.clip(np.asarray(lengths), 0, x.shape[1])[:, None])).all())


def plan_cases(T, seed=0):
    """The from-log-probs cases at one T: [(name, x (B,T,3) float32, lengths, blank, threshold, min_frames or None)]."""
    rng = np.random.default_rng(1000 * T + seed)
    B, C, blank, thr = 6, 3, 1, 0.95
    lengths = lengths_for(B, T, rng)
    x = make_log_probs(B, T, C, blank, thr, seed + T)
    cases = [("ragged", x, lengths, blank, thr, None),
             ("blank0", make_log_probs(B, T, C, 0, 0.5, seed + T + 1), lengths, 0, 0.5, None),
             ("nothing_dropped", x, lengths, blank, 1.5, None)]
    ties = x.copy()                                            # few distinct values: the arg-min is tied
    ties[:, :, blank] = rng.integers(-3, 1, (B, T)).astype(np.float32)
    cases.append(("everything_dropped", ties, lengths, blank, 0.0, None))
    natural = plan(x[:, :, blank], lengths, thr)[0]
    L = np.clip(lengths, 0, T)
    mf = np.array([natural[0] - 1, 5, 7, natural[3], natural[4] + 2, L[5] + 5], np.int64)
    cases.append(("min_frames", x, lengths, blank, thr, mf))
    same = x.copy()                                            # identical blank_lp: the tie rule alone decides
    same[:, :, blank] = np.float32(-0.01)
    cases.append(("identical", same, lengths, blank, thr, np.array([T, 3, 1, T // 2 + 1, 2, T], np.int64)))
    odd = ties.copy()
    col = odd[:, :, blank]
    for value in (np.nan, -np.inf, np.inf, -0.0, 0.0):
        col[rng.uniform(size=(B, T)) < 0.12] = value
    cases.append(("nan_inf", odd, lengths, blank, 0.9, np.array([T, T, T, 2, T // 2, 1], np.int64)))
    cases.append(("nan_inf_all_dropped", odd, lengths, blank, 0.0, np.array([1, T, 2, 3, T // 2, T], np.int64)))
    return cases
