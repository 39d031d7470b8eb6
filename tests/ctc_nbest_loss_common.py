"""float64 reference of the n-best loss -- the full-sum scores of an n-best list and the gradient of
sum_k g[b,k] * full[b,k] with respect to the un-replicated input -- and of the MWER risk on top of it (torch on the CPU
+ numpy; no product imports).

Per utterance b and LIVE hypothesis k, `ctc_common.torch_reference` on the single utterance with grad_costs = -g[b,k]
(full = -cost), in float64: the reference; in float32: the yardstick of the tolerances, as in tests/test_ctc_gpu.py.
d/d logits and the true d/d log_probs are summed over k.  An entry is live when it exists, is no longer than max_len,
holds only classes in [0,C) other than blank and fits into T_b frames; every other entry is DEAD: -inf (NaN when longer
than max_len), no contribution, and its weight never enters the arithmetic (the tests put NaN, inf and 1e30 there).

Bounds (tests/test_ctc_gpu.py): scores relative min(max(4 * e32, 1e-6), 1e-3); gradients absolute
max(4 * max|yard32 - ref64|, 1e-6).  The from-logits form reads logit - lse rounded once behind an fp32 log-sum-exp, so
its SCORES get T_b * 2^-22 * (max|logit| + log C) on top, the allowance tests/test_ctc_nbest_gpu.py documents.

MWER: over the live entries P = softmax(full), risk_b = sum_k P_k * (errors_k - mean_live(errors)), written with torch
autograd in float64 over the reference scores; an utterance without a live entry has risk 0.
"""
import numpy as np
import torch

import ctc_common as R

GARBAGE = (-2 ** 31, 2 ** 31 - 1, -7, 2 ** 30)     # what stands beyond an entry's length (tests/test_ctc_nbest_gpu.py)


def repeats(seq):
    return sum(1 for a, b in zip(seq, seq[1:]) if a == b)


def sentinel(T, C, seq, blank, max_len):
    """None for a live entry, else the score a dead one must have."""
    if seq is None:
        return -np.inf
    if len(seq) > max_len:
        return np.nan
    if any(not 0 <= c < C or c == blank for c in seq) or T < len(seq) + repeats(seq):
        return -np.inf
    return None


def pack(hyps, L):
    """(tokens (B,N,L) int64 with garbage beyond every length, lengths (B,N) int64 with -1 for a missing entry)."""
    B, N = len(hyps), len(hyps[0])
    tokens = torch.tensor(GARBAGE, dtype=torch.int64).repeat(B, N, (L + 3) // 4)[:, :, :L].clone()
    lengths = torch.full((B, N), -1, dtype=torch.int64)
    for b, hs in enumerate(hyps):
        for k, h in enumerate(hs):
            if h is not None:
                lengths[b, k] = len(h)
                tokens[b, k, :min(len(h), L)] = torch.tensor(h[:L], dtype=torch.int64)
    return tokens, lengths


def nbest_loss(logits, hyps, ils, weights, blank=0, max_len=511, dtype=torch.float64):
    """logits (T,B,C) tensor, hyps[b][k] a label list or None, ils the T_b, weights (B,N) (read at live entries only) ->
    (full (B,N) float64 with the dead entries' sentinels, d/d logits (T,B,C), true d/d log_probs (T,B,C)) in `dtype`
    arithmetic, returned as float64."""
    T, B, C = logits.shape
    N = len(hyps[0])
    full = np.zeros((B, N))
    dx, dlp = torch.zeros(T, B, C, dtype=torch.float64), torch.zeros(T, B, C, dtype=torch.float64)
    for b in range(B):
        for k, seq in enumerate(hyps[b]):
            dead = sentinel(ils[b], C, seq, blank, max_len)
            if dead is not None:
                full[b, k] = dead
                continue
            gc = torch.tensor([-float(weights[b][k])], dtype=torch.float64)      # (a list would pass through float32)
            cost, gx, gl = R.torch_reference(logits[:, b:b + 1], [seq], [ils[b]], blank, gc, dtype)
            full[b, k] = -float(cost[0])
            dx[:, b] += gx[:, 0]
            dlp[:, b] += gl[:, 0]
    return full, dx, dlp


class Ref(object):
    """The float64 reference and the fp32 yardstick of one case, and the bounds that follow from them."""

    def __init__(self, logits, hyps, ils, weights, blank=0, max_len=511):
        self.r64 = nbest_loss(logits, hyps, ils, weights, blank, max_len, torch.float64)
        self.r32 = nbest_loss(logits, hyps, ils, weights, blank, max_len, torch.float32)
        self.full, self.dx, self.dlp = self.r64
        self.live = np.isfinite(self.full)
        f32 = self.r32[0]
        want = self.full[self.live]
        e32 = float((np.abs(f32[self.live] - want) / np.maximum(np.abs(want), 1e-30)).max()) if want.size else 0.0
        self.b_score = min(max(4 * e32, 1e-6), 1e-3)
        self.b_dx = max(4 * float((self.r32[1] - self.dx).abs().max()), 1e-6)
        self.b_dlp = max(4 * float((self.r32[2] - self.dlp).abs().max()), 1e-6)
        T, _, C = logits.shape
        self.extra = [t * 2.0 ** -22 * (float(logits.abs().max()) + float(np.log(C))) for t in ils]


def mwer(full, errors, reduction="mean"):
    """(value, d value / d full (B,N)) of the MWER risk over reference scores `full` (B,N) float64 numpy with the dead
    entries' sentinels; the gradient is zero at dead entries."""
    live = np.isfinite(full)
    f = torch.tensor(np.where(live, full, 0.0), dtype=torch.float64, requires_grad=True)
    e = torch.as_tensor(np.asarray(errors, dtype=np.float64))
    risks = []
    for b in range(full.shape[0]):
        idx = torch.from_numpy(np.flatnonzero(live[b]))
        if idx.numel() == 0:
            risks.append(f[b].sum() * 0.0)
            continue
        p = torch.softmax(f[b, idx], 0)
        risks.append((p * (e[b, idx] - e[b, idx].mean())).sum())
    risk = torch.stack(risks)
    value = {"none": risk, "sum": risk.sum(), "mean": risk.mean()}[reduction]
    value.sum().backward()
    return value.detach().numpy(), f.grad.numpy() * live
