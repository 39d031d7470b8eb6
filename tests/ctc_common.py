"""float64 references of the CTC loss, its gradients and its forced alignment (torch on the CPU + numpy; no product
imports).

Loss and gradients: `torch.nn.functional.ctc_loss` on the CPU in float64 behind a float64 `log_softmax`.  Costs and
d/d logits are compared directly.  torch's native CTC backward returns grad * (exp(lp) - occ) for frames t < T_n (zero
beyond), not the derivative -grad * occ with respect to log_probs, so the true d/d log_probs is
torch's - exp(lp) * grad_cost[n] on the frames t < T_n.

Alignment: a float64 Viterbi over the state lattice (blank, y1, blank, ..., yU, blank) with the tie rule of
include/pika_ctc.h -- at the end state S-1 is preferred over S-2; a cell's predecessor is the stay s, then s-1, then
s-2 (a later candidate wins only when strictly greater) -- and a brute-force enumerator over all C^T frame labellings.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F


def pad_targets(seqs, width=None, fill=0):
    """list of label lists -> (B, width) int64 padded with `fill`."""
    width = max([len(s) for s in seqs] + [0]) if width is None else width
    out = torch.full((len(seqs), width), fill, dtype=torch.int64)
    for n, s in enumerate(seqs):
        out[n, :len(s)] = torch.tensor(s, dtype=torch.int64)
    return out


def torch_reference(logits, seqs, input_lengths, blank=0, grad_costs=None, dtype=torch.float64):
    """(costs (B,), d/d logits (T,B,C), true d/d log_probs (T,B,C)) of sum_n grad_costs[n] * cost_n, computed by torch
    on the CPU in `dtype` (float64: the reference; float32: the yardstick of the tolerances), returned as float64.
    Frames t >= T_n are zeroed before torch sees them.  Only feasible utterances make sense here."""
    T, B, C = logits.shape
    il = torch.as_tensor(input_lengths, dtype=torch.int64)
    tl = torch.tensor([len(s) for s in seqs], dtype=torch.int64)
    x = logits.detach().to("cpu", dtype).clone()
    live = (torch.arange(T)[:, None] < il[None, :])          # (T, B)
    x[~live] = 0.0
    x.requires_grad_(True)
    lp = F.log_softmax(x, dim=-1)
    lp.retain_grad()
    costs = F.ctc_loss(lp, pad_targets(seqs), il, tl, blank=blank, reduction="none", zero_infinity=False)
    gc = torch.ones(B, dtype=dtype) if grad_costs is None else torch.as_tensor(grad_costs).to("cpu", dtype)
    (costs * gc).sum().backward()
    true_dlp = lp.grad - lp.detach().exp() * gc[None, :, None] * live[:, :, None].to(dtype)
    return costs.detach().double(), x.grad.double(), true_dlp.double()


def states(seq, blank):
    """The extended label sequence l' (S = 2U+1,) and its skip mask."""
    ext = np.full(2 * len(seq) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(seq, dtype=np.int64)
    skip = np.zeros(len(ext), dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    return ext, skip


def _up(v, k):
    """v shifted up the state axis by k: out[s] = v[s-k], -inf below."""
    out = np.full(len(v), -np.inf)
    out[k:] = v[:len(v) - k]
    return out


def _down(v, k):
    """out[s] = v[s+k], -inf above."""
    out = np.full(len(v), -np.inf)
    out[:max(len(v) - k, 0)] = v[k:]
    return out


def dp_cost(lp, seq, blank=0):
    """-log P(seq | lp) by the plain alpha recurrence in float64.  lp: (T, C) log-probs of one utterance."""
    lp = np.asarray(lp, dtype=np.float64)
    ext, skip = states(seq, blank)
    a = np.full(len(ext), -np.inf)
    a[0] = lp[0, ext[0]]
    if len(ext) > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, lp.shape[0]):
        p1 = _up(a, 1)
        p2 = np.where(skip, _up(a, 2), -np.inf)
        with np.errstate(invalid="ignore"):
            a = lp[t, ext] + np.logaddexp(np.logaddexp(a, p1), p2)
    return -float(np.logaddexp(a[-1], a[-2]) if len(ext) > 1 else a[-1])


def forward_sweep(lp, seq, blank=0):
    """delta (T, S) and back-pointers (T, S) in {0, 1, 2}: how many states the best predecessor lies below."""
    lp = np.asarray(lp, dtype=np.float64)
    ext, skip = states(seq, blank)
    T, S = lp.shape[0], len(ext)
    e = lp[:, ext]
    delta = np.full((T, S), -np.inf)
    bp = np.zeros((T, S), dtype=np.int64)
    delta[0, 0] = e[0, 0]
    if S > 1:
        delta[0, 1] = e[0, 1]
    for t in range(1, T):
        p0 = delta[t - 1]
        p1 = _up(p0, 1)
        p2 = np.where(skip, _up(p0, 2), -np.inf)
        best, k = p0.copy(), np.zeros(S, dtype=np.int64)
        m = p1 > best
        best[m], k[m] = p1[m], 1
        m = p2 > best
        best[m], k[m] = p2[m], 2
        delta[t], bp[t] = e[t] + best, k
    return delta, bp


def backward_sweep(lp, seq, blank=0):
    """gamma (T, S): the best score from state s at frame t to the end, the frame's own emission included."""
    lp = np.asarray(lp, dtype=np.float64)
    ext, skip = states(seq, blank)
    T, S = lp.shape[0], len(ext)
    e = lp[:, ext]
    gamma = np.full((T, S), -np.inf)
    gamma[T - 1, S - 1] = e[T - 1, S - 1]
    if S > 1:
        gamma[T - 1, S - 2] = e[T - 1, S - 2]
    for t in range(T - 2, -1, -1):
        g = gamma[t + 1]
        n1 = _down(g, 1)
        n2 = _down(np.where(skip, g, -np.inf), 2)
        gamma[t] = e[t] + np.maximum(np.maximum(g, n1), n2)
    return gamma


def backtrace(delta, bp):
    """State path (T,) from the end (S-1 preferred over S-2 on a tie)."""
    T, S = delta.shape
    s = S - 2 if S > 1 and delta[T - 1, S - 2] > delta[T - 1, S - 1] else S - 1
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= bp[t, s]
    return path


def viterbi(lp, seq, blank=0):
    """(score, frame labels (T,), state path (T,), delta)."""
    delta, bp = forward_sweep(lp, seq, blank)
    path = backtrace(delta, bp)
    ext, _ = states(seq, blank)
    return float(delta[-1, path[-1]]), ext[path], path, delta


def rescore(lp, frame_labels):
    """Sum of lp[t, frame_labels[t]] in float64."""
    lp = np.asarray(lp, dtype=np.float64)
    fl = np.asarray(frame_labels, dtype=np.int64)
    return float(lp[np.arange(len(fl)), fl].sum())


def collapse(frame_labels, blank=0):
    """Merge repeats, drop blanks."""
    out, prev = [], None
    for c in [int(v) for v in frame_labels]:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def margin(lp, seq, blank=0):
    """Best score minus the best score of any path through a (t, s) cell off the optimal state path."""
    delta, bp = forward_sweep(lp, seq, blank)
    gamma = backward_sweep(lp, seq, blank)
    path = backtrace(delta, bp)
    e = np.asarray(lp, dtype=np.float64)[:, states(seq, blank)[0]]
    through = delta + gamma - e                       # the emission is in both
    off = np.ones(delta.shape, dtype=bool)
    off[np.arange(len(path)), path] = False
    through = through[off]
    through = through[np.isfinite(through)]
    if through.size == 0:
        return np.inf
    return float(delta[-1, path[-1]] - through.max())


def bound(delta, T):
    """T * 2^-23 * max|delta|: a path's fp32 score is T rounded additions on values no larger than the fp64 lattice's
    own (max picks an operand and does not round)."""
    return int(T) * 2.0 ** -23 * float(np.abs(delta[np.isfinite(delta)]).max())


def brute_force(lp, seq, blank=0):
    """(cost, best score, best frame labels) by enumerating all C^T frame labellings that collapse to seq.  Among
    equally good paths the first in the order of the tie rule's preference is not defined here: use it on inputs with
    a unique optimum.  (inf, -inf, None) when no labelling collapses to seq."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    total, best, arg = -np.inf, -np.inf, None
    for fl in itertools.product(range(C), repeat=T):
        if collapse(fl, blank) != list(seq):
            continue
        s = rescore(lp, fl)
        total = np.logaddexp(total, s)
        if s > best:
            best, arg = s, np.asarray(fl, dtype=np.int64)
    return -float(total), float(best), arg
