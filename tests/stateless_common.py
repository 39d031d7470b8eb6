"""The stateless prediction network's definition in float64 numpy, written straight from the formulas of
include/pika_stateless.h, with what the error bound of the tests needs: per output element the sum of the terms'
absolute values and the number of terms.

The bound: an fp32 sum of n products in any order, with or without fused multiply-add, differs from the exact value by
at most gamma(n + 1) * sum|terms|, gamma(m) = m u / (1 - m u), u = 2^-24.  Every comparison against float64 asserts
|got - ref| <= gamma(n + 2) * sum|terms|; the extra ulp covers the final rounding of the value itself."""
import argparse

import numpy as np

U32 = 2.0 ** -24


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U32 / (1.0 - m * U32)


def embed(y, E):
    """e[b,p,:] = E[y[b,p]] for y >= 0, else 0; float64."""
    y = np.asarray(y)
    e = np.zeros(y.shape + (E.shape[1],), np.float64)
    keep = y >= 0
    e[keep] = np.asarray(E, np.float64)[y[keep]]
    return e


def forward(y, E, w):
    """-> (z, abs_sum): z[b,u,d] = sum_j sum_c w[d,c,j] * e[b, u-(ctx-1)+j, g(d) cpg + c], and the sum of |terms|."""
    y = np.asarray(y)
    w = np.asarray(w, np.float64)
    D, cpg, ctx = w.shape
    B, U = y.shape
    e = embed(y, E)
    z = np.zeros((B, U, D))
    a = np.zeros((B, U, D))
    for d in range(D):
        g0 = (d // cpg) * cpg
        for j in range(ctx):
            for u in range(U):
                p = u - (ctx - 1) + j
                if p < 0:
                    continue
                for c in range(cpg):
                    term = w[d, c, j] * e[:, p, g0 + c]
                    z[:, u, d] += term
                    a[:, u, d] += np.abs(term)
    return z, a


def out_bound(a, w):
    D, cpg, ctx = np.asarray(w).shape
    return gamma(cpg * ctx + 2) * a


def backward(y, E, w, go):
    """go = dout * (z > 0), given.  -> (d_E, abs, count), (d_w, abs, count): the sums of the header, the sums of the terms'
    absolute values and the number of terms of every element."""
    y = np.asarray(y)
    E64, w = np.asarray(E, np.float64), np.asarray(w, np.float64)
    go = np.asarray(go, np.float64)
    D, cpg, ctx = w.shape
    B, U = y.shape
    V = E64.shape[0]
    e = embed(y, E)
    d_w, a_w = np.zeros_like(w), np.zeros_like(w)
    for d in range(D):
        g0 = (d // cpg) * cpg
        for c in range(cpg):
            for j in range(ctx):
                for u in range(U):
                    p = u - (ctx - 1) + j
                    if p < 0:
                        continue
                    term = go[:, u, d] * e[:, p, g0 + c]
                    d_w[d, c, j] += term.sum()
                    a_w[d, c, j] += np.abs(term).sum()
    n_w = np.full(w.shape, B * U)
    d_E, a_E, n_E = np.zeros((V, D)), np.zeros((V, D)), np.zeros((V, D))
    for b in range(B):
        for p in range(U):
            v = int(y[b, p])
            if v < 0:
                continue
            for j in range(ctx):
                u = p + (ctx - 1) - j
                if u >= U:
                    continue
                for g0 in range(0, D, cpg):
                    # w[d, i - g0, j] * go[b, u, d] for d, i in the group: (cpg d, cpg i)
                    terms = w[g0:g0 + cpg, :, j] * go[b, u, g0:g0 + cpg, None]
                    d_E[v, g0:g0 + cpg] += terms.sum(axis=0)
                    a_E[v, g0:g0 + cpg] += np.abs(terms).sum(axis=0)
                    n_E[v, g0:g0 + cpg] += cpg
    return (d_E, a_E, n_E), (d_w, a_w, n_w)


def within(got, ref, a, n):
    """|got - ref| <= gamma(n + 2) * sum|terms| everywhere -> (ok, the worst ratio of error to bound)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = gamma(np.asarray(n, np.float64) + 2) * a
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return bool((err <= bound).all()), float(ratio.max()) if ratio.size else 0.0


def labels(B, U, V, seed, blank=0):
    """Label rows that start with SOS: -1 padding at a tail, the token V - 1, blank in the middle, an all-equal row."""
    rng = np.random.RandomState(seed)
    y = rng.randint(0, V, size=(B, U)).astype(np.int64)
    y[:, 0] = blank
    if U >= 2:
        y[0, U - 1] = V - 1
    if U >= 3:
        y[0, U // 2] = blank
    if B >= 2:
        y[1, :] = min(1, V - 1)                # an all-equal row
    if B >= 3 and U >= 3:
        y[2, U - 2:] = -1                      # padding at the tail
    if B == 1 and U == 1:
        y[0, 0] = blank
    return y


def weights(V, D, cpg, ctx, seed):
    rng = np.random.RandomState(1000 + seed)
    E = rng.standard_normal((V, D)).astype(np.float32)
    w = (rng.standard_normal((D, cpg, ctx)) / np.sqrt(cpg * ctx)).astype(np.float32)
    return E, w


def context_of(hyp, ctx, blank=0):
    """The last ctx entries of [-1] * (ctx - 1) + [blank] + hyp."""
    return ([-1] * (ctx - 1) + [blank] + list(hyp))[-ctx:]


def tiny_opt(decoder_type="stateless", rnn_size=32, **more):
    opt = dict(rnn_size=rnn_size, local_rank=0, decoder_type=decoder_type, brnn=False, encoder_type='rnn', dropout=0.0,
               enc_layers=1, dec_layers=1, embd_dim=rnn_size, padding_idx=None)
    opt.update(more)
    return argparse.Namespace(**opt)
