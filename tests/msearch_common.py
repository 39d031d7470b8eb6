"""References of the one-symbol-per-frame ("modified") transducer beam search (include/pika_msearch.h); numpy and plain
Python, no product imports.

* `step` -- the step contract on one utterance with a Python tuple as the token sequence (a dict stands for the trie);
  dtype=np.float64 is the reference, dtype=np.float32 the same formulas in float32: the YARDSTICK.
* `search` -- `step` driven over a callable `logits_of(prefix, t)`.
* `k2_search` -- a k2 / icefall style `modified_beam_search` over the same callable, written independently of `step`.
* `TableModel` -- random table models for the callables; `planes_for` builds the modified loss's planes for one
  hypothesis from such a model."""
import numpy as np

NINF = -np.inf


def log_probs(logits, blank, sm_scale=1.0, penalty=0.0, dtype=np.float64):
    """(K,V) logits -> (K,V) lp = x - logsumexp x, x = sm_scale * logits - penalty [blank], evaluated in `dtype` as
    (x - max) - log(sum exp(x - max)); a row of -inf gives -inf."""
    with np.errstate(all="ignore"):
        x = dtype(sm_scale) * np.asarray(logits).astype(dtype)
        x[:, blank] = x[:, blank] - dtype(penalty)
        m = x.max(axis=1, keepdims=True)
        dead = ~(m > NINF)
        m = np.where(dead, dtype(0), m)
        d = x - m
        lp = d - np.log(np.exp(d).sum(axis=1, keepdims=True, dtype=dtype))
        return np.where(dead, dtype(NINF), lp).astype(dtype)


def merge_value(cs, dtype=np.float64):
    """m + log(sum exp(c_i - m)) over the members in rank order, m the first (largest)."""
    m, s = dtype(cs[0]), dtype(0)
    for c in cs:
        s = dtype(s + np.exp(dtype(dtype(c) - m)))
    return dtype(m + np.log(s))


def step(beam, logits, blank=0, sm_scale=1.0, penalty=0.0, dtype=np.float64):
    """beam: K entries (score, tokens tuple), score -inf for an empty slot; logits (K,V).
    -> (new beam (K entries), parent (K,), token (K,), info) with info = dict(cand (K,V), selected [(c, k, v)] in rank
    order, groups [[ranks]] in the new beam's order, merges: the number of candidates that joined another)."""
    K = len(beam)
    V = logits.shape[1]
    with np.errstate(all="ignore"):
        lp = log_probs(logits, blank, sm_scale, penalty, dtype)
        sc = np.array([s for s, _ in beam], dtype=dtype)
        cand = (sc[:, None] + lp).astype(dtype)
    cand[~(sc > NINF)] = NINF
    cand[np.isnan(cand)] = NINF
    order = np.argsort(-cand.ravel(), kind="stable")[:K]      # larger value, then lower k, then lower v
    selected = [(cand.ravel()[i], int(i) // V, int(i) % V) for i in order if cand.ravel()[i] > NINF]
    groups, by_key = [], {}
    for rank, (c, k, v) in enumerate(selected):
        key = beam[k][1] if v == blank else beam[k][1] + (v,)
        if key not in by_key:
            by_key[key] = len(groups)
            groups.append((key, [rank]))
        else:
            groups[by_key[key]][1].append(rank)
    merged = [(merge_value([selected[r][0] for r in ranks], dtype), ranks[0], key, ranks) for key, ranks in groups]
    merged.sort(key=lambda g: (-float(g[0]), g[1]))
    new = [(dtype(NINF), ())] * K
    parent, token = np.zeros(K, np.int64), np.full(K, blank, np.int64)
    for j, (s, rep, key, _) in enumerate(merged):
        new[j] = (s, key)
        parent[j], token[j] = selected[rep][1], selected[rep][2]
    info = dict(cand=cand, selected=selected, groups=[g[3] for g in merged],
                merges=len(selected) - len(merged))
    return new, parent, token, info


def start(K, dtype=np.float64):
    return [(dtype(0), ())] + [(dtype(NINF), ())] * (K - 1)


def rows_of(logits_of, beam, t, V):
    """The (K,V) float64 logits of a beam at frame t; zeros for the empty slots."""
    return np.stack([np.asarray(logits_of(tok, t), np.float64) if s > NINF else np.zeros(V) for s, tok in beam])


def search(logits_of, T, V, K, blank=0, sm_scale=1.0, penalty=0.0, dtype=np.float64):
    """`step` over T frames -> (final beam, per-frame infos)."""
    beam, infos = start(K, dtype), []
    for t in range(T):
        beam, _, _, info = step(beam, rows_of(logits_of, beam, t, V), blank, sm_scale, penalty, dtype)
        infos.append(info)
    return beam, infos


def k2_search(logits_of, T, V, K, blank=0, sm_scale=1.0, penalty=0.0):
    """icefall's modified_beam_search (max_sym_per_frame = 1) in float64: per frame, the top K of
    {hyp score + log_prob} over all (hyp, symbol), added to a new hypothesis list that log-adds equal token sequences.
    -> {tokens: score}"""
    B = {(): 0.0}
    for t in range(T):
        A, B = list(B.items()), {}
        flat = []
        for h, (tok, s) in enumerate(A):
            lp = log_probs(np.asarray(logits_of(tok, t), np.float64)[None], blank, sm_scale, penalty)[0]
            flat += [(s + lp[v], h, v) for v in range(V)]
        flat = [f for f in flat if f[0] > NINF]
        flat.sort(key=lambda f: -f[0])
        for val, h, v in flat[:K]:
            tok = A[h][0] if v == blank else A[h][0] + (v,)
            B[tok] = np.logaddexp(B[tok], val) if tok in B else val
    return B


class TableModel(object):
    """logits_of(prefix, t) = E[t] + P[last token, blank for the empty prefix] + R[len(prefix) % 5]: a function of
    the prefix and the frame alone, as a transducer's joint is."""

    def __init__(self, T, V, seed, blank=0, scale=2.0):
        rng = np.random.RandomState(seed)
        self.E, self.P, self.R = (scale * rng.randn(n, V) for n in (T, V, 5))
        self.blank, self.T, self.V = blank, T, V

    def __call__(self, prefix, t):
        return self.E[t] + self.P[prefix[-1] if prefix else self.blank] + self.R[len(prefix) % 5]


def planes_for(model, tokens, T, blank=0, sm_scale=1.0, penalty=0.0):
    """The (1,T,U+1) float64 planes of the modified loss for one hypothesis: row (t,u) is the model's log-probs after the
    prefix tokens[:u]."""
    U = len(tokens)
    pb, pl = np.full((1, T, U + 1), NINF), np.full((1, T, U + 1), NINF)
    for t in range(T):
        for u in range(U + 1):
            lp = log_probs(np.asarray(model(tuple(tokens[:u]), t))[None], blank, sm_scale, penalty)[0]
            pb[0, t, u] = lp[blank]
            if u < U:
                pl[0, t, u] = lp[tokens[u]]
    return pb, pl


def margins(infos, beam):
    """The smallest gap the float64 run leaves: between the last selected and the first unselected candidate of a
    frame, between selected candidates adjacent in rank, and between adjacent final scores."""
    gap = np.inf
    for info in infos:
        c = np.sort(info["cand"].ravel()[info["cand"].ravel() > NINF])[::-1]
        n = len(info["selected"])
        if len(c) > n:
            gap = min(gap, c[n - 1] - c[n])
        if n > 1:
            gap = min(gap, np.min(c[:n - 1] - c[1:n]))
    fin = np.array([s for s, _ in beam if s > NINF])
    if len(fin) > 1:
        gap = min(gap, np.min(fin[:-1] - fin[1:]))
    return float(gap)
