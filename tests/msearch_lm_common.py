"""Reference of the one-symbol-per-frame beam search with LM / hotword fusion (include/pika_msearch_lm.h); numpy and
plain Python on `msearch_common` (the log-probs, the merge), `ctc_lm_common.RefLm` (the walk through an automaton) and
`ctc_bias_common.hot_lm` (a compiled phrase list as a `RefLm`).

A beam is K entries (F, am, bonus, tokens tuple, states tuple), F = am = -inf for an empty slot.  `step` is the contract
of the header on one utterance: the C best of F[k] + lp[k,v] (larger value, lower k, lower v), the walks, the merge of
the acoustic scores in rank order from the representative, the K best groups by G = am + bonus.  dtype=np.float64 is the
reference; dtype=np.float32 is the same with am, lp, the merge and F in float32 -- the YARDSTICK.  The bonus is float64
in both, as on the device, and an increment is rounded to fp32 once, as the device's walk returns it.
`lms` is a list of one or two `RefLm`, `weights` their weights (lm_weight[, bias_weight])."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msearch_common as M  # noqa: E402

NINF = -np.inf
EMPTY = (NINF, NINF, 0.0, (), None)


def f32(v):
    """A Python float that fp32 holds exactly: what the device gets is what the reference gets."""
    return float(np.float32(v))


def start(K, lms, dtype=np.float64):
    return [(dtype(0), dtype(0), 0.0, (), tuple(lm.start for lm in lms))] + [EMPTY] * (K - 1)


def fuse(am, bonus, dtype):
    """fp((double)am + bonus)"""
    return dtype(np.float64(am) + np.float64(bonus))


def walk(lms, weights, length_bonus, bonus, states, v):
    """One label from (bonus, states): (bonus', states') or None when an automaton does not reach it."""
    out, nxt = np.float64(bonus), []
    for lm, w, s in zip(lms, weights, states):
        st = lm.step(s, v, np.float64)
        if st is None:
            return None
        inc = np.float32(st[0])                 # rounded once, as lm_step returns it
        if not np.isfinite(inc):
            return None
        out = out + np.float64(w) * np.float64(inc)
        nxt.append(st[1])
    return out + np.float64(length_bonus), tuple(nxt)


def bonus_of(lms, weights, length_bonus, tokens):
    """(bonus, states) of a token sequence from the start states, by the device's formula; None: unreachable."""
    cur = (np.float64(0.0), tuple(lm.start for lm in lms))
    for v in tokens:
        cur = walk(lms, weights, length_bonus, cur[0], cur[1], v)
        if cur is None:
            return None
    return cur


def step(beam, logits, lms, weights, length_bonus, C, blank=0, sm_scale=1.0, penalty=0.0, dtype=np.float64):
    """-> (new beam (K entries), parent (K,), token (K,), info); info = dict(cand (K,V): F[k] + lp, lp (K,V), selected
    [(c, k, v)] in rank order, entries [(a', key, bonus', states') or None (dropped)] per selected, groups [(G, merged
    am, representative's rank, key, [ranks])] of ALL groups in the order of the cut, merges)."""
    K, V = len(beam), logits.shape[1]
    with np.errstate(all="ignore"):
        lp = M.log_probs(logits, blank, sm_scale, penalty, dtype)
        F = np.array([e[0] for e in beam], dtype=dtype)
        cand = (F[:, None] + lp).astype(dtype)
    cand[~(F > NINF)] = NINF
    cand[np.isnan(cand)] = NINF
    flat = cand.ravel()
    order = np.argsort(-flat, kind="stable")[:C]               # larger value, then lower k, then lower v
    selected = [(flat[i], int(i) // V, int(i) % V) for i in order if flat[i] > NINF]
    entries, groups, by_key = [], [], {}
    for rank, (_, k, v) in enumerate(selected):
        _, am, bonus, tok, states = beam[k]
        a = dtype(dtype(am) + lp[k, v])
        if v == blank:
            ent = (a, tok, np.float64(bonus), states)
        else:
            w = walk(lms, weights, length_bonus, bonus, states, v)
            ent = None if w is None else (a, tok + (v,), w[0], w[1])
        entries.append(ent)
        if ent is None:
            continue
        if ent[1] not in by_key:
            by_key[ent[1]] = len(groups)
            groups.append([ent[1], [rank]])
        else:
            groups[by_key[ent[1]]][1].append(rank)
    merged = []
    for key, ranks in groups:
        am = M.merge_value([entries[r][0] for r in ranks], dtype)
        merged.append((fuse(am, entries[ranks[0]][2], dtype), am, ranks[0], key, ranks))
    merged.sort(key=lambda g: (-float(g[0]), g[2]))
    merged = [g for g in merged if g[0] > NINF]
    new = [EMPTY] * K
    parent, token = np.zeros(K, np.int64), np.full(K, blank, np.int64)
    for j, (G, am, rep, key, _) in enumerate(merged[:K]):
        new[j] = (G, am, entries[rep][2], key, entries[rep][3])
        parent[j], token[j] = selected[rep][1], selected[rep][2]
    info = dict(cand=cand, lp=lp, selected=selected, entries=entries, groups=merged,
                merges=sum(e is not None for e in entries) - len(groups))
    return new, parent, token, info


def rows_of(logits_of, beam, t, V):
    """The (K,V) float64 logits of a beam at frame t; zeros for the empty slots."""
    return np.stack([np.asarray(logits_of(e[3], t), np.float64) if e[0] > NINF else np.zeros(V) for e in beam])


def search(logits_of, T, V, K, C, lms, weights, length_bonus=0.0, blank=0, sm_scale=1.0, penalty=0.0, dtype=np.float64):
    """`step` over T frames -> (final beam, per-frame infos)."""
    beam, infos = start(K, lms, dtype), []
    for t in range(T):
        beam, _, _, info = step(beam, rows_of(logits_of, beam, t, V), lms, weights, length_bonus, C, blank, sm_scale,
                                penalty, dtype)
        infos.append(info)
    return beam, infos


def results(beam, lms, weights, use_final=True, dtype=np.float64):
    """-> [(tokens, score, am)] of the live entries: with use_final fp(((double)am + bonus) + w * final + ...), the
    entries without a final state dropped, sorted again (ties: the rank before); otherwise F in the beam's order."""
    out = []
    for rank, (F, am, bonus, tok, states) in enumerate(beam):
        if not F > NINF:
            continue
        score = F
        if use_final:
            s = np.float64(am) + np.float64(bonus)
            for lm, w, st in zip(lms, weights, states):
                fin = lm.final(st, np.float64)
                if fin is None:
                    s = None
                    break
                s = s + np.float64(w) * np.float64(np.float32(fin))
            if s is None or not dtype(s) > NINF:
                continue
            score = dtype(s)
        out.append((-float(score), rank, tok, score, am))
    if use_final:
        out.sort(key=lambda x: (x[0], x[1]))
    return [(tok, score, am) for _, _, tok, score, am in out]


def margins(infos, final=None):
    """The smallest gap the float64 run leaves at a decision: at the pre-selection (between the last selected and the
    first unselected candidate, and between selected candidates adjacent in rank), at the cut to K (between groups
    adjacent in the order of the fused score, down to the first group cut off), and, with `final` (a `results` list),
    between adjacent final scores."""
    gap = np.inf
    for info in infos:
        c = np.sort(info["cand"].ravel()[info["cand"].ravel() > NINF])[::-1]
        n = len(info["selected"])
        if len(c) > n:
            gap = min(gap, c[n - 1] - c[n])
        if n > 1:
            gap = min(gap, np.min(c[:n - 1] - c[1:n]))
        K = info["cand"].shape[0]
        G = np.array([float(g[0]) for g in info["groups"][:K + 1]])
        if len(G) > 1:
            gap = min(gap, np.min(G[:-1] - G[1:]))
    if final is not None and len(final) > 1:
        s = np.array([float(f[1]) for f in final])
        gap = min(gap, np.min(s[:-1] - s[1:]))
    return float(gap)


def yardstick_error(infos64, infos32, beam64, beam32):
    """The float32 run's worst error against the float64 run, where both made the same decisions (inf otherwise): the
    candidates, and the F and am of the final beam."""
    if [e[3] for e in beam64] != [e[3] for e in beam32]:
        return np.inf
    err = max([max(abs(float(a[0]) - float(c[0])), abs(float(a[1]) - float(c[1])))
               for a, c in zip(beam64, beam32) if a[0] > NINF] + [0.0])
    for i, y in zip(infos64, infos32):
        fin = i["cand"] > NINF
        if fin.any():
            err = max(err, float(np.max(np.abs(y["cand"][fin].astype(np.float64) - i["cand"][fin]))))
        if [g[3] for g in i["groups"]] != [g[3] for g in y["groups"]]:
            return np.inf
        for g, h in zip(i["groups"], y["groups"]):
            err = max(err, abs(float(g[0]) - float(h[0])), abs(float(g[1]) - float(h[1])))
    return err
