"""One step of the RNN-T beam search (include/pika_decode.h, include/pika_decode_step.h) as a plain float64 reference, the
table of cases the two advance kernels are tested on, and the builders of their inputs.  Nothing here needs a GPU:
tests/test_beam_step_refs.py checks the reference and the table on their own, tests/test_beam_step_gpu.py runs
`pika_beam_advance` and `pika_beam_advance_logits` against them.

The reference (`advance_ref`) is written from the contract text of include/pika_decode.h and the reference lines it cites
(decoder/beam_transducer.py:82-187, transducer_decoder.py:188-202), with loops per utterance and per slot.
"""
import functools

import numpy as np

EOS = -1
DEAD32 = np.float32(-1e20)
COLS = 192                      # columns per range of the thresholded entry point (PIKA_DFC2_COLS)
GUARD = 64                      # sentinel elements on either side of every buffer
SM_SCALE, LM_SCALE = 0.8, 0.3
STEP_T = 3                      # steps taken before the call (0 in the `first` cases)
HIST = 8                        # rows of ks_hist (ys_hist: one more)
N_BEST = 2
MARGIN = 1e-3                   # at |score| <= 64; grows with the score beyond that

MUTANTS = ("tie_order_reversed", "finish_reads_slot_frame", "n_ys_one_less", "n_ys_one_more", "lm_not_subtracted",
           "lm_from_slot", "dup_ignores_live", "dup_applies_to_empty", "dup_stops_at_64", "fin_without_clamp",
           "fin_n_clamped", "fin_inherits_parent", "eos_top_any_slot", "first_adds_scores", "max_hyp_lowered")

INT_FIELDS = ("y", "t_idx", "hyp_len", "ks_hist", "ys_hist", "eos_top", "fin_n", "prev_k", "y_raw")
LOGITS_FIELDS = ("step_t", "max_hyp", "stop")


# ---- the reference -------------------------------------------------------------------------------------------------
def disabled_rows(y, hyp, hyp_len, beam_prune, mutant=None):
    """Rows that may not have children (:100-114): eos rows, and -- with beam_prune -- a live row whose NON-EMPTY partial
    hypothesis equals that of an earlier live row that is not disabled itself."""
    K = len(y)
    dead = np.zeros(K, bool)
    seen = set()
    for i in range(K):
        n = int(hyp_len[i])
        key = (n,) + tuple(int(v) for v in hyp[i, :min(n, 64) if mutant == "dup_stops_at_64" else n])
        if y[i] == EOS:
            dead[i] = True
            if mutant == "dup_ignores_live" and n > 0:
                seen.add(key)
        elif beam_prune and (n > 0 or mutant == "dup_applies_to_empty"):
            if key in seen:
                dead[i] = True
            else:
                seen.add(key)
    return dead


def candidate_values(x_b, scores, lm_scores, lm_scale, dead, first, mutant=None):
    """(K, V) float64 candidate values of one utterance; rows that do not compete are NaN."""
    x = x_b.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    logp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    K = x.shape[0]
    vals = np.full(x.shape, np.nan)
    for k in range(K):
        if first:
            if k == 0:
                vals[0] = logp[0] + (float(scores[0]) if mutant == "first_adds_scores" else 0.0)
        elif dead[k]:
            vals[k] = float(DEAD32)
        else:
            vals[k] = (logp[k] + float(scores[k])) + lm_scale * float(lm_scores[k])
    return vals


def best_candidates(vals, n, reverse_ties=False):
    """Flat indices of the n best competing candidates: value descending, then flat index k*V + v ascending."""
    flat = vals.reshape(-1)
    comp = np.flatnonzero(~np.isnan(flat))
    n = min(n, len(comp))
    v = flat[comp]
    thr = np.partition(v, len(v) - n)[len(v) - n]
    keep = comp[v >= thr]                              # ascending flat index
    if reverse_ties:
        keep = keep[::-1]
    order = np.argsort(-flat[keep], kind="stable")
    return keep[order][:n]


def advance_ref(state, logits, sm_scale, lm_scale, first, beam_prune, blk, mutant=None):
    """state -> state' of ONE search step in numpy float64.  `state`: name -> array of every state buffer of the ABI
    (scores, lm_scores f32 (B,K); y, t_idx, hyp_len (B,K), hyp (B,K,L), num_frames, max_len, fin_n (B,), ks_hist (S,B,K),
    ys_hist (S+1,B,K), step_t (1,) i64; eos_top (B,) u8; fin_score f32, fin_step, fin_k i64 (B,fin_cap)); logits (B,K,V) f32.

    Fixed points:
      * the inputs are the fp32 arrays the kernel gets; x = sm_scale * logits is the fp32 product (the kernel's input by
        contract); everything after it is float64: log-softmax, (logp + scores) + lm_scale * lm_scores, the subtraction
        of lm_scale * lm_scores[parent] (lm_scale itself is the fp32 argument);
      * a disabled row is float32(-1e20) on every column; on the first step only row 0 competes and nothing is added;
      * selection: the K best of the K*V candidates by value descending, then flat index k*V + v ascending;
        parent = idx // V, sym = idx % V;
      * fin = (sym == blk and t_idx[parent] == num_frames - 1) or (step_t + 2 > max_len);
      * a slot that does not finish takes its parent's labels (+ sym if it is not blank), hyp_len = parent's + (sym != blk);
        a finishing slot keeps its own hyp and hyp_len; t_idx' = t_idx[parent];
      * ks_hist[step_t] = parent, ys_hist[step_t + 1] = y', y_raw = sym, prev_k = parent, y' = -1 on finish;
      * the finished list is appended in slot order at min(fin_n + rank, fin_cap - 2) with fin_step = step_t + 1; fin_n
        counts on past the clamp; eos_top |= (y'[0] == -1).
    Returns the new state (scores, fin_score float64) with `new_len` (B,K) added: what a slot contributes to max_hyp.
    step_t is NOT incremented here (pika_beam_advance leaves that to its caller; `advance_logits_ref` adds it)."""
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    B, K = s["y"].shape
    V = logits.shape[-1]
    fin_cap = s["fin_score"].shape[1]
    x = (np.float32(sm_scale) * logits.astype(np.float32)).astype(np.float32).reshape(B, K, V)
    lms = float(np.float32(lm_scale))
    step = int(s["step_t"][0])
    out = {k: v.copy() for k, v in s.items()}
    out["scores"] = s["scores"].astype(np.float64)
    out["fin_score"] = s["fin_score"].astype(np.float64)
    out["prev_k"] = np.zeros((B, K), np.int64)
    out["y_raw"] = np.zeros((B, K), np.int64)
    out["new_len"] = np.zeros((B, K), np.int64)
    for b in range(B):
        dead = disabled_rows(s["y"][b], s["hyp"][b], s["hyp_len"][b], beam_prune, mutant)
        vals = candidate_values(x[b], s["scores"][b], s["lm_scores"][b], lms, dead, first, mutant)
        idx = best_candidates(vals, K, mutant == "tie_order_reversed")
        n_ys = step + 2 - (mutant == "n_ys_one_less") + (mutant == "n_ys_one_more")
        rank = 0
        for i in range(K):
            parent, sym = int(idx[i]) // V, int(idx[i]) % V
            lm_of = i if mutant == "lm_from_slot" else parent
            score = vals.reshape(-1)[idx[i]] - (0.0 if mutant == "lm_not_subtracted" else lms * float(s["lm_scores"][b, lm_of]))
            t_of = i if mutant == "finish_reads_slot_frame" else parent
            fin = (sym == blk and s["t_idx"][b, t_of] == s["num_frames"][b] - 1) or n_ys > s["max_len"][b]
            out["scores"][b, i] = score
            out["prev_k"][b, i] = parent
            out["y_raw"][b, i] = sym
            out["t_idx"][b, i] = s["t_idx"][b, parent]
            out["ks_hist"][step, b, i] = parent
            y_new = EOS if fin else sym
            out["y"][b, i] = y_new
            out["ys_hist"][step + 1, b, i] = y_new
            if fin and mutant != "fin_inherits_parent":
                out["new_len"][b, i] = s["hyp_len"][b, i]
            else:
                n = int(s["hyp_len"][b, parent])
                out["hyp"][b, i, :n] = s["hyp"][b, parent, :n]
                if sym != blk and not fin:
                    out["hyp"][b, i, n] = sym
                    n += 1
                out["hyp_len"][b, i] = out["new_len"][b, i] = n
            if fin:
                pos = int(s["fin_n"][b]) + rank
                if mutant != "fin_without_clamp":
                    pos = min(pos, fin_cap - 2)
                if pos < fin_cap:
                    out["fin_score"][b, pos] = score
                    out["fin_step"][b, pos] = step + 1
                    out["fin_k"][b, pos] = i
                rank += 1
            if y_new == EOS and (i == 0 or mutant == "eos_top_any_slot"):
                out["eos_top"][b] = 1
        out["fin_n"][b] = s["fin_n"][b] + rank
        if mutant == "fin_n_clamped":
            out["fin_n"][b] = min(out["fin_n"][b], fin_cap - 2)
    return out


def advance_logits_ref(state, logits, sm_scale, lm_scale, beam_prune, blk, n_best, mutant=None):
    """The thresholded entry point: `advance_ref` with first = (step_t == 0), plus step_t' = step_t + 1,
    max_hyp' = max(max_hyp, max over slots of new_len), stop' = all_b(eos_top' and fin_n' >= n_best), and the `sync`
    protocol (int32[8]): a call that finds *stop set writes sync[4] = 1 and nothing else; otherwise the counters of the
    other parity ([2q], [2q+1], [5+q], q = (step_t + 1) & 1) read zero afterwards, [5 + (step_t & 1)] too once stop is set."""
    if int(state["stop"][0]):
        out = {k: np.array(v, copy=True) for k, v in state.items()}
        out["sync"][4] = 1
        return out
    step = int(state["step_t"][0])
    out = advance_ref(state, logits, sm_scale, lm_scale, step == 0, beam_prune, blk, mutant)
    out["step_t"][0] = step + 1
    mh = int(out["new_len"].max())
    out["max_hyp"][0] = mh if mutant == "max_hyp_lowered" else max(int(state["max_hyp"][0]), mh)
    stop = int(all(out["eos_top"][b] and out["fin_n"][b] >= n_best for b in range(len(out["fin_n"]))))
    out["stop"][0] = stop
    par = step & 1
    q = par ^ 1
    out["sync"][2 * par] = out["sync"][2 * par + 1] = -1          # this parity's arrival scratch: not compared
    out["sync"][2 * q] = out["sync"][2 * q + 1] = out["sync"][5 + q] = 0
    if stop:
        out["sync"][5 + par] = 0
    return out


def compare(got, want, state0, score_ok, logits_entry=False, y_raw=True):
    """Names of the compared fields in which `got` differs from `want` (the reference's result for `state0`).
    hyp only on [0, hyp_len') of each slot; the finished arrays on [0, min(fin_n', fin_cap - 1)): the untouched entries and
    the ones the step appended; integers for equality; scores / fin_score through score_ok(got, want) -> bool array."""
    bad = []
    for k in INT_FIELDS + (LOGITS_FIELDS if logits_entry else ()):
        if k == "y_raw" and not y_raw:
            continue
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)):
            bad.append(k)
    B, K = want["y"].shape
    fin_cap = want["fin_score"].shape[1]
    for b in range(B):
        for i in range(K):
            n = int(want["hyp_len"][b, i])
            if not np.array_equal(got["hyp"][b, i, :n], want["hyp"][b, i, :n]) and "hyp" not in bad:
                bad.append("hyp")
        n = min(int(want["fin_n"][b]), fin_cap - 1)
        for k in ("fin_step", "fin_k"):
            if not np.array_equal(got[k][b, :n], want[k][b, :n]) and k not in bad:
                bad.append(k)
        if not score_ok(np.asarray(got["fin_score"][b, :n]), want["fin_score"][b, :n]).all() and "fin_score" not in bad:
            bad.append("fin_score")
    if not score_ok(np.asarray(got["scores"]), want["scores"]).all():
        bad.append("scores")
    if logits_entry:
        cmp_sync = [j for j in range(8) if want["sync"][j] != -1]
        if not np.array_equal(np.asarray(got["sync"])[cmp_sync], want["sync"][cmp_sync]):
            bad.append("sync")
    return bad


def close64(got, want):
    """Two float64 evaluations of the same step (reference against reference, mutants, BeamState._advance)."""
    return np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want)) + 1e-7 * (np.abs(want) > 1e19) * np.abs(want)


# ---- decisive inputs -----------------------------------------------------------------------------------------------
def top_is_decisive(x_b, st, first, beam_prune):
    """(decisive, has_tie) for one utterance: any two of the top K + 1 candidates (the reference's order) are either equal
    by construction -- the same fp32 x in the same row, or in two rows with identical x, scores and lm_scores; dead
    candidates among themselves -- or differ by more than MARGIN * max(1, |score| / 64)."""
    K, V = x_b.shape
    dead = disabled_rows(st["y"], st["hyp"], st["hyp_len"], beam_prune)
    vals = candidate_values(x_b, st["scores"], st["lm_scores"], float(np.float32(LM_SCALE)), dead, first)
    idx = best_candidates(vals, K + 1)
    row_class = {}
    cls = []
    for k in range(K):
        key = ("dead",) if (dead[k] and not first) else (x_b[k].tobytes(), float(st["scores"][k]), float(st["lm_scores"][k]))
        cls.append(row_class.setdefault(key, k))
    keys = [(cls[i // V], None if (dead[i // V] and not first) else x_b[i // V, i % V].tobytes()) for i in idx]
    v = vals.reshape(-1)[idx]
    ok, tie = True, False
    for j in range(len(idx) - 1):
        if keys[j] == keys[j + 1]:
            assert v[j] == v[j + 1]
            tie = True
        elif not v[j] - v[j + 1] > MARGIN * max(1.0, abs(v[j]) / 64.0):
            ok = False
    return ok, tie


# ---- per-utterance states ------------------------------------------------------------------------------------------
NF = 6


def _generic(rng, K, V, L, blk):
    lab_lo = 1 if V > 1 else 0
    st = dict(scores=(rng.standard_normal(K) * 2 - 5).astype(np.float32),
              lm_scores=rng.standard_normal(K).astype(np.float32),
              y=rng.integers(0, V, K).astype(np.int64), t_idx=rng.integers(0, NF, K).astype(np.int64), num_frames=NF,
              max_len=1000, hyp=rng.integers(lab_lo, V, (K, L)).astype(np.int64),
              hyp_len=rng.integers(1, min(L - 2, 6) + 1, K).astype(np.int64), eos_top=0, fin_n=2)
    x = (rng.standard_normal((K, V)) * 2.5).astype(np.float32)
    x[:, blk] += 2.0
    return st, x


def _boost(st, rows, by=6.0):
    top = float(st["scores"].max())
    for j, r in enumerate(rows):
        st["scores"][r] = np.float32(top + by + 0.37 * j)


def _copy_hyp(st, src, dst):
    st["hyp"][dst] = st["hyp"][src]
    st["hyp_len"][dst] = st["hyp_len"][src]


def _three(K):
    """Three slots k1 < k2 < k3 spread over the beam (K >= 3)."""
    return 0 if K < 5 else 1, K // 2, K - 1


def build_utterance(cls, rng, K, V, L, blk, step):
    """One utterance of state class `cls` (see STATE_CLASSES): (state dict, raw logits (K,V) f32)."""
    st, x = _generic(rng, K, V, L, blk)
    if cls in ("generic", "first_nonzero"):
        pass
    elif cls == "eos_top_set":
        st["eos_top"] = 1
    elif cls == "all_eos":
        st["y"][:] = EOS
    elif cls == "single_live":
        st["y"][:] = EOS
        st["y"][K // 2] = min(1, V - 1)
    elif cls == "dup_live":
        k1, k2 = 0, K - 1
        st["y"][[k1, k2]] = min(1, V - 1)
        _copy_hyp(st, k1, k2)
        _boost(st, [k2])
    elif cls == "dup_eos":                        # k1 eos; k2 its twin, live: stays; k3 a twin of both: disabled by k2
        k1, k2, k3 = _three(K)
        st["y"][k1] = EOS
        st["y"][[k2, k3]] = min(1, V - 1)
        _copy_hyp(st, k1, k2)
        _copy_hyp(st, k1, k3)
        _boost(st, [k2, k3])
    elif cls in ("diff_first", "diff_last"):
        k1, k2 = 0, K - 1
        st["y"][[k1, k2]] = min(1, V - 1)
        st["hyp_len"][k1] = 4
        _copy_hyp(st, k1, k2)
        p = 0 if cls == "diff_first" else 3
        st["hyp"][k2, p] = (st["hyp"][k1, p] % (V - 1)) + 1
        _boost(st, [k2])
    elif cls == "long70":                         # k2 differs from k1 at position 65 only; k3 equals k1
        k1, k2, k3 = _three(K)
        st["y"][[k1, k2, k3]] = min(1, V - 1)
        st["hyp_len"][k1] = 70
        _copy_hyp(st, k1, k2)
        _copy_hyp(st, k1, k3)
        st["hyp"][k2, 65] = (st["hyp"][k1, 65] % (V - 1)) + 1
        _boost(st, [k2, k3])
    elif cls == "three_way":
        k1, k2, k3 = _three(K)
        st["y"][[k1, k2, k3]] = min(1, V - 1)
        _copy_hyp(st, k1, k2)
        _copy_hyp(st, k1, k3)
        _boost(st, [k2, k3])
    elif cls == "dup_empty":
        k1, k2, k3 = _three(K)
        st["y"][[k1, k2, k3]] = blk
        st["hyp_len"][[k1, k2, k3]] = 0
        _boost(st, [k2, k3])
    elif cls in ("blank_parent_last", "blank_parent_conv"):
        p = K - 1                                  # the best row; its blank wins slot 0
        st["y"][p] = min(1, V - 1)
        st["hyp_len"][p] = 1 + st["hyp_len"][:p].max()        # (no accidental twin)
        _boost(st, [p])
        x[p, blk] = x[p].max() + 9.0
        st["t_idx"][:] = rng.integers(0, NF - 2, K)
        st["t_idx"][p if cls == "blank_parent_last" else 0] = NF - 1
    elif cls == "only_nonzero_finish":
        p, q = K - 1, 0
        st["y"][[p, q]] = min(1, V - 1)
        st["hyp_len"][p] = 1 + st["hyp_len"][:p].max()
        _boost(st, [q, p], by=4.0)
        _boost(st, [p], by=4.0)
        lab = (blk + 1) % V
        x[p, lab] = x[p].max() + 12.0
        x[q, blk] = x[q].max() + 12.0
        st["t_idx"][:] = rng.integers(0, NF - 2, K)
        st["t_idx"][q] = NF - 1
    elif cls == "maxlen":
        st["max_len"] = step + 1
    elif cls == "maxlen_next":
        st["max_len"] = step + 2
    elif cls == "fin_clamp":
        st["max_len"] = step + 1
        st["fin_n"] = "cap-4"
    elif cls == "tie_kth":                         # K - 2 distinct values, then four equal ones across the K-th place
        r = K // 2
        st["y"][r] = min(1, V - 1)
        st["hyp_len"][r] = 1 + np.delete(st["hyp_len"], r).max()
        _boost(st, [r], by=12.0)
        cols = rng.choice(V, K + 2, replace=False)
        x[r] = (-6.0 - np.abs(rng.standard_normal(V))).astype(np.float32)
        x[r, cols[:K - 2]] = (3.0 + 0.5 * np.arange(K - 2)).astype(np.float32)
        x[r, cols[K - 2:]] = 1.0
    elif cls == "all_equal":
        r = K // 2
        st["y"][r] = min(1, V - 1)
        st["hyp_len"][r] = 1 + np.delete(st["hyp_len"], r).max()
        _boost(st, [r], by=12.0)
        x[r] = 0.7
    elif cls == "pool_tie":                        # 300 equal values at the bound, K - 3 values above it
        r = K // 2
        st["y"][r] = min(1, V - 1)
        st["hyp_len"][r] = 1 + np.delete(st["hyp_len"], r).max()
        _boost(st, [r], by=14.0)
        n_above = max(K - 3, 0)
        cols = rng.choice(V, 300 + n_above, replace=False)
        x[r] = (-6.0 - np.abs(rng.standard_normal(V))).astype(np.float32)
        x[r, cols[:n_above]] = (3.0 + 0.5 * np.arange(n_above)).astype(np.float32)
        x[r, cols[n_above:]] = 1.0
    elif cls == "cross_row_tie":                   # two identical rows with different hypotheses
        k1, k2 = (0, K - 1) if K < 5 else (1, K - 2)
        st["y"][[k1, k2]] = min(1, V - 1)
        st["hyp_len"][k1], st["hyp_len"][k2] = 2, 3
        x[k2] = x[k1]
        _boost(st, [k1])
        st["scores"][k2] = st["scores"][k1]
        st["lm_scores"][k2] = st["lm_scores"][k1]
    else:
        raise KeyError(cls)
    return st, x


# What each state class is for (the table names them per utterance)
STATE_CLASSES = {
    "generic": "a live beam with lm_scores != 0 (lm_scale = 0.3 everywhere)",
    "first_nonzero": "step_t = 0 over non-zero scores, y, hyp_len and lm_scores",
    "all_eos": "every slot eos: every candidate dead, selection = row 0, columns 0..K-1",
    "single_live": "one live slot",
    "dup_live": "a duplicate of an earlier live slot: disabled",
    "dup_eos": "a duplicate of an earlier eos slot: NOT disabled (and a third twin, disabled by the second)",
    "diff_first": "equal-length hypotheses that differ in the first label only",
    "diff_last": "equal-length hypotheses that differ in the last label only",
    "long70": "hypotheses of 70 labels that differ at position 65 only, and a true twin of 70 labels",
    "three_way": "three slots with one hypothesis",
    "dup_empty": "several empty hypotheses: not disabled",
    "blank_parent_last": "blank wins slot 0 from a parent at num_frames - 1 while slot 0's own t_idx is not: slot 0 finishes",
    "blank_parent_conv": "the converse: slot 0's own t_idx is num_frames - 1, the parent's is not: no finish",
    "only_nonzero_finish": "slot 0 takes a label, a later slot finishes",
    "maxlen": "step_t + 2 > max_len: every slot finishes",
    "maxlen_next": "step_t + 2 == max_len: nobody finishes by length",
    "eos_top_set": "eos_top already set",
    "fin_clamp": "fin_n = fin_cap - 4 and K >= 4 slots finish: the clamp at fin_cap - 2, fin_n grows by K",
    "tie_kth": "a row with four equal values across the K-th place",
    "all_equal": "a row of equal logits",
    "pool_tie": "300 equal values at the bound with fewer than K above (POOL_CAP tie path of row_survivors)",
    "cross_row_tie": "two identical live rows with identical scores and different hypotheses",
}


# ---- the case table ------------------------------------------------------------------------------------------------
def _case(name, K, V, L, utts, **kw):
    c = dict(name=name, K=K, V=V, L=L, utts=tuple(utts), B=len(utts), first=False, beam_prune=1, blk=0, tags=(),
             entries=("advance", "logits"), seed=1)
    c.update(kw)
    return c


# tags: "ties" (an exact tie among some utterance's top K + 1: torch.topk may order it otherwise), "misaligned" (logits
# start 4 bytes off 16-byte alignment), "ldl_pad" (ldl > splits * 192), "no_y_raw" (y_raw = NULL), "max_hyp" (*max_hyp
# starts above every length).  Waves of the thresholded kernel at K = 64: L = 100 -> 16, L = 160 -> 8, L = 200 -> 4.
CASES = [
    _case("k1_v64", 1, 64, 8, ["generic", "all_eos", "maxlen"], tags=("ties",)),
    _case("k2_v65", 2, 65, 8, ["dup_live", "blank_parent_last", "blank_parent_conv"]),
    _case("k2_v65_stop", 2, 65, 8, ["blank_parent_last"]),
    _case("k3_v191", 3, 191, 9, ["dup_eos", "diff_first", "diff_last", "three_way", "dup_empty"]),
    _case("k3_v191_noprune", 3, 191, 9, ["dup_eos", "diff_first", "diff_last", "three_way", "dup_empty"], beam_prune=0),
    _case("k5_vk", 5, 5, 10, ["generic", "single_live", "all_eos"], tags=("ties",)),
    _case("k5_vk_first", 5, 5, 10, ["first_nonzero"], first=True),
    _case("k5_v192_first", 5, 192, 10, ["first_nonzero", "all_eos", "eos_top_set"], first=True, tags=("ldl_pad",)),
    _case("k5_v65_alldone", 5, 65, 10, ["maxlen", "maxlen", "fin_clamp"], tags=("max_hyp",)),
    _case("k5_v1000_ties", 5, 1000, 10, ["pool_tie", "cross_row_tie", "tie_kth"], tags=("ties",)),
    _case("k16_v1000", 16, 1000, 12, ["generic", "only_nonzero_finish", "fin_clamp"], tags=("max_hyp",)),
    _case("k16_v1000_ties", 16, 1000, 12, ["pool_tie", "tie_kth", "all_equal"], tags=("ties", "no_y_raw")),
    _case("k16_v6268_misaligned", 16, 6268, 12, ["generic"], tags=("misaligned",)),
    _case("k16_v12288", 16, 12288, 12, ["generic"], entries=("logits",)),
    _case("k17_v193", 17, 193, 80, ["maxlen", "maxlen_next", "long70"], blk=2),
    _case("k17_v193_noprune", 17, 193, 80, ["long70", "three_way", "dup_live"], beam_prune=0),
    _case("k33_v333", 33, 333, 12, ["generic", "eos_top_set", "single_live", "blank_parent_last", "dup_live"],
          blk=5, tags=("no_y_raw",)),
    _case("k64_v8192", 64, 8192, 100, ["generic", "three_way", "all_eos"], tags=("ties",)),
    _case("k64_vk", 64, 64, 160, ["generic", "dup_eos", "fin_clamp"]),
    _case("k64_v193", 64, 193, 200, ["generic", "maxlen", "only_nonzero_finish", "diff_last", "cross_row_tie"],
          tags=("ties",)),
    _case("k64_v65_l230", 64, 65, 230, ["long70"], entries=("advance",)),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
MULTI_STEP = [dict(name="steps_k5_v65", K=5, V=65, L=12, B=3, steps=6), dict(name="steps_k33_v193", K=33, V=193, L=12, B=3, steps=6)]


class Win:
    """A buffer of the ABI as a window inside a larger allocation with GUARD sentinel elements on both sides."""
    PATTERN = {np.dtype(np.float32): np.float32(-12345.625), np.dtype(np.int64): np.int64(-0x5A5A5A5A5A5A),
               np.dtype(np.int32): np.int32(-0x5A5A5A), np.dtype(np.uint8): np.uint8(0xA5)}

    def __init__(self, arr, lo=GUARD):
        arr = np.ascontiguousarray(arr)
        self.shape, self.lo, self.n = arr.shape, lo, arr.size
        self.full = np.full(lo + arr.size + GUARD, self.PATTERN[arr.dtype], arr.dtype)
        self.full[lo:lo + arr.size] = arr.reshape(-1)

    @property
    def view(self):
        return self.full[self.lo:self.lo + self.n].reshape(self.shape)

    def intact(self, full=None):
        full = self.full if full is None else full
        pat = self.PATTERN[self.full.dtype]
        return bool((full[:self.lo] == pat).all() and (full[self.lo + self.n:] == pat).all())

    @staticmethod
    def window_of(win, full):
        return full[win.lo:win.lo + win.n].reshape(win.shape)


def draw_utterance(cls, seed, b, step_no, K, V, L, blk, step, first, beam_prune):
    """`build_utterance` with the first draw whose top K + 1 candidates are decisive (asserted: never skipped)."""
    for attempt in range(400):
        rng = np.random.default_rng([seed, b, step_no, attempt])
        st, x = build_utterance(cls, rng, K, V, L, blk, step)
        x_s = (np.float32(SM_SCALE) * x).astype(np.float32)
        ok, tie = top_is_decisive(x_s, st, first, beam_prune)
        if ok:
            return st, x, tie
    raise AssertionError("no decisive draw for %s utterance %d" % (cls, b))


def assemble(utts, K, V, L, blk, step, fin_cap, tags=()):
    """Per-utterance states -> the buffers of the ABI (name -> Win)."""
    B = len(utts)
    rng = np.random.default_rng(7)
    fin_n = np.array([fin_cap - 4 if u["fin_n"] == "cap-4" else u["fin_n"] for u in utts], np.int64)
    a = dict(
        scores=np.stack([u["scores"] for u in utts]), lm_scores=np.stack([u["lm_scores"] for u in utts]),
        y=np.stack([u["y"] for u in utts]), t_idx=np.stack([u["t_idx"] for u in utts]),
        num_frames=np.array([u["num_frames"] for u in utts], np.int64), max_len=np.array([u["max_len"] for u in utts], np.int64),
        hyp=np.stack([u["hyp"] for u in utts]), hyp_len=np.stack([u["hyp_len"] for u in utts]),
        ks_hist=rng.integers(0, K, (HIST, B, K)).astype(np.int64), ys_hist=rng.integers(0, V, (HIST + 1, B, K)).astype(np.int64),
        step_t=np.array([step], np.int64), eos_top=np.array([u["eos_top"] for u in utts], np.uint8),
        fin_score=rng.standard_normal((B, fin_cap)).astype(np.float32), fin_step=rng.integers(1, 9, (B, fin_cap)).astype(np.int64),
        fin_k=rng.integers(0, K, (B, fin_cap)).astype(np.int64), fin_n=fin_n,
        prev_k=np.full((B, K), -3, np.int64), y_raw=np.full((B, K), -3, np.int64),
        stop=np.zeros(1, np.int32), max_hyp=np.array([50 if "max_hyp" in tags else 0], np.int64),
        sync=np.array([0, 0, 0, 0, 0, 7, 7, 9], np.int32), cand_ws=np.zeros(B * K * K * 8, np.uint8))
    q = (step & 1) ^ 1
    a["sync"][2 * q], a["sync"][2 * q + 1] = 3, 1 << 16           # what the step before left in its own parity's scratch
    return {k: Win(v) for k, v in a.items()}


def plain(state):
    """name -> a copy of the window of every buffer."""
    return {k: w.view.copy() for k, w in state.items()}


def make_state(case, seed=None):
    """Every buffer of the ABI for `case` (name -> Win), the raw logits (B,K,V) f32 as a Win, and has_tie.  The draw of
    every utterance is decisive (see top_is_decisive) or this raises."""
    K, V, L, blk = case["K"], case["V"], case["L"], case["blk"]
    step = 0 if case["first"] else STEP_T
    seed = case["seed"] if seed is None else seed
    utts, xs, tie = [], [], False
    for b, cls in enumerate(case["utts"]):
        st, x, t = draw_utterance(cls, seed, b, 0, K, V, L, blk, step, case["first"], case["beam_prune"])
        utts.append(st)
        xs.append(x)
        tie |= t
    fin_cap = 2 * K + 6
    state = assemble(utts, K, V, L, blk, step, fin_cap, case["tags"])
    logits = Win(np.stack(xs), lo=GUARD + (1 if "misaligned" in case["tags"] else 0))
    return state, logits, tie


def range_statistics(x, ldl_extra=0):
    """(rows, V) fp32 scaled logits -> pmax, psum (rows * splits) f32 and the padded logits (rows, ldl) with columns [V, ldl)
    at -inf, as pika_dfc2_logits would leave them: built in torch (float64 sums, rounded once)."""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x))
    rows, V = xt.shape
    splits = (V + COLS - 1) // COLS
    ldl = splits * COLS + ldl_extra
    pad = torch.full((rows, ldl), -float("inf"), dtype=torch.float32)
    pad[:, :V] = xt
    r = pad[:, :splits * COLS].view(rows, splits, COLS).double()
    pmax = r.max(dim=2).values
    psum = torch.exp(r - pmax.unsqueeze(2)).sum(dim=2)
    return pmax.float().reshape(-1).numpy(), psum.float().reshape(-1).numpy(), pad.numpy(), splits, ldl


def yardstick_scores(state, logits, want, first):
    """The contract's formula in fp32 with plain torch ops on the CPU, for the candidates the reference selected:
    torch.log_softmax of the fp32 x, the two adds in the contract's order, the subtraction.  (B,K) float32."""
    import torch
    B, K = state["y"].shape
    x = torch.from_numpy((np.float32(SM_SCALE) * logits).astype(np.float32))
    lp = torch.log_softmax(x, dim=2).numpy()
    lms = np.float32(LM_SCALE)
    out = np.zeros((B, K), np.float32)
    for b in range(B):
        for i in range(K):
            p, sym = int(want["prev_k"][b, i]), int(want["y_raw"][b, i])
            v = lp[b, p, sym]
            if not first:
                v = np.float32(np.float32(v + state["scores"][b, p]) + np.float32(lms * state["lm_scores"][b, p]))
            out[b, i] = np.float32(v - np.float32(lms * state["lm_scores"][b, p]))
    return out


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Everything the tests of one case share, computed once and never modified: (state Wins, logits Win, has_tie,
    want (pika_beam_advance), want_logits (pika_beam_advance_logits), yardstick error over the live selected candidates)."""
    case = CASE_BY_NAME[name]
    state, logits, tie = make_state(case)
    s0 = plain(state)
    want = advance_ref(s0, logits.view, SM_SCALE, LM_SCALE, case["first"], case["beam_prune"], case["blk"])
    want_l = advance_logits_ref(s0, logits.view, SM_SCALE, LM_SCALE, case["beam_prune"], case["blk"], N_BEST)
    live = np.abs(want["scores"]) < 1e19
    y32 = yardstick_scores(s0, logits.view, want, case["first"])
    yard = float(np.abs(y32.astype(np.float64) - want["scores"])[live].max()) if live.any() else 0.0
    return state, logits, tie, want, want_l, yard


def gpu_score_ok(yard):
    """The GPU tolerance of a case: 4 x the yardstick's error, at least 4 ulp of the score; dead candidates (|score| >
    1e19) equal the fp32 rounding of the reference's value exactly."""
    def ok(got, want):
        got = np.asarray(got, np.float32)
        w32 = want.astype(np.float32)
        dead = np.abs(want) > 1e19
        tol = np.maximum(4.0 * yard, 4.0 * np.spacing(np.abs(w32)).astype(np.float64))
        return np.where(dead, got == w32, np.abs(got.astype(np.float64) - want) <= tol)
    return ok


def kernel_error(got, want):
    live = np.abs(want) < 1e19
    return float(np.abs(np.asarray(got, np.float64) - want)[live].max()) if live.any() else 0.0


def frame_rule(state, blk):
    """What the caller does between two steps: t_idx += 1 where y' == blk, clamped to num_frames - 1."""
    t = state["t_idx"] + (state["y"] == blk)
    state["t_idx"][...] = np.minimum(t, state["num_frames"][:, None] - 1)


def multi_step_start(cfg):
    """The clean state a search starts from (BeamState.__init__), utterances of 2, 3 and 4 frames, max_len 4 / 30 / 30."""
    K, V, L, B = cfg["K"], cfg["V"], cfg["L"], cfg["B"]
    utts = []
    for b in range(B):
        utts.append(dict(scores=np.zeros(K, np.float32), lm_scores=np.zeros(K, np.float32), y=np.zeros(K, np.int64),
                         t_idx=np.zeros(K, np.int64), num_frames=2 + b, max_len=4 if b == 0 else 30,
                         hyp=np.zeros((K, L), np.int64), hyp_len=np.zeros(K, np.int64), eos_top=0, fin_n=0))
    return assemble(utts, K, V, L, 0, 0, K * HIST + 1)


def multi_step_logits(cfg, s, step_no):
    """Fresh logits (B,K,V) and lm_scores (B,K) for step `step_no` over state `s` (plain arrays), decisive per utterance."""
    K, V, B = cfg["K"], cfg["V"], cfg["B"]
    xs, lms = [], []
    for b in range(B):
        for attempt in range(400):
            rng = np.random.default_rng([99, b, step_no, attempt, K])
            x = (rng.standard_normal((K, V)) * 2.5).astype(np.float32)
            x[:, 0] += 3.0
            lm = rng.standard_normal(K).astype(np.float32)
            st = dict(y=s["y"][b], hyp=s["hyp"][b], hyp_len=s["hyp_len"][b], scores=s["scores"][b], lm_scores=lm)
            ok, _ = top_is_decisive((np.float32(SM_SCALE) * x).astype(np.float32), st, step_no == 0, 1)
            if ok:
                break
        else:
            raise AssertionError("no decisive draw for step %d utterance %d" % (step_no, b))
        xs.append(x)
        lms.append(lm)
    return np.stack(xs), np.stack(lms)
