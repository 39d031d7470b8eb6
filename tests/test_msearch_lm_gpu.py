"""The one-symbol-per-frame beam search with LM / hotword fusion on the device (include/pika_msearch_lm.h,
csrc/msearch.hip: the NFST = 1, 2 instantiations of the frame step).

As in tests/test_msearch_gpu.py, step validity is judged from the kernel's OWN previous state, frame by frame, in
float64 (tests/msearch_lm_common.py); the tolerance of a case is 2 x the worst error of the float32 yardstick (the same
formulas in numpy float32) against float64 on that case's inputs; measured: profiles/msearch_lm_parity.txt."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_bias_common as CB  # noqa: E402
import ctc_lm_common as CL  # noqa: E402
import msearch_common as M  # noqa: E402
import msearch_lm_common as ML  # noqa: E402
import test_msearch_gpu as TG  # noqa: E402

pytestmark = pytest.mark.gpu
NINF = -np.inf
REPORT = []
HOT = [(1, 2), (3,)]          # reaches every non-blank class


def device_lm(ref, dev):
    from pika_amd.ctc import CtcNgramLm
    return CtcNgramLm(ref.fst, ref.backoff_id, ref.label_offset, dev)


def hotwords(phrases, V, boost, dev, blank=0):
    """(the device phrase list, the same graph as a reference LM)"""
    from pika_amd.ctc import CtcHotwords
    return CtcHotwords(phrases, V, boost, blank, dev), CB.hot_lm(phrases, V, boost, blank)


def beam_of(state):
    """The kernel's state on the host: per utterance K entries (float32 F, float32 am, tokens tuple)."""
    hyp, ln = (t.cpu().numpy() for t in state.hyps())
    F, am = state.scores.cpu().numpy(), state.am_scores.cpu().numpy()
    return [[(F[b, k], am[b, k], tuple(int(v) for v in hyp[b, k, :max(ln[b, k], 0)])) for k in range(state.beam)]
            for b in range(state.batch)]


def as_ref(prev, lms, weights, lb, dtype):
    """The kernel's slots as a reference beam: bonus and states recomputed from the tokens."""
    out = []
    for F, am, tok in prev:
        if F > NINF:
            bonus, states = ML.bonus_of(lms, weights, lb, tok)
            out.append((dtype(F), dtype(am), bonus, tok, states))
        else:
            out.append(ML.EMPTY)
    return out


def check_step(prev, new, parent, token, rows32, lms, weights, lb, C, blank, sm_scale, penalty):
    """One utterance, one frame.  -> (kernel error, yardstick error, merges of the reference); the exact properties are
    asserted here."""
    K = len(prev)
    _, _, _, ref = ML.step(as_ref(prev, lms, weights, lb, np.float64), rows32.astype(np.float64), lms, weights, lb, C,
                           blank, sm_scale, penalty, np.float64)
    _, _, _, yard = ML.step(as_ref(prev, lms, weights, lb, np.float32), rows32, lms, weights, lb, C, blank, sm_scale,
                            penalty, np.float32)
    cand, lp = ref["cand"], ref["lp"]
    fin = cand > NINF
    yerr = float(np.max(np.abs(yard["cand"][fin].astype(np.float64) - cand[fin]))) if fin.any() else 0.0
    # the yardstick's merged am and fused scores against float64 on the yardstick's own groups
    for G32, am32, rep, key, ranks in yard["groups"]:
        members = [(yard["selected"][r][1], yard["selected"][r][2]) for r in ranks]
        a64 = [np.float64(prev[k][1]) + lp[k, v] for k, v in members]
        m64 = M.merge_value(a64)
        yerr = max(yerr, abs(float(am32) - float(m64)), abs(float(G32) - float(m64 + yard["entries"][rep][2])))
    live = [j for j in range(K) if new[j][0] > NINF]
    assert live == list(range(len(live))), "live slots sit at the front"
    scores = [float(new[j][0]) for j in live]
    assert scores == sorted(scores, reverse=True), "best first"
    keys = [new[j][2] for j in live]
    assert len(set(keys)) == len(keys), "equal token sequences were merged"
    for j in range(len(live), K):
        assert parent[j] == 0 and token[j] == blank and new[j][1] == NINF
    where = {tok: k for k, (F, _, tok) in enumerate(prev) if F > NINF}
    order = np.sort(cand[fin])[::-1]
    cut = order[C - 1] if len(order) >= C else NINF            # the weakest pre-selected candidate
    nxt = order[C] if len(order) > C else NINF                  # the best one left out
    kerr, inexact = 0.0, 0
    for j in live:
        k, v = int(parent[j]), int(token[j])
        assert prev[k][0] > NINF and 0 <= v < cand.shape[1] and cand[k, v] > NINF
        assert keys[j] == (prev[k][2] if v == blank else prev[k][2] + (v,)), "the key is exact"
        fresh = ML.bonus_of(lms, weights, lb, keys[j])
        assert fresh is not None, "a token no automaton reaches does not appear"
        fused = np.float32(np.float64(new[j][1]) + fresh[0])
        inexact += int(fused != new[j][0])
        kerr = max(kerr, abs(float(new[j][0]) - float(fused)))                 # scores == fp32(am + bonus)
        kerr = max(kerr, float(cut - cand[k, v]))                              # (k, v) was among the C best
        # the candidates that spell this sequence: the sequence itself + blank, its parent sequence + its last token
        members = []
        if keys[j] in where:
            members.append((where[keys[j]], blank))
        if keys[j] and keys[j][:-1] in where:
            members.append((where[keys[j][:-1]], keys[j][-1]))
        members = [m for m in members if cand[m] > NINF]
        assert (k, v) in members
        members.sort(key=lambda m: -cand[m])
        a = {m: np.float64(prev[m[0]][1]) + lp[m] for m in members}
        options = [[m] for m in members] + ([members] if len(members) == 2 else [])
        errs = []
        for o in options:
            if (k, v) not in o:
                continue
            rep = o[0]                                                         # the best-ranked member leads the sum
            e = abs(float(new[j][1]) - float(a[rep] + np.log(sum(np.exp(a[m] - a[rep]) for m in o))))
            # a member is in the group only if it was pre-selected, and out of it only if it was not
            left_out = [float(cand[m] - nxt) if len(order) > C else np.inf for m in members if m not in o]
            e = max([e] + [float(cut - cand[m]) for m in o] + left_out)
            errs.append(e)
        kerr = max(kerr, min(errs))
        kerr = max(kerr, float(max(cand[m] for m in members if cand[m] >= cand[k, v]) - cand[k, v]))
    # the cut to K: a group of the float64 step that is not in the new beam is no better than the weakest kept one
    # (or hangs on a candidate at the edge of the pre-selection)
    kept = set(keys)
    weakest = min(scores) if len(live) == K else NINF
    for G, am, rep, key, ranks in ref["groups"]:
        if key not in kept:
            edge = max(float(ref["selected"][r][0]) for r in ranks) - float(nxt) if len(order) > C else np.inf
            kerr = max(kerr, min(float(G) - weakest, edge))
    return kerr, yerr, ref["merges"], inexact


def run_case(dev, name, dlm, lms, weights, lb, B, K, C, V, T, lens, ld, blank, sm_scale, penalty, models,
             need_merges=False):
    from pika_amd import ModifiedLmBeamState
    state = ModifiedLmBeamState(B, T, dlm, K, blank, weights[0], lb, C, dev)
    nf = torch.tensor(lens, device=dev)
    buf = torch.zeros((B * K, ld), dtype=torch.float32, device=dev)
    kerr = yerr = 0.0
    merges = inexact = 0
    prev = beam_of(state)
    for b in range(B):
        assert prev[b][0] == (0.0, 0.0, ()) and all(e[0] == NINF and e[1] == NINF for e in prev[b][1:])
    for t in range(T):
        rows = np.concatenate([models[b]([(e[0], e[2]) for e in prev[b]], t) for b in range(B)])
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        parent, token = state.advance(buf[:, :V], nf, sm_scale, penalty)
        new, parent, token = beam_of(state), parent.cpu().numpy(), token.cpu().numpy()
        frames = state.frames.cpu().tolist()
        for b in range(B):
            if t < lens[b]:
                assert frames[b] == t + 1
                ke, ye, mg, ix = check_step(prev[b], new[b], parent[b], token[b], rows[b * K:(b + 1) * K], lms, weights,
                                            lb, C, blank, sm_scale, penalty)
                kerr, yerr, merges, inexact = max(kerr, ke), max(yerr, ye), merges + mg, inexact + ix
            else:
                assert frames[b] == lens[b] and parent[b].tolist() == list(range(K)) and (token[b] == blank).all()
                assert [(e[0].tobytes(), e[1].tobytes(), e[2]) for e in new[b]] == \
                    [(e[0].tobytes(), e[1].tobytes(), e[2]) for e in prev[b]]
        prev = new
    assert not state.overflowed.any()
    print("msearch_lm parity %-40s kernel %.3e yardstick %.3e merges %d inexact F %d" % (name, kerr, yerr, merges, inexact))
    REPORT.append((name, kerr, yerr))
    assert not need_merges or merges > 0
    assert kerr <= 2 * yerr, (name, kerr, yerr)
    return state


# ---- zero weights: the plain search, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("V,K,T,pad", [(5, 4, 7, 3), (67, 16, 12, 0), (1031, 64, 7, 0), (1031, 64, 7, 1)])
def test_zero_weights_equal_the_plain_search(hip_device, V, K, T, pad):
    """pad = 3: scalar loads; pad = 0 with V = 67: scalar loads (ld % 4 != 0), with V = 1031: ld = V is odd as well, so
    pad = 1 (ld = 1032) is the case of the 16-byte loads."""
    from pika_amd import ModifiedBeamState, ModifiedLmBeamState
    dev, B, lens, ld = hip_device, 3, [0, 1, T], V + pad
    dlm, _ = hotwords(HOT, V, 1.0, dev)
    plain = ModifiedBeamState(B, T, K, 0, dev)
    fused = ModifiedLmBeamState(B, T, dlm, K, 0, 0.0, 0.0, K, dev)
    models = [TG.Rows(T, V, 300 + b, mask=V - 1) for b in range(B)]
    nf = torch.tensor(lens, device=dev)
    buf = torch.zeros((B * K, ld), dtype=torch.float32, device=dev)
    for t in range(T):
        prev = TG.beam_of(plain)
        rows = np.concatenate([models[b](prev[b], t) for b in range(B)])
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        p0, t0 = plain.advance(buf[:, :V], nf, 0.9, 0.25)
        p1, t1 = fused.advance(buf[:, :V], nf, 0.9, 0.25)
        assert torch.equal(p0, p1) and torch.equal(t0, t1), t
        assert plain.scores.cpu().numpy().tobytes() == fused.scores.cpu().numpy().tobytes(), t
        assert fused.am_scores.cpu().numpy().tobytes() == fused.scores.cpu().numpy().tobytes(), t
        assert all(torch.equal(a, c) for a, c in zip(plain.hyps(), fused.hyps())), t
    assert torch.equal(plain.frames, fused.frames)
    a, c = plain.results(nbest=K), fused.results(nbest=K, use_final=False)
    assert all(torch.equal(x, y) for x, y in zip(a, c[:3])) and torch.equal(c[2], c[3])


@pytest.mark.parametrize("ld", [1034, 1032])
def test_selection_overflow_takes_the_exact_slow_path(hip_device, ld):
    """The inputs of tests/test_msearch_gpu.py's overflow test (the collect pass holds 1024 entries; here more are at or
    before the threshold), through the fused state with C = 64 at zero weights: byte-equal to the plain state."""
    from pika_amd import ModifiedBeamState, ModifiedLmBeamState
    V, K, dev = 1031, 64, hip_device
    rng = np.random.RandomState(5)
    dlm, _ = hotwords(HOT, V, 1.0, dev)
    plain = ModifiedBeamState(1, 4, K, 0, dev)
    fused = ModifiedLmBeamState(1, 4, dlm, K, 0, 0.0, 0.0, 64, dev)
    nf = torch.tensor([4], device=dev)
    buf = torch.zeros((K, ld), dtype=torch.float32, device=dev)
    first = np.full((K, V), -30.0, np.float32)
    first[:, 1:K + 1] = -1.0 * np.arange(K, dtype=np.float32)
    big = np.arange(0, V, 64) if ld % 4 else np.array([v for i in range(0, V // 4, 64) for v in range(4 * i, 4 * i + 4)])
    assert len(big) * (K - 1) + 1 > 1024
    second = np.full((K, V), -200.0, np.float32)
    second[:, big] = (10.0 + 0.05 * rng.rand(K, len(big))).astype(np.float32)
    for rows in (first, second, second):
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        p0, t0 = plain.advance(buf[:, :V], nf)
        p1, t1 = fused.advance(buf[:, :V], nf)
        assert torch.equal(p0, p1) and torch.equal(t0, t1)
        assert plain.scores.cpu().numpy().tobytes() == fused.scores.cpu().numpy().tobytes()
        assert all(torch.equal(a, c) for a, c in zip(plain.hyps(), fused.hyps()))
    assert int((fused.scores > NINF).sum()) == K


# ---- every step is valid ---------------------------------------------------------------------------------------------
SHAPES = [(5, 2, 2, 12), (5, 4, 64, 12), (67, 16, 32, 9), (1031, 4, 8, 7)]       # (V, K, C, T)


def automata(kind, V, seed, dev):
    """-> (what the state takes as `lm`, the reference automata, their weights)"""
    from pika_amd.ctc import CtcBiasedLm
    lmw, bw = ML.f32(0.5), ML.f32(1.25)
    phrases = HOT if V == 5 else CB.seeded_phrases(V, 0, seed, 4)
    if kind == "hot":
        dhot, rhot = hotwords(phrases, V, 1.5, dev)
        return dhot, [rhot], [lmw]
    ref = CL.make_lm(V, 0, seed, order=3, unreachable=(V - 2,))
    if kind == "lm":
        return device_lm(ref, dev), [ref], [lmw]
    dhot, rhot = hotwords(phrases, V, 1.5, dev)
    return CtcBiasedLm(device_lm(ref, dev), dhot, bw), [ref, rhot], [lmw, bw]


@pytest.mark.parametrize("kind", ["lm", "lm+hot", "hot"])
@pytest.mark.parametrize("V,K,C,T", SHAPES)
def test_every_step_is_valid(hip_device, kind, V, K, C, T):
    """B = 3 with lengths {0, 1, T}; rows shifted by +-80, a masked class and a dead row; ld > V (scalar loads) for the
    hotword cases, ld = V rounded up to 4 (16-byte loads) for the pair."""
    B, lens = 3, [0, 1, T]
    i = SHAPES.index((V, K, C, T))
    dlm, lms, weights = automata(kind, V, 40 + i, hip_device)
    ld = V + 3 if kind == "hot" else ((V + 3) // 4 * 4 if kind == "lm+hot" else V)
    models = [TG.Rows(T, V, 2000 * i + b, mask=V - 1) for b in range(B)]
    run_case(hip_device, "%s V=%d K=%d C=%d T=%d ld=%d" % (kind, V, K, C, T, ld), dlm, lms, weights, ML.f32(0.25), B, K, C,
             V, T, lens, ld, 0, 0.9, 0.25, models)


@pytest.mark.parametrize("V,K,C,T", [(5, 4, 8, 7), (67, 16, 16, 12)])
def test_forced_merges(hip_device, V, K, C, T):
    """Logits that do not depend on the prefix and favour blank: "a" + b and "a b" + blank are both pre-selected.  The
    reference merges (asserted), so the kernel has to; the merged entry's bonus is its members' (check_step compares
    scores - am_scores with the bonus of the tokens)."""
    B = 2
    dlm, rhot = hotwords(HOT, V, 1.0, hip_device)
    lmw, lb = ML.f32(0.5), ML.f32(0.25)
    models = [TG.Rows(T, V, 77 + b, shift=False, kill=False, scale=0.3, prefix_free=True) for b in range(B)]
    for m in models:
        m.E[:, :3] += np.float32([2.0, 1.0, 0.8])
        m.E[:, 3:] -= 3.0
    for b in range(B):        # the reference alone: it merges
        _, infos = ML.search(lambda tok, t: models[b].E[t].astype(np.float64), T, V, K, C, [rhot], [lmw], lb)
        assert sum(i["merges"] for i in infos) > 0
    run_case(hip_device, "merges V=%d K=%d C=%d T=%d" % (V, K, C, T), dlm, [rhot], [lmw], lb, B, K, C, V, T, [T, T], V, 0,
             1.0, 0.0, models, need_merges=True)


# ---- end to end ------------------------------------------------------------------------------------------------------
# seeds 0..9 per configuration (T, V, K, C); REJECTED: those whose float64 run leaves a margin (pre-selection, cut to K,
# final scores with and without the final costs) of at most 2 tol, or whose float32 run decides differently (found on
# the CPU: python tests/test_msearch_lm_gpu.py)
E2E = {(12, 9, 4, 4): (), (12, 9, 4, 8): (), (20, 40, 8, 16): (0,)}
E2E_W = (ML.f32(0.5), ML.f32(0.25), 0.9, 0.1)          # lm_weight, length_bonus, sm_scale, blank_penalty
_E2E_CACHE = {}


def e2e_reference(T, V, K, C, seed):
    key = (T, V, K, C, seed)
    if key not in _E2E_CACHE:
        lmw, lb, sm, pen = E2E_W
        lm = CL.make_lm(V, 0, 100 + seed, order=3)
        model = M.TableModel(T, V, 31 * seed + V)
        model32 = lambda tok, t: model(tok, t).astype(np.float32).astype(np.float64)      # noqa: E731
        beam, infos = ML.search(model32, T, V, K, C, [lm], [lmw], lb, 0, sm, pen)
        ybeam, yinfos = ML.search(model32, T, V, K, C, [lm], [lmw], lb, 0, sm, pen, np.float32)
        yerr = ML.yardstick_error(infos, yinfos, beam, ybeam)
        fins = [ML.results(beam, [lm], [lmw], uf) for uf in (True, False)]
        yfin = ML.results(ybeam, [lm], [lmw], True, np.float32)
        if [f[0] for f in yfin] == [f[0] for f in fins[0]]:
            yerr = max([yerr] + [abs(float(a[1]) - float(c[1])) for a, c in zip(fins[0], yfin)])
        else:
            yerr = np.inf
        margin = min(ML.margins(infos, fins[0]), ML.margins(infos, fins[1]))
        _E2E_CACHE[key] = (model, lm, fins, 2 * yerr, margin)
    return _E2E_CACHE[key]


def rejected(T, V, K, C):
    out = []
    for seed in range(10):
        _, _, _, tol, margin = e2e_reference(T, V, K, C, seed)
        if not margin > 2 * tol:
            out.append(seed)
    return tuple(out)


@pytest.mark.parametrize("T,V,K,C", sorted(E2E))
def test_end_to_end_equals_the_reference(hip_device, T, V, K, C):
    from pika_amd import ModifiedLmBeamState
    cfg, dev = (T, V, K, C), hip_device
    assert rejected(*cfg) == E2E[cfg] and len(E2E[cfg]) <= 2
    lmw, lb, sm, pen = E2E_W
    seeds = [s for s in range(10) if s not in E2E[cfg]]
    for seed in seeds:               # (one LM per seed: one state per seed, B = 1)
        model, lm, fins, tol, _ = e2e_reference(T, V, K, C, seed)
        state = ModifiedLmBeamState(1, T, device_lm(lm, dev), K, 0, lmw, lb, C, dev)
        nf = torch.full((1,), T, device=dev)
        for t in range(T):
            prev = beam_of(state)[0]
            rows = np.stack([np.asarray(model(e[2], t), np.float64) if e[0] > NINF else np.zeros(V)
                             for e in prev]).astype(np.float32)
            state.advance(torch.from_numpy(rows).to(dev), nf, sm, pen)
        for want, use_final in zip(fins, (True, False)):
            tokens, lengths, scores, am = (t.cpu().numpy()[0] for t in state.results(nbest=K, use_final=use_final))
            for j in range(K):
                if j < len(want):
                    tok, s, a = want[j]
                    assert lengths[j] == len(tok) and tuple(tokens[j, :len(tok)]) == tok, (seed, use_final, j)
                    assert (tokens[j, len(tok):] == -1).all()
                    assert abs(float(scores[j]) - float(s)) <= tol and abs(float(am[j]) - float(a)) <= tol
                else:
                    assert lengths[j] == -1 and scores[j] == NINF and am[j] == NINF and (tokens[j] == -1).all()


# ---- hotwords do what they are for -----------------------------------------------------------------------------------
def spoken(frames, V, peak=6.0):
    """Prefix-free logits: frame t favours class frames[t] (a tuple: (class, logit) pairs beside the default peak)."""
    out = np.zeros((len(frames), V), np.float32)
    for t, f in enumerate(frames):
        for c, val in (f if isinstance(f, tuple) else ((f, peak),)):
            out[t, c] = val
    return out


def decode(state, logits, dev):
    K = state.beam
    nf = torch.full((1,), len(logits), device=dev)
    for row in logits:
        state.advance(torch.from_numpy(np.tile(row, (K, 1))).to(dev), nf)
    return state


def test_hotwords_pull_their_phrase_to_the_top(hip_device):
    from pika_amd import ModifiedBeamState, ModifiedLmBeamState
    dev, V, K, phrase, rival = hip_device, 6, 8, (1, 2, 3), (1, 2, 4)
    logits = spoken([1, 0, 2, 0, ((4, 6.0), (3, 5.0)), 0], V)        # the last label: 4 ahead of 3 by one
    tokens, lengths, scores = (t.cpu().numpy()[0] for t in decode(ModifiedBeamState(1, 6, K, 0, dev), logits,
                                                                  dev).results(nbest=K))
    got = {tuple(tokens[j, :lengths[j]]): float(scores[j]) for j in range(K) if lengths[j] >= 0}
    assert tuple(tokens[0, :lengths[0]]) == rival and phrase in got
    margin = got[rival] - got[phrase]                                 # what the plain search misses the phrase by
    assert 0.5 < margin < 1.5
    for boost, top in ((margin / 3 + 0.05, phrase), (margin / 3 - 0.05, rival)):
        dlm, rhot = hotwords([phrase], V, boost, dev)
        state = decode(ModifiedLmBeamState(1, 6, dlm, K, 0, 1.0, 0.0, 2 * K, dev), logits, dev)
        for use_final in (True, False):
            tok, ln, sc, am = (t.cpu().numpy()[0] for t in state.results(nbest=K, use_final=use_final))
            assert tuple(tok[0, :ln[0]]) == top, (boost, use_final)
            for j in range(K):
                if ln[j] >= 0:                                        # the fused score is am + BIAS, by the string rules
                    bias = CB.hot_bias([phrase], tuple(tok[j, :ln[j]]), ML.f32(boost), final=use_final)
                    assert abs(float(sc[j]) - float(am[j]) - bias) <= 1e-5, (j, use_final)
    # half spoken: the credit of the match in progress is refunded at the end
    boost = 2.0
    dlm, _ = hotwords([phrase], V, boost, dev)
    state = decode(ModifiedLmBeamState(1, 4, dlm, K, 0, 1.0, 0.0, 2 * K, dev), spoken([1, 0, 2, 0], V), dev)
    for use_final in (False, True):
        tok, ln, sc, am = (t.cpu().numpy()[0] for t in state.results(nbest=1, use_final=use_final))
        assert tuple(tok[0, :ln[0]]) == (1, 2)
        want = CB.hot_bias([phrase], (1, 2), boost, final=use_final)
        assert want == (0.0 if use_final else 2 * boost) and abs(float(sc[0]) - float(am[0]) - want) <= 1e-5


# ---- state handling --------------------------------------------------------------------------------------------------
def snapshot(state):
    """What a fused search state means, as bytes (the trie's slot numbers depend on which lane inserted first)."""
    return TG.snapshot(state) + [state.am_scores.cpu().numpy().tobytes()]


def test_state_handling_and_determinism(hip_device):
    from pika_amd import ModifiedLmBeamState
    from pika_amd.ctc import CtcBiasedLm
    B, K, C, V, T, dev = 4, 8, 16, 37, 6, hip_device
    ref = CL.make_lm(V, 0, 9, order=3, unreachable=(5,))
    dhot, _ = hotwords(CB.seeded_phrases(V, 0, 9, 4), V, 1.5, dev)
    dlm = CtcBiasedLm(device_lm(ref, dev), dhot, 1.25)
    logits = TG.fixed_logits(B, K, V, 9, 3, dev)
    nf = torch.tensor([9, 4, 0, 6], device=dev)

    def run():
        s = ModifiedLmBeamState(B, T, dlm, K, 0, 0.5, 0.25, C, dev)
        outs = [s.advance(l, nf) for l in logits]
        return s, outs
    s1, o1 = run()
    s2, o2 = run()
    assert snapshot(s1) == snapshot(s2)                            # two runs: the same bits
    assert all(torch.equal(a, c) and torch.equal(p, q) for (a, p), (c, q) in zip(o1, o2))
    assert s1.frames.tolist() == [6, 4, 0, 6] and s1.overflowed.tolist() == [True, False, False, False]
    ident = torch.arange(K, device=dev)
    assert torch.equal(o1[6][0][0], ident) and bool((o1[6][1][0] == 0).all())
    # an inactive utterance keeps its bytes (the whole blob but the outputs is the state)
    frozen, blob = snapshot(s1), s1._state.clone()
    s1.advance(logits[0], nf)
    assert snapshot(s1) == frozen and torch.equal(s1._state, blob)
    # results() only reads, and the final costs live on the side: True, False, True gives the first answer again
    r = [[t.clone() for t in s1.results(nbest=K, use_final=uf)] for uf in (True, False, True)]
    assert torch.equal(s1._state, blob)
    assert all(torch.equal(a, c) for a, c in zip(r[0], r[2])) and not torch.equal(r[0][2], r[1][2])
    assert torch.equal(r[1][2], s1.scores) and torch.equal(r[1][3], s1.am_scores)
    sc = r[0][2].cpu().numpy()
    assert all(list(row[row > NINF]) == sorted(row[row > NINF], reverse=True) for row in sc)
    # reset(which) leaves the other utterances' bytes alone
    per = blob.numel()
    s1.reset(which=torch.tensor([True, False, False, True]))
    assert s1.frames.tolist() == [0, 4, 0, 0] and not s1.overflowed.any()
    after = s1.results(nbest=K, use_final=False)
    for a, c in zip(r[1], after):
        assert torch.equal(a[1:3], c[1:3])
    assert after[1][0].tolist() == [0] + [-1] * (K - 1) and after[2][0].tolist() == [0.0] + [NINF] * (K - 1)
    BK, N8 = B * K, (per - ((32 * B * K + 8 * B + 15) // 16 * 16)) // B
    for lo, size in ((0, 8), (8 * BK, 4), (12 * BK, 4), (16 * BK, 4), (20 * BK, 4), (24 * BK, 4), (28 * BK, 4)):
        for b in (1, 2):
            a, e = lo + size * K * b, lo + size * K * (b + 1)
            assert torch.equal(s1._state[a:e], blob[a:e])
    head = per - B * N8
    for b in (1, 2):
        assert torch.equal(s1._state[head + b * N8:head + (b + 1) * N8], blob[head + b * N8:head + (b + 1) * N8])
    # a restarted stream decodes as a fresh one
    s3 = ModifiedLmBeamState(B, T, dlm, K, 0, 0.5, 0.25, C, dev)
    for l in logits[:3]:
        s1.advance(l, torch.tensor([3, 0, 0, 0], device=dev))
        s3.advance(l, torch.tensor([3, 0, 0, 0], device=dev))
    assert all(torch.equal(a[0], c[0]) for a, c in zip(s1.results(nbest=K), s3.results(nbest=K)))
    tok, ln, _, _ = s3.results(nbest=K, max_len=2, use_final=False)
    full, ln2, _, _ = s3.results(nbest=K, use_final=False)
    assert torch.equal(ln, ln2) and torch.equal(tok, full[:, :, :2]) and 1 <= int(ln.max()) <= 3
    h, hl = s3.hyps()
    assert torch.equal(h, full) and torch.equal(hl, ln2)
    # the automata are checked against V and the device at advance
    from pika_amd.ctc import CtcHotwords
    small = ModifiedLmBeamState(1, 4, CtcHotwords(HOT, 4, 1.0, 0, dev), 2, 0, 1.0, 0.0, 2, dev)
    with pytest.raises(ValueError, match="backoff_id"):
        small.advance(torch.zeros(2, 8, device=dev), torch.tensor([4]))         # label 5 is a class of V = 8


def test_captured_advance_equals_the_eager_loop(hip_device):
    """Two eager steps, then one captured step replayed for the rest (the default hardware queues)."""
    from pika_amd import ModifiedLmBeamState
    from pika_amd.ctc import CtcBiasedLm
    B, K, C, V, T, dev = 3, 4, 8, 67, 8, hip_device
    ref = CL.make_lm(V, 1, 4, order=3)
    dhot, _ = hotwords(CB.seeded_phrases(V, 1, 4, 4), V, 1.5, dev, blank=1)
    dlm = CtcBiasedLm(device_lm(ref, dev), dhot, 1.25)
    logits = TG.fixed_logits(B, K, V, T, 11, dev)
    nf = torch.tensor([8, 5, 8], device=dev)
    eager = ModifiedLmBeamState(B, T, dlm, K, 1, 0.5, 0.25, C, dev)
    want = [eager.advance(l, nf, 0.9, 0.2) for l in logits]
    torch.cuda.synchronize()
    state = ModifiedLmBeamState(B, T, dlm, K, 1, 0.5, 0.25, C, dev)
    buf = torch.empty_like(logits[0])
    for l, (p, t) in zip(logits[:2], want[:2]):
        buf.copy_(l)
        out = state.advance(buf, nf, 0.9, 0.2)
        assert torch.equal(out[0], p) and torch.equal(out[1], t)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = state.advance(buf, nf, 0.9, 0.2)
    for l, (p, t) in zip(logits[2:], want[2:]):
        buf.copy_(l)
        g.replay()
        assert torch.equal(out[0], p) and torch.equal(out[1], t)
    assert snapshot(state) == snapshot(eager)


# ---- modified_beam_search_lm on the tiny rnn model -------------------------------------------------------------------
def reference_search(net64, enc, x_len, K, C, sm_scale, lms, weights, lb):
    """The float64 fused search per utterance on the model's own weights (CPU), as test_msearch_gpu.reference_search."""
    out = []
    with torch.no_grad():
        for b in range(enc.shape[0]):
            cache = {}

            def logits_of(tok, t, b=b, cache=cache):
                if tok not in cache:
                    o, _ = net64.decoder(net64.embed(torch.tensor([[0] + list(tok)])))
                    cache[tok] = o[0, -1]
                z = torch.cat((enc[b, t], cache[tok]))
                h = torch.tanh(net64.fc1(z)) * torch.sigmoid(net64.fc_gate(z))
                return net64.fc2(h).numpy()
            beam, infos = ML.search(logits_of, int(x_len[b]), net64.output_dim, K, C, lms, weights, lb, 0, sm_scale, 0.0)
            fin = ML.results(beam, lms, weights, True)
            out.append((fin, ML.margins(infos, fin)))
    return out


def test_modified_beam_search_lm_on_the_tiny_model(hip_device):
    from pika_amd import modified_beam_search, modified_beam_search_lm
    dev = hip_device
    net, (x, x_len) = TG.tiny("rnn", dev)
    xd, V = x.to(dev), net.output_dim
    K, C, sm, lmw, lb = 4, 8, 0.85, ML.f32(0.5), ML.f32(0.25)
    ref_lm = CL.make_lm(V, 0, 3, order=3)
    dlm = device_lm(ref_lm, dev)
    runs = [modified_beam_search_lm(net, xd, x_len, dlm, beam=K, nbest=K, sm_scale=sm, use_graph=g, precision="fp32",
                                    lm_weight=lmw, length_bonus=lb, candidates=C) for g in (True, False)]
    for a, c in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(a, c)                                    # graph and eager: bit-identical
    tokens, lengths, scores, am = (t.cpu().numpy() for t in runs[0][:4])
    net64, _ = TG.tiny("rnn", "cpu")
    with torch.no_grad():
        enc64 = net64.encoder(x).double()
    ref = reference_search(net64.double(), enc64, x_len, K, C, sm, [ref_lm], [lmw], lb)
    for b, (fin, margin) in enumerate(ref):
        got = {tuple(tokens[b, j, :lengths[b, j]]): (scores[b, j], am[b, j]) for j in range(K) if lengths[b, j] >= 0}
        for tok, s, a in fin:
            if tok in got:                                          # the tolerance is tests/test_msearch_gpu.py's
                assert np.isclose(got[tok][0], float(s), rtol=1e-5, atol=1e-4), (b, tok)
                assert np.isclose(got[tok][1], float(a), rtol=1e-5, atol=1e-4), (b, tok)
        if margin > 2e-4:                                           # wider than the score noise allowed above
            assert [tuple(tokens[b, j, :lengths[b, j]]) for j in range(K) if lengths[b, j] >= 0] == [f[0] for f in fin], b
    # zero weights and a phrase list that reaches every class: modified_beam_search, bit for bit
    dhot, _ = hotwords(HOT, V, 1.0, dev)
    t0, l0, s0, _ = modified_beam_search(net, xd, x_len, beam=K, nbest=K, sm_scale=sm, precision="fp32")
    t1, l1, s1, a1, _ = modified_beam_search_lm(net, xd, x_len, dhot, beam=K, nbest=K, sm_scale=sm, precision="fp32",
                                                lm_weight=0.0, length_bonus=0.0, candidates=K, use_final=False)
    assert torch.equal(t0, t1) and torch.equal(l0, l1) and torch.equal(s0, s1) and torch.equal(s1, a1)


if __name__ == "__main__":      # the seeds the margin rule rejects, found on the CPU
    for cfg in sorted(E2E):
        print(cfg, rejected(*cfg))
