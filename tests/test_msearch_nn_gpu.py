"""The one-symbol-per-frame beam search with a neural LM fused in, on the device (include/pika_msearch_nn.h,
csrc/msearch.hip: the DENSE instantiations of the frame step).

The method is tests/test_msearch_lm_gpu.py's: every step is judged from the kernel's OWN previous state in float64
(tests/msearch_nn_common.py on tests/msearch_lm_common.py), the `bonus` view is compared with the value recomputed from
the tokens, and the tolerance of a case is 2 x the worst error of the float32 yardstick against float64 on that case's
own inputs (the factor 2: the kernel's summation order is another, equally valid one).  Measured:
profiles/msearch_nn_parity.txt."""
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
import msearch_nn_common as MN  # noqa: E402
import test_msearch_gpu as TG  # noqa: E402
import test_msearch_lm_gpu as TL  # noqa: E402

pytestmark = pytest.mark.gpu
NINF = -np.inf
NNW, NNS = ML.f32(0.3), ML.f32(0.8)


def beam_of(state):
    """The kernel's state on the host: per utterance K entries (float32 F, float32 am, float64 bonus, tokens tuple)."""
    hyp, ln = (t.cpu().numpy() for t in state.hyps())
    F, am, bonus = state.scores.cpu().numpy(), state.am_scores.cpu().numpy(), state.bonus.cpu().numpy()
    return [[(F[b, k], am[b, k], bonus[b, k], tuple(int(v) for v in hyp[b, k, :max(ln[b, k], 0)]))
             for k in range(state.beam)] for b in range(state.batch)]


def as_ref(prev, lms, weights, lb, dtype):
    """The kernel's slots as a reference beam: bonus and states recomputed from the tokens."""
    out = []
    for F, am, _, tok in prev:
        if F > NINF:
            bonus, states = ML.bonus_of(lms, weights, lb, tok)
            out.append((dtype(F), dtype(am), bonus, tok, states))
        else:
            out.append(ML.EMPTY)
    return out


def check_step(prev, new, parent, token, rows32, L64, L32, weights, lb, C, blank, sm_scale, penalty):
    """One utterance, one frame, as test_msearch_lm_gpu.check_step; L64 / L32: the automata followed by the dense LM in
    float64 / in float32.  -> (kernel error, yardstick error, merges of the reference)."""
    K = len(prev)
    _, _, _, ref = ML.step(as_ref(prev, L64, weights, lb, np.float64), rows32.astype(np.float64), L64, weights, lb, C,
                           blank, sm_scale, penalty, np.float64)
    _, _, _, yard = ML.step(as_ref(prev, L32, weights, lb, np.float32), rows32, L32, weights, lb, C, blank, sm_scale,
                            penalty, np.float32)
    cand, lp = ref["cand"], ref["lp"]
    fin = cand > NINF
    yerr = float(np.max(np.abs(yard["cand"][fin].astype(np.float64) - cand[fin]))) if fin.any() else 0.0
    for G32, am32, rep, key, ranks in yard["groups"]:
        members = [(yard["selected"][r][1], yard["selected"][r][2]) for r in ranks]
        m64 = M.merge_value([np.float64(prev[k][1]) + lp[k, v] for k, v in members])
        b64 = ML.bonus_of(L64, weights, lb, key)
        yerr = max(yerr, abs(float(am32) - float(m64)))
        if b64 is not None:                 # the yardstick's bonus and fused score against float64, from the tokens
            yerr = max(yerr, abs(float(yard["entries"][rep][2]) - float(b64[0])), abs(float(G32) - float(m64 + b64[0])))
    live = [j for j in range(K) if new[j][0] > NINF]
    assert live == list(range(len(live))), "live slots sit at the front"
    scores = [float(new[j][0]) for j in live]
    assert scores == sorted(scores, reverse=True), "best first"
    keys = [new[j][3] for j in live]
    assert len(set(keys)) == len(keys), "equal token sequences were merged"
    for j in range(len(live), K):
        assert parent[j] == 0 and token[j] == blank and new[j][1] == NINF
    where = {tok: k for k, (F, _, _, tok) in enumerate(prev) if F > NINF}
    order = np.sort(cand[fin])[::-1]
    cut = order[C - 1] if len(order) >= C else NINF
    nxt = order[C] if len(order) > C else NINF
    kerr = 0.0
    for j in live:
        k, v = int(parent[j]), int(token[j])
        assert prev[k][0] > NINF and 0 <= v < cand.shape[1] and cand[k, v] > NINF
        assert keys[j] == (prev[k][3] if v == blank else prev[k][3] + (v,)), "the key is exact"
        fresh = ML.bonus_of(L64, weights, lb, keys[j])
        assert fresh is not None, "a token that does not exist does not appear"
        assert new[j][0] == np.float32(np.float64(new[j][1]) + new[j][2]), "F = fp32(am + bonus), the kernel's own"
        kerr = max(kerr, abs(float(new[j][2]) - float(fresh[0])))                 # the bonus view, from the tokens
        kerr = max(kerr, abs(float(new[j][0]) - float(np.float64(new[j][1]) + fresh[0])) - 0.5 * float(np.spacing(
            np.float32(abs(new[j][0])))))                                         # (less the rounding of F itself)
        kerr = max(kerr, float(cut - cand[k, v]))
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
            rep = o[0]
            e = abs(float(new[j][1]) - float(a[rep] + np.log(sum(np.exp(a[m] - a[rep]) for m in o))))
            left_out = [float(cand[m] - nxt) if len(order) > C else np.inf for m in members if m not in o]
            errs.append(max([e] + [float(cut - cand[m]) for m in o] + left_out))
        kerr = max(kerr, min(errs))
        kerr = max(kerr, float(max(cand[m] for m in members if cand[m] >= cand[k, v]) - cand[k, v]))
    kept = set(keys)
    weakest = min(scores) if len(live) == K else NINF
    for G, am, rep, key, ranks in ref["groups"]:
        if key not in kept:
            edge = max(float(ref["selected"][r][0]) for r in ranks) - float(nxt) if len(order) > C else np.inf
            kerr = max(kerr, min(float(G) - weakest, edge))
    return kerr, yerr, ref["merges"]


def automata(kind, V, seed, dev):
    """-> (`lm` of the state, reference automata, their weights, lm_weight): dense alone, + an n-gram, + the n-gram and
    a phrase list on a NEGATIVE weight (the subtraction of LODR)."""
    from pika_amd.ctc import CtcBiasedLm
    lmw, bw = ML.f32(0.5), ML.f32(-0.3)
    if kind == "nn":
        return None, [], [], lmw
    ref = CL.make_lm(V, 0, seed, order=3, unreachable=(V - 2,))
    if kind == "nn+lm":
        return TL.device_lm(ref, dev), [ref], [lmw], lmw
    phrases = TL.HOT if V == 5 else CB.seeded_phrases(V, 0, seed, 4)
    dhot, rhot = TL.hotwords(phrases, V, 1.5, dev)
    return CtcBiasedLm(TL.device_lm(ref, dev), dhot, bw), [ref, rhot], [lmw, bw], lmw


def run_case(dev, name, kind, B, K, C, V, VL, T, off, ld, lld, seed, lb=ML.f32(0.25), sm_scale=0.9, penalty=0.25):
    from pika_amd import ModifiedNnLmBeamState
    lens = {3: [0, 1, T], 2: [T - 2, T], 1: [T]}[B]
    dlm, lms, weights, lmw = automata(kind, V, seed, dev)
    table = MN.make_table(V, VL, seed + 1)
    L64 = lms + [MN.table_lm(table, NNS, off, np.float64)]
    L32 = lms + [MN.table_lm(table, NNS, off, np.float32)]
    weights = weights + [NNW]
    models = [TG.Rows(T, V, 50 * seed + b, mask=V - 1, kill=K > 1) for b in range(B)]
    state = ModifiedNnLmBeamState(B, T, K, 0, NNW, NNS, off, dlm, lmw, lb, C, dev)
    nf = torch.tensor(lens, device=dev)
    buf = torch.zeros((B * K, ld), dtype=torch.float32, device=dev)
    lbuf = torch.zeros((B * K, lld), dtype=torch.float32, device=dev)
    kerr = yerr = 0.0
    merges = 0
    prev = beam_of(state)
    for b in range(B):
        assert prev[b][0] == (0.0, 0.0, 0.0, ()) and all(e[0] == NINF and e[1] == NINF for e in prev[b][1:])
    for t in range(T):
        rows = np.concatenate([models[b]([(e[0], e[3]) for e in prev[b]], t) for b in range(B)])
        lrows = np.concatenate([MN.lm_rows(table, [e[3] for e in prev[b]], [e[0] > NINF for e in prev[b]])
                                for b in range(B)])
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        lbuf[:, :VL] = torch.from_numpy(lrows).to(dev)
        parent, token = state.advance(buf[:, :V], lbuf[:, :VL], nf, sm_scale, penalty)
        new, parent, token = beam_of(state), parent.cpu().numpy(), token.cpu().numpy()
        frames = state.frames.cpu().tolist()
        for b in range(B):
            if t < lens[b]:
                assert frames[b] == t + 1
                ke, ye, mg = check_step(prev[b], new[b], parent[b], token[b], rows[b * K:(b + 1) * K], L64, L32,
                                        weights, lb, C, 0, sm_scale, penalty)
                kerr, yerr, merges = max(kerr, ke), max(yerr, ye), merges + mg
            else:
                assert frames[b] == lens[b] and parent[b].tolist() == list(range(K)) and (token[b] == 0).all()
                assert [tuple(np.asarray(x).tobytes() for x in e[:3]) + (e[3],) for e in new[b]] == \
                    [tuple(np.asarray(x).tobytes() for x in e[:3]) + (e[3],) for e in prev[b]]
        prev = new
    assert not state.overflowed.any()
    print("msearch_nn parity %-52s kernel %.3e yardstick %.3e merges %d" % (name, kerr, yerr, merges))
    TL.REPORT.append((name, kerr, yerr))
    assert kerr <= 2 * yerr, (name, kerr, yerr)
    return merges


# ---- (a) every step is valid -----------------------------------------------------------------------------------------
# (B, K, C, V, V_lm, T, nn_label_offset, ld, lm_ld): scalar loads (5, 67), 16-byte loads (264), a wider LM vocabulary on
# an offset with 16-byte LM rows beside scalar acoustic rows (67 / 72), many merges (K = C = 64 on 5 classes)
SHAPES = [(3, 1, 1, 5, 5, 6, 0, 5, 5), (3, 4, 8, 67, 67, 12, 0, 67, 67), (2, 4, 4, 260, 260, 10, 0, 264, 264),
          (2, 16, 32, 67, 70, 12, 3, 67, 72), (1, 64, 64, 5, 5, 40, 0, 5, 5)]


@pytest.mark.parametrize("kind", ["nn", "nn+lm", "nn+lm+hot"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-K%d-C%d-V%d-VL%d-T%d" % s[:6])
def test_every_step_is_valid(hip_device, kind, shape):
    B, K, C, V, VL, T, off, ld, lld = shape
    i = SHAPES.index(shape)
    merges = run_case(hip_device, "%s B=%d K=%d C=%d V=%d V_lm=%d T=%d off=%d ld=%d lm_ld=%d" % ((kind,) + shape), kind,
                      B, K, C, V, VL, T, off, ld, lld, 60 + i)
    assert K < 64 or merges > 0


# ---- (b) the two equalities, bit for bit -----------------------------------------------------------------------------
def head(state):
    """The fused blob's head but the trie nodes (their numbers depend on which lane's insertion came first), and the
    slots' tokens."""
    BK, B = state.batch * state.beam, state.batch
    raw = state._state.cpu().numpy()
    parts = [raw[:16 * BK].tobytes(), raw[20 * BK:32 * BK + 8 * B].tobytes()]
    return parts + [t.cpu().numpy().tobytes() for t in state.hyps()]


@pytest.mark.parametrize("V,K,C,T,pad", [(5, 4, 8, 7, 3), (67, 16, 32, 12, 0), (260, 4, 4, 8, 4)])
def test_zero_nn_weight_equals_the_fused_search(hip_device, V, K, C, T, pad):
    from pika_amd import ModifiedLmBeamState, ModifiedNnLmBeamState
    dev, B, lens = hip_device, 3, [0, 1, T]
    dlm, _, _, lmw = automata("nn+lm+hot", V, 7, dev)
    fused = ModifiedLmBeamState(B, T, dlm, K, 0, lmw, 0.25, C, dev)
    dense = ModifiedNnLmBeamState(B, T, K, 0, 0.0, NNS, 0, dlm, lmw, 0.25, C, dev)
    models = [TG.Rows(T, V, 300 + b, mask=V - 1) for b in range(B)]
    nf = torch.tensor(lens, device=dev)
    buf = torch.zeros((B * K, V + pad), dtype=torch.float32, device=dev)
    lm_rows = [(3.0 * torch.randn(B * K, V + pad, generator=torch.Generator().manual_seed(t))).to(dev) for t in range(T)]
    for t in range(T):
        prev = TL.beam_of(fused)
        rows = np.concatenate([models[b]([(e[0], e[2]) for e in prev[b]], t) for b in range(B)])
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        p0, t0 = fused.advance(buf[:, :V], nf, 0.9, 0.25)
        p1, t1 = dense.advance(buf[:, :V], lm_rows[t][:, :V], nf, 0.9, 0.25)
        assert torch.equal(p0, p1) and torch.equal(t0, t1), t
        assert head(fused) == head(dense), t
    for uf in (True, False):
        assert all(torch.equal(a, c) for a, c in zip(fused.results(nbest=K, use_final=uf),
                                                     dense.results(nbest=K, use_final=uf)))


@pytest.mark.parametrize("V,K,T,pad", [(5, 4, 7, 3), (67, 16, 12, 0), (1031, 64, 7, 1)])
def test_dense_alone_at_zero_weights_equals_the_plain_search(hip_device, V, K, T, pad):
    from pika_amd import ModifiedBeamState, ModifiedNnLmBeamState
    dev, B, lens = hip_device, 3, [0, 1, T]
    plain = ModifiedBeamState(B, T, K, 0, dev)
    dense = ModifiedNnLmBeamState(B, T, K, 0, 0.0, 1.0, 0, None, 0.5, 0.0, K, dev)
    models = [TG.Rows(T, V, 300 + b, mask=V - 1) for b in range(B)]
    nf = torch.tensor(lens, device=dev)
    buf = torch.zeros((B * K, V + pad), dtype=torch.float32, device=dev)
    lm_rows = (3.0 * torch.randn(B * K, V, generator=torch.Generator().manual_seed(V))).to(dev)
    for t in range(T):
        prev = TG.beam_of(plain)
        rows = np.concatenate([models[b](prev[b], t) for b in range(B)])
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        p0, t0 = plain.advance(buf[:, :V], nf, 0.9, 0.25)
        p1, t1 = dense.advance(buf[:, :V], lm_rows, nf, 0.9, 0.25)
        assert torch.equal(p0, p1) and torch.equal(t0, t1), t
        assert TG.snapshot(plain) == TG.snapshot(dense), t          # F, frames, overflowed, tokens and len
        assert dense.am_scores.cpu().numpy().tobytes() == dense.scores.cpu().numpy().tobytes()
        assert not dense.bonus.any()
    a, c = plain.results(nbest=K), dense.results(nbest=K)
    assert all(torch.equal(x, y) for x, y in zip(a, c[:3])) and torch.equal(c[2], c[3])


@pytest.mark.parametrize("ld", [1034, 1032])
def test_selection_overflow_with_a_dense_row(hip_device, ld):
    """The inputs of test_msearch_lm_gpu.test_selection_overflow_takes_the_exact_slow_path with an LM row beside every
    acoustic row, at zero weights: F, tokens, parent and token are the plain state's."""
    from pika_amd import ModifiedBeamState, ModifiedNnLmBeamState
    V, K, dev = 1031, 64, hip_device
    rng = np.random.RandomState(5)
    plain = ModifiedBeamState(1, 4, K, 0, dev)
    dense = ModifiedNnLmBeamState(1, 4, K, 0, 0.0, 1.0, 0, None, 0.5, 0.0, K, dev)
    nf = torch.tensor([4], device=dev)
    buf = torch.zeros((K, ld), dtype=torch.float32, device=dev)
    lm_rows = torch.from_numpy(rng.randn(K, ld).astype(np.float32)).to(dev)[:, :V]
    first = np.full((K, V), -30.0, np.float32)
    first[:, 1:K + 1] = -1.0 * np.arange(K, dtype=np.float32)
    big = np.arange(0, V, 64) if ld % 4 else np.array([v for i in range(0, V // 4, 64) for v in range(4 * i, 4 * i + 4)])
    assert len(big) * (K - 1) + 1 > 1024
    second = np.full((K, V), -200.0, np.float32)
    second[:, big] = (10.0 + 0.05 * rng.rand(K, len(big))).astype(np.float32)
    for rows in (first, second, second):
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        p0, t0 = plain.advance(buf[:, :V], nf)
        p1, t1 = dense.advance(buf[:, :V], lm_rows, nf)
        assert torch.equal(p0, p1) and torch.equal(t0, t1)
        assert TG.snapshot(plain) == TG.snapshot(dense)
    assert int((dense.scores > NINF).sum()) == K


# ---- (c) candidates that do not exist --------------------------------------------------------------------------------
def test_labels_the_lm_cannot_score_do_not_appear(hip_device):
    """V = 6 acoustic classes on an LM of 4: labels 4 and 5 fall outside it; label 2's LM logit is -inf and label 3's
    NaN in the first frame; in the second the slot that spells (1,) gets a row of -inf: only its blank extends."""
    from pika_amd import ModifiedNnLmBeamState
    dev, K, C, V, VL = hip_device, 4, 16, 6, 4        # (C: every finite candidate)
    state = ModifiedNnLmBeamState(1, 3, K, 0, 0.5, 1.0, 0, None, 0.5, 0.0, C, dev)
    nf = torch.tensor([3], device=dev)
    ac = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0, 9.0], device=dev).repeat(K, 1)       # the acoustic best is label 5
    lm = torch.zeros((K, VL), device=dev)
    lm[0] = torch.tensor([0.0, 0.5, -float("inf"), float("nan")])
    lm[1:] = float("nan")                                                             # dead slots: never read
    state.advance(ac, lm, nf)
    got = [e[3] for e in beam_of(state)[0] if e[0] > NINF]
    assert got == [(1,), ()]
    lp = torch.log_softmax(torch.tensor([0.0, 0.5], dtype=torch.float64), 0)[1]       # (-inf and NaN take no part)
    assert abs(float(state.bonus[0, 0]) - 0.5 * float(lp)) <= 1e-6 and float(state.bonus[0, 1]) == 0.0
    lm = torch.zeros((K, VL), device=dev)
    lm[0] = -float("inf")                                                             # slot 0 spells (1,)
    lm[2:] = float("nan")
    state.advance(ac, lm, nf)
    beam = [e for e in beam_of(state)[0] if e[0] > NINF]
    got = [e[3] for e in beam]
    assert set(got) == {(1,), (), (2,), (3,)} and all(np.isfinite(e[0]) and np.isfinite(e[2]) for e in beam)
    # an LM row of +inf: no finite maximum, the labels of every slot die and the blanks stay
    # (the 16 candidates are cut by the acoustic score before the LM is asked: here the blanks are among them)
    lm = torch.full((K, VL), float("inf"), device=dev)
    _, token = state.advance(ac.flip(1).contiguous(), lm, nf)
    assert [e[3] for e in beam_of(state)[0] if e[0] > NINF] == got and bool((token == 0).all())


# ---- (d) (e) (f) a captured step, the time record, two runs ------------------------------------------------------------
def fixed_run(dev, capture, times=False, T=8):
    from pika_amd import ModifiedBeamTimes, ModifiedNnLmBeamState
    B, K, C, V, VL = 3, 4, 8, 67, 70
    dlm, _, _, lmw = automata("nn+lm+hot", V, 4, dev)
    logits = TG.fixed_logits(B, K, V, T, 11, dev)
    lm_logits = TG.fixed_logits(B, K, VL, T, 12, dev)
    nf = torch.tensor([8, 5, 8], device=dev)
    state = ModifiedNnLmBeamState(B, T, K, 0, NNW, NNS, 3, dlm, lmw, 0.25, C, dev)
    rec = ModifiedBeamTimes(state) if times else None
    buf, lbuf = torch.empty_like(logits[0]), torch.empty_like(lm_logits[0])
    outs, graph, out = [], None, None
    for t in range(T):
        buf.copy_(logits[t])
        lbuf.copy_(lm_logits[t])
        if capture and t >= 2:
            if graph is None:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = state.advance(buf, lbuf, nf, 0.9, 0.2)
            graph.replay()
        else:
            out = state.advance(buf, lbuf, nf, 0.9, 0.2)
        if rec is not None:
            rec.step(*out)
        outs.append((out[0].clone(), out[1].clone()))
    return state, outs, rec


def snapshot(state):
    return TL.snapshot(state) + [state.bonus.cpu().numpy().tobytes()]


def test_captured_advance_and_two_runs(hip_device):
    """Two eager steps, then one captured step replayed for the rest, equal the eager loop byte for byte; two eager runs
    give the same bits."""
    eager, want, _ = fixed_run(hip_device, False)
    again, outs2, _ = fixed_run(hip_device, False)
    assert snapshot(eager) == snapshot(again)
    assert all(torch.equal(a, c) and torch.equal(p, q) for (a, p), (c, q) in zip(want, outs2))
    state, outs, _ = fixed_run(hip_device, True)
    assert all(torch.equal(a, c) and torch.equal(p, q) for (a, p), (c, q) in zip(want, outs))
    assert snapshot(state) == snapshot(eager)
    assert int((eager.scores > NINF).sum()) > 4 and bool(eager.bonus.ne(0).any())


def test_time_record_next_to_the_dense_state(hip_device):
    """`ModifiedBeamTimes` beside the new state: the times of replaying (parent, token) on the host."""
    state, outs, rec = fixed_run(hip_device, False, times=True)
    B, K, lens = state.batch, state.beam, [8, 5, 8]
    rows = [[[] for _ in range(K)] for _ in range(B)]
    for t, (parent, token) in enumerate(outs):
        parent, token = parent.cpu().tolist(), token.cpu().tolist()
        for b in range(B):
            if t < lens[b]:
                rows[b] = [rows[b][parent[b][j]] + ([t] if token[b][j] != 0 else []) for j in range(K)]
    got, (hyp, ln) = rec.hyps().cpu().numpy(), [x.cpu().numpy() for x in state.hyps()]
    assert not rec.lost.any() and int(ln.max()) >= 2
    for b in range(B):
        for j in range(K):
            n = max(int(ln[b, j]), 0)
            assert got[b, j, :n].tolist() == (rows[b][j] if ln[b, j] >= 0 else []) and (got[b, j, n:] == -1).all()
    tok, lens_, _, _ = state.results(nbest=K)
    when = rec.results(tok, lens_).cpu().numpy()
    assert (when[:, 0, 0] >= 0).all()


# ---- (g) modified_beam_search_nnlm on the tiny rnn model ---------------------------------------------------------------
# per configuration (candidates, with an n-gram): seeds 0..9 of the LstmLm's weights; SKIPPED: the seeds at which a
# decision of the float64 run is closer than 2e-4, the width of the score tolerance of tests/test_msearch_gpu.py (found
# on the CPU: python tests/test_msearch_nn_gpu.py); at most 2 of 10
E2E = {(4, False): (), (8, True): (6,)}
E2E_K, E2E_SM, E2E_LB = 4, 0.85, ML.f32(0.25)
_E2E_CACHE = {}


def e2e_lm(seed, V):
    from pika_amd.model.lm import LstmLm
    torch.manual_seed(1000 + seed)
    return LstmLm(V, 8, 16).eval()


def e2e_reference(C, ngram, seed):
    key = (C, ngram, seed)
    if key not in _E2E_CACHE:
        net64, (x, x_len) = TG.tiny("rnn", "cpu")
        with torch.no_grad():
            enc64 = net64.encoder(x).double()
        V = net64.output_dim
        lms, weights = ([CL.make_lm(V, 0, 3, order=3)], [ML.f32(0.5)]) if ngram else ([], [])
        _E2E_CACHE[key] = MN.lstm_reference(net64.double(), e2e_lm(seed, V).double(), enc64, x_len, E2E_K, C, E2E_SM,
                                            NNW, NNS, 0, lms, weights, E2E_LB)
    return _E2E_CACHE[key]


def skipped(C, ngram):
    return tuple(s for s in range(10) if not min(m for _, m in e2e_reference(C, ngram, s)) > 2e-4)


@pytest.mark.parametrize("C,ngram", sorted(E2E))
def test_modified_beam_search_nnlm_on_the_tiny_model(hip_device, C, ngram):
    from pika_amd import modified_beam_search_nnlm
    dev, K = hip_device, E2E_K
    assert skipped(C, ngram) == E2E[(C, ngram)] and len(E2E[(C, ngram)]) <= 2
    net, (x, x_len) = TG.tiny("rnn", dev)
    xd, V = x.to(dev), net.output_dim
    dlm = TL.device_lm(CL.make_lm(V, 0, 3, order=3), dev) if ngram else None
    for seed in [s for s in range(10) if s not in E2E[(C, ngram)]]:
        nnlm = e2e_lm(seed, V).to(dev)
        runs = [modified_beam_search_nnlm(net, xd, x_len, nnlm, beam=K, nbest=K, sm_scale=E2E_SM, use_graph=g,
                                          precision="fp32", nn_weight=NNW, nn_scale=NNS, lm=dlm, lm_weight=ML.f32(0.5),
                                          length_bonus=E2E_LB, candidates=C)
                for g in ((True, False) if seed == 0 else (True,))]
        for a, c in zip(runs[0][:4], runs[-1][:4]):
            assert torch.equal(a, c)                                # graph and eager: bit-identical
        tokens, lengths, scores, am = (t.cpu().numpy() for t in runs[0][:4])
        for b, (fin, _) in enumerate(e2e_reference(C, ngram, seed)):
            got = [tuple(tokens[b, j, :lengths[b, j]]) for j in range(K) if lengths[b, j] >= 0]
            assert got == [f[0] for f in fin], (seed, b)            # tokens, lengths and order
            for j, (tok, s, a) in enumerate(fin):
                assert np.isclose(scores[b, j], float(s), rtol=1e-5, atol=1e-4), (seed, b, j)
                assert np.isclose(am[b, j], float(a), rtol=1e-5, atol=1e-4), (seed, b, j)


def test_nnlm_at_zero_weight_is_modified_beam_search(hip_device):
    from pika_amd import modified_beam_search, modified_beam_search_nnlm
    dev, K = hip_device, 4
    net, (x, x_len) = TG.tiny("rnn", dev)
    xd = x.to(dev)
    nnlm = e2e_lm(0, net.output_dim).to(dev)
    t0, l0, s0, _ = modified_beam_search(net, xd, x_len, beam=K, nbest=K, sm_scale=0.85, precision="fp32")
    t1, l1, s1, a1, _ = modified_beam_search_nnlm(net, xd, x_len, nnlm, beam=K, nbest=K, sm_scale=0.85, precision="fp32",
                                                  nn_weight=0.0, lm=None, length_bonus=0.0, candidates=K)
    assert torch.equal(t0, t1) and torch.equal(l0, l1) and torch.equal(s0, a1) and torch.equal(s1, a1)


if __name__ == "__main__":      # the seeds the margin rule skips, found on the CPU
    for cfg in sorted(E2E):
        print(cfg, skipped(*cfg), [round(min(m for _, m in e2e_reference(cfg[0], cfg[1], s)), 6) for s in range(10)])
