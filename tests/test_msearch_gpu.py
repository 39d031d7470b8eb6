"""The one-symbol-per-frame beam search on the device (include/pika_msearch.h, csrc/msearch.hip).

Step validity is judged from the kernel's OWN previous state, frame by frame, in float64; the tolerance of a case is
2 x the worst error of the float32 yardstick (tests/msearch_common.py, the same formulas in numpy float32) against
float64 on that case's inputs -- the "kernel <= 2 x yardstick" rule; measured: profiles/msearch_parity.txt."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msearch_common as M  # noqa: E402

pytestmark = pytest.mark.gpu
NINF = -np.inf
REPORT = []      # (case, kernel error, yardstick error); also printed: `pytest -s` shows the lines


def beam_of(state):
    """The kernel's state on the host: per utterance K entries (float32 score, tokens tuple)."""
    hyp, ln = (t.cpu().numpy() for t in state.hyps())
    sc = state.scores.cpu().numpy()
    return [[(sc[b, k], tuple(int(v) for v in hyp[b, k, :max(ln[b, k], 0)])) for k in range(state.beam)]
            for b in range(state.batch)]


def check_step(prev, new, parent, token, rows32, blank, sm_scale, penalty, K):
    """One utterance, one frame.  -> (kernel error, yardstick error); the exact properties are asserted here."""
    prev64 = [(np.float64(s), tok) for s, tok in prev]
    _, _, _, ref = M.step(prev64, rows32.astype(np.float64), blank, sm_scale, penalty, np.float64)
    ybeam, _, _, yard = M.step([(np.float32(s), tok) for s, tok in prev], rows32, blank, sm_scale, penalty, np.float32)
    cand = ref["cand"]
    fin = cand > NINF
    yerr = float(np.max(np.abs(yard["cand"][fin].astype(np.float64) - cand[fin]))) if fin.any() else 0.0
    # the yardstick's merged scores against float64 on the yardstick's own groups
    for (s32, _), ranks in zip(ybeam, yard["groups"]):
        members = [cand[yard["selected"][r][1], yard["selected"][r][2]] for r in ranks]
        yerr = max(yerr, abs(float(s32) - float(M.merge_value(sorted(members, reverse=True)))))
    n_fin = int(fin.sum())
    want = min(K, n_fin)
    live = [j for j in range(K) if new[j][0] > NINF]
    assert live == list(range(len(live))), "live slots sit at the front"
    scores = [float(new[j][0]) for j in live]
    assert scores == sorted(scores, reverse=True), "best first"
    keys = [new[j][1] for j in live]
    assert len(set(keys)) == len(keys), "equal token sequences were merged"
    for j in range(len(live), K):
        assert parent[j] == 0 and token[j] == blank
    where = {tok: k for k, (s, tok) in enumerate(prev) if s > NINF}
    kerr, core, optional = 0.0, [], []
    for j in live:
        k, v = int(parent[j]), int(token[j])
        assert prev[k][0] > NINF and 0 <= v < cand.shape[1]
        assert keys[j] == (prev[k][1] if v == blank else prev[k][1] + (v,)), "the key is exact"
        # the candidates that spell this sequence: the sequence itself + blank, its parent sequence + its last token
        members = []
        if keys[j] in where:
            members.append((where[keys[j]], blank))
        if keys[j] and keys[j][-1] != blank and keys[j][:-1] in where:
            members.append((where[keys[j][:-1]], keys[j][-1]))
        members = [m for m in members if cand[m] > NINF]
        assert (k, v) in members
        members.sort(key=lambda m: -cand[m])
        options = [[m] for m in members] + ([members] if len(members) == 2 else [])
        errs = [abs(float(new[j][0]) - float(M.merge_value([cand[m] for m in o]))) for o in options]
        kerr = max(kerr, min(errs))
        # which members the kernel merged shows in the score; a member too small to show (the options are one number)
        # is OPTIONAL: the count below decides
        eps = 4 * float(np.spacing(np.float32(abs(new[j][0]) + 1.0)))
        fits = [o for o, e in zip(options, errs) if e <= min(errs) + eps and (k, v) in o]
        assert fits, "parent and token are a member of the group"
        sure = [m for m in members if all(m in o for o in fits)]
        core += sure
        optional += [m for m in members if m not in sure and any(m in o for o in fits)]
        top = max(cand[m] for o in fits for m in o)
        kerr = max(kerr, float(top - cand[k, v]))                             # the representative is the group's best
    assert len(core) <= want <= len(core) + len(optional) and len(set(core + optional)) == len(core + optional)
    optional.sort(key=lambda m: -cand[m])
    selected = core + optional[:want - len(core)]
    if want:
        order = np.sort(cand[fin])[::-1]
        sel = np.array([cand[m] for m in selected])
        kerr = max(kerr, float(order[want - 1] - sel.min()))                  # every selected one is among the K best
        mask = fin.copy()
        for m in selected:
            mask[m] = False
        if mask.any():
            kerr = max(kerr, float(cand[mask].max() - sel.min()))             # no unselected one beats the weakest
    return kerr, yerr, ref["merges"]


class Rows(object):
    """Logits for a beam: E[t] + Q[a hash of the token sequence], rows shifted by +-80, one class masked to -inf in
    every row, and from frame 2 on the row of slot 1 all -inf."""

    def __init__(self, T, V, seed, shift=True, mask=None, kill=True, scale=2.0, prefix_free=False):
        rng = np.random.RandomState(seed)
        self.E = (scale * rng.randn(max(T, 1), V)).astype(np.float32)
        self.Q = (0.0 if prefix_free else scale) * rng.randn(8, V).astype(np.float32)
        self.shift, self.mask, self.kill, self.V = shift, mask, kill, V

    def __call__(self, beam, t):
        K = len(beam)
        rows = np.zeros((K, self.V), np.float32)
        for k, (s, tok) in enumerate(beam):
            rows[k] = self.E[t] + self.Q[hash(tok) % 8]
            if self.shift:
                rows[k] += (0.0, 80.0, -80.0)[k % 3]
        if self.mask is not None:
            rows[:, self.mask] = NINF
        if self.kill and t >= 2 and K > 1:
            rows[1] = NINF
        return rows


def run_case(dev, name, B, K, V, T, lens, ld, blank, sm_scale, penalty, models, need_merges=False):
    from pika_amd import ModifiedBeamState
    state = ModifiedBeamState(B, T, K, blank, dev)
    nf = torch.tensor(lens, device=dev)
    buf = torch.zeros((B * K, ld), dtype=torch.float32, device=dev)
    kerr = yerr = 0.0
    merges = 0
    prev = beam_of(state)
    for b in range(B):
        assert prev[b][0] == (0.0, ()) and all(s == NINF for s, _ in prev[b][1:])
    for t in range(T):
        rows = np.concatenate([models[b](prev[b], t) for b in range(B)])
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        parent, token = state.advance(buf[:, :V], nf, sm_scale, penalty)
        new, parent, token = beam_of(state), parent.cpu().numpy(), token.cpu().numpy()
        frames = state.frames.cpu().tolist()
        for b in range(B):
            if t < lens[b]:
                assert frames[b] == t + 1
                ke, ye, mg = check_step(prev[b], new[b], parent[b], token[b], rows[b * K:(b + 1) * K], blank, sm_scale,
                                        penalty, K)
                kerr, yerr, merges = max(kerr, ke), max(yerr, ye), merges + mg
            else:
                assert frames[b] == lens[b] and parent[b].tolist() == list(range(K)) and (token[b] == blank).all()
                assert [s.tobytes() for s, _ in new[b]] == [s.tobytes() for s, _ in prev[b]]
                assert [tok for _, tok in new[b]] == [tok for _, tok in prev[b]]
        prev = new
    assert not state.overflowed.any()
    print("msearch parity %-34s kernel %.3e yardstick %.3e merges %d" % (name, kerr, yerr, merges))
    REPORT.append((name, kerr, yerr))
    assert not need_merges or merges > 0
    assert kerr <= 2 * yerr, (name, kerr, yerr)
    return state


VS, KS, TS = (2, 5, 67, 1031), (1, 2, 4, 63, 64), (1, 7, 40)
STEP_CASES = [(V, K, TS[(i + j) % 3]) for i, V in enumerate(VS) for j, K in enumerate(KS)] + [(8200, 4, 7)]


@pytest.mark.parametrize("V,K,T", STEP_CASES)
def test_every_step_is_valid(hip_device, V, K, T):
    """B = 3 with lengths {0, 1, T}; rows shifted by +-80, a masked class and a dead row in every case; ld > V (scalar
    loads, and for V = 1031 a 16-byte row stride with a tail) in every second one."""
    B, lens = 3, [0, 1, T]
    i = STEP_CASES.index((V, K, T))
    ld = V if i % 2 == 0 else (V + 1 if V == 1031 else V + 3)
    blank = 0 if V == 2 else 1
    mask = None if V == 2 else V - 1
    models = [Rows(T, V, 1000 * i + b, mask=mask) for b in range(B)]
    run_case(hip_device, "V=%d K=%d T=%d ld=%d" % (V, K, T, ld), B, K, V, T, lens, ld, blank, 0.9, 0.25, models)


@pytest.mark.parametrize("V,K,T", [(5, 4, 7), (5, 64, 7), (67, 16, 12)])
def test_forced_merges(hip_device, V, K, T):
    """Logits that do not depend on the prefix and favour blank: "a" + b and "a b" + blank are both among the K best.
    The reference merges (asserted), so the kernel has to."""
    B = 2
    models = [Rows(T, V, 77 + b, shift=False, kill=False, scale=0.3, prefix_free=True) for b in range(B)]
    for m in models:          # blank and two labels carry the mass: "" + a and "a" + blank both stay in the beam
        m.E[:, :3] += np.float32([2.0, 1.0, 0.8])
        m.E[:, 3:] -= 3.0
    for b in range(B):        # the reference alone: it merges
        beam, infos = M.search(lambda tok, t: models[b].E[t].astype(np.float64), T, V, K)
        assert sum(i["merges"] for i in infos) > 0
    run_case(hip_device, "merges V=%d K=%d T=%d" % (V, K, T), B, K, V, T, [T, T], V, 0, 1.0, 0.0, models, need_merges=True)


@pytest.mark.parametrize("ld", [1034, 1032])
def test_selection_overflow_takes_the_exact_slow_path(hip_device, ld):
    """The collect pass holds 1024 entries.  64 rows whose 17 (scalar loads, ld % 4 != 0) or 20 (16-byte loads) large
    values all sit on the elements ONE lane reads, rows in strictly descending order of score: the threshold is row 63's
    maximum and 63 * 17 + 1 (63 * 20 + 1) entries are at or before it."""
    from pika_amd import ModifiedBeamState
    V, K, dev = 1031, 64, hip_device
    rng = np.random.RandomState(5)
    state = ModifiedBeamState(1, 4, K, 0, dev)
    nf = torch.tensor([4], device=dev)
    buf = torch.zeros((K, ld), dtype=torch.float32, device=dev)
    first = np.full((K, V), -30.0, np.float32)
    first[:, 1:K + 1] = -1.0 * np.arange(K, dtype=np.float32)       # 64 labels, scores one apart
    big = np.arange(0, V, 64) if ld % 4 else np.array([v for i in range(0, V // 4, 64) for v in range(4 * i, 4 * i + 4)])
    assert len(big) * (K - 1) + 1 > 1024
    second = np.full((K, V), -200.0, np.float32)          # (below every row's large values whatever its score)
    second[:, big] = (10.0 + 0.05 * rng.rand(K, len(big))).astype(np.float32)
    prev = beam_of(state)
    kerr = yerr = 0.0
    for t, rows in enumerate((first, second, second)):
        buf[:, :V] = torch.from_numpy(rows).to(dev)
        parent, token = state.advance(buf[:, :V], nf)
        new = beam_of(state)
        ke, ye, _ = check_step(prev[0], new[0], parent[0].cpu().numpy(), token[0].cpu().numpy(), rows, 0, 1.0, 0.0, K)
        kerr, yerr, prev = max(kerr, ke), max(yerr, ye), new
        if t == 0:
            assert sum(s > NINF for s, _ in new[0]) == K
    print("msearch parity %-34s kernel %.3e yardstick %.3e" % ("overflow ld=%d" % ld, kerr, yerr))
    REPORT.append(("overflow ld=%d" % ld, kerr, yerr))
    assert kerr <= 2 * yerr


# seeds 0..9 per configuration; REJECTED: those whose float64 run leaves a selection margin or a gap between adjacent
# final scores of at most 2 tol (found on the CPU: python tests/test_msearch_gpu.py)
E2E = {(12, 9, 4): (), (20, 40, 8): ()}


def e2e_reference(T, V, K, seed):
    model = M.TableModel(T, V, 31 * seed + V)
    model32 = lambda tok, t: model(tok, t).astype(np.float32).astype(np.float64)      # noqa: E731  (what the device gets)
    beam, infos = M.search(model32, T, V, K, 0, 0.9, 0.1)
    ybeam, yinfos = M.search(model32, T, V, K, 0, 0.9, 0.1, np.float32)
    same = [tok for _, tok in beam] == [tok for _, tok in ybeam]
    yerr = max(abs(float(a) - float(c)) for (a, _), (c, _) in zip(beam, ybeam) if a > NINF) if same else np.inf
    if same:
        for i, y in zip(infos, yinfos):
            fin = i["cand"] > NINF
            yerr = max(yerr, float(np.max(np.abs(y["cand"][fin].astype(np.float64) - i["cand"][fin]))))
    return model, beam, 2 * yerr, M.margins(infos, beam)


def rejected(T, V, K):
    out = []
    for seed in range(10):
        _, _, tol, margin = e2e_reference(T, V, K, seed)
        if not margin > 2 * tol:
            out.append(seed)
    return tuple(out)


@pytest.mark.parametrize("T,V,K", sorted(E2E))
def test_end_to_end_equals_the_reference(hip_device, T, V, K):
    from pika_amd import ModifiedBeamState
    assert rejected(T, V, K) == E2E[(T, V, K)] and len(E2E[(T, V, K)]) <= 2      # at most one seed in five
    seeds = [s for s in range(10) if s not in E2E[(T, V, K)]]
    refs = [e2e_reference(T, V, K, s) for s in seeds]
    B, dev = len(seeds), hip_device
    state = ModifiedBeamState(B, T, K, 0, dev)
    nf = torch.full((B,), T, device=dev)
    for t in range(T):
        prev = beam_of(state)
        rows = np.concatenate([M.rows_of(refs[b][0], [(np.float64(s), tok) for s, tok in prev[b]], t, V)
                               for b in range(B)]).astype(np.float32)
        state.advance(torch.from_numpy(rows).to(dev), nf, 0.9, 0.1)
    tokens, lengths, scores = (t.cpu().numpy() for t in state.results(nbest=K))
    for b, (_, beam, tol, _) in enumerate(refs):
        for j, (s, tok) in enumerate(beam):
            if s > NINF:
                assert lengths[b, j] == len(tok) and tuple(tokens[b, j, :len(tok)]) == tok, (seeds[b], j)
                assert (tokens[b, j, len(tok):] == -1).all() and abs(float(scores[b, j]) - float(s)) <= tol
            else:
                assert lengths[b, j] == -1 and scores[b, j] == NINF and (tokens[b, j] == -1).all()


def snapshot(state):
    """What a search state means, as bytes: scores, frames, overflow flags and every slot's tokens.  (The blob itself
    also holds padding and the trie's table, whose slot numbers depend on which lane's insertion came first.)"""
    hyp, ln = state.hyps()
    return [t.cpu().numpy().tobytes() for t in (state.scores, state.frames, state.overflowed, hyp, ln)]


def fixed_logits(B, K, V, T, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return [(2.0 * torch.randn(B * K, V, generator=g)).to(dev) for _ in range(T)]


def test_state_handling_and_determinism(hip_device):
    from pika_amd import ModifiedBeamState
    B, K, V, T, dev = 4, 8, 37, 6, hip_device
    logits = fixed_logits(B, K, V, 9, 3, dev)
    nf = torch.tensor([9, 4, 0, 6], device=dev)

    def run():
        s = ModifiedBeamState(B, T, K, 0, dev)
        outs = [s.advance(l, nf) for l in logits]
        return s, outs
    s1, o1 = run()
    s2, o2 = run()
    assert snapshot(s1) == snapshot(s2)                            # bit-identical
    assert all(torch.equal(a, c) and torch.equal(p, q) for (a, p), (c, q) in zip(o1, o2))
    # num_frames > max_frames: frames stop at max_frames, overflowed is set, the state freezes
    assert s1.frames.tolist() == [6, 4, 0, 6] and s1.overflowed.tolist() == [True, False, False, False]
    ident = torch.arange(K, device=dev)
    assert torch.equal(o1[6][0][0], ident) and bool((o1[6][1][0] == 0).all())
    frozen = snapshot(s1)
    s1.advance(logits[0], nf)
    assert snapshot(s1) == frozen
    # an utterance of 0 frames never moves; every inactive one returns the identity
    assert torch.equal(o1[0][0][2], ident) and torch.equal(o1[5][0][1], ident)
    # reset(which): only the selected streams restart
    before = [t.clone() for t in s1.results(nbest=K)]
    s1.reset(which=torch.tensor([True, False, False, True]))
    after = s1.results(nbest=K)
    assert s1.frames.tolist() == [0, 4, 0, 0] and not s1.overflowed.any()
    for a, c in zip(before, after):
        assert torch.equal(a[1:3], c[1:3])
    assert after[1][0].tolist() == [0] + [-1] * (K - 1) and after[2][0].tolist() == [0.0] + [NINF] * (K - 1)
    # a restarted stream decodes as a fresh one
    s3 = ModifiedBeamState(B, T, K, 0, dev)
    for l in logits[:3]:
        s1.advance(l, torch.tensor([3, 0, 0, 0], device=dev))
        s3.advance(l, torch.tensor([3, 0, 0, 0], device=dev))
    assert all(torch.equal(a[0], c[0]) for a, c in zip(s1.results(nbest=K), s3.results(nbest=K)))
    # results(max_len) clips the tokens, not the lengths; hyps() is the same walk
    tok, ln, _ = s3.results(nbest=K, max_len=2)
    full, ln2, _ = s3.results(nbest=K)
    assert torch.equal(ln, ln2) and torch.equal(tok, full[:, :, :2]) and 1 <= int(ln.max()) <= 3
    h, hl = s3.hyps()
    assert torch.equal(h, full) and torch.equal(hl, ln2)


def test_captured_advance_equals_the_eager_loop(hip_device):
    from pika_amd import ModifiedBeamState
    B, K, V, T, dev = 3, 4, 67, 8, hip_device
    logits = fixed_logits(B, K, V, T, 11, dev)
    nf = torch.tensor([8, 5, 8], device=dev)
    eager = ModifiedBeamState(B, T, K, 1, dev)
    want = [eager.advance(l, nf, 0.9, 0.2) for l in logits]
    torch.cuda.synchronize()
    state = ModifiedBeamState(B, T, K, 1, dev)
    buf = torch.empty_like(logits[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = state.advance(buf, nf, 0.9, 0.2)
    for l, (p, t) in zip(logits, want):
        buf.copy_(l)
        g.replay()
        assert torch.equal(out[0], p) and torch.equal(out[1], t)
    assert snapshot(state) == snapshot(eager)


# ---- modified_beam_search on the tiny models -------------------------------------------------------------------------
def tiny(dec, device):
    import model_common as C
    import decode_common as D
    from oracle.pika_ref import seeded_state_dict
    from pika_amd.model import transducer, encoder
    net = C.build(transducer, encoder, dec)
    net.load_state_dict(seeded_state_dict(net, C.SEED))
    D.tweak(net)
    return net.eval().to(device), D.inputs()


def reference_search(net64, enc, x_len, K, sm_scale):
    """The float64 search per utterance on the model's own weights (CPU): prediction network and joint in float64 on
    `enc`, the encoder output (the encoder's kernels are float32 by construction) as float64."""
    out = []
    with torch.no_grad():
        rnn = net64.decoder_type == 'rnn'
        for b in range(enc.shape[0]):
            cache = {}

            def logits_of(tok, t, b=b, cache=cache):
                if tok not in cache:
                    seq = torch.tensor([[0] + list(tok)])
                    if rnn:
                        o, _ = net64.decoder(net64.embed(seq))
                        cache[tok] = o[0, -1]
                    else:
                        cache[tok] = net64.decoder(seq)[0, -1]
                z = torch.cat((enc[b, t], cache[tok]))
                h = torch.tanh(net64.fc1(z)) * torch.sigmoid(net64.fc_gate(z))
                return net64.fc2(h).numpy()
            beam, infos = M.search(logits_of, int(x_len[b]), net64.output_dim, K, 0, sm_scale, 0.0)
            out.append((beam, M.margins(infos, beam)))
    return out


@pytest.mark.parametrize("dec", ["rnn", "transformer"])
def test_modified_beam_search_on_the_tiny_models(hip_device, dec):
    from pika_amd import modified_beam_search
    net, (x, x_len) = tiny(dec, hip_device)
    xd = x.to(hip_device)
    K, sm = 4, 0.85
    runs = [modified_beam_search(net, xd, x_len, beam=K, nbest=K, sm_scale=sm, use_graph=g, precision="fp32")
            for g in (True, False)]
    for a, c in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a, c)                                    # graph and eager: bit-identical
    tokens, lengths, scores = (t.cpu().numpy() for t in runs[0][:3])
    assert runs[0][3].shape[:2] == (x.shape[0], 17)
    # against the float64 reference on the same weights; the tolerance is tests/test_decode.py's
    net64, _ = tiny(dec, "cpu")
    with torch.no_grad():
        enc64 = net64.encoder(x).double()
    ref = reference_search(net64.double(), enc64, x_len, K, sm)
    for b, (beam, margin) in enumerate(ref):
        got = {tuple(tokens[b, j, :lengths[b, j]]): scores[b, j] for j in range(K) if lengths[b, j] >= 0}
        for s, tok in beam:
            if tok in got:
                assert np.isclose(got[tok], float(s), rtol=1e-5, atol=1e-4), (dec, b, tok)
        if margin > 2e-4:                                           # wider than the score noise allowed above
            assert tuple(tokens[b, 0, :lengths[b, 0]]) == beam[0][1] and beam[0][1] in got, (dec, b)
    # beam = 1 is the per-frame arg-max
    t1, l1, s1, enc = modified_beam_search(net, xd, x_len, beam=1, nbest=1, sm_scale=sm, precision="fp32")
    ref1 = reference_search(net64, enc64, x_len, 1, sm)
    for b, (beam, margin) in enumerate(ref1):
        greedy, score = greedy_loop(net, enc[b], int(x_len[b]), sm)
        assert t1[b, 0, :int(l1[b, 0])].tolist() == greedy and abs(float(s1[b, 0]) - score) < 1e-4, (dec, b)
        if margin > 2e-4:
            assert tuple(greedy) == beam[0][1]


@torch.no_grad()
def greedy_loop(net, enc, T, sm_scale):
    """Modified greedy search in plain torch on the device: one arg-max per frame."""
    from pika_amd import gemm as G
    old, G.PRECISION = G.PRECISION, "fp32"
    try:
        rnn = net.decoder_type == 'rnn'
        hyp, score = [], 0.0

        def pred():
            seq = torch.tensor([[0] + hyp], device=enc.device)
            return net.decoder(net.embed(seq))[0][0, -1] if rnn else net.decoder(seq)[0, -1]
        p = pred()
        for t in range(T):
            z = torch.cat((enc[t], p)).unsqueeze(0)
            h = torch.tanh(net.fc1(z)) * torch.sigmoid(net.fc_gate(z))
            lp = torch.log_softmax(sm_scale * net.fc2(h)[0].double(), dim=-1)
            v = int(lp.argmax())
            score += float(lp[v])
            if v != 0:
                hyp.append(v)
                p = pred()
        return hyp, score
    finally:
        G.PRECISION = old


if __name__ == "__main__":      # the seeds the margin rule rejects, found on the CPU
    for cfg in sorted(E2E):
        print(cfg, rejected(*cfg))
