"""The streaming one-symbol-per-frame beam search on the device (include/pika_msearch_stream.h, csrc/msearch.hip):
`ModifiedBeamStream` around both states against the un-streamed device state, the forced commit against the definition,
the rebase against float64, a blob that was never reset, a captured chunk, and `ModifiedStreamDecoder` on the tiny model.

The plain cases' inputs are such that the CPU stream alone does not overflow under the case's commit schedule (asserted
on a CPU run of the same schedule).  The LM form has no CPU path: its cases assert the flag on the device run."""
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
import msearch_stream_common as S  # noqa: E402

pytestmark = pytest.mark.gpu
NINF = -np.inf
ROOT = 0x7ffffffe

# (V, K, max_frames, T) -> (the chunk; a commit follows every chunk, the scale of the model's table: 64 slots over 5
# classes hold every deviation of the last frames, and only a nearly flat table lets them die within 6 frames)
CASES = {(7, 4, 8, 40): (3, 0.3), (5, 64, 6, 24): (1, 0.05), (67, 16, 8, 32): (2, 0.3), (7, 1, 4, 20): (3, 0.3)}


def lens_of(T):
    return [T, 0, T - 7]


@pytest.mark.parametrize("V,K,mf,T", sorted(CASES))
def test_a_committing_stream_equals_the_one_shot_search(hip_device, V, K, mf, T):
    from pika_amd import ModifiedBeamState, ModifiedBeamStream
    (chunk, scale), lens = CASES[(V, K, mf, T)], lens_of(T)
    models = [S.PeakedModel(T, V, 40 + b, scale=scale) for b in range(3)]
    cpu = ModifiedBeamStream(3, mf, K, 0, device="cpu")                     # the condition of the case
    S.feed(cpu, models, lens, chunk, each_chunk=True, sm_scale=0.9, penalty=0.1)
    assert not cpu.overflowed.any()
    state = ModifiedBeamState(3, T, K, 0, hip_device)
    _, want = S.feed(state, models, lens, T, sm_scale=0.9, penalty=0.1)
    stream = ModifiedBeamStream(3, mf, K, 0, device=hip_device)
    ident = torch.arange(K, device=hip_device).repeat(3, 1)

    def after(obj, kind, out, committed):
        if kind == "commit":
            assert torch.equal(out[2], ident)
            assert torch.equal(obj.frames + obj.retired, obj.consumed)
    committed, trace = S.feed(stream, models, lens, chunk, each_chunk=True, sm_scale=0.9, penalty=0.1, after=after)
    assert not stream.overflowed.any() and not state.overflowed.any()
    S.same_trace(trace, want)                    # scores (bits), tokens, lengths, order, parent and token at every step
    assert stream.consumed.tolist() == lens and int(stream.retired.sum()) > 0
    assert (stream.offset == 0).all() and (stream.bonus_offset == 0).all()
    if K == 1:
        assert stream.frames.tolist() == [0, 0, 0] and (stream.hyps()[1] == 0).all()


@pytest.mark.parametrize("sched", ["five", "never"])
def test_the_other_commit_schedules_on_the_device(hip_device, sched):
    """(V, K, T) = (7, 4, 40) in chunks of 8 frames: a commit after every 5 frames (max_frames = 8), which falls in the
    middle of an offered chunk, and no commit at all (max_frames = 40)."""
    from pika_amd import ModifiedBeamState, ModifiedBeamStream
    V, K, T, chunk = 7, 4, 40, 8
    mf, every, lens = (8, 5, lens_of(T)) if sched == "five" else (T, None, lens_of(T))
    models = [S.PeakedModel(T, V, 40 + b) for b in range(3)]
    cpu = ModifiedBeamStream(3, mf, K, 0, device="cpu")                     # the condition of the case
    S.feed(cpu, models, lens, chunk, every, sm_scale=0.9, penalty=0.1)
    assert not cpu.overflowed.any()
    state = ModifiedBeamState(3, T, K, 0, hip_device)
    _, want = S.feed(state, models, lens, T, sm_scale=0.9, penalty=0.1)
    stream = ModifiedBeamStream(3, mf, K, 0, device=hip_device)
    commits = []
    committed, trace = S.feed(stream, models, lens, chunk, every, sm_scale=0.9, penalty=0.1,
                              after=lambda obj, kind, out, c: commits.append(kind) if kind == "commit" else None)
    assert not stream.overflowed.any()
    S.same_trace(trace, want)
    assert stream.consumed.tolist() == lens
    if sched == "five":
        assert len(commits) == T // 5 and int(stream.retired.sum()) > 0 and sum(map(len, committed)) > 0
    else:
        assert not commits and stream.retired.tolist() == [0, 0, 0] and stream.frames.tolist() == lens


# ---- which ------------------------------------------------------------------------------------------------------------
def regions(stream, b):
    """The bytes of the blob and of the side record that belong to stream b, as one list of byte strings: its rows of
    every head array, frames and overflowed, its table; retired, offset and bonus_offset."""
    s = stream.state
    B, K, raw = s.batch, s.beam, s._state
    BK = B * K
    sizes = (8, 4, 4, 4, 4, 4, 4) if stream.lm else (4, 4, 4)          # the head arrays' element sizes, in blob order
    out, at = [], 0
    for sz in sizes:
        out.append(raw[at + sz * K * b:at + sz * K * (b + 1)])
        at += sz * BK
    out += [raw[at + 4 * b:at + 4 * b + 4], raw[at + 4 * B + 4 * b:at + 4 * B + 4 * b + 4]]
    head = (at + 8 * B + 15) & ~15
    table = (raw.numel() - head) // B
    out.append(raw[head + table * b:head + table * (b + 1)])
    out += [stream.retired[b:b + 1], stream.offset[b:b + 1], stream.bonus_offset[b:b + 1]]
    return [t.cpu().numpy().tobytes() for t in out]


@pytest.mark.parametrize("with_lm", [False, True])
def test_which_leaves_the_other_streams_alone(hip_device, with_lm):
    from pika_amd import ModifiedBeamStream
    V, K, T0, dev = 7, 4, 12, hip_device
    models = [S.PeakedModel(T0, V, 40 + b, boost=10.0 if with_lm else 6.0) for b in range(3)]
    lm = automata("lm+hot", V, 5, dev)[0] if with_lm else None
    kw = dict(lm=lm, length_bonus=0.25, candidates=2 * K) if with_lm else {}
    some, every = (ModifiedBeamStream(3, T0, K, 0, device=dev, **kw) for _ in range(2))
    for s in (some, every):
        S.feed(s, models, [T0] * 3, T0)
    before = regions(some, 1)
    tails1 = [t.clone() for t in some.hyps()]
    tokens, lengths, slot_map = some.commit(which=[True, False, True], rebase=True, max_tail=1)
    full = every.commit(rebase=True, max_tail=1)
    assert regions(some, 1) == before                                   # blob and side record: byte for byte
    for a, c in zip(tails1, some.hyps()):
        assert torch.equal(a[1], c[1])
    assert int(lengths[1]) == 0 and bool((tokens[1] == -1).all()) and slot_map[1].tolist() == list(range(K))
    assert int(some.frames[1]) == T0 and int(every.frames[1]) < T0 and int(some.retired[1]) == 0
    for b in (0, 2):                                                    # the selected streams: as a commit of all
        assert torch.equal(tokens[b], full[0][b]) and lengths[b] == full[1][b] and torch.equal(slot_map[b], full[2][b])
        assert torch.equal(some.scores[b], every.scores[b]) and some.frames[b] == every.frames[b]
        assert some.retired[b] == every.retired[b] > 0 and some.offset[b] == every.offset[b] != 0
        assert some.bonus_offset[b] == every.bonus_offset[b]
        for a, c in zip(some.hyps(), every.hyps()):
            assert torch.equal(a[b], c[b])


# ---- the LM blob ------------------------------------------------------------------------------------------------------
def automata(kind, V, seed, dev):
    """-> (what the state takes as `lm`: one automaton, or two -- an n-gram LM and a compiled phrase list --, the
    reference automata, their weights)"""
    from pika_amd.ctc import CtcBiasedLm, CtcHotwords, CtcNgramLm
    ref = CL.make_lm(V, 0, seed, order=3)
    lm = CtcNgramLm(ref.fst, ref.backoff_id, ref.label_offset, dev)
    if kind == "lm":
        return lm, [ref], [ML.f32(0.5)]
    phrases = CB.seeded_phrases(V, 0, seed, 4)
    return (CtcBiasedLm(lm, CtcHotwords(phrases, V, 1.5, 0, dev), 1.25), [ref, CB.hot_lm(phrases, V, 1.5, 0)],
            [ML.f32(0.5), ML.f32(1.25)])


def lm_arrays(state):
    """bonus, am, lmst, lmst2 of the blob (the layout of include/pika_msearch_lm.h), as bytes per array."""
    BK, raw = state.batch * state.beam, state._state
    return [raw[a * BK:b * BK].cpu().numpy().tobytes() for a, b in ((0, 8), (12, 16), (24, 28), (28, 32))]


@pytest.mark.parametrize("kind", ["lm", "lm+hot"])
@pytest.mark.parametrize("double", [False, True])
def test_a_committing_lm_stream_equals_the_one_shot_search(hip_device, kind, double):
    from pika_amd import ModifiedBeamStream, ModifiedLmBeamState
    V, K, mf, T, chunk = 7, 4, 12, 24, 2
    C, lens, dev = (2 * K if double else K), lens_of(T), hip_device
    lm = automata(kind, V, 5, dev)[0]
    models = [S.PeakedModel(T, V, 60 + b, boost=10.0) for b in range(3)]
    rec = {"one": [], "stream": []}

    def recorder(name):
        def after(obj, kind_, out, committed):
            if kind_ != "step":
                return
            state = getattr(obj, "state", obj)
            entry = lm_arrays(state)
            for use_final in (True, False):
                tok, ln, sc, am = (t.cpu().numpy() for t in obj.results(nbest=K, use_final=use_final))
                entry.append([(tuple(committed[b]) + tuple(tok[b, j, :ln[b, j]]), sc[b, j].tobytes(), am[b, j].tobytes())
                              if ln[b, j] >= 0 else None for b in range(3) for j in range(K)])
            rec[name].append(entry)
        return after
    one = ModifiedLmBeamState(3, T, lm, K, 0, 0.5, 0.25, C, dev)
    _, want = S.feed(one, models, lens, T, sm_scale=0.9, penalty=0.1, after=recorder("one"))
    stream = ModifiedBeamStream(3, mf, K, 0, lm, 0.5, 0.25, C, dev)
    committed, trace = S.feed(stream, models, lens, chunk, each_chunk=True, sm_scale=0.9, penalty=0.1,
                              after=recorder("stream"))
    assert not stream.overflowed.any() and not one.overflowed.any()
    S.same_trace(trace, want)                                          # F, tokens, order, parent, token
    assert len(rec["one"]) == len(rec["stream"]) == T
    for i, (a, c) in enumerate(zip(rec["one"], rec["stream"])):       # bonus, am, both states, results with / without
        assert a == c, i
    assert stream.consumed.tolist() == lens and int(stream.retired.sum()) > 0 and sum(map(len, committed)) > 0


# ---- the forced commit -------------------------------------------------------------------------------------------------
def slots_of(stream):
    """Every array of the blob per slot, as the host sees it: (score, node, len[, am, bonus, lmst, lmst2])."""
    s = stream.state
    BK, B, K, raw = s.batch * s.beam, s.batch, s.beam, s._state
    if stream.lm:
        parts = [(8, 12, torch.float32), (16, 20, torch.int32), (20, 24, torch.int32), (12, 16, torch.float32),
                 (0, 8, torch.float64), (24, 28, torch.int32), (28, 32, torch.int32)]
    else:
        parts = [(0, 4, torch.float32), (4, 8, torch.int32), (8, 12, torch.int32)]
    return [raw[a * BK:b * BK].view(dt).view(B, K).cpu().numpy().copy() for a, b, dt in parts]


@pytest.mark.parametrize("with_lm", [0, 1, 2])
def test_forced_commit_follows_the_definition(hip_device, with_lm):
    """with_lm: 0 the plain blob; 1, 2 the LM blob with candidates = with_lm * K (the capacity rule divides by C)."""
    from pika_amd import ModifiedBeamStream
    V, K, B, T0, dev = 7, 4, 6, 12, hip_device
    m = 1 if with_lm else 2                        # max_tail (the LM's costs keep the sequences short)
    flat = [M.TableModel(T0, V, 70 + b, scale=1.0) for b in range(B)]
    kw = dict(lm=automata("lm+hot", V, 5, dev)[0], length_bonus=1.5, candidates=with_lm * K) if with_lm else {}
    stream = ModifiedBeamStream(B, T0, K, 0, device=dev, **kw)
    S.feed(stream, flat, [T0] * B, T0)
    before, arr0, frames = S.tails(stream), slots_of(stream), stream.frames.clone()
    tokens, lengths, slot_map = (t.cpu() for t in stream.commit(max_tail=m, max_len=5))
    after, arr1 = S.tails(stream), slots_of(stream)
    dropped = 0
    for b in range(B):
        best = before[b][0][1]
        live, common = [e[1] for e in before[b] if e], 0
        while all(len(q) > common and q[common] == best[common] for q in live):
            common += 1
        d = len(best) - m if len(best) - common > m else common
        assert lengths[b] == d and tuple(tokens[b, :min(d, 5)].tolist()) == best[:min(d, 5)]
        assert (tokens[b, min(d, 5):] == -1).all()
        keep = [k for k, e in enumerate(before[b]) if e and e[1][:d] == best[:d]]      # descend from the new root
        dropped += len(live) - len(keep)
        print("forced commit, stream %d: best %d labels, %d shared, %d committed, %d of %d slots stay"
              % (b, len(best), common, d, len(keep), len(live)))
        assert slot_map[b].tolist() == keep + list(range(len(keep), K))
        for j, k in enumerate(keep):                                   # the survivors: every array moved with the slot
            assert after[b][j][1] == before[b][k][1][d:]
            assert arr1[2][b, j] == arr0[2][b, k] - d
            for x0, x1 in zip(arr0[:1] + arr0[3:], arr1[:1] + arr1[3:]):
                assert x1[b, j].tobytes() == x0[b, k].tobytes()
        assert len(after[b][0][1]) <= m
        for j in range(len(keep), len(live)):                          # vacated: as a reset leaves an empty slot
            assert arr1[0][b, j] == NINF and arr1[1][b, j] == ROOT and arr1[2][b, j] == 0
            if with_lm:
                assert arr1[3][b, j] == NINF and arr1[4][b, j] == 0.0 and arr1[5][b, j] == 0 and arr1[6][b, j] == 0
        keys = len({q[d:i] for q in (before[b][k][1] for k in keep) for i in range(d + 1, len(q) + 1)})
        tail = max(len(before[b][k][1]) - d for k in keep)
        nsel = stream.state.candidates if with_lm else K
        assert int(stream.frames[b]) == min(int(frames[b]), max(-(-keys // nsel), tail))
    assert dropped > 0 and torch.equal(stream.frames + stream.retired, frames)
    # the stream goes on from the compacted beam: the next step is that of a state that holds the same beam
    S.feed(stream, flat, [T0] * B, T0)            # (nothing is offered beyond T0: inactive, the identity)
    assert [[e and e[1] for e in row] for row in S.tails(stream)] == [[e and e[1] for e in row] for row in after]


# ---- rebase -----------------------------------------------------------------------------------------------------------
def test_rebase_against_float64(hip_device):
    from pika_amd import ModifiedBeamStream
    V, K, mf, T, dev = 7, 4, 8, 40, hip_device
    seeds, used = (40, 41, 42), 0
    for seed in seeds:
        model = S.PeakedModel(T, V, seed)
        model32 = lambda tok, t: model(tok, t).astype(np.float32).astype(np.float64)   # noqa: E731  (what the device gets)
        beam, infos = M.search(model32, T, V, K, 0, 0.9, 0.1)
        ybeam, yinfos = M.search(model32, T, V, K, 0, 0.9, 0.1, np.float32)
        assert [tok for _, tok in beam] == [tok for _, tok in ybeam]
        yerr = max(abs(float(a) - float(c)) for (a, _), (c, _) in zip(beam, ybeam) if a > NINF)
        for i, y in zip(infos, yinfos):
            fin = i["cand"] > NINF
            yerr = max(yerr, float(np.max(np.abs(y["cand"][fin].astype(np.float64) - i["cand"][fin]))))
        tol = 2 * yerr
        if not M.margins(infos, beam) > 2 * tol:                       # the margin rule of tests/test_msearch_gpu.py
            continue
        used += 1
        stream = ModifiedBeamStream(1, mf, K, 0, device=dev)

        def after(obj, kind, out, committed):
            if kind == "commit" and bool(obj.scores[0, 0] > NINF):
                assert float(obj.scores[0, 0]) == 0.0
        committed, _ = S.feed(stream, [model], [T], 3, each_chunk=True, sm_scale=0.9, penalty=0.1,
                              commit=dict(rebase=True), after=after)
        assert not stream.overflowed.any() and float(stream.offset[0]) != 0.0
        off = float(stream.offset[0])
        for (s, tok), e in zip(beam, S.tails(stream)[0]):
            if s > NINF:
                assert tuple(committed[0]) + e[1] == tok
                print("rebase seed %d: |offset + score - float64| = %.3e (tol %.3e)" % (seed, abs(off + float(e[0]) - s), tol))
                assert abs(off + float(e[0]) - float(s)) <= tol
            else:
                assert e is None
        assert float(stream.scores[0, 0]) == 0.0 and abs(off - float(beam[0][0])) <= tol   # the magnitude is in the offset
    assert used >= 2


@pytest.mark.parametrize("kind", ["lm", "lm+hot"])
def test_lm_rebase_against_the_stream_without_it(hip_device, kind):
    """Two LM streams on the same peaked inputs, one committing with rebase and one without: tokens and order equal at
    every step, am + offset and F + offset + bonus_offset equal the un-rebased am and F within 2 x the error of the
    float32 yardstick (tests/msearch_lm_common.py) against float64 on the stream's inputs, for the streams whose float64
    run leaves a margin above twice that (the margin rule); slot 0 holds am = bonus = F = 0 right after a commit."""
    from pika_amd import ModifiedBeamStream
    V, K, C, mf, T, chunk, dev = 7, 4, 8, 12, 24, 2, hip_device
    lens, lb = lens_of(T), 0.25
    lm, refs, weights = automata(kind, V, 5, dev)
    models = [S.PeakedModel(T, V, 60 + b, boost=10.0) for b in range(3)]
    tol = {}
    for b in (0, 2):
        m32 = lambda tok, t, m=models[b]: m(tok, t).astype(np.float32).astype(np.float64)   # noqa: E731
        beam, infos = ML.search(m32, lens[b], V, K, C, refs, weights, lb, 0, 0.9, 0.1)
        ybeam, yinfos = ML.search(m32, lens[b], V, K, C, refs, weights, lb, 0, 0.9, 0.1, np.float32)
        yerr = ML.yardstick_error(infos, yinfos, beam, ybeam)
        if ML.margins(infos, ML.results(beam, refs, weights, use_final=False)) > 4 * yerr:
            tol[b] = 2 * yerr
    assert tol, "the margin rule rejected every stream"

    def bonus_of(stream):
        BK = stream.batch * K
        return stream.state._state[:8 * BK].view(torch.float64).view(stream.batch, K)
    plain = ModifiedBeamStream(3, mf, K, 0, lm, 0.5, lb, C, dev)
    _, want = S.feed(plain, models, lens, chunk, each_chunk=True, sm_scale=0.9, penalty=0.1)
    based = ModifiedBeamStream(3, mf, K, 0, lm, 0.5, lb, C, dev)
    seen = []

    def after(obj, kind_, out, committed):
        if kind_ != "commit":
            return
        live = obj.scores[:, 0] > NINF
        assert bool((obj.scores[live, 0] == 0).all()) and bool((obj.state.am_scores[live, 0] == 0).all())
        assert bool((bonus_of(obj)[live, 0] == 0).all())
        seen.append(obj.bonus_offset.clone())
    committed, got = S.feed(based, models, lens, chunk, each_chunk=True, sm_scale=0.9, penalty=0.1,
                            commit=dict(rebase=True), after=after)
    assert not plain.overflowed.any() and not based.overflowed.any() and (plain.offset == 0).all()
    assert len(got) == len(want)
    for b in tol:                                                       # tokens and order, step by step
        for i, (g, w) in enumerate(zip(got, want)):
            assert [e and e[1] for e in g[2][b]] == [e and e[1] for e in w[2][b]], (b, i)
            assert (g[0][b] == w[0][b]).all() and (g[1][b] == w[1][b]).all(), (b, i)
    off, boff = based.offset.unsqueeze(1), based.bonus_offset.unsqueeze(1)
    am = (based.state.am_scores.double() + off).cpu().numpy()
    F = (based.scores.double() + off + boff).cpu().numpy()
    bonus = (bonus_of(based) + boff).cpu().numpy()
    am0, F0, bonus0 = plain.state.am_scores.cpu().numpy(), plain.scores.cpu().numpy(), bonus_of(plain).cpu().numpy()
    for b, t in tol.items():
        live = F0[b] > NINF
        assert live.any() and (np.isfinite(F[b]) == live).all()
        print("lm rebase %s stream %d: |am| %.3e |F| %.3e |bonus| %.3e (tol %.3e); offset %.4f bonus_offset %.4f" % (
            kind, b, np.abs(am[b] - am0[b])[live].max(), np.abs(F[b] - F0[b])[live].max(),
            np.abs(bonus[b] - bonus0[b])[live].max(), t, float(based.offset[b]), float(based.bonus_offset[b])))
        assert np.abs(am[b] - am0[b])[live].max() <= t and np.abs(F[b] - F0[b])[live].max() <= t
        assert np.abs(bonus[b] - bonus0[b])[live].max() <= 1e-9         # (fp64 sums of a few dozen terms below 100)
        assert float(based.offset[b]) != 0.0 and float(based.bonus_offset[b]) != 0.0
        assert float(based.offset[b]) != float(based.bonus_offset[b])
    assert float(based.offset[1]) == 0.0 and float(based.bonus_offset[1]) == 0.0      # the stream of no frames
    assert any(bool((s[[0, 2]] != 0).all()) for s in seen)              # a nonzero bonus_offset right after a commit


# ---- a blob that was never reset ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xff, 0x3f])
@pytest.mark.parametrize("with_lm", [False, True])
def test_commit_on_a_blob_that_was_never_reset_stays_inside(hip_device, with_lm, fill):
    """One launch (max_tail = 1, rebase) on garbage DATA, per fill: 0xff bytes (no live slot, frames = -1), or 0x3f bytes
    (every slot live with the same node, len and frames far beyond max_frames, every key its own parent).  Every index
    is clamped by construction; the call returns and writes only inside its blob and its outputs (guard words around
    each)."""
    from pika_amd import _lib
    lib, dev = _lib.lib(), hip_device
    B, K, C, mf, L, G = 2, 64, 64, 5, 7, 256
    nstate = lib.pika_msearch_lm_state_bytes(B, K, C, mf) if with_lm else lib.pika_msearch_state_bytes(B, K, mf)
    sizes = [nstate, lib.pika_msearch_stream_side_bytes(B), 8 * B * L, 8 * B, 8 * B * K,
             lib.pika_msearch_commit_scratch_bytes(B, K, mf)]
    bufs = [torch.full((n + 2 * G,), 0x5a, dtype=torch.uint8, device=dev) for n in sizes]
    bufs[0][G:G + nstate] = fill
    bufs[1][G:G + sizes[1]] = 0
    state, side, tokens, lengths, slot_map, scratch = (b.data_ptr() + G for b in bufs)
    stream = torch.cuda.current_stream().cuda_stream
    if with_lm:
        rc = lib.pika_msearch_lm_commit(state, side, B, K, C, mf, None, 1, 1, L, tokens, lengths, slot_map, scratch,
                                        stream)
    else:
        rc = lib.pika_msearch_commit(state, side, B, K, mf, None, 1, 1, L, tokens, lengths, slot_map, scratch, stream)
    assert rc == 0
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:G] == 0x5a).all()) and bool((b[-G:] == 0x5a).all())
    ln = bufs[3][G:G + 8 * B].view(torch.int64)
    sm = bufs[4][G:G + 8 * B * K].view(torch.int64)
    assert bool(((ln >= 0) & (ln <= mf)).all()) and bool(((sm >= 0) & (sm < K)).all())


# ---- a captured chunk --------------------------------------------------------------------------------------------------
def test_captured_chunk_and_commit_equal_the_eager_loop(hip_device):
    from pika_amd import ModifiedBeamStream
    B, K, V, mf, dev, chunk, reps = 3, 4, 67, 16, hip_device, 4, 6
    g = torch.Generator().manual_seed(21)
    logits = [(0.5 * torch.randn(B * K, V, generator=g)) for _ in range(chunk * reps)]
    for t, l in enumerate(logits):
        l[:, (7 * t) % V] += 5.0                   # a dominant class per frame
    logits = [l.to(dev) for l in logits]
    ends = torch.tensor([24, 9, 17], device=dev)

    def snap(stream, out):
        hyp, ln = stream.hyps()
        return [t.cpu().numpy().tobytes() for t in (stream.scores, stream.frames, stream.retired, stream.overflowed,
                                                    stream.offset, hyp, ln) + tuple(out)]

    def body(stream, bufs, nf):
        outs = [stream.advance(l, nf, 0.9, 0.2) for l in bufs]
        return outs, stream.commit(max_tail=3, rebase=True)
    eager, want = ModifiedBeamStream(B, mf, K, 1, device=dev), []
    for r in range(reps):
        nf = torch.minimum(ends, torch.tensor(chunk * (r + 1), device=dev))
        outs, com = body(eager, logits[chunk * r:chunk * (r + 1)], nf)
        want.append(snap(eager, [t for o in outs for t in o] + list(com)))
    torch.cuda.synchronize()
    assert not eager.overflowed.any() and int(eager.retired.sum()) > 0
    stream = ModifiedBeamStream(B, mf, K, 1, device=dev)
    bufs = [torch.empty_like(logits[0]) for _ in range(chunk)]
    nf = torch.zeros(B, dtype=torch.int64, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs, com = body(stream, bufs, nf)
    stream.reset()                                 # (a capture runs nothing; all the same: from the start)
    for r in range(reps):
        for buf, l in zip(bufs, logits[chunk * r:chunk * (r + 1)]):
            buf.copy_(l)
        nf.copy_(torch.minimum(ends, torch.tensor(chunk * (r + 1), device=dev)))
        graph.replay()
        assert snap(stream, [t for o in outs for t in o] + list(com)) == want[r], r


# ---- ModifiedStreamDecoder on the tiny model ---------------------------------------------------------------------------
def tiny(dec, device):
    import model_common as C
    import decode_common as D
    from oracle.pika_ref import seeded_state_dict
    from pika_amd.model import transducer, encoder
    net = C.build(transducer, encoder, dec)
    net.load_state_dict(seeded_state_dict(net, C.SEED))
    D.tweak(net)
    return net.eval().to(device), D.inputs()


def float64_margins(net64, enc, x_len, K, sm_scale):
    """Per utterance the float64 search on the model's own weights (CPU) -> (best tokens, its smallest margin)."""
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
            beam, infos = M.search(logits_of, int(x_len[b]), net64.output_dim, K, 0, sm_scale, 0.0)
            out.append((beam[0][1], M.margins(infos, beam)))
    return out


def test_stream_decoder_on_the_tiny_model(hip_device):
    from pika_amd import ModifiedStreamDecoder, modified_beam_search
    net, (x, x_len) = tiny("rnn", hip_device)
    K, sm, dev = 4, 0.85, hip_device
    tokens, lengths, scores, enc = modified_beam_search(net, x.to(dev), x_len, beam=K, nbest=K, sm_scale=sm,
                                                        use_graph=False, precision="fp32")
    tokens, lengths, scores = (t.cpu().numpy() for t in (tokens, lengths, scores))
    B, T = enc.shape[:2]
    net64, _ = tiny("rnn", "cpu")
    with torch.no_grad():
        enc64 = net64.encoder(x).double()
    ref = float64_margins(net64.double(), enc64, x_len, K, sm)
    xl = torch.as_tensor(x_len).to(dev).long().clamp(0, T)
    for chunk in (1, 5, 17):
        dec = ModifiedStreamDecoder(net, B, 24, beam=K, sm_scale=sm, precision="fp32")
        for start in range(0, T, chunk):
            piece = enc[:, start:start + chunk]
            dec.advance(piece, (xl - start).clamp(0, piece.shape[1]))
            dec.commit()
        assert not dec.stream.overflowed.any() and torch.equal(dec.stream.consumed.long(), xl)
        ctok, clen, ttok, tlen, tsc = (t.cpu().numpy() for t in dec.results(nbest=K))
        print("stream decoder, chunks of %d: committed %s of %s labels" % (chunk, clen.tolist(), lengths[:, 0].tolist()))
        for b in range(B):
            got = {tuple(ctok[b, :clen[b]]) + tuple(ttok[b, j, :tlen[b, j]]): tsc[b, j] for j in range(K) if tlen[b, j] >= 0}
            want = {tuple(tokens[b, j, :lengths[b, j]]): scores[b, j] for j in range(K) if lengths[b, j] >= 0}
            for tok, s in want.items():
                if tok in got:
                    assert np.isclose(got[tok], s, rtol=1e-5, atol=1e-4), (chunk, b, tok)
            if ref[b][1] > 2e-4:
                first = tuple(ctok[b, :clen[b]]) + tuple(ttok[b, 0, :tlen[b, 0]])
                assert first == tuple(tokens[b, 0, :lengths[b, 0]]) == ref[b][0], (chunk, b)
                assert first in got and np.isclose(tsc[b, 0], scores[b, 0], rtol=1e-5, atol=1e-4), (chunk, b)
                assert set(got) == set(want), (chunk, b)               # the same hypotheses: all of them were compared
        dec.reset(which=[True] + [False] * (B - 1))                    # the selected stream starts over
        assert dec.stream.consumed.tolist()[0] == 0 and dec.results()[1].tolist()[0] == 0
        assert dec.stream.consumed.tolist()[1:] == xl.tolist()[1:]
    # forced commits drop slots: afterwards slot j's (h, c) is the LSTM's state on [blank] + committed + tail j, which
    # holds only if the state was re-ordered by slot_map (and by parent) at every turn
    dec = ModifiedStreamDecoder(net, B, 24, beam=K, sm_scale=sm, precision="fp32")
    moved = 0
    for start in range(0, T, 5):
        piece = enc[:, start:start + 5]
        dec.advance(piece, (xl - start).clamp(0, piece.shape[1]))
        slot_map = dec.commit(max_tail=1)[2]
        moved += int((slot_map != torch.arange(K, device=dev)).sum())
    ctok, clen, ttok, tlen, _ = (t.cpu().numpy() for t in dec.results(nbest=K))
    assert moved > 0 and int(clen.sum()) > 0
    from pika_amd import gemm as G
    old, G.PRECISION = G.PRECISION, "fp32"
    try:
        with torch.no_grad():
            for b in range(B):
                for j in range(K):
                    if tlen[b, j] >= 0:
                        seq = [0] + list(ctok[b, :clen[b]]) + list(ttok[b, j, :tlen[b, j]])
                        _, (h, c) = net.decoder(net.embed(torch.tensor([seq], device=dev)))
                        assert torch.allclose(h[:, 0], dec._pred[0][:, b * K + j], rtol=1e-5, atol=1e-5), (b, j)
                        assert torch.allclose(c[:, 0], dec._pred[1][:, b * K + j], rtol=1e-5, atol=1e-5), (b, j)
    finally:
        G.PRECISION = old
    net_t, _ = tiny("transformer", "cpu")
    with pytest.raises(NotImplementedError):
        ModifiedStreamDecoder(net_t, B, 24)
