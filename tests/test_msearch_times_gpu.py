"""GPU tests of the time stamps of the one-symbol-per-frame beam search (include/pika_msearch_times.h).  The record is an
integer function of the (parent, token) pairs the search's kernels emit, so it is compared with the pure-Python replay
of those pairs (tests/msearch_times_common.py) as integers, after every step and every commit."""
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
import msearch_times_common as TC  # noqa: E402

pytestmark = pytest.mark.gpu
NINF = -np.inf


def automata(kind, V, seed, dev):
    """What a state takes as `lm`: an n-gram LM, or that and a compiled phrase list."""
    from pika_amd.ctc import CtcBiasedLm, CtcHotwords, CtcNgramLm
    ref = CL.make_lm(V, 0, seed, order=3)
    lm = CtcNgramLm(ref.fst, ref.backoff_id, ref.label_offset, dev)
    if kind == "lm":
        return lm
    return CtcBiasedLm(lm, CtcHotwords(CB.seeded_phrases(V, 0, seed, 4), V, 1.5, 0, dev), 1.25)


def record_bytes(times):
    """Every byte of the record that the layout names: seen, lost, cur and the two planes (not the head's padding)."""
    raw, B = times._rec.cpu().numpy(), times.batch
    return raw[:12 * B].tobytes() + raw[(12 * B + 15) & ~15:].tobytes()


# ---- 6: exact replay ---------------------------------------------------------------------------------------------------
# (B, K, V, T, max_frames, model): greedy; a beam that is no power of two; the full wave with heavy merging; an odd
# max_frames below T (utterance 0 overflows: its record stays as it was); the wide rows; len across 64 and 256
PLAIN = [(3, 1, 7, 20, 20, "peaked"), (3, 3, 5, 40, 40, "table"), (2, 64, 5, 40, 40, "flat"), (3, 3, 5, 40, 37, "table"),
         (2, 4, 8200, 6, 6, "frame"), (1, 4, 6, 300, 300, "dense")]


def models_of(kind, B, V, T):
    if kind == "peaked":
        return [S.PeakedModel(T, V, 40 + b) for b in range(B)]
    if kind == "table":
        return [M.TableModel(T, V, 50 + b) for b in range(B)]
    if kind == "flat":
        return [M.TableModel(T, V, 60 + b, scale=0.05) for b in range(B)]
    if kind == "frame":
        return [TC.FrameModel(T, V, 70 + b) for b in range(B)]
    return [S.PeakedModel(T, V, 80 + b, p_blank=0.08) for b in range(B)]


def ragged(B, T):
    return [T, 0, T // 2][:B] if B == 3 else ([T, T // 2] if B == 2 else [T])


@pytest.mark.parametrize("B,K,V,T,mf,kind", PLAIN)
def test_the_record_equals_the_replay_after_every_step(hip_device, B, K, V, T, mf, kind):
    from pika_amd import ModifiedBeamState, ModifiedBeamTimes
    lens = ragged(B, T)
    state = ModifiedBeamState(B, mf, K, 0, hip_device)
    tr = TC.Tracker(ModifiedBeamTimes(state))
    S.feed(state, models_of(kind, B, V, T), lens, T, sm_scale=0.9, penalty=0.1, after=tr)   # compares after every step
    assert tr.n == T and tr.ref.consumed == [min(n, mf) for n in lens] and not tr.times.lost.any()
    assert state.overflowed.tolist() == [n > mf for n in lens]
    ln = state.hyps()[1]
    assert int(ln.max()) > 0
    if kind == "dense":
        assert int(ln.max()) > 256
    if kind == "flat":
        assert sum(1 for h in tr.history if len(set(h[1][0].tolist())) < K) > 0       # slots shared parents: merges


@pytest.mark.parametrize("kind", ["lm", "lm+hot"])
@pytest.mark.parametrize("double", [False, True])
def test_the_lm_search_record_equals_the_replay_and_results_find_their_slots(hip_device, kind, double):
    from pika_amd import ModifiedBeamTimes, ModifiedLmBeamState
    V, K, T, dev = 7, 4, 24, hip_device
    C, lens = (2 * K if double else K), [T, 0, T - 7]
    state = ModifiedLmBeamState(3, T, automata(kind, V, 5, dev), K, 0, 0.5, 0.25, C, dev)
    tr = TC.Tracker(ModifiedBeamTimes(state))
    S.feed(state, [S.PeakedModel(T, V, 60 + b, boost=10.0) for b in range(3)], lens, T, sm_scale=0.9, penalty=0.1,
           after=tr)
    assert tr.n == T and not tr.times.lost.any()
    entries_of(state, tr.times, dict(use_final=True), dict(use_final=False))


def entries_of(state, times, *kws):
    """7: results by entry == the record of the slot whose hyps() row is the entry; a missing entry and an entry longer
    than L give -1."""
    K = state.beam
    htok, hlen = (t.cpu().numpy() for t in state.hyps())
    rows = times.hyps().cpu().numpy()
    slot = [{tuple(htok[b, k, :hlen[b, k]]): k for k in range(K) if hlen[b, k] >= 0} for b in range(state.batch)]
    found = missing = cut = 0
    for kw in kws:
        for L in (None, 2):
            out = state.results(nbest=K, max_len=L, **kw)
            got = times.results(out[0], out[1]).cpu().numpy()
            tok, ln = out[0].cpu().numpy(), out[1].cpu().numpy()
            assert got.shape == tok.shape
            for b in range(state.batch):
                for e in range(K):
                    n = ln[b, e]
                    if n < 0:
                        missing += 1
                        assert (got[b, e] == -1).all()
                    elif n > tok.shape[2]:
                        cut += 1
                        assert (got[b, e] == -1).all()
                    else:
                        found += 1
                        k = slot[b][tuple(tok[b, e, :n])]
                        assert got[b, e, :n].tolist() == rows[b, k, :n].tolist() and (got[b, e, n:] == -1).all()
    assert found > 0 and missing > 0 and cut > 0


def test_plain_results_by_entry(hip_device):
    from pika_amd import ModifiedBeamState, ModifiedBeamTimes
    V, K, T = 7, 4, 24
    state = ModifiedBeamState(3, T, K, 0, hip_device)
    tr = TC.Tracker(ModifiedBeamTimes(state), check=False)
    S.feed(state, [S.PeakedModel(T, V, 60 + b) for b in range(3)], [T, 0, T - 7], T, after=tr)
    entries_of(state, tr.times, {})


# ---- 8: the record names a path of the lattice ---------------------------------------------------------------------------
def path_case(K, V=5, T=12):
    """The first seed whose float64 search keeps a margin above 2 tol, tol = 2 x the error of the float32 yardstick."""
    for seed in range(10):
        model = M.TableModel(T, V, 31 * seed + K)
        model32 = lambda tok, t, m=model: m(tok, t).astype(np.float32).astype(np.float64)      # noqa: E731
        beam, infos = M.search(model32, T, V, K, 0, 0.9, 0.1)
        ybeam, yinfos = M.search(model32, T, V, K, 0, 0.9, 0.1, np.float32)
        if [tok for _, tok in beam] != [tok for _, tok in ybeam]:
            continue
        yerr = max(abs(float(a) - float(c)) for (a, _), (c, _) in zip(beam, ybeam) if a > NINF)
        for i, y in zip(infos, yinfos):
            fin = i["cand"] > NINF
            yerr = max(yerr, float(np.max(np.abs(y["cand"][fin].astype(np.float64) - i["cand"][fin]))))
        if M.margins(infos, beam) > 4 * yerr:
            return model32, beam, 2 * yerr
    raise AssertionError("no seed with a margin")


@pytest.mark.parametrize("K", [1, 4, 16])
def test_the_times_are_a_path_of_the_lattice_below_the_score(hip_device, K):
    from pika_amd import ModifiedBeamState, ModifiedBeamTimes
    V, T = 5, 12
    model32, beam, tol = path_case(K)
    state = ModifiedBeamState(1, T, K, 0, hip_device)
    tr = TC.Tracker(ModifiedBeamTimes(state), check=False)
    S.feed(state, [type("W", (), {"V": V, "__call__": staticmethod(model32)})()], [T], T, sm_scale=0.9, penalty=0.1,
           after=tr)
    tok, ln, sc = (t.cpu().numpy() for t in state.results(nbest=K))
    got = tr.times.results(*state.results(nbest=K)[:2]).cpu().numpy()
    for j, (s, want) in enumerate(beam):
        if not s > NINF:
            continue
        n = ln[0, j]
        assert tuple(tok[0, j, :n]) == want
        value = TC.path_value(model32, want, got[0, j, :n], T, 0, 0.9, 0.1)      # increasing, in [0, T), one per label
        print("msearch times path K=%d entry %d: path %.6f score %.6f tol %.2e" % (K, j, value, sc[0, j], tol))
        assert value <= float(sc[0, j]) + tol
        if K == 1:
            assert abs(value - float(sc[0, j])) <= tol


# ---- 9: streams ----------------------------------------------------------------------------------------------------------
SCHEDULES = {"chunk1": dict(chunk=1, each_chunk=True), "chunk3": dict(chunk=3, each_chunk=True),
             "five": dict(chunk=8, every=5), "tail0": dict(chunk=3, each_chunk=True, commit=dict(max_tail=0)),
             "tail2": dict(chunk=8, every=5, commit=dict(max_tail=2)),
             "never1": dict(chunk=1), "never3": dict(chunk=3), "never8": dict(chunk=8)}


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("K,with_lm", [(4, False), (16, False), (4, True), (16, True)])
def test_streams_under_every_schedule(hip_device, K, with_lm, sched):
    from pika_amd import ModifiedBeamState, ModifiedBeamStream, ModifiedBeamTimes, ModifiedLmBeamState
    V, T, dev, kw = 7, 40, hip_device, SCHEDULES[sched]
    lens = [T, 0, T - 7]
    mods = [S.PeakedModel(T, V, 40 + b, boost=10.0 if with_lm else 6.0, scale=0.3 if K == 4 else 0.1) for b in range(3)]
    lm = automata("lm+hot", V, 5, dev) if with_lm else None
    skw = dict(lm=lm, length_bonus=0.25, candidates=2 * K) if with_lm else {}
    mf = 40
    if sched in ("chunk1", "chunk3", "five", "tail0", "tail2"):          # max_frames = 8 where the schedule fits
        cpu = ModifiedBeamStream(3, 8, K, 0, device="cpu")
        S.feed(cpu, mods, lens, **kw)
        if not with_lm and not cpu.overflowed.any():
            mf = 8
    stream = ModifiedBeamStream(3, mf, K, 0, device=dev, **skw)
    tr = TC.Tracker(ModifiedBeamTimes(stream))
    # the tracker asserts after every step and commit: record == replay on the live slots, committed ++ any live tail
    # strictly increasing, every commit's output == the definition on the record read just before it
    committed, _ = S.feed(stream, mods, lens, after=tr, sm_scale=0.9, penalty=0.1, **kw)
    assert not stream.overflowed.any() and not tr.times.lost.any() and stream.consumed.tolist() == lens
    assert [len(c) for c in committed] == [len(c) for c in tr.committed]
    if sched.startswith("never"):
        assert not tr.commits
        one = (ModifiedLmBeamState(3, T, lm, K, 0, 0.5, 0.25, 2 * K, dev) if with_lm
               else ModifiedBeamState(3, T, K, 0, dev))
        tr1 = TC.Tracker(ModifiedBeamTimes(one), check=False)
        S.feed(one, mods, lens, T, sm_scale=0.9, penalty=0.1, after=tr1)
        assert record_bytes(tr.times) == record_bytes(tr1.times)         # any chunking: the one-shot record's bytes
        assert torch.equal(tr.times.hyps(), tr1.times.hyps())
    else:
        assert tr.commits and sum(map(len, tr.committed)) > 0


@pytest.mark.parametrize("with_lm", [False, True])
def test_which_leaves_the_other_streams_records_alone(hip_device, with_lm):
    from pika_amd import ModifiedBeamStream, ModifiedBeamTimes
    V, K, T0, dev = 7, 4, 12, hip_device
    mods = [S.PeakedModel(T0, V, 40 + b, boost=10.0 if with_lm else 6.0) for b in range(3)]
    skw = dict(lm=automata("lm+hot", V, 5, dev), length_bonus=0.25, candidates=2 * K) if with_lm else {}
    stream = ModifiedBeamStream(3, T0, K, 0, device=dev, **skw)
    tr = TC.Tracker(ModifiedBeamTimes(stream), check=False)
    S.feed(stream, mods, [T0] * 3, T0, after=tr)
    times, B = tr.times, 3

    def part(b):
        raw, n = times._rec, 4 * K * T0
        head = (12 * B + 15) & ~15
        return [raw[o + 4 * b:o + 4 * b + 4].cpu().numpy().tobytes() for o in (0, 4 * B, 8 * B)] + \
            [raw[head + p * B * n + b * n:head + p * B * n + (b + 1) * n].cpu().numpy().tobytes() for p in (0, 1)]
    before, rows = part(1), times.hyps()
    which = [True, False, True]
    tokens, lengths, slot_map = stream.commit(which=which, max_tail=1)
    when = times.commit(lengths, slot_map, which)
    assert part(1) == before and (when[1] == -1).all() and int(lengths[0]) > 0 and (when[0, :int(lengths[0])] >= 0).all()
    assert torch.equal(times.hyps()[1], rows[1])
    stream.reset(which)
    times.reset(which)
    assert part(1) == before and torch.equal(times.hyps()[1], rows[1])
    assert (times.hyps()[0] == -1).all() and times._seen.tolist() == [0, T0, 0]


# ---- 10: lost records ----------------------------------------------------------------------------------------------------
def test_lost_records(hip_device):
    from pika_amd import ModifiedBeamState, ModifiedBeamTimes
    V, K, T, dev = 5, 3, 12, hip_device
    mods = [S.PeakedModel(T, V, 10 + b, p_blank=0.1) for b in range(3)]
    state = ModifiedBeamState(3, T, K, 0, dev)
    tr = TC.Tracker(ModifiedBeamTimes(state), check=False, skip=(4,))
    S.feed(state, mods, [T, 4, T], T, after=tr)          # utterance 1 was inactive at the skipped step: it is not lost
    times = tr.times
    assert times.lost.tolist() == [True, False, True]
    hyps, ln = times.hyps().cpu().numpy(), state.hyps()[1].cpu().numpy()
    assert (hyps[0] == -1).all() and (hyps[2] == -1).all() and (hyps[1] >= 0).any()
    for k, r in enumerate(tr.ref.rows[1]):
        if ln[1, k] >= 0:
            assert hyps[1, k].tolist() == r + [-1] * (T - len(r))
    tok, n, _ = state.results(nbest=K)
    got = times.results(tok, n)
    assert (got[0] == -1).all() and (got[2] == -1).all() and torch.equal(got[1], times.hyps()[1])
    times.reset([True, False, False])
    assert times.lost.tolist() == [False, False, True]
    # the state reset without the record: lost at the next step, for that utterance only
    state = ModifiedBeamState(2, T, K, 0, dev)
    tr = TC.Tracker(ModifiedBeamTimes(state), check=False)
    S.feed(state, mods[:2], [6, 6], 6, after=tr)
    state.reset([True, False])
    nf = torch.tensor([7, 7], device=dev)
    parent, token = state.advance(torch.randn(2 * K, V, device=dev), nf)
    tr.times.step(parent, token)
    assert tr.times.lost.tolist() == [True, False] and (tr.times.hyps()[0] == -1).all()
    assert tr.times._seen.tolist() == [6, 7]


# ---- 11: guard words -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xff, 0x3f])
@pytest.mark.parametrize("with_lm", [False, True])
def test_records_and_blobs_that_were_never_reset_stay_inside(hip_device, with_lm, fill):
    """Garbage DATA in the record and in the blob (0xff: no live slot, cur = -1, len = -1; 0x3f: every slot live, len and
    frames far beyond max_frames), garbage parent / token / lengths / slot_map: every index is clamped, the calls return
    and write only inside the record and their outputs (guard words around each)."""
    from pika_amd import _lib
    lib, dev = _lib.lib(), hip_device
    B, K, mf, L, G = 2, 64, 5, 7, 256
    C = 64 if with_lm else 0
    nstate = lib.pika_msearch_lm_state_bytes(B, K, C, mf) if with_lm else lib.pika_msearch_state_bytes(B, K, mf)
    ntimes = lib.pika_msearch_times_bytes(B, K, mf)
    sizes = [nstate, ntimes, lib.pika_msearch_stream_side_bytes(B), 8 * B * K, 8 * B * K, 8 * B * K * L, 8 * B * K * L,
             8 * B * K, 8 * B * K * L, 8 * B, 8 * B * L]
    bufs = [torch.full((n + 2 * G,), 0x5a, dtype=torch.uint8, device=dev) for n in sizes]
    for i in (0, 1, 3, 4, 6, 7, 9):                 # state, record, parent, token, tokens, lengths (B,K), lengths (B,)
        bufs[i][G:G + sizes[i]] = fill
    bufs[2][G:G + sizes[2]] = 0
    state, times, side, parent, token, hyp, tokens, lengths, out, clen, cout = (b.data_ptr() + G for b in bufs)
    stream = torch.cuda.current_stream().cuda_stream
    state0 = bufs[0].clone()
    for cur_seen in (None, 1):                      # as filled; then with seen = consumed - 1, so that the step copies
        if cur_seen is not None:
            frames_at = (32 if with_lm else 12) * B * K
            frames = bufs[0][G + frames_at:G + frames_at + 4 * B].view(torch.int32)
            bufs[1][G:G + 4 * B].view(torch.int32).copy_(frames - 1)
            bufs[1][G + 4 * B:G + 8 * B] = 0
        assert lib.pika_msearch_times_step(times, state, side, B, K, C, mf, parent, token, 0, stream) == 0
        assert lib.pika_msearch_times_hyps(times, state, B, K, C, mf, L, hyp, stream) == 0
        assert lib.pika_msearch_times_results(times, state, B, K, C, mf, K, L, tokens, lengths, out, stream) == 0
        assert lib.pika_msearch_times_commit(times, state, B, K, C, mf, None, clen, parent, L, cout, stream) == 0
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b[:G] == 0x5a).all()) and bool((b[-G:] == 0x5a).all())
        assert torch.equal(bufs[0], state0)         # the blob is only read


# ---- 12: graph capture ---------------------------------------------------------------------------------------------------
def test_captured_steps_and_commit_equal_the_eager_loop(hip_device):
    from pika_amd import ModifiedBeamStream, ModifiedBeamTimes
    B, K, V, mf, dev, chunk, reps = 3, 4, 67, 16, hip_device, 4, 6
    g = torch.Generator().manual_seed(21)
    logits = [(0.5 * torch.randn(B * K, V, generator=g)) for _ in range(chunk * reps)]
    for t, l in enumerate(logits):
        l[:, (7 * t) % V] += 5.0                   # a dominant class per frame
    logits = [l.to(dev) for l in logits]
    ends = torch.tensor([24, 9, 17], device=dev)

    def snap(stream, times, when):
        return [t.cpu().numpy().tobytes() for t in (stream.scores, stream.frames, stream.retired, times.hyps(),
                                                    times._seen, times._lost, when) + stream.hyps()]

    def body(stream, times, bufs, nf):
        for l in bufs:
            times.step(*stream.advance(l, nf, 0.9, 0.2))
        _, lengths, slot_map = stream.commit(max_tail=3)
        return times.commit(lengths, slot_map)
    eager, want = ModifiedBeamStream(B, mf, K, 1, device=dev), []
    etimes = ModifiedBeamTimes(eager)
    for r in range(reps):
        nf = torch.minimum(ends, torch.tensor(chunk * (r + 1), device=dev))
        when = body(eager, etimes, logits[chunk * r:chunk * (r + 1)], nf)
        want.append(snap(eager, etimes, when))
    torch.cuda.synchronize()
    assert not eager.overflowed.any() and int(eager.retired.sum()) > 0 and not etimes.lost.any()
    stream = ModifiedBeamStream(B, mf, K, 1, device=dev)
    times = ModifiedBeamTimes(stream)
    bufs = [torch.empty_like(logits[0]) for _ in range(chunk)]
    nf = torch.zeros(B, dtype=torch.int64, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        when = body(stream, times, bufs, nf)
    stream.reset()                                 # (a capture runs nothing; all the same: from the start)
    times.reset()
    for r in range(reps):
        for buf, l in zip(bufs, logits[chunk * r:chunk * (r + 1)]):
            buf.copy_(l)
        nf.copy_(torch.minimum(ends, torch.tensor(chunk * (r + 1), device=dev)))
        graph.replay()
        assert snap(stream, times, when) == want[r], r


# ---- 13, 14: the drivers -------------------------------------------------------------------------------------------------
def tiny(dec, device):
    import model_common as C
    import decode_common as D
    from oracle.pika_ref import seeded_state_dict
    from pika_amd.model import transducer, encoder
    net = C.build(transducer, encoder, dec)
    net.load_state_dict(seeded_state_dict(net, C.SEED))
    D.tweak(net)
    return net.eval().to(device), D.inputs()


def test_the_drivers_on_the_tiny_model(hip_device):
    from pika_amd import (ModifiedBeamState, ModifiedBeamTimes, ModifiedStreamDecoder, modified_beam_search,
                          modified_beam_search_lm, modified_beam_search_timed)
    net, (x, x_len) = tiny("rnn", hip_device)
    K, sm, dev = 4, 0.85, hip_device
    x = x.to(dev)
    lm = automata("lm", net.output_dim, 5, dev)

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
    plain = modified_beam_search(net, x, x_len, beam=K, nbest=K, sm_scale=sm)
    fused = modified_beam_search_lm(net, x, x_len, lm, beam=K, nbest=K, sm_scale=sm)
    record = ModifiedBeamTimes(ModifiedBeamState(2, 8, K, 0, dev))              # 14: a record beside the old paths
    assert record.hyps().shape == (2, K, 8)
    assert same(plain, modified_beam_search(net, x, x_len, beam=K, nbest=K, sm_scale=sm))
    assert same(fused, modified_beam_search_lm(net, x, x_len, lm, beam=K, nbest=K, sm_scale=sm))
    B, T = plain[3].shape[:2]
    xl = torch.as_tensor(x_len).to(dev).long().clamp(0, T)
    for graph in (True, False):
        timed = modified_beam_search_timed(net, x, x_len, beam=K, nbest=K, sm_scale=sm, use_graph=graph)
        ref = plain if graph else modified_beam_search(net, x, x_len, beam=K, nbest=K, sm_scale=sm, use_graph=False)
        assert same(timed[:3] + timed[4:], ref) and timed[3].shape == timed[0].shape
        check_times(timed[0], timed[1], timed[3], xl)
    ltimed = modified_beam_search_timed(net, x, x_len, lm, beam=K, nbest=K, sm_scale=sm)
    assert same(ltimed[:4] + ltimed[5:], fused)
    check_times(ltimed[0], ltimed[1], ltimed[4], xl)
    # the stream decoder: fp32 products, so that chunking changes no bit of the logits
    one = modified_beam_search_timed(net, x, x_len, beam=K, nbest=K, sm_scale=sm, use_graph=False, precision="fp32")
    enc = one[4]
    want = {(b, tuple(one[0][b, j, :n].tolist())): one[3][b, j, :n].tolist()
            for b in range(B) for j, n in enumerate(one[1][b].tolist()) if n >= 0}
    for chunk in (1, 5, 17):
        for forced in (False, True):
            dec = ModifiedStreamDecoder(net, B, T if not forced else 24, beam=K, sm_scale=sm, precision="fp32")
            assert dec.track_times() is dec.times
            for start in range(0, T, chunk):
                piece = enc[:, start:start + chunk]
                dec.advance(piece, (xl - start).clamp(0, piece.shape[1]))
                if forced:
                    out = dec.commit(max_tail=1)
                    assert len(out) == 3
            with pytest.raises(RuntimeError):
                dec.track_times()
            ctok, clen, ttok, tlen, tsc, ctime, ttime = (t.cpu().numpy() for t in dec.results_timed(nbest=K))
            assert not dec.times.lost.any() and ctime.shape == ctok.shape and ttime.shape == ttok.shape
            assert (int(clen.sum()) > 0) == forced
            matched = 0
            for b in range(B):
                assert ((ctime[b, :clen[b]] >= 0).all()) and (ctime[b, clen[b]:] == -1).all()
                for j in range(K):
                    if tlen[b, j] < 0:
                        continue
                    whole = ctime[b, :clen[b]].tolist() + ttime[b, j, :tlen[b, j]].tolist()
                    assert TC.increasing(whole) and all(0 <= t < int(xl[b]) for t in whole), (chunk, forced, b, j)
                    key = (b, tuple(ttok[b, j, :tlen[b, j]].tolist()))
                    if not forced and key in want:  # no commits: the one-shot call's times (the two drivers form
                        matched += 1               # their logits by different products: a hypothesis may differ)
                        assert whole == want[key], (chunk, b, j)
            assert forced or matched >= B, (chunk, matched)
    dec = ModifiedStreamDecoder(net, B, T, beam=K, sm_scale=sm, precision="fp32")   # tracking off: nothing changes
    dec.advance(enc[:, :5])
    assert dec.times is None
    with pytest.raises(RuntimeError):
        dec.results_timed()


def check_times(tokens, lengths, times, xl):
    tokens, lengths, times = (t.cpu().numpy() for t in (tokens, lengths, times))
    seen = 0
    for b in range(tokens.shape[0]):
        for j in range(tokens.shape[1]):
            n = lengths[b, j]
            if n < 0:
                assert (times[b, j] == -1).all()
                continue
            row = times[b, j, :n].tolist()
            assert TC.increasing(row) and all(0 <= t < int(xl[b]) for t in row) and (times[b, j, n:] == -1).all()
            seen += n
    assert seen > 0
