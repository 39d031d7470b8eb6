"""CPU checks of the time stamps of the one-symbol-per-frame beam search: the reference record against the reference
search, what a time record means (a path of the modified lattice whose value the score bounds), and the plain-torch
`ModifiedBeamTimes` on a CPU state and through a CPU stream under every commit schedule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msearch_common as M  # noqa: E402
import msearch_stream_common as S  # noqa: E402
import msearch_times_common as TC  # noqa: E402

NINF = -np.inf
V, T = 5, 12


def models():
    return [("table", M.TableModel(T, V, 3)), ("peaked", S.PeakedModel(T, V, 4))]


def test_replay_on_a_hand_made_history():
    # two slots; frame 0: slot 0 emits 3, slot 1 is slot 0 with blank; frame 1: inactive; frame 2: both from old slot 1
    h = [("step", [[0, 0]], [[3, 0]], [True]), ("step", [[0, 1]], [[0, 0]], [False]),
         ("step", [[1, 1]], [[2, 4]], [True])]
    rows, outs = TC.replay(h, 1, 2)
    assert rows == [[[1], [1]]] and outs == []
    h.append(("step", [[0, 1]], [[1, 0]], [True]))
    rows, _ = TC.replay(h, 1, 2)
    assert rows == [[[1, 2], [1]]]
    # a commit of one label with the slots swapped: the earliest of the live slots' entries, then the tails
    h.append(("commit", [1], [[1, 0]], [2]))
    rows, outs = TC.replay(h, 1, 2)
    assert outs == [[[1]]] and rows == [[[], [2]]]
    r = TC.Replay(1, 2)
    r.rows = [[[4, 9], [2, 9, 11]]]
    assert r.commit([2], [[0, 1]], [2]) == [[2, 9]] and r.rows == [[[], [11]]]
    assert r.commit([0], [[0, 1]], [2], [False]) == [None] and r.rows == [[[], [11]]]


@pytest.mark.parametrize("K", [1, 3, 8])
def test_the_search_with_times_agrees_with_replay_and_names_a_path(K):
    for name, model in models():
        beam, times, history = TC.timed_search(model, T, V, K, 0, 0.9, 0.1)
        rows, _ = TC.replay(history, 1, K)
        live = 0
        for k, (score, tokens) in enumerate(beam):
            if not score > NINF:
                continue
            live += 1
            assert rows[0][k] == times[k], (name, k)
            value = TC.path_value(model, tokens, times[k], T, 0, 0.9, 0.1)     # increasing, in range, one per label
            assert value <= score + 1e-9, (name, k, value, score)
            if K == 1:
                assert abs(value - score) <= 1e-9, (name, value, score)       # nothing merges
        assert live == min(K, live) and live >= 1


@pytest.mark.parametrize("K", [1, 3, 8])
def test_cpu_record_on_a_cpu_state_equals_replay(K):
    from pika_amd import ModifiedBeamState, ModifiedBeamTimes
    lens = [T, 0, T // 2]
    mods = [S.PeakedModel(T, V, 10 + b) for b in range(3)]
    state = ModifiedBeamState(3, T, K, 0, device="cpu", dtype=torch.float64)
    tr = TC.Tracker(ModifiedBeamTimes(state))
    S.feed(state, mods, lens, T, sm_scale=0.9, penalty=0.1, after=tr)          # compares after every step
    assert tr.n == T and tr.ref.consumed == lens and not tr.times.lost.any()
    tok, ln, sc = state.results(nbest=K)
    got = tr.times.results(tok, ln).numpy()
    hyps = tr.times.hyps().numpy()
    assert (got == hyps).all()                                                 # a plain state's entries are its slots
    for b in (0, 2):
        for k in range(K):
            if ln[b, k] >= 0:
                n = int(ln[b, k])
                value = TC.path_value(mods[b], tok[b, k, :n].tolist(), got[b, k, :n], lens[b], 0, 0.9, 0.1)
                assert value <= float(sc[b, k]) + 1e-9
    assert (got[1, 0] == -1).all() and int(ln[1, 0]) == 0
    # max_len shorter than an entry: -1 everywhere for that entry; hyps is cut
    n0 = int(ln[0, 0])
    if n0 > 1:
        tok2, ln2, _ = state.results(nbest=1, max_len=n0 - 1)
        assert (tr.times.results(tok2, ln2)[0, 0] == -1).all()
        assert tr.times.hyps(max_len=n0 - 1)[0, 0].tolist() == hyps[0, 0, :n0 - 1].tolist()


SCHEDULES = [dict(chunk=1, each_chunk=True), dict(chunk=3, each_chunk=True), dict(chunk=8, every=5),
             dict(chunk=3, each_chunk=True, commit=dict(max_tail=0)), dict(chunk=8, every=5, commit=dict(max_tail=2)),
             dict(chunk=1), dict(chunk=3), dict(chunk=8)]


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("sched", range(len(SCHEDULES)))
def test_cpu_stream_schedules(K, sched):
    from pika_amd import ModifiedBeamState, ModifiedBeamStream, ModifiedBeamTimes
    kw, Ts = SCHEDULES[sched], 24
    commits = "each_chunk" in kw or "every" in kw
    lens = [Ts, 0, Ts - 7]
    mods = [S.PeakedModel(Ts, 7, 40 + b) for b in range(3)]
    stream = ModifiedBeamStream(3, Ts, K, 0, device="cpu")
    tr = TC.Tracker(ModifiedBeamTimes(stream))
    # (the tracker asserts: record == replay and committed ++ any live tail strictly increasing after every step and
    # commit; every commit's output == the definition on the records read just before it)
    committed, _ = S.feed(stream, mods, lens, after=tr, sm_scale=0.9, penalty=0.1, **kw)
    assert not stream.overflowed.any() and not tr.times.lost.any()
    assert [len(c) for c in committed] == [len(c) for c in tr.committed]
    if commits:
        assert len(tr.commits) > 0 and sum(map(len, tr.committed)) > 0
    else:                                                                       # any chunking: the one-shot's times
        one = ModifiedBeamState(3, Ts, K, 0, device="cpu")
        tr1 = TC.Tracker(ModifiedBeamTimes(one))
        S.feed(one, mods, lens, Ts, sm_scale=0.9, penalty=0.1, after=tr1)
        assert torch.equal(tr.times.hyps(), tr1.times.hyps()) and (tr.times.hyps() >= 0).any()


def test_cpu_lost_records_and_reset():
    from pika_amd import ModifiedBeamState, ModifiedBeamTimes
    mods = [S.PeakedModel(T, V, 10 + b, p_blank=0.1) for b in range(3)]
    state = ModifiedBeamState(3, T, 3, 0, device="cpu")
    tr = TC.Tracker(ModifiedBeamTimes(state), check=False, skip=(4,))
    S.feed(state, mods, [T, 4, T], T, after=tr)         # utterance 1 was inactive at the skipped step: it is not lost
    assert tr.times.lost.tolist() == [True, False, True]
    hyps = tr.times.hyps()
    assert (hyps[0] == -1).all() and (hyps[2] == -1).all() and (hyps[1] >= 0).any()
    for k, r in enumerate(tr.ref.rows[1]):                                      # the others are unaffected
        if state.scores[1, k] > NINF:
            assert hyps[1, k].tolist() == r + [-1] * (T - len(r))
    tr.times.reset([True, False, False])
    assert tr.times.lost.tolist() == [False, False, True]
    with pytest.raises(TypeError):
        ModifiedBeamTimes(object())
