"""The streaming one-symbol-per-frame beam search on the CPU (`ModifiedBeamStream` on the dict tries of
`ModifiedBeamState`; the definition of include/pika_msearch_stream.h): a stream that commits equals the one-shot search
bit for bit, and the commit's own properties.

Shape: V = 7, K = 4, T = 40, max_frames = 8; chunks of {1, 3, 8, 40} frames; commits never (max_frames = 40), after
every chunk, after every 5 frames.  Between two commits a stream holds the tail the last commit left plus the frames
since, so "after every chunk" with chunks of 8 and 40 frames cannot fit max_frames = 8 whatever the input (K = 4 distinct
hypotheses differ, so a commit leaves frames >= 1): those two cases run with max_frames = 40, as "never" does.  The
seeds are fixed so that no run here overflows (asserted, on this CPU run)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import msearch_stream_common as S  # noqa: E402

V, K, T, MF = 7, 4, 40, 8
LENS = [T, 0, 33]
SEEDS = (3, 4, 5)
NINF = -np.inf


def models():
    return [S.PeakedModel(T, V, s) for s in SEEDS]


_ONE = {}


def oneshot(dtype):
    """The one-shot run, once per dtype; shared and not modified."""
    from pika_amd import ModifiedBeamState
    if dtype not in _ONE:
        state = ModifiedBeamState(len(LENS), T, K, 0, "cpu", dtype)
        _, trace = S.feed(state, models(), LENS, T, sm_scale=0.9, penalty=0.1)
        assert not state.overflowed.any()
        _ONE[dtype] = trace
    return _ONE[dtype]


def schedule(chunk, sched):
    """-> (max_frames, every, each_chunk)"""
    if sched == "never":
        return T, None, False
    if sched == "chunk":
        return (MF if chunk < MF else T), None, True
    return MF, 5, False


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("sched", ["never", "chunk", "five"])
@pytest.mark.parametrize("chunk", [1, 3, 8, 40])
def test_a_committing_stream_equals_the_one_shot_search(chunk, sched, dtype):
    from pika_amd import ModifiedBeamStream
    mf, every, each = schedule(chunk, sched)
    stream = ModifiedBeamStream(len(LENS), mf, K, 0, device="cpu", dtype=dtype)
    rooms = []

    def after(obj, kind, out, committed):
        if kind == "step":
            rooms.append(("step", obj.room.clone()))
        else:
            rooms.append(("commit", obj.room.clone(), out[1].clone()))
            assert torch.equal(out[2], torch.arange(K).repeat(len(LENS), 1))       # exact: nothing moves
    committed, trace = S.feed(stream, models(), LENS, chunk, every, each, 0.9, 0.1, after=after)
    assert not stream.overflowed.any()
    S.same_trace(trace, oneshot(dtype))          # committed + tail: tokens, lengths, order, score bits, parent, token
    assert stream.consumed.tolist() == LENS
    assert (stream.offset == 0).all() and (stream.bonus_offset == 0).all()
    assert torch.equal(stream.frames + stream.retired, stream.consumed) and (stream.room == mf - stream.frames).all()
    grew = 0
    for prev, cur in zip(rooms, rooms[1:]):
        if cur[0] == "commit":
            assert (cur[1] >= prev[1]).all()                         # a commit never takes room
            assert ((cur[1] > prev[1]) | (cur[2] == 0) | (prev[1] == cur[1])).all()
            grew += int((cur[1] > prev[1]).sum())
    if sched != "never":
        assert grew > 0 and sum(len(c) for c in committed) > 0       # room grows at a commit, and text comes out
        assert int(stream.retired.sum()) > 0


def test_beam_one_commits_everything():
    from pika_amd import ModifiedBeamState, ModifiedBeamStream
    m = [S.PeakedModel(20, V, 11)]
    state = ModifiedBeamState(1, 20, 1, 0, "cpu")
    _, want = S.feed(state, m, [20], 20)
    stream = ModifiedBeamStream(1, 4, 1, 0, device="cpu")

    def after(obj, kind, out, committed):
        if kind == "commit":                                          # an empty tail, frames at its minimum
            assert obj.frames.tolist() == [0] and obj.room.tolist() == [4]
            assert obj.hyps()[1].tolist() == [[0]]
    committed, trace = S.feed(stream, m, [20], 3, each_chunk=True, after=after)
    S.same_trace(trace, want)
    assert tuple(committed[0]) == want[-1][2][0][0][1] and stream.consumed.tolist() == [20]
    assert not stream.overflowed.any()


def state_bytes(stream):
    s = stream.state
    return [t.numpy().tobytes() for t in (s.scores, s.frames, s.overflowed, stream.retired, stream.offset) + s.hyps()]


def test_which_leaves_the_other_streams_alone():
    from pika_amd import ModifiedBeamStream
    stream = ModifiedBeamStream(3, T, K, 0, device="cpu")
    S.feed(stream, models(), [12, 12, 12], 12)
    one = ModifiedBeamStream(3, T, K, 0, device="cpu")
    S.feed(one, models(), [12, 12, 12], 12)
    tokens, lengths, slot_map = stream.commit(which=[True, False, True], rebase=True)
    full = one.commit(rebase=True)
    before, after = state_bytes(one), state_bytes(stream)
    assert lengths[1] == 0 and (tokens[1] == -1).all() and slot_map[1].tolist() == list(range(K))
    assert int(stream.retired[1]) == 0 and float(stream.offset[1]) == 0.0
    assert int(stream.frames[1]) == 12 and int(one.frames[1]) < 12
    for b in (0, 2):                                                  # the selected streams: as a commit of all
        assert torch.equal(tokens[b], full[0][b]) and lengths[b] == full[1][b]
        assert torch.equal(stream.scores[b], one.scores[b]) and stream.frames[b] == one.frames[b]
    fresh = ModifiedBeamStream(3, T, K, 0, device="cpu")
    S.feed(fresh, models(), [12, 12, 12], 12)
    for x, y in zip((fresh.scores[1], fresh.frames[1], fresh.hyps()[0][1], fresh.hyps()[1][1]),
                    (stream.scores[1], stream.frames[1], stream.hyps()[0][1], stream.hyps()[1][1])):
        assert x.numpy().tobytes() == y.numpy().tobytes()             # byte-identical
    assert before != after
    # reset(which) restarts the state and the side record of the selected streams alone
    stream.reset(which=[True, False, False])
    assert stream.retired.tolist()[0] == 0 and float(stream.offset[0]) == 0.0 and int(stream.frames[0]) == 0
    assert int(stream.retired[2]) == int(one.retired[2]) and float(stream.offset[2]) == float(one.offset[2]) != 0.0


def test_a_stream_of_no_frames():
    from pika_amd import ModifiedBeamStream
    stream = ModifiedBeamStream(2, MF, K, 0, device="cpu")
    tokens, lengths, slot_map = stream.commit()
    assert lengths.tolist() == [0, 0] and (tokens == -1).all() and tokens.shape == (2, MF)
    assert stream.consumed.tolist() == [0, 0] and stream.room.tolist() == [MF, MF]
    parent, token = stream.advance(torch.zeros(2 * K, V), torch.tensor([0, 0]))
    assert parent.tolist() == [list(range(K))] * 2 and (token == 0).all()
    assert stream.commit(rebase=True)[1].tolist() == [0, 0] and (stream.offset == 0).all()
    assert stream.scores.tolist() == [[0.0] + [NINF] * (K - 1)] * 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_forced_commit(dtype):
    """max_tail = 2 on a beam that random logits keep apart."""
    from pika_amd import ModifiedBeamStream
    import msearch_common as M
    B, T0 = 3, 12
    flat = [M.TableModel(T0, V, 70 + b, scale=1.0) for b in range(B)]
    stream = ModifiedBeamStream(B, T0, K, 0, device="cpu", dtype=dtype)
    S.feed(stream, flat, [T0] * B, T0)
    before = S.tails(stream)
    frames = stream.frames.clone()
    tokens, lengths, slot_map = stream.commit(max_tail=2, max_len=5)
    after = S.tails(stream)
    dropped = 0
    for b in range(B):
        best = before[b][0][1]
        live, common = [e[1] for e in before[b] if e], 0
        while all(len(q) > common and q[common] == best[common] for q in live):
            common += 1
        d = len(best) - 2 if len(best) - common > 2 else common
        assert lengths[b] == d and tuple(tokens[b, :min(d, 5)].tolist()) == best[:min(d, 5)]
        assert (tokens[b, min(d, 5):] == -1).all()
        keep = [k for k, e in enumerate(before[b]) if e and e[1][:d] == best[:d]]     # descend from the new root
        dropped += K - len(keep)
        assert slot_map[b, :len(keep)].tolist() == keep                                # the survivors, in order
        assert slot_map[b, len(keep):].tolist() == list(range(len(keep), K))
        for j, k in enumerate(keep):
            assert after[b][j][1] == before[b][k][1][d:] and after[b][j][0].tobytes() == before[b][k][0].tobytes()
        assert len(after[b][0][1]) <= 2
        for j in range(len(keep), K):                                                  # vacated: as after a reset
            assert after[b][j] is None and stream.scores[b, j] == NINF and stream.state._node[b][j] == 0
        tail = max(len(after[b][j][1]) for j in range(len(keep)))
        keys = len(stream.state._tries[b][1]) - 1
        assert int(stream.frames[b]) == min(int(frames[b]), max(-(-keys // K), tail))
    assert dropped > 0 and torch.equal(stream.frames + stream.retired, frames)


def test_rebase():
    from pika_amd import ModifiedBeamStream
    ref = ModifiedBeamStream(len(LENS), MF, K, 0, device="cpu", dtype=torch.float64)
    c0, t0 = S.feed(ref, models(), LENS, 3, each_chunk=True, sm_scale=0.9, penalty=0.1)

    def after(obj, kind, out, committed):
        if kind == "commit":
            live = obj.scores[:, 0] > NINF
            assert (obj.scores[live, 0] == 0).all()                   # right after the commit
    # float32: 40 frames of a few roundings each at a magnitude below 64 (one ulp: 7.6e-6) stay below 1e-3
    for dtype, tol in ((torch.float64, 1e-9), (torch.float32, 1e-3)):
        s = ModifiedBeamStream(len(LENS), MF, K, 0, device="cpu", dtype=dtype)
        c1, t1 = S.feed(s, models(), LENS, 3, each_chunk=True, sm_scale=0.9, penalty=0.1, commit=dict(rebase=True),
                        after=after)
        assert c1 == c0 and not s.overflowed.any()
        assert [[e and e[1] for e in row] for row in t1[-1][2]] == [[e and e[1] for e in row] for row in t0[-1][2]]
        absolute = s.offset.unsqueeze(1) + s.scores.double()
        live = ref.scores > NINF
        assert torch.equal(live, s.scores > NINF) and float((absolute - ref.scores)[live].abs().max()) <= tol
        assert (s.offset[[0, 2]] != 0).all() and float(s.offset[1]) == 0.0 and (s.bonus_offset == 0).all()
        assert float(s.scores[live].abs().max()) < 40.0               # the magnitude went to the offset


def test_argument_checks():
    from pika_amd import ModifiedBeamStream
    s = ModifiedBeamStream(2, MF, K, 0, device="cpu")
    with pytest.raises(ValueError, match="max_tail"):
        s.commit(max_tail=-2)
    with pytest.raises(ValueError, match="max_len"):
        s.commit(max_len=0)
    with pytest.raises(ValueError, match="batch"):
        s.commit(which=[True])
    with pytest.raises(ValueError, match="num_frames"):
        s.advance(torch.zeros(2 * K, V), torch.tensor([1]))
    with pytest.raises(ValueError, match="num_frames"):
        s.advance(torch.zeros(2 * K, V), torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="candidates"):
        ModifiedBeamStream(2, MF, K, 0, candidates=8, device="cpu")
    with pytest.raises(ValueError):
        ModifiedBeamStream(2, MF, 65, 0, device="cpu")
