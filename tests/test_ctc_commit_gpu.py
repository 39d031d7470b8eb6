"""`CtcBeamStream.commit` on the MI355X, against the one-shot searches and the float64 reference with the commit hook
(tests/ctc_commit_common.py; tests/test_ctc_commit_refs.py asserts on the CPU that the inputs below converge).

The exact commit's criterion is exact: the labels committed so far followed by the tail that `results` returns are, bit
for bit (`torch.equal` on tokens, lengths and scores), what `ctc_beam_search` / `ctc_beam_search_lm` give on the whole
tensor -- whatever the chunking, with a commit after every chunk, and also when the stream consumes twice the frames it
has room for.  The forced commit is checked in two halves: what it does to the beam, exactly, against the beam before
it; and the search that follows, against the float64 reference with the same hook, by the separated-case rules of
tests/test_ctc_stream_gpu.py (bound = max(4 x the float32 yardstick's largest score error, 1e-6 * max|score|); a case
is separated when the reference's margin exceeds 2 * bound; labels and scores are compared on separated cases only)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_commit_common as M  # noqa: E402
import ctc_lm_common as L  # noqa: E402

pytestmark = pytest.mark.gpu

LM_KW = M.LM_KW
REF_LM = L.make_lm(M.C, 0, M.LM_SEED, order=3)
PHRASES = [(3, 5), (7, 7, 2), (9,)]
_DEVICE = {}


class Variant(object):
    """One of the three searches: how to make its stream and how to run its one-shot call."""

    def __init__(self, name, dev, beam):
        from pika_amd import ctc
        self.name, self.dev, self.beam = name, dev, beam
        if "lm" not in _DEVICE:
            lm = ctc.CtcNgramLm(REF_LM.fst, REF_LM.backoff_id, REF_LM.label_offset, device=dev)
            _DEVICE["lm"] = lm
            _DEVICE["biased"] = ctc.CtcBiasedLm(lm, ctc.CtcHotwords(PHRASES, M.C, boost=1.5, device=dev), 0.75)
        self.lm = None if name == "plain" else _DEVICE[name]
        self.finals = (True,) if self.lm is None else (True, False)

    def stream(self, max_frames, batch=M.B):
        from pika_amd import ctc
        kw = {} if self.lm is None else dict(lm=self.lm, **LM_KW)
        return ctc.CtcBeamStream(batch, max_frames, beam=self.beam, device=self.dev, **kw)

    def one_shot(self, x, ils, use_final=True):
        from pika_amd import ctc
        if self.lm is None:
            return ctc.ctc_beam_search(x, torch.tensor(ils), beam=self.beam, nbest=self.beam)
        return ctc.ctc_beam_search_lm(x, torch.tensor(ils), self.lm, beam=self.beam, nbest=self.beam, use_final=use_final,
                                      **LM_KW)

    def results(self, stream, use_final=True):
        return stream.results(nbest=self.beam, use_final=use_final)


def chunk_lengths(ils, start, k):
    return [int(min(max(il - start, 0), k)) for il in ils]


def take(committed, out):
    """Appends the labels of one commit's outputs (host copies) to the per-stream lists."""
    tokens, lengths = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert tokens.dtype == np.int32 and lengths.dtype == np.int32
    for b, done in enumerate(committed):
        n = int(lengths[b])
        assert 0 <= n <= tokens.shape[1] and (tokens[b, n:] == -1).all() and (tokens[b, :n] >= 0).all()
        done.extend(int(v) for v in tokens[b, :n])


def assert_joined(committed, got, want, T):
    """committed labels + the tails of `got` == the one-shot outputs `want` (token width T), bit for bit."""
    tokens, lengths = got[0].cpu().numpy(), got[1].cpu().numpy()
    wt, wl = want[0].cpu().numpy(), want[1].cpu().numpy()
    for b, done in enumerate(committed):
        for k in range(tokens.shape[1]):
            n = int(lengths[b, k])
            assert (tokens[b, k, max(n, 0):] == -1).all()
            if n < 0:
                assert wl[b, k] == -1 and (wt[b, k] == -1).all(), (b, k)
                continue
            full = done + [int(v) for v in tokens[b, k, :n]]
            assert wl[b, k] == len(full) and wt[b, k, :len(full)].tolist() == full, (b, k, full, wt[b, k].tolist())
            assert (wt[b, k, len(full):] == -1).all()
    for g, w in zip(got[2:], want[2:]):
        assert g.dtype == w.dtype and torch.equal(g, w)


def labels_of(out, b):
    """The real entries of stream b: [(label tuple, scores...)] in output order, and the number of missing ones."""
    tokens, lengths = out[0].cpu().numpy(), out[1].cpu().numpy()
    rest = [o.cpu().numpy() for o in out[2:]]
    real = [(tuple(int(v) for v in tokens[b, k, :lengths[b, k]]),) + tuple(r[b, k] for r in rest)
            for k in range(tokens.shape[1]) if lengths[b, k] >= 0]
    missing = [k for k in range(tokens.shape[1]) if lengths[b, k] < 0]
    assert missing == list(range(len(real), tokens.shape[1])), "missing entries come last"
    for k in missing:
        assert (tokens[b, k] == -1).all() and all(r[b, k] == -np.inf for r in rest)
    return real


# ---------------------------------------------------------------------------------------------------------------
# 1. exact, same capacity: any chunking, a commit after every chunk
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", M.BEAMS)
@pytest.mark.parametrize("name", ["plain", "lm", "biased"])
def test_committed_plus_tail_equals_one_shot(hip_device, name, beam):
    v = Variant(name, hip_device, beam)
    x = torch.from_numpy(M.LP1.copy()).to(hip_device)
    want = {uf: v.one_shot(x, M.ILS1, uf) for uf in v.finals}
    stream = v.stream(M.T1)
    for cname, sizes in M.CHUNKINGS1:
        stream.reset()
        committed, outs, start = [[] for _ in range(M.B)], [], 0
        for k in sizes:
            lens = chunk_lengths(M.ILS1, start, k)
            before = stream._state.clone() if 0 in lens else None
            stream.advance(x[start:start + k], lens)
            if before is not None:                      # a stream that gets no frame is left exactly as it was
                rec = stream._hdr.shape[1] * 4
                tables = (stream._state.numel() - M.B * rec) // M.B
                for b in [b for b, n in enumerate(lens) if n == 0]:
                    for lo, hi in ((b * tables, (b + 1) * tables), (M.B * tables + b * rec, M.B * tables + (b + 1) * rec)):
                        assert torch.equal(stream._state[lo:hi], before[lo:hi]), (cname, start, b)
            outs.append(stream.commit())
            assert outs[-1][0].shape == (M.B, M.T1) and outs[-1][1].shape == (M.B,)
            start += k
        for out in outs:
            take(committed, out)
        print("CTCCOMMIT %s beam %d chunks %-6s committed %s of %s labels" % (
            name, beam, cname, [len(c) for c in committed], want[True][1][:, 0].tolist()))
        for uf in v.finals:
            assert_joined(committed, v.results(stream, uf), want[uf], M.T1)
        assert stream.consumed.tolist() == M.ILS1 and stream.overflowed.tolist() == [False] * M.B


# ---------------------------------------------------------------------------------------------------------------
# 2. exact, beyond capacity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", M.BEAMS)
@pytest.mark.parametrize("name", ["plain", "lm"])
def test_a_stream_consumes_more_than_it_holds(hip_device, name, beam):
    v = Variant(name, hip_device, beam)
    x = torch.from_numpy(M.LP2.copy()).to(hip_device)
    want = v.one_shot(x, [M.T2] * M.B)
    stream = v.stream(M.MAXF2)
    assert stream.max_frames < M.T2
    committed, outs, peak = [[] for _ in range(M.B)], [], []
    for s in range(0, M.T2, M.CHUNK2):
        stream.advance(x[s:s + M.CHUNK2])
        peak.append(stream.frames.clone())
        outs.append(stream.commit())
    for out in outs:
        take(committed, out)
    print("CTCCOMMIT beyond capacity %s beam %d: peak frames %s of %d, committed %s" % (
        name, beam, torch.stack(peak).max(0).values.tolist(), M.MAXF2, [len(c) for c in committed]))
    assert stream.overflowed.tolist() == [False] * M.B
    assert stream.consumed.tolist() == [M.T2] * M.B
    assert (stream.room == M.MAXF2 - stream.frames).all() and int(stream.room.min()) >= 0
    assert all(len(c) > 0 for c in committed)           # (the refs test: both searches share a prefix on these inputs)
    assert_joined(committed, v.results(stream), want, M.T2)
    # without commits the same capacity ends at frame 80: on the host as before ...
    quiet = v.stream(M.MAXF2)
    for s in range(0, M.MAXF2, M.CHUNK2):
        quiet.advance(x[s:s + M.CHUNK2])
    with pytest.raises(ValueError, match="max_frames"):
        quiet.advance(x[M.MAXF2:M.MAXF2 + M.CHUNK2])
    assert quiet.frames.tolist() == [M.MAXF2] * M.B and quiet.consumed.tolist() == [M.MAXF2] * M.B
    # ... and on the device, where a commit that selects no stream has only lifted the host's bound
    quiet = v.stream(M.MAXF2)
    out = quiet.commit(which=[False] * M.B)
    assert out[1].tolist() == [0] * M.B and bool((out[0] == -1).all())
    for s in range(0, M.MAXF2 + M.CHUNK2, M.CHUNK2):
        assert quiet.overflowed.tolist() == [False] * M.B
        quiet.advance(x[s:s + M.CHUNK2])
    assert quiet.overflowed.tolist() == [True] * M.B and quiet.consumed.tolist() == [M.MAXF2] * M.B
    assert quiet.room.tolist() == [0] * M.B


# ---------------------------------------------------------------------------------------------------------------
# 3. which
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "biased"])
def test_commit_of_a_subset_leaves_the_others_alone(hip_device, name):
    v = Variant(name, hip_device, 4)
    x = torch.from_numpy(M.LP1.copy()).to(hip_device)
    stream = v.stream(M.T1)
    stream.advance(x[:24])
    before = stream._state.clone()
    old = v.results(stream, False)
    tokens, lengths = stream.commit(which=torch.tensor([1, 0, 1], device=hip_device))
    rec = stream._hdr.shape[1] * 4
    tables = (stream._state.numel() - M.B * rec) // M.B
    assert torch.equal(stream._state[tables:2 * tables], before[tables:2 * tables])
    lo = M.B * tables + rec
    assert torch.equal(stream._state[lo:lo + rec], before[lo:lo + rec])
    assert lengths[1].item() == 0 and bool((tokens[1] == -1).all())
    for b in (0, 2):
        assert lengths[b].item() == len(M.common_prefix([h[0] for h in labels_of(old, b)]))
    assert not torch.equal(stream._state[:tables], before[:tables])
    new = v.results(stream, False)
    assert labels_of(new, 1) == labels_of(old, 1)
    assert stream.frames.tolist()[1] == 24 and stream.consumed.tolist() == [24] * M.B


# ---------------------------------------------------------------------------------------------------------------
# 4. bookkeeping
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", M.BEAMS)
@pytest.mark.parametrize("name", ["plain", "lm"])
def test_bookkeeping_after_every_commit(hip_device, name, beam):
    v = Variant(name, hip_device, beam)
    x = torch.from_numpy(M.LP1.copy()).to(hip_device)
    stream = v.stream(M.T1)
    start = 0
    for k in M.fixed(3, M.T1):
        stream.advance(x[start:start + k], chunk_lengths(M.ILS1, start, k))
        start += k
        old, frames_old = v.results(stream, False), stream.frames.tolist()
        _, lengths = stream.commit()
        new, frames, consumed = v.results(stream, False), stream.frames.tolist(), stream.consumed.tolist()
        assert consumed == [min(start, il) for il in M.ILS1]
        for b in range(M.B):
            labels = [h[0] for h in labels_of(old, b)]
            prefix, keep, tails = M.apply_commit(labels)
            assert len(keep) == len(labels) and lengths[b].item() == len(prefix)
            live, tail, want = M.recharge(tails, beam, frames_old[b])
            assert frames[b] == want, (b, start, frames[b], want, live, tail)
            assert frames[b] % 8 == consumed[b] % 8 and frames[b] <= frames_old[b]
            assert frames[b] + stream._hdr[b, 3].item() == consumed[b]
            assert [h[0] for h in labels_of(new, b)] == tails and max(len(l) for l in tails) <= frames[b]
            assert [h[1:] for h in labels_of(new, b)] == [h[1:] for h in labels_of(old, b)]


# ---------------------------------------------------------------------------------------------------------------
# 5. / 6. forced
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", M.TAILS)
@pytest.mark.parametrize("beam", M.BEAMS)
@pytest.mark.parametrize("name", ["plain", "lm"])
def test_forced_commit_keeps_the_descendants_of_the_best_prefix(hip_device, name, beam, m):
    v = Variant(name, hip_device, beam)
    x = torch.from_numpy(M.LP5.copy()).to(hip_device)
    stream = v.stream(M.T6)
    for s in range(0, M.T5, 8):
        stream.advance(x[s:s + 8])
    old = v.results(stream, False)
    tokens, lengths = stream.commit(max_tail=m)
    new = v.results(stream, False)
    forced = 0
    for b in range(M.B):
        before, after = labels_of(old, b), labels_of(new, b)
        done = tuple(tokens[b, :lengths[b]].tolist())
        prefix, keep, tails = M.apply_commit([h[0] for h in before], m)
        assert done == prefix == before[0][0][:len(done)] and len(before[0][0]) - len(done) <= m
        assert after == [(tl,) + before[i][1:] for i, tl in zip(keep, tails)]      # old order, the scores' bits
        forced += len(keep) < len(before)
        assert stream.consumed.tolist()[b] == M.T5 and stream.frames.tolist()[b] % 8 == 0
    print("CTCCOMMIT forced %s beam %d max_tail %d: %d of %d streams dropped entries" % (name, beam, m, forced, M.B))


@pytest.mark.parametrize("m", M.TAILS)
@pytest.mark.parametrize("beam", M.BEAMS)
def test_search_after_a_forced_commit_against_fp64(hip_device, beam, m):
    v = Variant("plain", hip_device, beam)
    x = torch.from_numpy(M.LP5.copy()).to(hip_device)
    stream = v.stream(M.T6)
    stream.advance(x[:M.T5])
    tokens, lengths = stream.commit(max_tail=m)
    stream.advance(x[M.T5:])
    got = v.results(stream)
    assert stream.consumed.tolist() == [M.T6] * M.B
    for b in range(M.B):
        lp = M.LP5[:, b]
        done64, h64, margin = M.beam_search(lp, beam, beam, commits=[M.T5], max_tail=m)
        done32, h32, _ = M.beam_search(lp, beam, beam, dtype=np.float32, commits=[M.T5], max_tail=m)
        s64 = dict(h64)
        err = max([abs(s - s64[l]) for l, s in h32 if l in s64 and done32 == done64] + [0.0])
        bound = max(4 * err, 1e-6 * max(abs(s) for _, s in h64))
        separated = margin > 2 * bound
        real = labels_of(got, b)
        done = tuple(tokens[b, :lengths[b]].tolist())
        e_ref = max([abs(float(s) - ws) for (_, s), (_, ws) in zip(real, h64)] + [0.0]) if separated else float("nan")
        print("CTCCOMMIT forced+16 beam %d max_tail %d stream %d: score err %.3g (bound %.3g, margin %.3g, %s)" % (
            beam, m, b, e_ref, bound, margin, "separated" if separated else "NOT separated"))
        labels = [l for l, _ in real]
        assert len(set(labels)) == len(labels) and all(a[1] >= c[1] for a, c in zip(real, real[1:]))
        if separated:
            assert done == done64 and labels == [l for l, _ in h64], (b, done, done64)
            assert e_ref <= bound, (b, e_ref, bound)


# ---------------------------------------------------------------------------------------------------------------
# 7. graph capture
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "lm"])
def test_captured_advance_and_commit_equal_eager(hip_device, name):
    dev, k = hip_device, 8
    v = Variant(name, dev, 4)
    x = torch.from_numpy(M.LP1.copy()).to(dev)
    stream, eager = v.stream(M.T1), v.stream(M.T1)
    buf = x[:k].clone()
    lens = torch.full((M.B,), k, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up off the default stream (it allocates the scratch)
        stream.advance(buf, lens)
        stream.commit()
    torch.cuda.current_stream().wait_stream(side)
    stream.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stream.advance(buf, lens)
        out = stream.commit()
    stream.reset()
    committed, committed_eager = [[] for _ in range(M.B)], [[] for _ in range(M.B)]
    for s in range(0, M.T1, k):
        cl = torch.tensor(chunk_lengths(M.ILS1, s, k), dtype=torch.int32)
        buf.copy_(x[s:s + k])
        lens.copy_(cl)
        graph.replay()
        eager.advance(x[s:s + k], cl.to(dev))
        want = eager.commit()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
        take(committed, out)
        take(committed_eager, want)
    assert committed == committed_eager and sum(len(c) for c in committed) > 0
    for a, b in zip(v.results(stream), v.results(eager)):
        assert torch.equal(a, b)
    assert_joined(committed, v.results(stream), v.one_shot(x, M.ILS1), M.T1)
    assert stream.consumed.tolist() == M.ILS1 and stream.overflowed.tolist() == [False] * M.B
