"""What the tests of the time stamps of the one-symbol-per-frame beam search share (include/pika_msearch_times.h): the
reference record `Replay` / `replay` -- pure numpy and Python, the definition applied to the (parent, token, active)
triples of the steps and to the commits --, `timed_search`, the reference search of `msearch_common` carrying times by
the representative rule, the path check, and `Tracker`, the hook that keeps a `ModifiedBeamTimes` and a `Replay` next to
a search that `msearch_stream_common.feed` drives.  No imports from test files."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msearch_common as M  # noqa: E402

NINF = -np.inf


class Replay(object):
    """The definition on Python lists: rows[b][k] is the record of slot k, as long as the slot's token sequence for a
    live slot (the rows of empty slots are never read: an empty slot is nobody's parent)."""

    def __init__(self, B, K, blank=0):
        self.B, self.K, self.blank = B, K, blank
        self.rows = [[[] for _ in range(K)] for _ in range(B)]
        self.consumed = [0] * B

    def step(self, parent, token, active):
        for b in range(self.B):
            if not active[b]:
                continue
            t, old = self.consumed[b], self.rows[b]
            self.consumed[b] = t + 1
            self.rows[b] = [list(old[int(parent[b][j])]) + ([t] if int(token[b][j]) != self.blank else [])
                            for j in range(self.K)]

    def commit(self, lengths, slot_map, live, selected=None):
        """live[b]: the number of live slots after the commit -> per stream the committed times (None: unselected)."""
        out = []
        for b in range(self.B):
            if selected is not None and not selected[b]:
                out.append(None)
                continue
            d, old = int(lengths[b]), self.rows[b]
            src = [int(s) for s in slot_map[b]]
            out.append([min(old[src[j]][i] for j in range(int(live[b]))) for i in range(d)] if live[b] else [-1] * d)
            self.rows[b] = [old[src[j]][d:] for j in range(self.K)]
        return out


def replay(history, B, K, blank=0):
    """history: ("step", parent (B,K), token (B,K), active (B,)) and ("commit", lengths (B,), slot_map (B,K), live (B,)
    [, selected (B,)]) -> (rows, [the output of every commit])."""
    r, outs = Replay(B, K, blank), []
    for ev in history:
        if ev[0] == "step":
            r.step(*ev[1:])
        else:
            outs.append(r.commit(*ev[1:]))
    return r.rows, outs


def timed_search(logits_of, T, V, K, blank=0, sm_scale=1.0, penalty=0.0, dtype=np.float64):
    """`msearch_common.search` carrying times by the representative rule: new slot j takes the times of the old slot of
    its group's best-ranked member, plus the frame when that member's symbol is a label.
    -> (beam, times per slot, history for `replay`)"""
    beam, times, history = M.start(K, dtype), [[] for _ in range(K)], []
    for t in range(T):
        beam, parent, token, info = M.step(beam, M.rows_of(logits_of, beam, t, V), blank, sm_scale, penalty, dtype)
        new = []
        for j, ranks in enumerate(info["groups"]):
            _, k, v = info["selected"][ranks[0]]                # the representative
            new.append(list(times[k]) + ([t] if v != blank else []))
        times = new + [[] for _ in range(K - len(new))]
        history.append(("step", parent[None], token[None], [True]))
    return beam, times, history


def path_value(logits_of, tokens, times, consumed, blank=0, sm_scale=1.0, penalty=0.0):
    """Checks that `times` is a time record of `tokens` over `consumed` frames -- strictly increasing, inside
    [0, consumed), one per label -- and returns the float64 log-probability of the path of the modified lattice "label i
    at frame times[i], blank elsewhere", the logits taken from the model on the path's own prefixes."""
    tokens, times = [int(v) for v in tokens], [int(v) for v in times]
    assert len(times) == len(tokens), (tokens, times)
    assert all(a < b for a, b in zip(times, times[1:])), times
    assert all(0 <= t < consumed for t in times), (times, consumed)
    at, prefix, total = dict(zip(times, tokens)), (), 0.0
    for t in range(consumed):
        lp = M.log_probs(np.asarray(logits_of(prefix, t), np.float64)[None], blank, sm_scale, penalty)[0]
        v = at.get(t, blank)
        total += lp[v]
        if v != blank:
            prefix = prefix + (v,)
    return total


class FrameModel(object):
    """A model for wide rows: logits_of(prefix, t) = E[t] + R[len(prefix) % 5] + a shift by the last token; no V x V
    table."""

    def __init__(self, T, V, seed, blank=0, scale=2.0):
        rng = np.random.RandomState(seed)
        self.E, self.R = scale * rng.randn(T, V), scale * rng.randn(5, V)
        self.blank, self.T, self.V = blank, T, V

    def __call__(self, prefix, t):
        return np.roll(self.E[t], (prefix[-1] if prefix else 0) % 3) + self.R[len(prefix) % 5]


def increasing(seq):
    return all(a < b for a, b in zip(seq, seq[1:]))


class Tracker(object):
    """The `after` hook of `msearch_stream_common.feed`: steps `times` (a `ModifiedBeamTimes` of the fed object) and a
    `Replay` side by side and compares them on the live slots after every step and every commit; keeps the history, the
    committed times per stream and what every commit returned.  skip: step numbers (from 0) at which the record's step is
    left out on purpose."""

    def __init__(self, times, check=True, skip=()):
        self.times, self.check, self.skip = times, check, set(skip)
        self.B, self.K = times.batch, times.beam
        self.ref = Replay(self.B, self.K, times.blank)
        self.history, self.committed, self.commits, self.n = [], [[] for _ in range(self.B)], [], 0
        self.prev, self.pre = [0] * self.B, None

    def consumed(self, obj):
        return (obj.consumed if hasattr(obj, "commit") else obj.frames).cpu().tolist()

    def slots(self, obj):
        """-> (the record's rows, the slots' lengths) as numpy"""
        ln = obj.hyps()[1].cpu().numpy()
        return self.times.hyps().cpu().numpy(), ln

    def compare(self, obj, where):
        got, ln = self.slots(obj)
        for b in range(self.B):
            for k in range(self.K):
                n = ln[b, k]
                if n < 0:
                    assert (got[b, k] == -1).all(), (where, b, k)
                    continue
                assert len(self.ref.rows[b][k]) == n, (where, b, k)
                assert got[b, k, :n].tolist() == self.ref.rows[b][k] and (got[b, k, n:] == -1).all(), (where, b, k)

    def monotone(self, obj, where):
        got, ln = self.slots(obj)
        for b in range(self.B):
            for k in range(self.K):
                if ln[b, k] >= 0:
                    assert increasing(self.committed[b] + got[b, k, :ln[b, k]].tolist()), (where, b, k)

    def __call__(self, obj, kind, out, committed):
        if kind == "step":
            parent, token = out
            now = self.consumed(obj)
            active = [a != p for a, p in zip(now, self.prev)]
            self.prev = now
            self.history.append(("step", parent.cpu().numpy().copy(), token.cpu().numpy().copy(), active))
            self.ref.step(*self.history[-1][1:])
            if self.n not in self.skip:
                self.times.step(parent, token)
            self.n += 1
        else:
            tokens, lengths, slot_map = out
            pre = self.pre                                      # the record's own rows just before the search's commit
            live = (obj.scores > NINF).sum(dim=1).cpu().tolist()
            when = self.times.commit(lengths, slot_map).cpu().numpy()
            ev = ("commit", lengths.cpu().numpy().copy(), slot_map.cpu().numpy().copy(), live)
            self.history.append(ev)
            want = self.ref.commit(*ev[1:])
            for b in range(self.B):
                d = int(ev[1][b])
                if self.check:
                    assert when[b, :d].tolist() == want[b] and (when[b, d:] == -1).all(), (self.n, b)
                    # the definition on the pre-commit records of the kernel itself
                    mine = [min(int(pre[b, ev[2][b, j], i]) for j in range(live[b])) for i in range(d)]
                    assert when[b, :d].tolist() == mine, (self.n, b)
                self.committed[b] += when[b, :d].tolist()
            self.commits.append(when)
        if self.check:
            self.compare(obj, (kind, self.n))
            self.monotone(obj, (kind, self.n))
        self.pre = self.slots(obj)[0]
