"""What the tests of the streaming one-symbol-per-frame beam search share (include/pika_msearch_stream.h): a peaked model
on `msearch_common.TableModel` and a driver that feeds a `ModifiedBeamStream` -- or a bare state, the one-shot run -- from
such models, frame by frame.  No imports from test files.

The model.  An exact commit gives back only what EVERY live hypothesis shares, and random logits never let a beam
converge.  A per-frame dominant class added to a `TableModel` alone does not help either: a hypothesis that left the
dominant path once pays once and follows the dominant classes ever after, so the beam keeps the cheapest deviations of
the whole past and its common ancestor never moves.  `PeakedModel` therefore adds the frame's dominant class only while
the prefix is the one the dominant path spells: a hypothesis off that path sees the (nearly flat) table alone, loses
about log V per frame, and is pushed out by the deviations of the latest frames.  It is a function of (prefix, frame) --
of the WHOLE prefix, which is why the driver evaluates it on committed + tail."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msearch_common as M  # noqa: E402

NINF = -np.inf


class PeakedModel(object):
    def __init__(self, T, V, seed, blank=0, boost=6.0, scale=0.3, p_blank=0.5):
        rng = np.random.RandomState(seed)
        self.table = M.TableModel(T, V, seed + 1, blank, scale)
        labels = [v for v in range(V) if v != blank]
        self.path = [blank if rng.rand() < p_blank else labels[rng.randint(len(labels))] for _ in range(T)]
        self.on_path, cur = [], ()
        for v in self.path:                      # the prefix the dominant path has spelled before frame t
            self.on_path.append(cur)
            cur = cur if v == blank else cur + (v,)
        self.boost, self.T, self.V = boost, T, V

    def __call__(self, prefix, t):
        row = np.array(self.table(prefix, t))
        if tuple(prefix) == self.on_path[t]:
            row[self.path[t]] += self.boost
        return row


def tails(obj):
    """Per stream, per slot: (score as the state holds it, the slot's uncommitted tokens) -- None for an empty slot."""
    hyp, ln = (t.cpu().numpy() for t in obj.hyps())
    sc = obj.scores.cpu().numpy()
    return [[(sc[b, k], tuple(int(v) for v in hyp[b, k, :ln[b, k]])) if ln[b, k] >= 0 else None
             for k in range(sc.shape[1])] for b in range(sc.shape[0])]


def whole(obj, committed):
    """`tails` with the committed text in front: what the one-shot search holds."""
    return [[None if e is None else (e[0].tobytes(), tuple(committed[b]) + e[1]) for e in row]
            for b, row in enumerate(tails(obj))]


def feed(obj, models, lens, chunk, every=None, each_chunk=False, sm_scale=1.0, penalty=0.0, commit=None, after=None):
    """Feeds `obj` -- a `ModifiedBeamStream`, or a bare state: the one-shot run -- max(lens) frames in chunks of `chunk`
    frames: num_frames grows by a chunk at a time, every `advance` is one frame.  Commits (`commit`: the keyword
    arguments) come after every `every` frames and / or after each chunk.  Stream b's rows are its models[b] on
    committed + tail at its own frame `consumed[b]`.
    -> (committed texts, trace): trace holds (parent, token, whole(...)) after every step;
    after(obj, kind, out, committed) is called after every step ("step", (parent, token)) and after every commit
    ("commit", (tokens, lengths, slot_map))."""
    B, K, V = obj.batch, obj.beam, models[0].V
    T, dev = max(lens), obj.device
    is_stream = hasattr(obj, "commit")
    committed, trace, steps = [[] for _ in range(B)], [], 0

    def do_commit():
        out = obj.commit(**(commit or {}))
        tokens, lengths = out[0].cpu().numpy(), out[1].cpu().numpy()
        for b in range(B):
            committed[b] += [int(v) for v in tokens[b, :lengths[b]]]
        if after is not None:
            after(obj, "commit", out, committed)

    for start in range(0, T, chunk):
        nf = torch.tensor([min(n, start + chunk) for n in lens], dtype=torch.int64, device=dev)
        for _ in range(start, min(start + chunk, T)):
            at = (obj.consumed if is_stream else obj.frames).cpu().tolist()
            rows = np.zeros((B * K, V))
            for b, row in enumerate(tails(obj)):
                for k, e in enumerate(row):
                    if e is not None and at[b] < lens[b]:
                        rows[b * K + k] = models[b](tuple(committed[b]) + e[1], at[b])
            logits = torch.from_numpy(rows).to(obj.dtype).to(dev)
            parent, token = obj.advance(logits, nf, sm_scale, penalty)
            trace.append((parent.cpu().numpy().copy(), token.cpu().numpy().copy(), whole(obj, committed)))
            if after is not None:
                after(obj, "step", (parent, token), committed)
            steps += 1
            if is_stream and every and steps % every == 0:
                do_commit()
        if is_stream and each_chunk:
            do_commit()
    return committed, trace


def same_trace(a, b):
    """Two traces agree: parent, token and every slot's score bits and whole token sequence, step by step."""
    assert len(a) == len(b)
    for i, ((p, t, w), (q, u, x)) in enumerate(zip(a, b)):
        assert (p == q).all() and (t == u).all(), i
        assert w == x, i
