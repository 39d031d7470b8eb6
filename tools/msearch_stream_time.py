"""HIP-event times of the streaming one-symbol-per-frame beam search (include/pika_msearch_stream.h).

    python tools/msearch_stream_time.py [--runs 10] [--warmup 3] [--out profiles/msearch_stream_time.txt]

At (B, K, V) = (64, 4, 5000) and (64, 16, 5000), max_frames = 64, float32 logits with a dominant label per frame (the
same rows for every slot, so the beam keeps the cheapest deviations of the whole past and a tail of n labels stands after
n frames):
* `ModifiedBeamStream.advance` next to the bare `ModifiedBeamState.advance`, 50 eager frame steps each (the reset is
  before the bracket): what the stream's subtraction of `retired` costs per step;
* one `commit()` on a beam with about 5 and about 50 uncommitted labels (the blob and the side record are restored
  before every bracket; the commit clears and rebuilds the stream's table, 2 K max_frames keys, whatever the tail);
* a chunk of 8 frame steps and one commit as one captured graph.
The variants alternate inside one loop, every one is warmed up, medians of `runs` with minimum and maximum.  Reported,
not gated: nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import ModifiedBeamState, ModifiedBeamStream

STEPS, MAX_FRAMES, CHUNK = 50, 64, 8


def peaked(B, K, V, frames, dev):
    """One (B K, V) tensor per frame: small noise and a dominant label that changes from frame to frame."""
    g = torch.Generator().manual_seed(K)
    out = []
    for t in range(frames):
        rows = 0.5 * torch.randn(B, 1, V, generator=g).expand(B, K, V).reshape(B * K, V).clone()
        rows[:, 1 + (37 * t) % (V - 1)] += 8.0
        out.append(rows.to(dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "msearch_stream_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("msearch_stream_time.py: no HIP device")
    dev = torch.device("cuda")
    lines = ["device: %s   runs %d, warm-up %d; max_frames %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup, MAX_FRAMES)]
    variants, per, notes = [], {}, {}
    for B, K, V in ((64, 4, 5000), (64, 16, 5000)):
        shape = "(B,K,V) = (%d,%d,%d)" % (B, K, V)
        logits = peaked(B, K, V, STEPS, dev)
        nf = torch.full((B,), STEPS, dtype=torch.int64, device=dev)
        state = ModifiedBeamState(B, MAX_FRAMES, K, 0, dev)
        stream = ModifiedBeamStream(B, MAX_FRAMES, K, 0, device=dev)

        def run(obj, logits=logits, nf=nf):
            for l in logits:
                obj.advance(l, nf)
        for name, obj in (("state.advance", state), ("stream.advance", stream)):
            name = "%s, %d eager steps, %s" % (name, STEPS, shape)
            variants.append((name, (obj.reset, lambda obj=obj, run=run: run(obj))))
            per[name] = STEPS
        for tail in (5, 50):                    # a stream with `tail` frames behind it, saved; restored before a bracket
            s = ModifiedBeamStream(B, MAX_FRAMES, K, 0, device=dev)
            for l in logits[:tail]:
                s.advance(l, nf)
            saved = (s.state._state.clone(), s._side.clone())
            labels = float(s.hyps()[1][:, 0].float().mean())
            lengths = s.commit()[1]
            torch.cuda.synchronize()

            def restore(s=s, saved=saved):
                s.state._state.copy_(saved[0])
                s._side.copy_(saved[1])
            name = "commit() after %d frames, %s" % (tail, shape)
            variants.append((name, (restore, s.commit)))
            per[name] = 1
            notes[name] = "best tail %.1f labels, %.1f of them committed" % (labels, float(lengths.float().mean()))
            if tail == 5:
                bufs = logits[tail:tail + CHUNK]
                nf8 = torch.full((B,), tail + CHUNK, dtype=torch.int64, device=dev)
                restore()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for l in bufs:
                        s.advance(l, nf8)
                    s.commit()
                name = "%d steps + commit, one graph, %s" % (CHUNK, shape)
                variants.append((name, (restore, graph.replay)))
                per[name] = 1
    times = measure(variants, args.warmup, args.runs)
    for name, _ in variants:
        t = times[name]
        lines.append("  %-58s %8.3f [%8.3f, %8.3f]   %7.1f us per %s%s" % (
            name, statistics.median(t), min(t), max(t), 1e3 * statistics.median(t) / per[name],
            "step" if per[name] > 1 else "call", "   (" + notes[name] + ")" if name in notes else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
