"""HIP-event times of the time stamps of the one-symbol-per-frame beam search (include/pika_msearch_times.h).

    python tools/msearch_times_time.py [--runs 10] [--warmup 3] [--out profiles/msearch_times_time.txt]

At (B, K, V) = (64, 4, 5000) and (64, 16, 5000), with max_frames = 1000 and max_frames = 64, float32 logits with a
dominant label per frame (the same rows for every slot, so a hypothesis of n labels stands after n frames):
* `advance` alone next to `advance + times.step`, 50 frame steps each from a reset state, eager and as one captured graph;
* one `times.commit` next to the stream's own `commit` on a beam with about 5 and about 50 uncommitted labels (blob,
  side record and time record are restored before every bracket);
* one `times.results` for the entries of a `results(nbest=K)` call after 50 frames.
The variants alternate inside one loop, every one is warmed up, medians of `runs` with minimum and maximum.  Reported,
not gated: nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from msearch_stream_time import peaked
from pika_amd import ModifiedBeamState, ModifiedBeamStream, ModifiedBeamTimes

STEPS = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "msearch_times_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("msearch_times_time.py: no HIP device")
    dev = torch.device("cuda")
    lines = ["device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup)]
    variants, per, notes = [], {}, {}
    for B, K, V in ((64, 4, 5000), (64, 16, 5000)):
        logits = peaked(B, K, V, STEPS, dev)
        nf = torch.full((B,), STEPS, dtype=torch.int64, device=dev)
        for mf in (1000, 64):
            shape = "(B,K,V,max_frames) = (%d,%d,%d,%d)" % (B, K, V, mf)
            state = ModifiedBeamState(B, mf, K, 0, dev)
            times = ModifiedBeamTimes(state)

            def reset(state=state, times=times):
                state.reset()
                times.reset()

            def plain(state=state, logits=logits, nf=nf):
                for l in logits:
                    state.advance(l, nf)

            def timed(state=state, times=times, logits=logits, nf=nf):
                for l in logits:
                    times.step(*state.advance(l, nf))
            graphs = []
            for fn in (plain, timed):
                reset()
                fn()                                        # (warm: the capture allocates nothing new)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                graphs.append(g)
            for name, fn in (("advance, eager", plain), ("advance + times.step, eager", timed),
                             ("advance, one graph", graphs[0].replay),
                             ("advance + times.step, one graph", graphs[1].replay)):
                name = "%s, %d steps, %s" % (name, STEPS, shape)
                variants.append((name, (reset, fn)))
                per[name] = STEPS
            reset()
            timed()
            tokens, lengths, _ = state.results(nbest=K)
            name = "times.results(nbest=%d) after %d frames, %s" % (K, STEPS, shape)
            variants.append((name, (lambda: None, lambda times=times, t=tokens, n=lengths: times.results(t, n))))
            per[name] = 1
            notes[name] = "best entry %.1f labels" % float(lengths[:, 0].float().mean())
            for tail in (5, 50):                # a stream with `tail` frames behind it, saved before and after its commit
                s = ModifiedBeamStream(B, mf, K, 0, device=dev)
                st = ModifiedBeamTimes(s)
                for l in logits[:tail]:
                    st.step(*s.advance(l, nf))
                before = (s.state._state.clone(), s._side.clone(), st._rec.clone())
                labels = float(s.hyps()[1][:, 0].float().mean())
                _, clen, slot_map = s.commit()
                after = (s.state._state.clone(), s._side.clone())
                torch.cuda.synchronize()

                def restore(s=s, st=st, saved=before):
                    s.state._state.copy_(saved[0])
                    s._side.copy_(saved[1])
                    st._rec.copy_(saved[2])

                def committed(s=s, st=st, saved=after, rec=before[2]):
                    s.state._state.copy_(saved[0])
                    s._side.copy_(saved[1])
                    st._rec.copy_(rec)
                for name, pair in (("stream.commit()", (restore, s.commit)),
                                   ("times.commit()", (committed, lambda st=st, n=clen, m=slot_map: st.commit(n, m)))):
                    name = "%s after %d frames, %s" % (name, tail, shape)
                    variants.append((name, pair))
                    per[name] = 1
                    notes[name] = "best tail %.1f labels, %.1f of them committed" % (labels, float(clen.float().mean()))
    result = measure(variants, args.warmup, args.runs)
    for name, _ in variants:
        t = result[name]
        lines.append("  %-84s %8.3f [%8.3f, %8.3f]   %7.1f us per %s%s" % (
            name, statistics.median(t), min(t), max(t), 1e3 * statistics.median(t) / per[name],
            "step" if per[name] > 1 else "call", "   (" + notes[name] + ")" if name in notes else ""))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
