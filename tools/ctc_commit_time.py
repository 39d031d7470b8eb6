"""HIP-event times of `CtcBeamStream.commit` next to its yardsticks, and of the paths it must not touch.

    python tools/ctc_commit_time.py [--runs 30] [--warmup 5] [--parent-lib PATH] > profiles/ctc_commit_time.txt

Shape: (T,B,C) = (240,32,5000), beam 16, plain and LM-fused (candidates 32, the seeded bigram LM of tools/ctc_timing.py),
max_frames = T.

  one commit() call   on a stream that has consumed 40, 120 and 240 frames without a commit (the state is put back from
                      a copy before every timed bracket), next to one reset() of all streams and to the advance's time per
                      frame -- the uncommitted feed of 8-frame chunks over its 240 frames -- from the same loop
  a chunked feed      of 8-frame chunks with a commit after every chunk, against the same feed without commits
  the untouched paths ctc_beam_search, ctc_beam_search_lm (whole calls) and the uncommitted chunked feed through this
                      tree's library and, with --parent-lib (a libpika_amd.so built from the parent commit), through the
                      parent's, alternating: the new median is to lie within the [min, max] of the parent's own runs

Every variant is warmed up, the variants alternate inside one loop so that drift hits them alike, each is bracketed by
two events on the current stream, and median, minimum and maximum are printed.  Nothing here is asserted anywhere.
Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import bigram_lm, library, load_parent, measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_commit_time.py: no HIP device")
    if args.runs < 20:
        sys.exit("ctc_commit_time.py: at least 20 runs")
    dev = torch.device("cuda")
    _lib.lib()
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    print("parent library: %s" % (args.parent_lib or "none (the untouched paths are timed in this tree alone)"))
    T, B, C, beam, cand, k = 240, 32, 5000, 16, 32, 8
    fst, backoff_id = bigram_lm(C, 0, 20, 11)
    lm = ctc.CtcNgramLm(fst, backoff_id, device=dev)
    g = torch.Generator().manual_seed(T)
    lp = torch.log_softmax(torch.randn(T, B, C, generator=g).to(dev), -1)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    lens = torch.full((B,), k, dtype=torch.int32, device=dev)

    def on(handle, fn):
        def run():
            with library(handle):
                fn()
        return run

    def plain():
        ctc.ctc_beam_search(lp, il, beam=beam)

    def fused():
        ctc.ctc_beam_search_lm(lp, il, lm, beam=beam, candidates=cand)
    variants = [("ctc_beam_search (whole call), this tree", plain), ("ctc_beam_search_lm (whole call), this tree", fused)]
    if parent is not None:
        variants += [("ctc_beam_search (whole call), parent", on(parent, plain)),
                     ("ctc_beam_search_lm (whole call), parent", on(parent, fused))]
    streams = {"plain": ctc.CtcBeamStream(B, T, beam=beam, device=dev),
               "LM": ctc.CtcBeamStream(B, T, beam=beam, lm=lm, candidates=cand, device=dev)}
    shared = {}
    for kind, stream in streams.items():
        def feed(commit, stream=stream):
            def run():
                for s in range(0, T, k):
                    stream.advance(lp[s:s + k], lens)
                    if commit:
                        stream.commit()
            return run
        variants.append(("stream %s, reset() of all %d streams" % (kind, B), stream.reset))
        variants.append(("stream %s, chunks of %d, this tree" % (kind, k), (stream.reset, feed(False))))
        if parent is not None:
            variants.append(("stream %s, chunks of %d, parent" % (kind, k),
                             (on(parent, stream.reset), on(parent, feed(False)))))
        variants.append(("stream %s, chunks of %d, commit() per chunk" % (kind, k), (stream.reset, feed(True))))
        # the states after 40, 120 and 240 uncommitted frames, and what one commit shares on them
        stream.reset()
        for frames in (40, 120, 240):
            while int(stream.frames[0]) < frames:
                s = int(stream.frames[0])
                stream.advance(lp[s:s + k], lens)
            saved = stream._state.clone()
            shared[(kind, frames)] = stream.commit()[1].float().mean().item()
            stream._state.copy_(saved)

            def restore(stream=stream, saved=saved):
                stream._state.copy_(saved)
            variants.append(("stream %s, one commit() after %d frames" % (kind, frames), (restore, stream.commit)))
    times = measure(variants, args.warmup, args.runs)
    print("\nT = %d, B = %d, C = %d, beam = %d, candidates = %d, max_frames = %d" % (T, B, C, beam, cand, T))
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, _ in variants:
        t = times[name]
        line = "  %-52s %8.3f [%8.3f, %8.3f]" % (name, med[name], min(t), max(t))
        kind = "LM" if name.startswith("stream LM") else "plain"
        quiet = med["stream %s, chunks of %d, this tree" % (kind, k)]
        if name.endswith("this tree") and name.startswith("stream"):
            line += "   the advance: %.1f us per frame" % (1e3 * quiet / T)
        if name.endswith("commit() per chunk"):
            line += "   %.1f us per commit over the uncommitted feed" % (1e3 * (med[name] - quiet) / (T // k))
        if "one commit()" in name:
            frames = int(name.split()[-2])
            line += "   %.1f labels committed per stream" % shared[(kind, frames)]
        print(line)


if __name__ == "__main__":
    main()
