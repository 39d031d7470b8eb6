"""HIP-event times of the streaming CTC beam search next to the one-shot searches on the same input.

    python tools/ctc_stream_time.py [--runs 30] [--warmup 5] [--parent-lib PATH] > profiles/ctc_stream_time.txt

Shape: (T,B,C) = (240,32,5000), beam 16, plain and LM-fused (candidates 32, the seeded bigram LM of tools/ctc_timing.py).
The utterance is fed to a `CtcBeamStream` in chunks of 8, 16 and 40 frames -- per chunk one row pass and one advance,
whole Python calls; the reset happens before the timed bracket and is timed on its own -- and the total is printed with
the per-chunk overhead: (total - the one-shot whole call) / chunks.  The same feed with one `results(nbest=1)` per chunk
gives the cost of a partial result.
The one-shot whole calls are also timed at (1000,32,5000), the second shape of the one-shot tools.

--parent-lib: a libpika_amd.so built from the parent commit.  The one-shot whole calls then run through both libraries,
alternating, so that "did the one-shot kernels change" is answered inside one session: the new median is to lie within
the [min, max] of the parent's own runs.  Without it the one-shot rows are this tree's alone.

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
        sys.exit("ctc_stream_time.py: no HIP device")
    if args.runs < 20:
        sys.exit("ctc_stream_time.py: at least 20 runs")
    dev = torch.device("cuda")
    _lib.lib()
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    print("parent library: %s" % (args.parent_lib or "none (one-shot times are this tree's)"))
    beam, C, cand, B = 16, 5000, 32, 32
    fst, backoff_id = bigram_lm(C, 0, 20, 11)
    lm = ctc.CtcNgramLm(fst, backoff_id, device=dev)

    for T in (240, 1000):
        g = torch.Generator().manual_seed(T)
        lp = torch.log_softmax(torch.randn(T, B, C, generator=g).to(dev), -1)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)

        def plain():
            ctc.ctc_beam_search(lp, il, beam=beam)

        def fused():
            ctc.ctc_beam_search_lm(lp, il, lm, beam=beam, candidates=cand)

        def on(handle, fn):
            def run():
                with library(handle):
                    fn()
            return run
        variants = [("ctc_beam_search (whole call), this tree", plain),
                    ("ctc_beam_search_lm (whole call), this tree", fused)]
        if parent is not None:
            variants += [("ctc_beam_search (whole call), parent", on(parent, plain)),
                         ("ctc_beam_search_lm (whole call), parent", on(parent, fused))]
        chunked = {}
        if T == 240:
            streams = {"plain": ctc.CtcBeamStream(B, T, beam=beam, device=dev),
                       "LM": ctc.CtcBeamStream(B, T, beam=beam, lm=lm, candidates=cand, device=dev)}
            lens = {k: torch.full((B,), k, dtype=torch.int32, device=dev) for k in (8, 16, 40)}

            def feed(stream, k, look):
                def run():
                    for s in range(0, T, k):
                        stream.advance(lp[s:s + k], lens[k])
                        if look:
                            stream.results(nbest=1)
                return (stream.reset, run)
            for kind, stream in streams.items():
                variants.append(("stream %s, reset() of all %d streams" % (kind, B), stream.reset))
                for k in (8, 16, 40):
                    for look in (False, True):
                        name = "stream %s, chunks of %d%s" % (kind, k, ", results(nbest=1) per chunk" if look else "")
                        chunked[name] = (kind, k, look)
                        variants.append((name, feed(stream, k, look)))
        times = measure(variants, args.warmup, args.runs)
        print("\nT = %d, B = %d, C = %d, beam = %d, candidates = %d" % (T, B, C, beam, cand))
        med = {name: statistics.median(t) for name, t in times.items()}
        base = {"plain": med["ctc_beam_search (whole call), parent" if parent else "ctc_beam_search (whole call), this tree"],
                "LM": med["ctc_beam_search_lm (whole call), parent" if parent
                          else "ctc_beam_search_lm (whole call), this tree"]}
        for name, _ in variants:
            t = times[name]
            line = "  %-58s %8.3f [%8.3f, %8.3f]" % (name, med[name], min(t), max(t))
            if name in chunked:
                kind, k, look = chunked[name]
                n = T // k
                if look:
                    quiet = med["stream %s, chunks of %d" % (kind, k)]
                    line += "   %.1f us per results call" % (1e3 * (med[name] - quiet) / n)
                else:
                    line += "   %d chunks, %.1f us over the one-shot call per chunk" % (n, 1e3 * (med[name] - base[kind]) / n)
            print(line)


if __name__ == "__main__":
    main()
