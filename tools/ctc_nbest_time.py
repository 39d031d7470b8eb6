"""HIP-event times of `ctc_nbest_align` next to the only route the parent commit has, and to the search itself.

    python tools/ctc_nbest_time.py [--runs 30] [--warmup 5] > profiles/ctc_nbest_time.txt

Shapes: (T,B,C) = (240,32,5000) and (1000,32,5000), beam 16 / nbest 16; the hypotheses are the search's own output
(tokens (B,16,T), lengths (B,16)), fed as they come.  Inputs: log_softmax(randn) at T = 240, whose transcripts have
about one label per frame, and at both T the same rows with the blank boosted on two frames of three ("speech-like":
about T / 3 labels).  At T = 1000 only the second exists: a transcript of plain randn rows has some 1000 labels there,
beyond the 511 that either route takes.

  the new call        ctc_nbest_align on the log-probs and ctc_nbest_align_from_logits on the same tensor read as logits
                      (the row pass for the log-sum-exps included)
  the replicated route   for the same hypotheses: repeat_interleave(nbest, dim=1) of the input -- the (T, B * nbest, C)
                      copy is inside the bracket -- then ctc_align and ctc_loss(reduction='none') on it
  the search          ctc_beam_search(beam 16, nbest 16), whole call

Every variant is warmed up, the variants alternate inside one loop so that drift hits them alike, each is bracketed by
two events on the current stream, and median, minimum and maximum are printed.  The acceptance condition -- the new call
takes less time than the replicated route at every shape -- is stated with its outcome; nothing is tuned and nothing
here is asserted anywhere.  Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_nbest_time.py: no HIP device")
    if args.runs < 20:
        sys.exit("ctc_nbest_time.py: at least 20 runs")
    dev = torch.device("cuda")
    _lib.lib()
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    B, C, beam, nbest = 32, 5000, 16, 16
    held = True
    for T, boosted in ((240, False), (240, True), (1000, True)):
        g = torch.Generator().manual_seed(T)
        x = torch.randn(T, B, C, generator=g).to(dev)
        if boosted:
            x[torch.arange(T, device=dev) % 3 != 0, :, 0] += 12.0
        lp = torch.log_softmax(x, -1)
        del x
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tokens, lengths, _ = ctc.ctc_beam_search(lp, il, beam=beam, nbest=nbest)
        U = int(lengths.max())
        # the old route's transcripts: (B * nbest, U) padded rows, lengths clamped to 0 for a missing entry
        tg = tokens.reshape(B * nbest, T)[:, :max(U, 1)].clamp(min=0).contiguous()
        tl = lengths.reshape(-1).clamp(min=0)
        ilr = il.repeat_interleave(nbest)

        def new():
            ctc.ctc_nbest_align(lp, il, tokens, lengths)

        def new_logits():
            ctc.ctc_nbest_align_from_logits(lp, il, tokens, lengths)

        def replicated():
            rep = lp.repeat_interleave(nbest, dim=1)
            ctc.ctc_align(rep, tg, ilr, tl)
            ctc.ctc_loss(rep, tg, ilr, tl, reduction="none")

        def search():
            ctc.ctc_beam_search(lp, il, beam=beam, nbest=nbest)
        variants = [("ctc_nbest_align", new), ("ctc_nbest_align_from_logits", new_logits),
                    ("replicated: repeat_interleave + ctc_align + ctc_loss", replicated),
                    ("ctc_beam_search (whole call)", search)]
        times = measure(variants, args.warmup, args.runs)
        med = {name: statistics.median(t) for name, t in times.items()}
        print("\nT = %d, B = %d, C = %d, beam = nbest = %d, %s; hypothesis lengths %d .. %d, max_len = %d" % (
            T, B, C, beam, "blank boosted on 2 frames of 3" if boosted else "plain randn rows", int(lengths.min()), U,
            min(T, 511)))
        for name, _ in variants:
            t = times[name]
            print("  %-54s %9.3f [%9.3f, %9.3f]" % (name, med[name], min(t), max(t)))
        old, srch = med[variants[2][0]], med[variants[3][0]]
        for name in (variants[0][0], variants[1][0]):
            ok = med[name] < old
            held = held and ok
            print("  %-28s %.2fx the replicated route's time (%s), %.1f%% of the search's" % (
                name, med[name] / old, "less: the condition holds" if ok else "NOT less: the condition FAILS",
                100.0 * med[name] / srch))
    print("\nacceptance condition (the new call takes less time than the replicated route at every shape): %s"
          % ("holds" if held else "DOES NOT HOLD"))


if __name__ == "__main__":
    main()
