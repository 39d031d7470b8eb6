"""HIP-event times of the n-best edit distances on the device next to the host routes a user had before them.

    python tools/ctc_edit_time.py [--runs 10] [--warmup 2] > profiles/ctc_edit_time.txt

Shapes: B = 32, beam 16 / nbest 16, C = 5000; the hypotheses are `ctc_beam_search`'s own output, fed as they come.  Inputs
as tools/ctc_nbest_loss_time.py: log_softmax(randn) at T = 240, whose transcripts have about one label per frame, and at
T = 240 and T = 1000 the same rows with the blank boosted on two frames of three (about T / 3 labels).  The reference
transcript of an utterance is its first hypothesis with one token in eight replaced, so both sides have about the same
number of labels.

  ctc_nbest_edit_distance      against  ctc_nbest_errors on the same DEVICE tensors: the function as it was the only
                                        route, its device-to-host copies, list building and upload included
  ctc_nbest_pairwise_distance  against  pika_amd.mbr.edit_distances over the same N * N pairs per utterance, from the same
                                        device tensors (copy, lists, the library's two-row DP on one thread, upload), and
                                        the bare library call on lists prepared beforehand

Every variant is warmed up, the variants alternate inside one loop, each is bracketed by two events on the current
stream -- the host routes end in copies that wait for the host, so the bracket holds their host time -- and median,
minimum and maximum are printed with the ratio new / old.  Results are compared for equality once per shape.  Nothing is
tuned and nothing here is asserted anywhere; no ratio was fixed in advance.  Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import ctc
from pika_amd.mbr import edit_distances


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_edit_time.py: no HIP device")
    if args.runs < 5:
        sys.exit("ctc_edit_time.py: at least 5 runs")
    dev = torch.device("cuda")
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    B, C, beam, nbest = 32, 5000, 16, 16
    for T, boosted in ((240, False), (240, True), (1000, True)):
        g = torch.Generator().manual_seed(T)
        x = torch.randn(T, B, C, generator=g).to(dev)
        if boosted:
            x[torch.arange(T, device=dev) % 3 != 0, :, 0] += 12.0
        lp = torch.log_softmax(x, -1)
        del x
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tokens, lengths, _ = ctc.ctc_beam_search(lp, il, beam=beam, nbest=nbest)
        del lp
        tl = lengths[:, 0].clamp(min=0)
        S = max(int(tl.max()), 1)
        targets = tokens[:, 0, :S].clone()
        swap = torch.arange(S, device=dev) % 8 == 3
        targets[:, swap] = torch.randint(1, C, (B, int(swap.sum())), generator=g, dtype=torch.int32).to(dev)
        out = {}

        def pairs_of(tok, ln):
            L = len(tok[0][0])
            return [(tok[b][i][:max(0, min(ln[b][i], L))], tok[b][j][:max(0, min(ln[b][j], L))])
                    for b in range(B) for i in range(nbest) for j in range(nbest)]
        prepared = pairs_of(tokens.cpu().tolist(), lengths.cpu().tolist())

        def new_errors():
            out["new"] = ctc.ctc_nbest_edit_distance(tokens, lengths, targets, tl)

        def old_errors():
            out["old"] = ctc.ctc_nbest_errors(tokens, lengths, targets, tl)

        def new_pairwise():
            out["pair_new"] = ctc.ctc_nbest_pairwise_distance(tokens, lengths)

        def old_pairwise():
            ln = lengths.cpu()
            d = torch.tensor(edit_distances(pairs_of(tokens.cpu().tolist(), ln.tolist())), dtype=torch.float32)
            dead = (ln < 0).unsqueeze(2) | (ln < 0).unsqueeze(1)
            out["pair_old"] = d.reshape(B, nbest, nbest).masked_fill(dead, 0.0).to(dev)

        def bare_pairwise():
            edit_distances(prepared)
        variants = [("ctc_nbest_edit_distance", new_errors), ("ctc_nbest_errors (host route)", old_errors),
                    ("ctc_nbest_pairwise_distance", new_pairwise),
                    ("mbr.edit_distances over N*N pairs (host route)", old_pairwise),
                    ("mbr.edit_distances, lists prepared (library call only)", bare_pairwise)]
        times = measure(variants, args.warmup, args.runs)
        med = {name: statistics.median(t) for name, t in times.items()}
        live = lengths[lengths >= 0]
        print("\nT = %d, B = %d, C = %d, beam = nbest = %d, %s; hypothesis lengths %d .. %d (mean %.0f), references %d .. %d"
              % (T, B, C, beam, "blank boosted on 2 frames of 3" if boosted else "plain randn rows", int(live.min()),
                 int(live.max()), float(live.float().mean()), int(tl.min()), int(tl.max())))
        for name, _ in variants:
            t = times[name]
            print("  %-58s %10.3f [%10.3f, %10.3f]" % (name, med[name], min(t), max(t)))
        for new, old in ((0, 1), (2, 3), (2, 4)):
            a, b = med[variants[new][0]], med[variants[old][0]]
            print("  %-28s %.5fx the time of: %s (%s)" % (variants[new][0], a / b, variants[old][0],
                                                         "faster" if a < b else "NOT faster"))
        print("  results equal: errors %s, pairwise %s" % (torch.equal(out["new"], out["old"]),
                                                           torch.equal(out["pair_new"], out["pair_old"])))


if __name__ == "__main__":
    main()
