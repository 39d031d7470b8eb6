"""HIP-event times of forward + backward of `ctc_nbest_loss` next to the route a user had before it.

    python tools/ctc_nbest_loss_time.py [--runs 20] [--warmup 3] > profiles/ctc_nbest_loss_time.txt

Shapes: (T,B,C) = (240,32,5000) and (1000,32,5000), beam 16 / nbest 16; the hypotheses are `ctc_beam_search`'s own output
on the same input, fed as they come, with max_len = the longest of them (a host int, read before the loop).  Inputs as
tools/ctc_nbest_time.py: log_softmax(randn) at T = 240, whose transcripts have about one label per frame, and at both T
the same rows with the blank boosted on two frames of three ("speech-like": about T / 3 labels); at T = 1000 only the
second exists, plain rows giving transcripts beyond the 511 labels either route takes.

  the new call          x.requires_grad_(); full = ctc_nbest_loss(x, ...); (full * w).sum().backward() -- and the same
                        through ctc_nbest_loss_from_logits on the same tensor read as logits (row pass included)
  the replicated route  x.requires_grad_(); rep = x.repeat_interleave(nbest, dim=1) -- the (T, B * nbest, C) copy is
                        inside the bracket -- then ctc_loss(rep, ..., reduction='none'), (costs * w).sum().backward():
                        the dense (T, B * nbest, C) gradient, and its sum over nbest by repeat_interleave's backward.
                        One chunk: the whole batch at once (2 * 4 * T * B * nbest * C bytes live), no batch chunking.

Both produce the (T,B,C) gradient of the same weighted sum of scores.  Every variant is warmed up, the variants
alternate inside one loop so that drift hits them alike, each is bracketed by two events on the current stream, and
median, minimum and maximum are printed with the ratio new / replicated.  Nothing is tuned and nothing here is asserted
anywhere; no ratio was fixed in advance.  Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_nbest_loss_time.py: no HIP device")
    if args.runs < 10:
        sys.exit("ctc_nbest_loss_time.py: at least 10 runs")
    dev = torch.device("cuda")
    lib = _lib.lib()
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
        U = max(int(lengths.max()), 1)
        w = torch.randn(B, nbest, generator=g).to(dev)
        # the old route's transcripts: (B * nbest, U) padded rows, lengths clamped to 0 for a missing entry
        tg = tokens.reshape(B * nbest, T)[:, :U].clamp(min=0).contiguous()
        tl = lengths.reshape(-1).clamp(min=0)
        ilr = il.repeat_interleave(nbest)
        wr = w.reshape(-1)
        grads = {}

        def new(fn, name):
            def run():
                leaf = lp.detach().requires_grad_(True)
                full = fn(leaf, il, tokens, lengths, max_len=U)
                (torch.nan_to_num(full, nan=0.0, neginf=0.0) * w).sum().backward()
                grads[name] = leaf.grad
            return run

        def replicated():
            leaf = lp.detach().requires_grad_(True)
            rep = leaf.repeat_interleave(nbest, dim=1)
            costs = ctc.ctc_loss(rep, tg, ilr, tl, reduction="none", zero_infinity=True)
            (costs * -wr).sum().backward()
            grads["replicated"] = leaf.grad
        variants = [("ctc_nbest_loss fwd+bwd", new(ctc.ctc_nbest_loss, "new")),
                    ("ctc_nbest_loss_from_logits fwd+bwd", new(ctc.ctc_nbest_loss_from_logits, "logits")),
                    ("replicated: repeat_interleave + ctc_loss fwd+bwd + sum", replicated)]
        times = measure(variants, args.warmup, args.runs)
        med = {name: statistics.median(t) for name, t in times.items()}
        print("\nT = %d, B = %d, C = %d, beam = nbest = %d, %s; hypothesis lengths %d .. %d, max_len = %d" % (
            T, B, C, beam, "blank boosted on 2 frames of 3" if boosted else "plain randn rows", int(lengths.min()), U, U))
        print("  workspace %.1f MB; replicated input + gradient %.1f MB" % (
            lib.pika_ctc_nbest_loss_workspace_bytes(B, nbest, T, U) / 1e6, 2 * 4.0 * T * B * nbest * C / 1e6))
        for name, _ in variants:
            t = times[name]
            print("  %-56s %9.3f [%9.3f, %9.3f]" % (name, med[name], min(t), max(t)))
        old = med[variants[2][0]]
        for name in (variants[0][0], variants[1][0]):
            print("  %-36s %.3fx the replicated route's time (%s)" % (
                name, med[name] / old, "faster" if med[name] < old else "NOT faster"))
        # both routes differentiate the same sum wherever every entry exists
        if int(lengths.min()) >= 0:
            print("  largest difference between the two routes' gradients: %.3g" % float(
                (grads["new"] - grads["replicated"]).abs().max()))


if __name__ == "__main__":
    main()
