"""HIP-event times of forward + backward of the CTC loss: pika_amd.ctc_loss, pika_amd.ctc_loss_from_logits and
torch.nn.functional.ctc_loss on the same device, same inputs.

    python tools/ctc_time.py [--runs 30] [--warmup 5] > profiles/ctc_time.txt

Shapes: the encoder's own (T = 240, B = 32, U = 50, C = 5000) and T = 1000.  Every timed call is one forward
(reduction='sum') + one backward to the (T,B,C) input, bracketed by two events on the current stream; each variant is
warmed up first, the variants alternate inside one loop so that drift hits them alike, and the median, minimum and
maximum of the runs are printed.  torch's path is timed from log-probs (as ours) and, for the fused boundary, behind
its own log_softmax.  Needs a GPU: there is no CPU timing.
"""
import argparse
import statistics
import sys

import torch
import torch.nn.functional as F

import pika_amd  # noqa: F401  (first: places the HIP runtime flag before torch initialises it)
from pika_amd import ctc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_time.py: no HIP device")
    if args.runs < 20:
        sys.exit("ctc_time.py: at least 20 runs")
    dev = torch.device("cuda")
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    for T, B, U, C in ((240, 32, 50, 5000), (1000, 32, 50, 5000)):
        g = torch.Generator().manual_seed(T)
        logits = torch.randn(T, B, C, generator=g).to(dev)
        targets = torch.randint(1, C, (B, U), generator=g).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = torch.full((B,), U, dtype=torch.int32, device=dev)
        il64, tl64 = il.long(), tl.long()
        lp = F.log_softmax(logits, -1)

        def ours_lp(x):
            return ctc.ctc_loss(x, targets, il, tl, reduction="sum")

        def ours_logits(x):
            return ctc.ctc_loss_from_logits(x, targets, il, tl, reduction="sum")

        def torch_lp(x):
            return F.ctc_loss(x, targets, il64, tl64, reduction="sum")

        def torch_logits(x):
            return F.ctc_loss(F.log_softmax(x, -1), targets, il64, tl64, reduction="sum")

        variants = [("pika_amd.ctc_loss(log_probs)", ours_lp, lp), ("torch F.ctc_loss(log_probs)", torch_lp, lp),
                    ("pika_amd.ctc_loss_from_logits(logits)", ours_logits, logits),
                    ("torch F.ctc_loss(log_softmax(logits))", torch_logits, logits)]
        times = {name: [] for name, _, _ in variants}
        values = {}

        def once(fn, src):
            x = src.detach().clone().requires_grad_(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = fn(x)
            loss.backward()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), float(loss)

        for name, fn, src in variants:
            for _ in range(args.warmup):
                once(fn, src)
        for _ in range(args.runs):
            for name, fn, src in variants:      # alternating
                ms, values[name] = once(fn, src)
                times[name].append(ms)
        print("\nT = %d, B = %d, U = %d, C = %d" % (T, B, U, C))
        for name, _, _ in variants:
            t = times[name]
            print("  %-42s %8.3f [%8.3f, %8.3f]   loss %.4f" % (name, statistics.median(t), min(t), max(t), values[name]))
        for ours, theirs in ((variants[0][0], variants[1][0]), (variants[2][0], variants[3][0])):
            a, b = statistics.median(times[ours]), statistics.median(times[theirs])
            print("  %s is %.2fx %s than %s" % (ours, max(a, b) / min(a, b), "FASTER" if a < b else "SLOWER", theirs))


if __name__ == "__main__":
    main()
