"""HIP-event times of the long-form loss, forward plus backward, next to its competitors, and its split by kernel.

    python tools/ctc_long_loss_time.py [--runs 10] [--warmup 2] > profiles/ctc_long_loss_time.txt

1. Long shapes, (T,B,U,C) = (3000,8,1500,64) and (1500,32,600,5000): `ctc_long_loss_from_logits` against torch's native
   device kernel, `F.ctc_loss` behind `log_softmax`, forward plus backward to d/d logits, alternating in one loop on the
   same device and the same seeded `randn` logits; whole-step time between two events, median of `runs`.  The costs of
   both are printed: faster and different would not be faster.
2. At (1000,32,334,5000), which the one-workgroup kernels can do: `ctc_long_loss_from_logits` against the existing
   `ctc_loss_from_logits`, the same way.  Reported, not gated: nothing replaces the existing path.
3. The split of the tiled path by kernel at every shape: device time of the kernels of each kind under torch.profiler,
   in runs of their own, median of `runs`.
No ratio was fixed in advance and nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc

KINDS = (("decoders' row pass (lse)", "ctc_rows_kernel"), ("row maxima", "lloss_rows_kernel"),
         ("label sort", "lloss_sort_kernel"), ("alpha/beta launches", "lloss_dp_kernel"), ("ll and costs", "lloss_finish_kernel"),
         ("gradient", "lloss_grad_kernel"))


def stats(v):
    return "%9.3f [%9.3f, %9.3f]" % (statistics.median(v), min(v), max(v))


def batch(T, B, U, C, seed, dev):
    """Seeded randn logits, random transcripts of U and fewer labels, full and shorter lengths, everything on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(T, B, C, generator=g, device=dev)
    rng = np.random.default_rng(seed)
    tl = np.maximum(U - rng.integers(0, U // 4 + 1, size=B), 1)
    tl[0] = U
    il = np.maximum(T - rng.integers(0, T // 8 + 1, size=B), 1)
    il[0] = T
    targets = rng.integers(1, C, size=(B, U))
    return (x, torch.from_numpy(targets).to(dev), torch.from_numpy(il).to(dev, torch.int32),
            torch.from_numpy(tl).to(dev, torch.int32))


def split(fn, runs):
    """{kind: [ms per run]}, {kind: launches per run} from the device times of the kernels of one call under torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    out, counts = {k: [] for k, _ in KINDS}, {}
    for _ in range(runs):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        total = {k: 0.0 for k, _ in KINDS}
        for e in prof.events():
            for k, needle in KINDS:
                if needle in e.name:
                    total[k] += float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
                    counts[k] = counts.get(k, 0) + 1
        for k in total:
            out[k].append(total[k] / 1000.0)
    return out, {k: v // runs for k, v in counts.items()}


def steps(x, targets, il, tl):
    """The three forward-plus-backward steps on one batch, each returning its costs."""
    x = x.clone().requires_grad_(True)
    il64, tl64 = il.long(), tl.long()

    def ours(fn):
        def step():
            costs = fn(x, targets, il, tl, reduction="none")
            torch.autograd.grad(costs.sum(), x)
            return costs.detach()
        return step

    def native():
        costs = F.ctc_loss(F.log_softmax(x, -1), targets, il64, tl64, reduction="none")
        torch.autograd.grad(costs.sum(), x)
        return costs.detach()
    return ours(ctc.ctc_long_loss_from_logits), native, ours(ctc.ctc_loss_from_logits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_long_loss_time.py: no HIP device")
    if args.runs < 5:
        sys.exit("ctc_long_loss_time.py: at least 5 runs")
    dev = torch.device("cuda")
    lib = _lib.lib()
    print("device: %s   runs %d, warm-up %d; forward plus backward, times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    for n, (T, B, U, C, rival) in enumerate(((3000, 8, 1500, 64, "torch"), (1500, 32, 600, 5000, "torch"),
                                             (1000, 32, 334, 5000, "ctc_loss_from_logits"))):
        tiled, native, existing = steps(*batch(T, B, U, C, n + 1, dev))
        other = native if rival == "torch" else existing
        name = "torch F.ctc_loss(log_softmax)" if rival == "torch" else rival
        print("\n%d. (T,B,U,C) = (%d,%d,%d,%d): %d tiles of %d states, %d launches of %d frames; workspace %.3f GB, dense "
              "gradient %.3f GB" % (n + 1, T, B, U, C, -(-(2 * U + 1) // ctc.LONG_LOSS_TILE), ctc.LONG_LOSS_TILE,
                                    -(-T // ctc.LONG_LOSS_FRAMES), ctc.LONG_LOSS_FRAMES,
                                    lib.pika_ctc_long_loss_workspace_bytes(B, T, U) / 2.0 ** 30, 4.0 * T * B * C / 2.0 ** 30))
        times = measure([("ctc_long_loss_from_logits", tiled), (name, other)], args.warmup, args.runs)
        for k in ("ctc_long_loss_from_logits", name):
            print("   %-30s %s" % (k, stats(times[k])))
        a, b = tiled().double(), other().double()
        print("   ratio tiled / %s: %.3fx; largest relative difference of the costs %.3g" % (
            name, statistics.median(times["ctc_long_loss_from_logits"]) / statistics.median(times[name]),
            float(((a - b).abs() / b.abs()).max())))
        try:
            parts, counts = split(tiled, args.runs)
            for k, _ in KINDS:
                print("   %-26s %5d launch(es) %s" % (k, counts.get(k, 0), stats(parts[k])))
            print("   sum of the kernels' device times   %9.3f  (the rest of the step is launch gaps, the wrapper and autograd)"
                  % sum(statistics.median(parts[k]) for k, _ in KINDS))
        except Exception as err:        # a profiler that cannot run here: the whole-step times stand alone
            print("   split unavailable: %s: %s" % (type(err).__name__, err))
        del tiled, native, existing, other
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
