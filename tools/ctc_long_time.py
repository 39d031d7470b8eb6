"""HIP-event times of the long-form alignment, its split by launch kind, and the precision of its normalisation.

    python tools/ctc_long_time.py [--runs 10] [--warmup 2] [--frames 90000] [--labels 15000] > profiles/ctc_long_time.txt

1. One recording at (T, U, C) = (90 000, 15 000, 5000) -- an hour at 40 ms per frame against its transcript; when the
   device's free memory does not hold it the shape is halved until it does, and the shape used is printed.  The input is
   the log-softmax of a PEAKED random model: unit normal logits with +12 on the class a random segmentation of the
   transcript puts at each frame, so a well-aligned path exists.  Whole-call time between two events, median of `runs`;
   the split into the row pass, the recurrence launches, the back-trace and the token outputs is the device time of the
   kernels of each kind under torch.profiler, per run, median of `runs`.
2. The precision claim of the normalisation on that shape: |scores - fp64 rescore of the returned path|, the path rebuilt
   from starts / ends and summed in float64 on the device.
3. At a shape both can do, (T,B,U,C) = (4000,1,511,5000): `ctc_long_align` next to `ctc_align`, alternating in one loop.
No ratio was fixed in advance and nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import statistics
import sys

import numpy as np
import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc

KINDS = (("row pass", "long_rows_kernel"), ("recurrence launches", "long_dp_kernel"), ("back-trace", "long_trace_kernel"),
         ("token outputs", "long_tokens_kernel"))


def peaked(T, U, C, seed, dev):
    """(log_probs (T,1,C) on the device, targets (1,U)): a random transcript, a random segmentation of it over T frames
    (every token a run of 1-3 frames, blanks between), +12 on the segmentation's class at every frame."""
    rng = np.random.default_rng(seed)
    seq = rng.integers(1, C, size=U)
    runs = rng.integers(1, 4, size=U)
    spare = T - int(runs.sum())
    assert spare >= U, "T too short for the segmentation"
    cuts = np.sort(rng.integers(0, spare - U + 1, size=U))      # blanks before token j: cuts[j] - cuts[j-1] + 1
    gaps = np.diff(np.concatenate([[0], cuts])) + 1
    labels = np.zeros(T, dtype=np.int64)
    t = 0
    for j in range(U):
        t += int(gaps[j])
        labels[t:t + runs[j]] = seq[j]
        t += int(runs[j])
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(T, 1, C, generator=g, device=dev)
    x[torch.arange(T, device=dev), 0, torch.from_numpy(labels).to(dev)] += 12.0
    x -= torch.logsumexp(x, -1, keepdim=True)
    return x, torch.from_numpy(seq)[None].to(dev)


def stats(v):
    return "%9.3f [%9.3f, %9.3f]" % (statistics.median(v), min(v), max(v))


def split(fn, runs):
    """{kind: [ms per run]} from the device times of the kernels of one call under torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    out = {k: [] for k, _ in KINDS}
    counts = {}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=90000)
    ap.add_argument("--labels", type=int, default=15000)
    ap.add_argument("--classes", type=int, default=5000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_long_time.py: no HIP device")
    if args.runs < 5:
        sys.exit("ctc_long_time.py: at least 5 runs")
    dev = torch.device("cuda")
    lib = _lib.lib()
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    T, U, C = args.frames, args.labels, args.classes
    free = torch.cuda.mem_get_info()[0]
    while 3 * 4 * T * C + lib.pika_ctc_long_align_scratch_bytes(1, T, U) > 0.8 * free and T > 1000:
        T, U = T // 2, U // 2
    scratch = lib.pika_ctc_long_align_scratch_bytes(1, T, U)
    print("\n1. long shape (T,B,U,C) = (%d,1,%d,%d): %d tiles of %d states, %d launches of %d frames; scratch %.3f GB "
          "(free device memory %.1f GB)" % (T, U, C, -(-(2 * U + 1) // ctc.LONG_ALIGN_TILE), ctc.LONG_ALIGN_TILE,
                                            -(-T // ctc.LONG_ALIGN_FRAMES), ctc.LONG_ALIGN_FRAMES, scratch / 2.0 ** 30,
                                            free / 2.0 ** 30))
    lp, targets = peaked(T, U, C, 1, dev)
    call = lambda: ctc.ctc_long_align(lp, targets)      # noqa: E731
    times = measure([("ctc_long_align", call)], args.warmup, args.runs)
    print("   ctc_long_align, whole call        %s" % stats(times["ctc_long_align"]))
    try:
        parts, counts = split(call, args.runs)
        for k, _ in KINDS:
            print("   %-22s %5d launch(es) %s" % (k, counts.get(k, 0), stats(parts[k])))
        print("   sum of the kernels' device times  %9.3f  (the rest of the whole call is launch gaps and the wrapper)"
              % sum(statistics.median(parts[k]) for k, _ in KINDS))
    except Exception as err:        # a profiler that cannot run here: the whole-call time stands alone
        print("   split unavailable: %s: %s" % (type(err).__name__, err))

    scores, starts, ends, ts = call()
    tok = targets[0].long()
    mark = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    mark.index_add_(0, starts[0].long(), tok)
    mark.index_add_(0, ends[0].long() + 1, -tok)
    labels = mark.cumsum(0)[:T]
    rescore = lp[:, 0].gather(1, labels[:, None]).double().sum()
    err = abs(float(scores[0].double() - rescore))
    print("\n2. normalisation: score %.6f, fp64 rescore of the returned path %.6f, |difference| %.3e "
          "(one fp32 ulp of the score: %.3e); frames on a label %d, mean token confidence %.4f" % (
              float(scores[0]), float(rescore), err, float(np.spacing(np.float32(abs(float(scores[0]))))),
              int((labels != 0).sum()), float((ts[0] / (ends[0] - starts[0] + 1)).exp().mean())))
    del lp, targets, scores, starts, ends, ts, mark, labels

    T, U = 4000, 511
    lp, targets = peaked(T, U, C, 2, dev)
    il, tl = torch.tensor([T], dtype=torch.int32, device=dev), torch.tensor([U], dtype=torch.int32, device=dev)
    times = measure([("ctc_long_align", lambda: ctc.ctc_long_align(lp, targets, il, tl)),
                     ("ctc_align", lambda: ctc.ctc_align(lp, targets, il, tl))], args.warmup, args.runs)
    a, b = ctc.ctc_long_align(lp, targets, il, tl), ctc.ctc_align(lp, targets, il, tl)
    print("\n3. (T,B,U,C) = (%d,1,%d,%d), alternating in one loop" % (T, U, C))
    for name in ("ctc_long_align", "ctc_align"):
        print("   %-16s %s" % (name, stats(times[name])))
    print("   ratio long / plane %.2fx; scores %.6f and %.6f" % (
        statistics.median(times["ctc_long_align"]) / statistics.median(times["ctc_align"]), float(a[0][0]), float(b[0][0])))


if __name__ == "__main__":
    main()
