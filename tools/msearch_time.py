"""HIP-event times of the frame step of the one-symbol-per-frame beam search (include/pika_msearch.h).

    python tools/msearch_time.py [--runs 10] [--warmup 3] > profiles/msearch_time.txt

`ModifiedBeamState.advance` alone at (B, K, V) = (64, 4, 5000) and (64, 16, 5000): 50 frame steps back to back on random
float32 logits (the reset happens before the timed bracket), whole Python calls, eager and as one captured graph of the
50 launches; the time per step, the bytes of logits a step reads (B K V 4, once from memory; the second pass over the
rows comes from the cache) and that traffic as a share of the HBM peak (8.0 TB/s spec).  The variants alternate inside
one loop, every one is warmed up, medians of `runs` with minimum and maximum.  Nothing here is asserted anywhere.
Needs a GPU.

Not measured by this tool: `pika_beam_advance_logits` on the same rows, and the whole `modified_beam_search` next to
`TransducerDecoder`'s stepwise path at the decode benchmark's model width.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import ModifiedBeamState

STEPS = 50
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("msearch_time.py: no HIP device")
    dev = torch.device("cuda")
    print("device: %s   runs %d, warm-up %d; %d frame steps per bracket; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup, STEPS))
    variants, shapes = [], {}
    for B, K, V in ((64, 4, 5000), (64, 16, 5000)):
        g = torch.Generator().manual_seed(K)
        logits = (3.0 * torch.randn(B * K, V, generator=g)).to(dev)
        nf = torch.full((B,), STEPS, dtype=torch.int64, device=dev)
        state = ModifiedBeamState(B, STEPS, K, 0, dev)

        def eager(state=state, logits=logits, nf=nf):
            for _ in range(STEPS):
                state.advance(logits, nf)
        eager()
        torch.cuda.synchronize()
        state.reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eager()
        for kind, fn in (("eager", eager), ("one graph", graph.replay)):
            name = "advance (B,K,V) = (%d,%d,%d), %s" % (B, K, V, kind)
            variants.append((name, (state.reset, fn)))
            shapes[name] = 4.0 * B * K * V
    times = measure(variants, args.warmup, args.runs)
    for name, _ in variants:
        t = times[name]
        per_step = statistics.median(t) / STEPS * 1e-3
        print("  %-46s %8.3f [%8.3f, %8.3f]   %6.1f us per step, %.2f MB of logits per step = %4.1f %% of the HBM peak"
              % (name, statistics.median(t), min(t), max(t), 1e6 * per_step, shapes[name] / 1e6,
                 100.0 * shapes[name] / per_step / HBM_PEAK))


if __name__ == "__main__":
    main()
