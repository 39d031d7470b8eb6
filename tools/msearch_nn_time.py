"""HIP-event times of the frame step of the one-symbol-per-frame beam search with a neural LM's rows fused in
(include/pika_msearch_nn.h) next to the plain step (include/pika_msearch.h) and the n-gram fused one
(include/pika_msearch_lm.h).

    python tools/msearch_nn_time.py [--runs 10] [--warmup 3] > profiles/msearch_nn_time.txt

As tools/msearch_lm_time.py: (B, K, V = V_lm) = (64, 4, 5000) and (64, 16, 5000), 50 frame steps back to back on the same
random float32 logits (and LM logits) as ONE captured graph of the 50 launches, the reset before the timed bracket, so
what is compared is the kernels.  Per shape: the plain step; with C = K and C = 2 K the n-gram fused step (the seeded
bigram LM of tools/ctc_timing.py, lm_weight 0.5), the dense step alone and the dense step with that automaton.  All
variants alternate inside one loop, every one is warmed up, medians of `runs` with minimum and maximum.  Nothing here is
asserted anywhere.  Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import bigram_lm, measure  # (first: it puts the repository on sys.path)
from pika_amd import ModifiedBeamState, ModifiedLmBeamState, ModifiedNnLmBeamState, ctc

STEPS = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("msearch_nn_time.py: no HIP device")
    dev = torch.device("cuda")
    print("device: %s   runs %d, warm-up %d; %d frame steps per bracket, one graph; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup, STEPS))
    V = 5000
    lm = ctc.CtcNgramLm(*bigram_lm(V, 0, 20, 11), device=dev)
    print("LM: %d states, %d arcs; the dense rows: float32 (B K, %d), nn_weight 0.3" % (lm.num_states, lm.num_arcs, V))
    variants, keep = [], []
    for B, K in ((64, 4), (64, 16)):
        g = torch.Generator().manual_seed(K)
        logits = (3.0 * torch.randn(B * K, V, generator=g)).to(dev)
        rows = (3.0 * torch.randn(B * K, V, generator=g)).to(dev)
        nf = torch.full((B,), STEPS, dtype=torch.int64, device=dev)
        states = [("plain", ModifiedBeamState(B, STEPS, K, 0, dev), ())]
        for C in (K, 2 * K):
            states.append(("n-gram C=%d" % C, ModifiedLmBeamState(B, STEPS, lm, K, 0, 0.5, 0.0, C, dev), ()))
            states.append(("dense C=%d" % C, ModifiedNnLmBeamState(B, STEPS, K, 0, 0.3, 1.0, 0, None, 0.5, 0.0, C, dev),
                           (rows,)))
            states.append(("dense C=%d, 1 FST" % C, ModifiedNnLmBeamState(B, STEPS, K, 0, 0.3, 1.0, 0, lm, 0.5, 0.0, C,
                                                                          dev), (rows,)))
        for kind, state, extra in states:
            def run(state=state, logits=logits, nf=nf, extra=extra):
                for _ in range(STEPS):
                    state.advance(logits, *(extra + (nf,)))
            run()
            torch.cuda.synchronize()
            state.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run()
            keep.append((state, graph, logits, rows, nf))
            variants.append(("(B,K,V) = (%d,%d,%d) %s" % (B, K, V, kind), (state.reset, graph.replay)))
    times = measure(variants, args.warmup, args.runs)
    plain = None
    for name, _ in variants:
        t = times[name]
        per_step = 1e3 * statistics.median(t) / STEPS
        if name.endswith("plain"):
            plain = per_step
        print("  %-44s %8.3f [%8.3f, %8.3f]   %6.1f us per step, %5.2f x the plain step"
              % (name, statistics.median(t), min(t), max(t), per_step, per_step / plain))


if __name__ == "__main__":
    main()
