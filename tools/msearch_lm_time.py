"""HIP-event times of the fused frame step of the one-symbol-per-frame beam search (include/pika_msearch_lm.h) next to
the plain one (include/pika_msearch.h).

    python tools/msearch_lm_time.py [--runs 10] [--warmup 3] > profiles/msearch_lm_time.txt

`ModifiedBeamState.advance` and `ModifiedLmBeamState.advance` at (B, K, V) = (64, 4, 5000) and (64, 16, 5000): 50 frame
steps back to back on the same random float32 logits as ONE captured graph of the 50 launches (the reset happens before
the timed bracket), so what is compared is the kernels and not the Python around them.  The fused step runs with
C = K and C = 2 K, with one automaton (the seeded bigram LM of tools/ctc_timing.py, about 110 000 arcs, lm_weight 0.5)
and with two (that LM and the 100 seeded phrases of tools/ctc_bias_time.py, boost 1.5).  All variants alternate inside
one loop, every one is warmed up, medians of `runs` with minimum and maximum; the plain step's time of the same loop is
what the fused ones are set against.  Nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import bigram_lm, measure  # (first: it puts the repository on sys.path)
from ctc_bias_time import hotword_list
from pika_amd import ModifiedBeamState, ModifiedLmBeamState, ctc

STEPS = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("msearch_lm_time.py: no HIP device")
    dev = torch.device("cuda")
    print("device: %s   runs %d, warm-up %d; %d frame steps per bracket, one graph; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup, STEPS))
    V = 5000
    lm = ctc.CtcNgramLm(*bigram_lm(V, 0, 20, 11), device=dev)
    hot = ctc.CtcHotwords(hotword_list(V, 0, 100, 13), V, boost=1.5, device=dev)
    pair = ctc.CtcBiasedLm(lm, hot, 1.0)
    print("LM: %d states, %d arcs; hotwords: 100 phrases of 2-6 tokens, %d states, %d arcs" % (
        lm.num_states, lm.num_arcs, hot.num_states, hot.num_arcs))
    variants, keep = [], []
    for B, K in ((64, 4), (64, 16)):
        g = torch.Generator().manual_seed(K)
        logits = (3.0 * torch.randn(B * K, V, generator=g)).to(dev)
        nf = torch.full((B,), STEPS, dtype=torch.int64, device=dev)
        states = [("plain", ModifiedBeamState(B, STEPS, K, 0, dev))]
        for C in (K, 2 * K):
            states.append(("fused C=%d, 1 FST" % C, ModifiedLmBeamState(B, STEPS, lm, K, 0, 0.5, 0.0, C, dev)))
            states.append(("fused C=%d, 2 FSTs" % C, ModifiedLmBeamState(B, STEPS, pair, K, 0, 0.5, 0.0, C, dev)))
        for kind, state in states:
            def run(state=state, logits=logits, nf=nf):
                for _ in range(STEPS):
                    state.advance(logits, nf)
            run()
            torch.cuda.synchronize()
            state.reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run()
            keep.append((state, graph, logits, nf))
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
