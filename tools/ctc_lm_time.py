"""HIP-event times of the CTC search with n-gram LM fusion next to the plain search on the same input.

    python tools/ctc_lm_time.py [--runs 30] [--warmup 5] > profiles/ctc_lm_time.txt

Shapes: (T,B,C) = (240,32,5000) and (1000,32,5000), beam 16, candidates 32.  The LM is generated from a seed: a unigram
state with an arc for every non-blank class, one bigram state per class with 20 arcs and a back-off arc (about 10^5
bigram arcs), costs in [0.3, 5].  Both searches are timed alone through the C ABI on the output of their row pass
(buffers allocated once), and as whole Python calls; the yardstick is the plain `ctc_beam_search`.

What bounds the fused search is read from ablations by input, not from counters: `candidates` 32 -> 8 -> 1 cuts the
n * candidates FST lookups per frame to almost none while the `beam` selection rounds, the slot work and the barriers of
a frame stay; a one-state LM (every class an arc of the start state, no back-off) halves the bisections of a lookup that
misses its bigram state.  Every variant is warmed up, the variants alternate inside one loop so that drift hits them
alike, each call is bracketed by two events on the current stream, and median, minimum and maximum are printed.
Nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import bigram_lm, fst_args, measure, unigram_lm  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_lm_time.py: no HIP device")
    if args.runs < 20:
        sys.exit("ctc_lm_time.py: at least 20 runs")
    dev = torch.device("cuda")
    lib = _lib.lib()
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    beam, C = 16, 5000
    fst, backoff_id = bigram_lm(C, 0, 20, 11)
    lm2 = ctc.CtcNgramLm(fst, backoff_id, device=dev)
    lm1 = ctc.CtcNgramLm(*unigram_lm(C, 0, 12), device=dev)
    print("LM: %d states, %d arcs (%d of them bigram arcs); one-state LM: %d arcs" % (
        lm2.num_states, lm2.num_arcs, lm2.num_arcs - (C - 1) - (lm2.num_states - 1), lm1.num_arcs))
    for T, B in ((240, 32), (1000, 32)):
        g = torch.Generator().manual_seed(T)
        lp = torch.log_softmax(torch.randn(T, B, C, generator=g).to(dev), -1)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        blank_lp = torch.empty((T, B), device=dev)
        rows = {}
        for K in (32, 8, 1):
            rows[K] = (torch.empty((T, B, K), device=dev), torch.empty((T, B, K), dtype=torch.int32, device=dev))
            _lib.check(lib.pika_ctc_decode_rows(lp.data_ptr(), lp.stride(0), lp.stride(1), il.data_ptr(), B, T, C, 0, K,
                                                0, blank_lp.data_ptr(), rows[K][0].data_ptr(), rows[K][1].data_ptr(),
                                                None, torch.cuda.current_stream().cuda_stream), "pika_ctc_decode_rows")
        tokens = torch.empty((B, 1, T), dtype=torch.int32, device=dev)
        lengths = torch.empty((B, 1), dtype=torch.int32, device=dev)
        scores = torch.empty((B, 1), device=dev)
        am = torch.empty((B, 1), device=dev)
        scratch = torch.empty(lib.pika_ctc_beam_scratch_bytes(B, T, beam), dtype=torch.uint8, device=dev)
        assert lib.pika_ctc_lm_scratch_bytes(B, T, beam, 32) == scratch.numel()

        def stream():
            return torch.cuda.current_stream().cuda_stream

        def plain():
            _lib.check(lib.pika_ctc_beam_search(lp.data_ptr(), lp.stride(0), lp.stride(1), None, blank_lp.data_ptr(),
                                                rows[32][0].data_ptr(), rows[32][1].data_ptr(), il.data_ptr(), B, T, C,
                                                0, beam, 1, tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(),
                                                scratch.data_ptr(), stream()), "pika_ctc_beam_search")

        def fused(lm, K):
            def run():
                _lib.check(lib.pika_ctc_lm_beam_search(
                    lp.data_ptr(), lp.stride(0), lp.stride(1), None, blank_lp.data_ptr(), rows[K][0].data_ptr(),
                    rows[K][1].data_ptr(), il.data_ptr(), B, T, C, 0, beam, 1, *fst_args(lm), K, 0.5, 0.0, 1,
                    tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), am.data_ptr(), scratch.data_ptr(),
                    stream()), "pika_ctc_lm_beam_search")
            return run

        variants = [("plain search, beam 16 (K = 32)", plain),
                    ("fused search, bigram LM, candidates 32", fused(lm2, 32)),
                    ("fused search, bigram LM, candidates 8", fused(lm2, 8)),
                    ("fused search, bigram LM, candidates 1", fused(lm2, 1)),
                    ("fused search, one-state LM, candidates 32", fused(lm1, 32)),
                    ("ctc_beam_search (whole call)", lambda: ctc.ctc_beam_search(lp, il, beam=beam)),
                    ("ctc_beam_search_lm (whole call)", lambda: ctc.ctc_beam_search_lm(lp, il, lm2, beam=beam,
                                                                                      candidates=32))]
        times = measure(variants, args.warmup, args.runs)
        print("\nT = %d, B = %d, C = %d, beam = %d" % (T, B, C, beam))
        med = {name: statistics.median(times[name]) for name, _ in variants}
        for name, _ in variants:
            t = times[name]
            line = "  %-44s %8.3f [%8.3f, %8.3f]" % (name, med[name], min(t), max(t))
            if "search, " in name:
                line += "   %6.2f us per frame" % (1e3 * med[name] / T)
            print(line)
        print("  fused / plain (search alone)                 %8.2f" % (
            med["fused search, bigram LM, candidates 32"] / med["plain search, beam 16 (K = 32)"]))
        print("  fused / plain (whole call)                   %8.2f" % (
            med["ctc_beam_search_lm (whole call)"] / med["ctc_beam_search (whole call)"]))


if __name__ == "__main__":
    main()
