"""HIP-event times of the CTC search with an LM and a hotword graph beside it, next to the search with the LM alone.

    python tools/ctc_bias_time.py [--runs 30] [--warmup 5] [--parent-lib PATH] > profiles/ctc_bias_time.txt

Shapes: (T,B,C) = (240,32,5000) and (1000,32,5000), beam 16, candidates 32.  The LM is the seeded bigram LM of
tools/ctc_timing.py (about 110 000 arcs); the hotword list holds 100 seeded phrases of 2-6 tokens, boost 1.5.  Timed
alone through the C ABI on the output of the row pass (buffers allocated once): the one-FST search, the two-FST search,
and the two-FST stream in chunks of 8 frames (row pass of each chunk included: a stream cannot have it done ahead).
`--parent-lib` names a libpika_amd.so built from the parent commit: its one-FST search then runs in the same loop, on
the same buffers, so that "nothing changed for one FST" is a measurement of one session on one device.  The variants
are warmed up and alternate inside one loop so that drift hits them alike; each call is bracketed by two events on the
current stream; median, minimum and maximum are printed.  The one-FST and two-FST results are compared before anything
is timed: with bias_weight 0 they must be bit-equal.  Nothing here is asserted anywhere else.  Needs a GPU.
"""
import argparse
import statistics
import sys

import numpy as np
import torch

from ctc_timing import bigram_lm, fst_args as fst, load_parent, measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc


def hotword_list(C, blank, n, seed):
    rng = np.random.RandomState(seed)
    classes = [c for c in range(C) if c != blank]
    out = []
    while len(out) < n:
        ph = tuple(int(v) for v in rng.choice(classes, size=int(rng.randint(2, 7))))
        if all(ph[:len(q)] != q and q[:len(ph)] != ph for q in out):
            out.append(ph)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_bias_time.py: no HIP device")
    if args.runs < 20:
        sys.exit("ctc_bias_time.py: at least 20 runs")
    dev = torch.device("cuda")
    lib = _lib.lib()
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    beam, C, K = 16, 5000, 32
    lm = ctc.CtcNgramLm(*bigram_lm(C, 0, 20, 11), device=dev)
    hot = ctc.CtcHotwords(hotword_list(C, 0, 100, 13), C, boost=1.5, device=dev)
    print("LM: %d states, %d arcs; hotwords: 100 phrases of 2-6 tokens, %d states, %d arcs" % (
        lm.num_states, lm.num_arcs, hot.num_states, hot.num_arcs))
    for T, B in ((240, 32), (1000, 32)):
        g = torch.Generator().manual_seed(T)
        lp = torch.log_softmax(torch.randn(T, B, C, generator=g).to(dev), -1)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        blank_lp = torch.empty((T, B), device=dev)
        top_val = torch.empty((T, B, K), device=dev)
        top_idx = torch.empty((T, B, K), dtype=torch.int32, device=dev)

        def stream():
            return torch.cuda.current_stream().cuda_stream
        _lib.check(lib.pika_ctc_decode_rows(lp.data_ptr(), lp.stride(0), lp.stride(1), il.data_ptr(), B, T, C, 0, K, 0,
                                            blank_lp.data_ptr(), top_val.data_ptr(), top_idx.data_ptr(), None, stream()),
                   "pika_ctc_decode_rows")
        outs = [(torch.empty((B, 1, T), dtype=torch.int32, device=dev), torch.empty((B, 1), dtype=torch.int32, device=dev),
                 torch.empty((B, 1), device=dev), torch.empty((B, 1), device=dev)) for _ in range(2)]
        scratch = torch.empty(lib.pika_ctc_lm2_scratch_bytes(B, T, beam, K), dtype=torch.uint8, device=dev)
        head = (lp.data_ptr(), lp.stride(0), lp.stride(1), None, blank_lp.data_ptr(), top_val.data_ptr(),
                top_idx.data_ptr(), il.data_ptr(), B, T, C, 0, beam, 1)

        def one(which, o=0):
            def run():
                _lib.check(which.pika_ctc_lm_beam_search(*(head + fst(lm) + (K, 0.5, 0.0, 1) + tuple(
                    v.data_ptr() for v in outs[o]) + (scratch.data_ptr(), stream()))), "pika_ctc_lm_beam_search")
            return run

        def two(bias_weight, o=1):
            def run():
                _lib.check(lib.pika_ctc_lm2_beam_search(*(head + fst(lm) + fst(hot) + (K, 0.5, bias_weight, 0.0, 1) + tuple(
                    v.data_ptr() for v in outs[o]) + (scratch.data_ptr(), stream()))), "pika_ctc_lm2_beam_search")
            return run
        chunked = ctc.CtcBeamStream(B, T, beam=beam, lm=ctc.CtcBiasedLm(lm, hot, 1.0), lm_weight=0.5, candidates=K,
                                    device=dev)

        def streamed():
            chunked.reset()
            for s in range(0, T, 8):
                chunked.advance(lp[s:s + 8])
        # results must not change: the two-FST kernel with weight 0 gives the one-FST kernel's bits; so does the parent
        one(lib)()
        two(0.0)()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(*outs))
        print("\nT = %d, B = %d, C = %d, beam = %d, candidates = %d" % (T, B, C, beam, K))
        print("  two-FST search with bias_weight 0 == one-FST search, bit for bit: %s" % same)
        if parent is not None:
            one(parent, 1)()
            torch.cuda.synchronize()
            print("  one-FST search of the parent's library == this tree's, bit for bit: %s" % all(
                torch.equal(a, b) for a, b in zip(*outs)))
        two(1.0)()
        torch.cuda.synchronize()
        moved = int((outs[0][0] != outs[1][0]).any(-1).any(-1).sum())
        print("  with bias_weight 1 the best hypothesis of %d of %d utterances differs from the LM-only one" % (moved, B))
        variants = [("one-FST search (LM)", one(lib)), ("two-FST search (LM + hotwords)", two(1.0))]
        if parent is not None:
            variants.append(("one-FST search, parent's library", one(parent)))
        variants.append(("two-FST stream, chunks of 8 (rows + advance)", streamed))
        times = measure(variants, args.warmup, args.runs)
        med = {name: statistics.median(times[name]) for name, _ in variants}
        for name, _ in variants:
            t = times[name]
            print("  %-46s %8.3f [%8.3f, %8.3f]   %6.2f us per frame" % (name, med[name], min(t), max(t),
                                                                         1e3 * med[name] / T))
        print("  two-FST / one-FST (same run)                   %8.3f" % (
            med["two-FST search (LM + hotwords)"] / med["one-FST search (LM)"]))
        if parent is not None:
            print("  one-FST, this tree / parent (same run)         %8.3f" % (
                med["one-FST search (LM)"] / med["one-FST search, parent's library"]))


if __name__ == "__main__":
    main()
