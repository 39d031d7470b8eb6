"""HIP-event times of the CTC decoders: the row pass (the one pass over the (T,B,C) input), the search, the greedy call.

    python tools/ctc_decode_time.py [--runs 30] [--warmup 5] > profiles/ctc_decode_time.txt

Shapes: (T,B,C) = (240,32,5000) and (1000,32,5000), beam 16.  The row pass is timed through the C ABI on buffers that
were allocated once (K = 1, K = 32, log-probs and logits form) and reported with its fraction of the 8 TB/s HBM peak,
bytes = 4 T B C; for comparison only, torch.topk(x, 32) + torch.logsumexp(x, -1) on the same tensor on the same
device, and the row pass on rows of equal values, where more candidates tie than its pool holds and it takes the
exact bisection route.  The search is timed alone on the row pass's output and reported in microseconds per frame.
Every variant is warmed up, the variants alternate inside one loop so that drift hits them alike, each call is bracketed by two events
on the current stream, and median, minimum and maximum are printed.  Nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc

HBM_PEAK = 8.0e12   # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_decode_time.py: no HIP device")
    if args.runs < 20:
        sys.exit("ctc_decode_time.py: at least 20 runs")
    dev = torch.device("cuda")
    lib = _lib.lib()
    print("device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup))
    beam = 16
    K = 2 * beam
    for T, B, C in ((240, 32, 5000), (1000, 32, 5000)):
        g = torch.Generator().manual_seed(T)
        logits = torch.randn(T, B, C, generator=g).to(dev)
        lp = torch.log_softmax(logits, -1)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        blank_lp = torch.empty((T, B), device=dev)
        lse = torch.empty((T, B), device=dev)
        top_val = torch.empty((T, B, K), device=dev)
        top_idx = torch.empty((T, B, K), dtype=torch.int32, device=dev)
        tokens = torch.empty((B, 1, T), dtype=torch.int32, device=dev)
        lengths = torch.empty((B, 1), dtype=torch.int32, device=dev)
        scores = torch.empty((B, 1), device=dev)
        scratch = torch.empty(lib.pika_ctc_beam_scratch_bytes(B, T, beam), dtype=torch.uint8, device=dev)

        def stream():
            return torch.cuda.current_stream().cuda_stream

        def rows(x, k, form):
            def run():
                _lib.check(lib.pika_ctc_decode_rows(x.data_ptr(), x.stride(0), x.stride(1), il.data_ptr(), B, T, C, 0, k,
                                                    form, blank_lp.data_ptr(), top_val.data_ptr(), top_idx.data_ptr(),
                                                    lse.data_ptr(), stream()), "pika_ctc_decode_rows")
            return run

        def search():
            _lib.check(lib.pika_ctc_beam_search(lp.data_ptr(), lp.stride(0), lp.stride(1), None, blank_lp.data_ptr(),
                                                top_val.data_ptr(), top_idx.data_ptr(), il.data_ptr(), B, T, C, 0, beam,
                                                1, tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(),
                                                scratch.data_ptr(), stream()), "pika_ctc_beam_search")

        def torch_rows():
            torch.topk(lp, K, dim=-1)
            torch.logsumexp(lp, -1)

        flat = torch.zeros_like(lp)     # every value ties: the row pass's exact selection, its slowest route
        row_variants = [("row pass K = 1, log-probs", rows(lp, 1, 0)), ("row pass K = 1, logits", rows(logits, 1, 1)),
                        ("row pass K = 32, logits", rows(logits, K, 1)), ("row pass K = 32, log-probs", rows(lp, K, 0)),
                        ("torch.topk(32) + torch.logsumexp", torch_rows)]
        # the search last in every round: it then reads the K = 32 log-prob rows left by the variant before it
        variants = row_variants[:3] + [("row pass K = 32, flat rows (exact route)", rows(flat, K, 0)),
                                       row_variants[4], row_variants[3], ("search, beam 16", search),
                                       ("ctc_greedy_decode (whole call)", lambda: ctc.ctc_greedy_decode(lp, il)),
                                       ("ctc_beam_search (whole call)", lambda: ctc.ctc_beam_search(lp, il, beam=beam))]
        times = measure(variants, args.warmup, args.runs)
        print("\nT = %d, B = %d, C = %d, beam = %d" % (T, B, C, beam))
        nbytes = 4.0 * T * B * C
        for name, _ in variants:
            t = times[name]
            med = statistics.median(t)
            line = "  %-42s %8.3f [%8.3f, %8.3f]" % (name, med, min(t), max(t))
            if name.startswith("row pass") or name.startswith("torch"):
                line += "   %5.1f%% of the HBM peak for 4TBC bytes" % (100.0 * nbytes / (med * 1e-3) / HBM_PEAK)
            if name.startswith("search"):
                line += "   %.2f us per frame" % (1e3 * med / T)
            print(line)


if __name__ == "__main__":
    main()
