"""HIP-event times of CTC-guided frame skipping (include/pika_frame_skip.h, pika_amd/frame_skip.py).

    python tools/frame_skip_time.py [--runs 10] [--warmup 3] [--out profiles/frame_skip_time.txt]

* plan + apply at (B, T, C, D) = (32, 240, 5000, 512) and at T = 1000, 20 calls per bracket: the kernels from logits and
  from log-probs next to the torch spelling of the same definition (log_softmax, mask, sorts, cumsum, gather: the
  package's own plain path run on the device); the from-logits row pass alone, with its share of the HBM peak
  (B T C 4 bytes read once over 8.0 TB/s, the specification's figure; 6.29 TB/s is what a float4 copy reaches);
* `modified_beam_search_skip` next to `modified_beam_search` at (B, beam, V) = (64, 4, 5000), H = 512, 60 frames, with
  the stateless network: keep ratios 1.0, 0.5 and 0.3 forced through a synthetic head (a module that returns fixed logits
  which put the blank posterior of every frame at 1/V or at almost 1).  The figure that matters is the cost at 1.0: the overhead when nothing can be skipped.
The variants alternate inside one loop, every one is warmed up, medians of `runs` with minimum and maximum.  Reported,
not gated: nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import _lib, ctc_skip_plan, frame_skip_apply, modified_beam_search, modified_beam_search_skip
from pika_amd.frame_skip import _torch_plan
from stateless_time import search_model

CALLS, V, HBM_PEAK = 20, 5000, 8.0e12


class FixedHead(torch.nn.Module):
    """A 'CTC head' that returns fixed logits: the keep ratio of the search is then what the logits were made for."""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, enc):
        return self.logits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "frame_skip_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_skip_time.py: no HIP device")
    dev = torch.device("cuda")
    lines = ["device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup)]
    variants, per, rows_of = [], {}, {}
    thr, blank = 0.95, 0

    # ---- plan + apply
    def add_shape(B, T, C, D):
        g = torch.Generator().manual_seed(T)
        logits = torch.randn(B, T, C, generator=g)
        logits[:, :, blank] += 9.0 + 3.0 * torch.randn(B, T, generator=g)      # blank posteriors on both sides of 0.95
        logits = logits.to(dev)
        log_probs = torch.log_softmax(logits, dim=2)
        feats = torch.randn(B, T, D, generator=g).to(dev)
        lengths = torch.randint(T // 2, T + 1, (B,), generator=g).to(dev, torch.int32)
        kept = ctc_skip_plan(logits, lengths, blank, thr, from_logits=True).kept_lengths
        shape = "(B,T,C,D) = (%d,%d,%d,%d), kept %.2f" % (B, T, C, D, float(kept.sum()) / float(lengths.sum()))

        def kernels(scores, from_logits):
            for _ in range(CALLS):
                frame_skip_apply(feats, ctc_skip_plan(scores, lengths, blank, thr, from_logits=from_logits))

        def spelled():
            log_thr = float(torch.tensor(thr).log())
            for _ in range(CALLS):
                plan = _torch_plan(torch.log_softmax(logits, dim=2)[:, :, blank], lengths, None, log_thr)
                index = plan.frame_index    # (the plain path of frame_skip_apply, spelled out for float32)
                got = feats.gather(1, index.clamp(min=0).long().unsqueeze(2).expand(B, T, D))
                torch.where((index >= 0).unsqueeze(2), got, torch.zeros_like(got))

        def rows():
            out = torch.empty((B, T), dtype=torch.float32, device=dev)
            for _ in range(CALLS):
                _lib.check(_lib.lib().pika_fskip_rows(logits.data_ptr(), logits.stride(0), logits.stride(1),
                                                      lengths.data_ptr(), B, T, C, blank, 1, out.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "pika_fskip_rows")
        for name, fn in (("plan + apply, kernels, from logits", lambda: kernels(logits, True)),
                         ("plan + apply, kernels, from log-probs", lambda: kernels(log_probs, False)),
                         ("plan + apply, torch spelling, from logits", spelled),
                         ("row pass alone, from logits", rows)):
            name = "%s, %d calls, %s" % (name, CALLS, shape)
            variants.append((name, fn))
            per[name] = CALLS
            if fn is rows:
                rows_of[name] = 4.0 * C * float(lengths.sum())        # bytes of the rows t < L
    for shape in ((32, 240, 5000, 512), (32, 1000, 5000, 512)):
        add_shape(*shape)

    # ---- the search
    B, T, K = 64, 60, 4
    model = search_model("stateless", dev)
    x = torch.randn(B, T, 40, device=dev)
    x_len = torch.full((B,), T, dtype=torch.int64)
    search = {}
    name = "modified_beam_search, stateless, graph, %d frames, (B,beam,V) = (%d,%d,%d)" % (T, B, K, V)
    variants.append((name, lambda: modified_beam_search(model, x, x_len, beam=K)))
    per[name], search["plain"] = 1, name
    for ratio in (1.0, 0.5, 0.3):
        g = torch.Generator().manual_seed(int(10 * ratio))
        keep = torch.rand(B, T, generator=g) < ratio if ratio < 1.0 else torch.ones(B, T, dtype=torch.bool)
        fixed = torch.zeros(B, T, V)
        fixed[:, :, blank] = torch.where(keep, torch.tensor(0.0), torch.tensor(30.0))      # posterior 1/V or ~1
        head = FixedHead(fixed.to(dev))
        name = "modified_beam_search_skip, keep %.1f (%.2f kept), same shape" % (ratio, float(keep.float().mean()))
        variants.append((name, lambda head=head: modified_beam_search_skip(model, x, x_len, head, threshold=thr, beam=K)))
        per[name], search[ratio] = 1, name

    times = measure(variants, args.warmup, args.runs)
    for name, _ in variants:
        t = times[name]
        med = statistics.median(t)
        tail = ""
        if name in rows_of:
            tail = "   %.2f TB/s, %.0f%% of the 8.0 TB/s HBM peak" % (
                rows_of[name] * per[name] / (med * 1e-3) / 1e12, 100.0 * rows_of[name] * per[name] / (med * 1e-3) / HBM_PEAK)
        lines.append("  %-100s %8.3f [%8.3f, %8.3f]   %7.1f us per call%s" % (name, med, min(t), max(t),
                                                                                1e3 * med / per[name], tail))
    plain = statistics.median(times[search["plain"]])
    lines.append("the search with skipping over the plain search (medians; above 1: slower):")
    for ratio in (1.0, 0.5, 0.3):
        lines.append("  keep %.1f   %.3f" % (ratio, statistics.median(times[search[ratio]]) / plain))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
