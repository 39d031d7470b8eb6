"""What the pruned (banded) RNN-T loss costs next to the full one.

The benchmark's lattice (B = 32, T = 1000, U = 50, V = 5000; inputs seed 1234, full length).  The band (S = 5) comes from
the package's own chain: the two planes of the full tensor -> `rnnt_loss_from_planes(return_occupancy=True)` ->
`rnnt_prune_ranges`; the pruned logits are the full tensor's rows of every frame's band.  Timed by HIP events on the
launch stream, forward plus backward through autograd, `--runs` runs each, alternating in one loop, medians reported:

  full      rnnt_loss_from_logits         on (B, T, U+1, V)
  pruned    rnnt_loss_pruned_from_logits  on (B, T, S, V)
  planes    rnnt_loss_from_planes         forward + backward on the two (B, T, U+1) planes
  search    rnnt_prune_ranges             alone
  writer    the backward of rnnt_loss_pruned (log-probs): row metadata + the flat dense-gradient writer over B*T*S*V*4
            bytes, with the bytes per second it reaches

    python tools/rnnt_pruned_time.py [--runs 10] [--warmup 2] [--out profiles/rnnt_pruned_time.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--labels", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--band", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_pruned_time.txt"))
    args = ap.parse_args()
    import pika_amd  # noqa: F401
    from bench import make_inputs
    from pika_amd.rnnt import (rnnt_loss_from_logits, rnnt_loss_from_planes, rnnt_loss_pruned,
                               rnnt_loss_pruned_from_logits, rnnt_prune_ranges)
    dev = torch.device("cuda:0")
    B, T, U, V, S = args.batch, args.frames, args.labels, args.vocab, args.band
    full, labels, tl, ul = make_inputs(B, T, U, V, dev, 1234)
    tl, ul = tl.int(), ul.int()
    blank_lp = full[..., 0].contiguous()
    label_lp = torch.gather(full[:, :, :U], 3, labels.long()[:, None, :, None].expand(B, T, U, 1))[..., 0]
    label_lp = torch.cat([label_lp, label_lp.new_full((B, T, 1), -1.0e30)], 2).contiguous()
    _, ob, ol = rnnt_loss_from_planes(blank_lp, label_lp, tl, ul, return_occupancy=True)
    ranges = rnnt_prune_ranges(ob, ol, tl, ul, S)
    idx = (ranges.long()[:, :, None] + torch.arange(S, device=dev)).clamp_max(U)
    band = torch.gather(full, 2, idx[..., None].expand(B, T, S, V)).contiguous()
    r = ranges.cpu().numpy()
    d = np.diff(r, axis=1)
    valid = bool((r[:, 0] == 0).all() and (r[:, -1] == max(0, U + 1 - S)).all() and (d >= 0).all() and (d <= S - 1).all())

    def fwd_bwd(fn, x, *rest):
        x.requires_grad_(True)

        def run():
            fn(x, *rest).sum().backward()
            x.grad = None
        return run

    pb, pl = blank_lp.clone().requires_grad_(True), label_lp.clone().requires_grad_(True)

    def planes():
        rnnt_loss_from_planes(pb, pl, tl, ul).sum().backward()
        pb.grad = pl.grad = None

    xw = band.clone().requires_grad_(True)
    state = {}

    def writer_fwd():
        state["c"] = rnnt_loss_pruned(xw, labels, ranges, tl, ul).sum()

    def writer_bwd():
        state.pop("c").backward()
        xw.grad = None

    legs = [("full", fwd_bwd(rnnt_loss_from_logits, full, labels, tl, ul), None),
            ("pruned", fwd_bwd(rnnt_loss_pruned_from_logits, band, labels, ranges, tl, ul), None),
            ("planes", planes, None),
            ("search", lambda: rnnt_prune_ranges(ob, ol, tl, ul, S), None),
            ("writer", writer_bwd, writer_fwd)]
    times = {name: [] for name, _, _ in legs}
    for i in range(args.warmup + args.runs):
        for name, fn, before in legs:
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    with torch.no_grad():
        c_full = rnnt_loss_from_logits(full, labels, tl, ul)
        c_pruned = rnnt_loss_pruned_from_logits(band, labels, ranges, tl, ul)
    wbytes = B * T * S * V * 4
    lines = [
        "tools/rnnt_pruned_time.py: B=%d T=%d U=%d V=%d S=%d, medians of %d alternating runs (ms)" % (B, T, U, V, S, args.runs),
        "full    rnnt_loss_from_logits        fwd+bwd %8.3f" % med["full"],
        "pruned  rnnt_loss_pruned_from_logits fwd+bwd %8.3f   ratio pruned/full %.3f" % (med["pruned"], med["pruned"] / med["full"]),
        "planes  rnnt_loss_from_planes        fwd+bwd %8.3f" % med["planes"],
        "search  rnnt_prune_ranges                    %8.3f" % med["search"],
        "writer  rnnt_loss_pruned backward (row metadata + dense writer, %.3f GB) %8.3f   %.2f TB/s" % (
            wbytes / 1e9, med["writer"], wbytes / med["writer"] / 1e9),
        "ranges valid: %s; mean cost full %.3f, pruned %.3f (pruned >= full: %s)" % (
            valid, float(c_full.mean()), float(c_pruned.mean()), bool((c_pruned >= c_full - 1e-5 * c_full.abs()).all())),
        json.dumps({"tool": "rnnt_pruned_time", "B": B, "T": T, "U": U, "V": V, "S": S, "runs": args.runs,
                    "median_ms": {k: round(v, 4) for k, v in med.items()}, "ratio": round(med["pruned"] / med["full"], 4),
                    "writer_TBps": round(wbytes / med["writer"] / 1e9, 3), "ranges_valid": valid}),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
