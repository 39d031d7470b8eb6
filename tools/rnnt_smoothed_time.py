"""What the smoothed simple planes cost next to the torch spelling they replace, alone and inside the pruned chain.

The benchmark's lattice (B = 32, T = 1000, U = 50, V = 5000, full length), random inputs, freshly initialised layers of
width `--width` (bench.py's config 2), band S = 5, in the arithmetic mode of the session.  Timed by HIP events on the
launch stream, forward plus backward, `--runs` runs each, alternating in one loop, medians reported:

  (a) planes   rnnt_simple_planes (plain torch, unchanged) against rnnt_smoothed_planes at scales (0, 0) and (0.25, 0) on
               the same am / lm, gradients of a fixed linear functional of the planes taken to both
  (b) chain    rnnt_pruned_joint_loss against rnnt_pruned_joint_loss_smoothed at (0, 0) and (0.25, 0), backward of
               0.5 simple + pruned down to enc, pred and every parameter
  (c) kernels  pika_prnnt_smoothed_fwd and pika_prnnt_smoothed_bwd alone (the three forward launches; the one backward
               launch), with the bytes of am and d_am they move and the rate, next to the floor of one forward read, one
               backward read and one write of d_am

    python tools/rnnt_smoothed_time.py [--runs 10] [--warmup 2] [--out profiles/rnnt_smoothed_time.txt]
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
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--band", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_smoothed_time.txt"))
    args = ap.parse_args()
    import pika_amd  # noqa: F401
    from pika_amd import gemm as G
    from pika_amd import rnnt
    dev = torch.device("cuda:0")
    B, T, U, V, H, S = args.batch, args.frames, args.labels, args.vocab, args.width, args.band
    torch.manual_seed(1234)
    fc1, fcg, fc2 = torch.nn.Linear(2 * H, H).to(dev), torch.nn.Linear(2 * H, H).to(dev), torch.nn.Linear(H, V).to(dev)
    sam, slm = torch.nn.Linear(H, V).to(dev), torch.nn.Linear(H, V).to(dev)
    layers = (fc1, fcg, fc2, sam, slm)
    params = [p for m in layers for p in m.parameters()]
    enc = torch.randn(B, T, H, device=dev, requires_grad=True)
    pred = torch.randn(B, U + 1, H, device=dev, requires_grad=True)
    labels = torch.randint(1, V, (B, U), device=dev, dtype=torch.int32)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul = torch.full((B,), U, dtype=torch.int32, device=dev)
    am = torch.randn(B, T, V, device=dev, requires_grad=True)
    lm = torch.randn(B, U + 1, V, device=dev, requires_grad=True)
    wb, wl = torch.randn(B, T, U + 1, device=dev), torch.randn(B, T, U + 1, device=dev)
    wl[:, :, U] = 0.0

    def planes(fn, **kw):
        def leg():
            bl, lb = fn(am, lm, labels, **kw)
            ((wb * bl).sum() + (wl * lb).sum()).backward()
            am.grad = lm.grad = None
        return leg

    def chain(fn, **kw):
        def leg():
            simple, loss, _ = fn(enc, pred, labels, tl, ul, *layers, s_range=S, **kw)
            (0.5 * simple + loss).backward()
            for p in params + [enc, pred]:
                p.grad = None
        return leg

    kernel_ms = {"fwd": [], "bwd": []}

    def kernels():                         # the C-ABI calls alone, bracketed by events inside pika_amd.rnnt
        rnnt.KERNEL_EVENTS = ev = {"fwd": [], "bwd": []}
        planes(rnnt.rnnt_smoothed_planes, lm_only_scale=0.25)()
        rnnt.KERNEL_EVENTS = None
        torch.cuda.synchronize()
        for k in ev:
            kernel_ms[k].append(sum(a.elapsed_time(b) for a, b in ev[k]))

    legs = [("planes_torch", planes(rnnt.rnnt_simple_planes)),
            ("planes_00", planes(rnnt.rnnt_smoothed_planes)),
            ("planes_25", planes(rnnt.rnnt_smoothed_planes, lm_only_scale=0.25)),
            ("chain_torch", chain(rnnt.rnnt_pruned_joint_loss)),
            ("chain_00", chain(rnnt.rnnt_pruned_joint_loss_smoothed)),
            ("chain_25", chain(rnnt.rnnt_pruned_joint_loss_smoothed, lm_only_scale=0.25)),
            ("kernels", kernels)]
    times = {name: [] for name, _ in legs}
    for i in range(args.warmup + args.runs):
        if i == args.warmup:
            kernel_ms = {"fwd": [], "bwd": []}
        for name, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    kf, kb = float(np.median(kernel_ms["fwd"])), float(np.median(kernel_ms["bwd"]))
    a_bytes = B * T * V * 4
    tiles = (U + 1 + 63) // 64             # the forward contraction and the backward read am once per 64 lattice columns
    fwd_bytes, bwd_bytes = (1 + tiles) * a_bytes, (1 + tiles) * a_bytes
    floor = 3 * a_bytes
    lines = [
        "tools/rnnt_smoothed_time.py: B=%d T=%d U=%d V=%d H=%d S=%d, mode %s, medians of %d alternating runs (ms)" % (
            B, T, U, V, H, S, G.PRECISION, args.runs),
        "(a) rnnt_simple_planes, plain torch                          fwd+bwd %9.3f" % med["planes_torch"],
        "    rnnt_smoothed_planes (0, 0)                              fwd+bwd %9.3f   ratio kernels/torch %.4f" % (
            med["planes_00"], med["planes_00"] / med["planes_torch"]),
        "    rnnt_smoothed_planes (0.25, 0)                           fwd+bwd %9.3f   ratio kernels/torch %.4f" % (
            med["planes_25"], med["planes_25"] / med["planes_torch"]),
        "(b) rnnt_pruned_joint_loss                                   fwd+bwd %9.3f" % med["chain_torch"],
        "    rnnt_pruned_joint_loss_smoothed (0, 0)                   fwd+bwd %9.3f   ratio %.4f" % (
            med["chain_00"], med["chain_00"] / med["chain_torch"]),
        "    rnnt_pruned_joint_loss_smoothed (0.25, 0)                fwd+bwd %9.3f   ratio %.4f" % (
            med["chain_25"], med["chain_25"] / med["chain_torch"]),
        "(c) pika_prnnt_smoothed_fwd: row max + gathers, contraction, planes  %9.3f   %.3f GB of am, %.2f TB/s" % (
            kf, fwd_bytes / 1e9, fwd_bytes / kf / 1e9),
        "    pika_prnnt_smoothed_bwd: am read, d_am written                   %9.3f   %.3f GB, %.2f TB/s" % (
            kb, bwd_bytes / 1e9, bwd_bytes / kb / 1e9),
        "    floor: one read of am forward, one backward, one write of d_am: %.3f GB; moved %.3f GB in %.3f ms" % (
            floor / 1e9, (fwd_bytes + bwd_bytes) / 1e9, kf + kb),
        json.dumps({"tool": "rnnt_smoothed_time", "B": B, "T": T, "U": U, "V": V, "H": H, "S": S, "mode": G.PRECISION,
                    "runs": args.runs, "median_ms": {k: round(v, 4) for k, v in med.items() if k != "kernels"},
                    "kernel_fwd_ms": round(kf, 4), "kernel_bwd_ms": round(kb, 4),
                    "kernel_fwd_TBps": round(fwd_bytes / kf / 1e9, 3), "kernel_bwd_TBps": round(bwd_bytes / kb / 1e9, 3),
                    "floor_GB": round(floor / 1e9, 3)}),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
