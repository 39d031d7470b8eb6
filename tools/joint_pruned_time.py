"""What the joint network and the loss cost on the pruned (banded) lattice next to the full one.

The benchmark's lattice (B = 32, T = 1000, U = 50, V = 5000, full length) with the joint width of bench.py's config 2
(encoder / prediction / joint width 1024), band S = 5, random inputs and freshly initialised layers, in the arithmetic mode
of the session (PIKA_GEMM_PRECISION, default "mixed").  Timed by HIP events on the launch stream, forward plus backward
through autograd down to enc, pred and every parameter, `--runs` runs each, alternating in one loop, medians reported:

  full      ops.joint(log_softmax=False) + rnnt_loss_from_logits on the (B, T, U+1) lattice
  pruned    rnnt_pruned_joint_loss in full: both projections of the simple joiner, planes, simple loss, band search,
            joint_pruned on (B, T, S), pruned loss; backward of simple + pruned
  gate_fwd  pika_joint_gate_banded_fwd alone, with the bytes per second of the (B, T, S, H) tensor it writes
  gate_bwd  pika_joint_gate_banded_bwd alone (it reads dh twice: encoder side, prediction side), with its bytes per second
  torch     the same gate spelled in torch: rnnt_prune_lm on p1 / pg, tanh * sigmoid, and its autograd backward

    python tools/joint_pruned_time.py [--runs 10] [--warmup 2] [--out profiles/joint_pruned_time.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_pruned_time.txt"))
    args = ap.parse_args()
    import pika_amd  # noqa: F401
    from pika_amd import gemm as G
    from pika_amd.model import ops
    from pika_amd.model.hipops import BandedGateFn
    from pika_amd.rnnt import rnnt_loss_from_logits, rnnt_prune_lm, rnnt_pruned_joint_loss
    dev = torch.device("cuda:0")
    B, T, U, V, H, S = args.batch, args.frames, args.labels, args.vocab, args.width, args.band
    torch.manual_seed(1234)
    fc1, fcg, fc2 = torch.nn.Linear(2 * H, H).to(dev), torch.nn.Linear(2 * H, H).to(dev), torch.nn.Linear(H, V).to(dev)
    sam, slm = torch.nn.Linear(H, V).to(dev), torch.nn.Linear(H, V).to(dev)
    params = [p for m in (fc1, fcg, fc2, sam, slm) for p in m.parameters()]
    enc = torch.randn(B, T, H, device=dev, requires_grad=True)
    pred = torch.randn(B, U + 1, H, device=dev, requires_grad=True)
    labels = torch.randint(1, V, (B, U), device=dev, dtype=torch.int32)
    tl = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul = torch.full((B,), U, dtype=torch.int32, device=dev)

    def clear():
        for p in params + [enc, pred]:
            p.grad = None

    def full():
        logits = ops.joint(enc, pred, fc1, fcg, fc2, log_softmax=False)
        rnnt_loss_from_logits(logits, labels, tl, ul).sum().backward()
        clear()

    state = {}

    def pruned():
        simple, loss, state["ranges"] = rnnt_pruned_joint_loss(enc, pred, labels, tl, ul, fc1, fcg, fc2, sam, slm, s_range=S)
        state["costs"] = (simple.detach(), loss.detach())
        (0.5 * simple + loss).backward()
        clear()

    pruned()
    ranges = state["ranges"]
    state["simple"], state["pruned"] = (float(c) / B for c in state["costs"])
    r = ranges.cpu().numpy()
    d = np.diff(r, axis=1)
    valid = bool((r[:, 0] == 0).all() and (r[:, -1] == max(0, U + 1 - S)).all() and (d >= 0).all() and (d <= S - 1).all())
    # the gate alone, on the four small products of these layers
    with torch.no_grad():
        e1 = ops.linear(enc, fc1.weight[:, :H].contiguous(), fc1.bias).float().contiguous()
        p1 = ops.linear(pred, fc1.weight[:, H:].contiguous()).float().contiguous()
        eg = ops.linear(enc, fcg.weight[:, :H].contiguous(), fcg.bias).float().contiguous()
        pg = ops.linear(pred, fcg.weight[:, H:].contiguous()).float().contiguous()
    small = [t.requires_grad_(True) for t in (e1, p1, eg, pg)]
    hdt = torch.bfloat16 if G.joint_in_bf16() else torch.float32
    dh = torch.randn(B, T, S, H, device=dev).to(hdt)

    def gate_fwd():
        state["h"] = BandedGateFn.apply(*small, ranges, S)

    def gate_bwd():
        state.pop("h").backward(dh)
        for t in small:
            t.grad = None

    def torch_gate():
        z1 = small[0].unsqueeze(2) + rnnt_prune_lm(small[1], ranges, S)
        zg = small[2].unsqueeze(2) + rnnt_prune_lm(small[3], ranges, S)
        (torch.tanh(z1) * torch.sigmoid(zg)).to(hdt).backward(dh)
        for t in small:
            t.grad = None

    legs = [("full", full, None), ("pruned", pruned, None), ("gate_fwd", gate_fwd, None), ("gate_bwd", gate_bwd, gate_fwd),
            ("torch", torch_gate, None)]
    times = {name: [] for name, _, _ in legs}
    for i in range(args.warmup + args.runs):
        for name, fn, before in legs:
            if before:
                before()
            e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1_.record()
            e1_.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1_))
    med = {k: float(np.median(v)) for k, v in times.items()}
    hbytes = B * T * S * H * dh.element_size()
    gate = med["gate_fwd"] + med["gate_bwd"]
    lines = [
        "tools/joint_pruned_time.py: B=%d T=%d U=%d V=%d H=%d S=%d, mode %s, medians of %d alternating runs (ms)" % (
            B, T, U, V, H, S, G.PRECISION, args.runs),
        "full      ops.joint + rnnt_loss_from_logits, (B,T,U+1) lattice  fwd+bwd %9.3f" % med["full"],
        "pruned    rnnt_pruned_joint_loss, band of %d                      fwd+bwd %9.3f   ratio pruned/full %.4f" % (
            S, med["pruned"], med["pruned"] / med["full"]),
        "gate_fwd  pika_joint_gate_banded_fwd (writes %.3f GB %s)        %9.3f   %.2f TB/s" % (
            hbytes / 1e9, str(hdt).split(".")[-1], med["gate_fwd"], hbytes / med["gate_fwd"] / 1e9),
        "gate_bwd  pika_joint_gate_banded_bwd (reads dh twice)                    %9.3f   %.2f TB/s" % (
            med["gate_bwd"], 2 * hbytes / med["gate_bwd"] / 1e9),
        "torch     rnnt_prune_lm + tanh * sigmoid, the same gate         fwd+bwd %9.3f   ratio kernels/torch %.4f" % (
            med["torch"], gate / med["torch"]),
        "ranges valid: %s; mean simple cost %.3f, mean pruned cost %.3f" % (valid, state["simple"], state["pruned"]),
        json.dumps({"tool": "joint_pruned_time", "B": B, "T": T, "U": U, "V": V, "H": H, "S": S, "mode": G.PRECISION,
                    "runs": args.runs, "median_ms": {k: round(v, 4) for k, v in med.items()},
                    "ratio": round(med["pruned"] / med["full"], 4), "gate_fwd_TBps": round(hbytes / med["gate_fwd"] / 1e9, 3),
                    "gate_bwd_TBps": round(2 * hbytes / med["gate_bwd"] / 1e9, 3), "ranges_valid": valid}),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
