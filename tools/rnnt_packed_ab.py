"""A/B of the padded and the packed (compact=True) RNN-T loss on one ragged batch.

The SURVEY 8d ragged M1 batch of bench.py (B = 32, T = 1000, U = 50, V = 5000; log-probs seed 1234, lengths seed 1236:
T_n ~ U{600..1000}, U_n ~ U{20..50}) runs as the padded (B, T, U+1, V) tensor and as its packed (N, V) rows.  One step
is forward + backward (`rnnt_loss(...).sum().backward()`), timed by HIP events on the launch stream; after the warm-up
the two layouts alternate, `--steps` steps each, over `--rounds` rounds.  The packed call's one host sync (the length
vectors) is inside its step.  Prints the algorithmic gradient-write bytes of each (N V 4 against B T U1 V 4), the
per-round ms and the medians, and one JSON line.  Costs must agree bit for bit, and so must the gradient on a sample of
live rows.

    python tools/rnnt_packed_ab.py [--steps 5] [--warmup 2] [--rounds 3]
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import pika_amd  # noqa: F401
    from bench import make_inputs
    from pika_amd.rnnt import rnnt_loss
    dev = torch.device("cuda:0")
    B, T, U, V = args.batch, args.frames, args.labels, args.vocab
    lp, labels, _, _ = make_inputs(B, T, U, V, dev, 1234)
    g = torch.Generator().manual_seed(1236)
    tl = torch.randint(int(0.6 * T), T + 1, (B,), generator=g).int()
    ul = torch.randint(int(0.4 * U), U + 1, (B,), generator=g).int()
    # the padded tensor is the benchmark's (B, T, U+1, V); the packed rows are its live cells
    lpk = torch.cat([lp[n, :tl[n], :ul[n] + 1].reshape(-1, V) for n in range(B)])
    yk = torch.cat([labels[n, :ul[n]] for n in range(B)])
    labels = torch.where(torch.arange(U, device=dev).unsqueeze(0) < ul.to(dev).unsqueeze(1), labels,
                         torch.full_like(labels, V))
    tl_d, ul_d = tl.to(dev), ul.to(dev)
    N = lpk.shape[0]
    lp.requires_grad_(True)
    lpk.requires_grad_(True)
    bytes_pad = B * T * (U + 1) * V * 4
    bytes_pk = N * V * 4
    print("batch B=%d T=%d U=%d V=%d, T_n in [%d, %d], U_n in [%d, %d]" % (B, T, U, V, int(tl.min()), int(tl.max()),
                                                                      int(ul.min()), int(ul.max())))
    print("gradient write, algorithmic: padded %.3f GB (B*T*U1*V*4), packed %.3f GB (N*V*4, N = %d): ratio %.4f" % (
        bytes_pad / 1e9, bytes_pk / 1e9, N, bytes_pk / bytes_pad))

    def step_padded():
        lp.grad = None
        c = rnnt_loss(lp, labels, tl_d, ul_d)
        c.sum().backward()
        return c

    def step_packed():
        lpk.grad = None
        c = rnnt_loss(lpk, yk, tl_d, ul_d, compact=True)
        c.sum().backward()
        return c

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for _ in range(args.warmup):
        cp = step_padded()
        ck = step_packed()
    torch.cuda.synchronize()
    costs_equal = bool(torch.equal(cp.detach(), ck.detach()))
    # a sample of live rows: packed row k of utterance n against the padded cell it came from
    rng = np.random.default_rng(0)
    roff = np.concatenate([[0], np.cumsum((tl * (ul + 1)).numpy())[:-1]])
    grad_equal = True
    for n in rng.choice(B, 4, replace=False):
        t = int(rng.integers(0, int(tl[n])))
        u = int(rng.integers(0, int(ul[n]) + 1))
        grad_equal &= bool(torch.equal(lpk.grad[int(roff[n]) + t * (int(ul[n]) + 1) + u], lp.grad[n, t, u]))
    print("costs bit-equal: %s, sampled gradient rows bit-equal: %s" % (costs_equal, grad_equal))
    rounds = []
    for r in range(args.rounds):
        a = timed(step_padded, args.steps)
        b = timed(step_packed, args.steps)
        rounds.append((a, b))
        print("round %d: padded %.3f ms/step, packed %.3f ms/step, ratio %.4f" % (r, a, b, b / a))
    pa = float(np.median([a for a, _ in rounds]))
    pb = float(np.median([b for _, b in rounds]))
    print("median: padded %.3f ms, packed %.3f ms, measured ratio %.4f (algorithmic bytes ratio %.4f)" % (
        pa, pb, pb / pa, bytes_pk / bytes_pad))
    print(json.dumps({"tool": "rnnt_packed_ab", "B": B, "T": T, "U": U, "V": V, "N": N, "steps": args.steps,
                      "rounds": [[round(a, 4), round(b, 4)] for a, b in rounds], "padded_ms": round(pa, 4),
                      "packed_ms": round(pb, 4), "ratio_ms": round(pb / pa, 4), "grad_bytes_padded": bytes_pad,
                      "grad_bytes_packed": bytes_pk, "ratio_bytes": round(bytes_pk / bytes_pad, 4),
                      "costs_bit_equal": costs_equal, "grad_rows_bit_equal": grad_equal}))


if __name__ == "__main__":
    main()
