"""What the forced alignment adds to a forward call of the RNN-T loss.

The benchmark's lattice (B = 32, T = 1000, U = 50, V = 5000; log-probs seed 1234), full-length and with the ragged
lengths of tools/rnnt_packed_ab.py (seed 1236: T_n ~ U{600..1000}, U_n ~ U{20..50}).  On buffers allocated once, through
the C ABI: (a) `pika_rnnt_loss_forward` alone and (b) `pika_rnnt_loss_forward` + `pika_rnnt_align`, timed by HIP events
on the launch stream, `--steps` calls each, alternating over `--rounds` rounds after the warm-up.  Prints the per-round
ms, the medians, their difference, and one JSON line per batch.  The kernels' own times come from a kernel trace of
the same run:

    timeout -k 10 300 python tools/rnnt_align_time.py && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- \
        python tools/rnnt_align_time.py --rounds 1 --steps 5 --warmup 2

(`rnnt_align_kernel<1>` next to `rnnt_alpha_beta_kernel<1>` in OUT's kernel statistics; each step under its own time
limit, the second only if the first succeeded).

    python tools/rnnt_align_time.py [--steps 20] [--warmup 3] [--rounds 3]
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import pika_amd  # noqa: F401
    from bench import make_inputs
    from pika_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    B, T, U, V = args.batch, args.frames, args.labels, args.vocab
    U1 = U + 1
    lp, labels, _, _ = make_inputs(B, T, U, V, dev, 1234)
    g = torch.Generator().manual_seed(1236)
    tl_r = torch.randint(int(0.6 * T), T + 1, (B,), generator=g).int().to(dev)
    ul_r = torch.randint(int(0.4 * U), U + 1, (B,), generator=g).int().to(dev)
    tl_f = torch.full((B,), T, dtype=torch.int32, device=dev)
    ul_f = torch.full((B,), U, dtype=torch.int32, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    scores = torch.empty(B, dtype=torch.float32, device=dev)
    frames = torch.empty((B, U), dtype=torch.int32, device=dev)
    ws = torch.empty(L.pika_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    scratch = torch.empty(L.pika_rnnt_align_scratch_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def forward(tl, ul):
        _lib.check(L.pika_rnnt_loss_forward(lp.data_ptr(), labels.data_ptr(), tl.data_ptr(), ul.data_ptr(), B, T, U1, V, 0,
                                            costs.data_ptr(), ws.data_ptr(), stream), "pika_rnnt_loss_forward")

    def forward_align(tl, ul):
        forward(tl, ul)
        _lib.check(L.pika_rnnt_align(ws.data_ptr(), tl.data_ptr(), ul.data_ptr(), None, B, T, U1, scores.data_ptr(),
                                     frames.data_ptr(), scratch.data_ptr(), stream), "pika_rnnt_align")

    def timed(fn, tl, ul, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn(tl, ul)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for name, tl, ul in (("full", tl_f, ul_f), ("ragged", tl_r, ul_r)):
        for _ in range(args.warmup):
            forward(tl, ul)
            forward_align(tl, ul)
        torch.cuda.synchronize()
        ok = bool((scores <= -costs + 1.0).all())       # best path <= all paths (fp32 slack of the long sums)
        f = frames.cpu().numpy()
        uln, tln = ul.cpu().numpy(), tl.cpu().numpy()
        for n in range(B):
            fn = f[n, :uln[n]]
            ok &= bool((np.diff(fn) >= 0).all() and (fn >= 0).all() and (fn <= tln[n] - 1).all() and (f[n, uln[n]:] == -1).all())
        rounds = []
        for r in range(args.rounds):
            a = timed(forward, tl, ul, args.steps)
            b = timed(forward_align, tl, ul, args.steps)
            rounds.append((a, b))
            print("%s round %d: forward %.4f ms, forward + align %.4f ms, difference %.4f ms" % (name, r, a, b, b - a))
        fa = float(np.median([a for a, _ in rounds]))
        fb = float(np.median([b for _, b in rounds]))
        print("%s median: forward %.4f ms, forward + align %.4f ms, align adds %.4f ms; paths valid: %s" % (
            name, fa, fb, fb - fa, ok))
        print(json.dumps({"tool": "rnnt_align_time", "batch": name, "B": B, "T": T, "U": U, "V": V, "steps": args.steps,
                          "rounds": [[round(a, 4), round(b, 4)] for a, b in rounds], "forward_ms": round(fa, 4),
                          "forward_align_ms": round(fb, 4), "align_adds_ms": round(fb - fa, 4), "paths_valid": ok}))


if __name__ == "__main__":
    main()
