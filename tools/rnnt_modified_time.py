"""What the modified-topology RNN-T calls cost next to their regular counterparts, from the same build.

The benchmark's lattice (B = 32, T = 1000, U = 50, V = 5000, S = 5; inputs seed 1234, full length).  Timed by HIP events
on the launch stream, forward plus backward through autograd, `--runs` runs each, all legs alternating in one loop on one
device, medians reported; every leg is a regular call and the modified call of the same inputs:

  planes   rnnt_loss_from_planes / _modified                 on the two (B, T, U+1) planes of the full tensor
  search   rnnt_prune_ranges / _modified                     on each topology's own occupancies
  pruned   rnnt_loss_pruned_from_logits / _modified          on the (B, T, S, V) rows of each topology's own band
  chain    rnnt_pruned_joint_loss_smoothed / _modified       H = 1024 joint, scales (0.25, 0), GEMM mode "mixed"

and the parity of the modified calls at this shape against float64 (the reference DP of tests/rnnt_modified_common.py):
costs and occupancies of the planes loss, costs of the pruned loss on its band.

    python tools/rnnt_modified_time.py [--runs 10] [--warmup 2] [--out profiles/rnnt_modified_time.txt]
                                       [--parity profiles/rnnt_modified_parity.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--labels", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=5000)
    ap.add_argument("--band", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_modified_time.txt"))
    ap.add_argument("--parity", default=os.path.join(ROOT, "profiles", "rnnt_modified_parity.txt"))
    args = ap.parse_args()
    import pika_amd  # noqa: F401
    from bench import make_inputs
    from pika_amd import gemm as G
    from pika_amd import rnnt as Rn
    import rnnt_modified_common as M
    dev = torch.device("cuda:0")
    B, T, U, V, S, H = args.batch, args.frames, args.labels, args.vocab, args.band, args.hidden
    full, labels, tl, ul = make_inputs(B, T, U, V, dev, 1234)
    tl, ul = tl.int(), ul.int()
    blank_lp = full[..., 0].contiguous()
    label_lp = torch.gather(full[:, :, :U], 3, labels.long()[:, None, :, None].expand(B, T, U, 1))[..., 0]
    label_lp = torch.cat([label_lp, label_lp.new_full((B, T, 1), -1.0e30)], 2).contiguous()

    topo = {"regular": (Rn.rnnt_loss_from_planes, Rn.rnnt_prune_ranges, Rn.rnnt_loss_pruned_from_logits,
                        Rn.rnnt_pruned_joint_loss_smoothed),
            "modified": (Rn.rnnt_loss_from_planes_modified, Rn.rnnt_prune_ranges_modified,
                         Rn.rnnt_loss_pruned_modified_from_logits, Rn.rnnt_pruned_joint_loss_modified)}
    torch.manual_seed(0)
    layers = [torch.nn.Linear(i, o).to(dev) for i, o in [(2 * H, H), (2 * H, H), (H, V), (H, V), (H, V)]]
    params = [p for m in layers for p in (m.weight, m.bias)]
    g = torch.Generator().manual_seed(1)
    enc = torch.randn(B, T, H, generator=g).to(dev).requires_grad_(True)
    pred = torch.randn(B, U + 1, H, generator=g).to(dev).requires_grad_(True)

    legs, keep = [], {}
    for name, (planes_fn, search_fn, pruned_fn, chain_fn) in topo.items():
        _, ob, ol = planes_fn(blank_lp, label_lp, tl, ul, return_occupancy=True)
        ranges = search_fn(ob, ol, tl, ul, S)
        idx = (ranges.long()[:, :, None] + torch.arange(S, device=dev)).clamp_max(U)
        band = torch.gather(full, 2, idx[..., None].expand(B, T, S, V)).contiguous().requires_grad_(True)
        pb, pl = blank_lp.clone().requires_grad_(True), label_lp.clone().requires_grad_(True)
        keep[name] = (ob, ol, ranges, band)

        def planes(fn=planes_fn, pb=pb, pl=pl):
            fn(pb, pl, tl, ul).sum().backward()
            pb.grad = pl.grad = None

        def search(fn=search_fn, ob=ob, ol=ol):
            fn(ob, ol, tl, ul, S)

        def pruned(fn=pruned_fn, band=band, ranges=ranges):
            fn(band, labels, ranges, tl, ul).sum().backward()
            band.grad = None

        def chain(fn=chain_fn):
            s, p, _ = fn(enc, pred, labels, tl, ul, *layers, s_range=S, lm_only_scale=0.25)
            (0.5 * s + p).backward()
            enc.grad = pred.grad = None
            for q in params:
                q.grad = None

        legs += [("planes " + name, planes), ("search " + name, search), ("pruned " + name, pruned), ("chain " + name, chain)]
    legs.sort(key=lambda kv: kv[0])                      # regular / modified of one call next to each other ...
    times = {name: [] for name, _ in legs}
    for i in range(args.warmup + args.runs):
        # ... and which of the two goes first alternates, so neither always runs behind a different call
        order = legs if i % 2 == 0 else [legs[j ^ 1] for j in range(len(legs))]
        for name, fn in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = ["tools/rnnt_modified_time.py: B=%d T=%d U=%d V=%d S=%d H=%d, GEMM mode %s, fwd+bwd, medians of %d alternating "
             "runs (ms)" % (B, T, U, V, S, H, G.PRECISION, args.runs)]
    for call in ("planes", "search", "pruned", "chain"):
        r, m = med[call + " regular"], med[call + " modified"]
        lines.append("%-7s regular %9.3f   modified %9.3f   modified/regular %.3f" % (call, r, m, m / r))
    lines.append(json.dumps({"tool": "rnnt_modified_time", "B": B, "T": T, "U": U, "V": V, "S": S, "H": H, "runs": args.runs,
                             "mode": G.PRECISION, "median_ms": {k: round(v, 4) for k, v in med.items()}}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)

    # parity of the modified calls at this shape against float64
    ob, ol, ranges, band = keep["modified"]
    tl_n, ul_n, r_n = tl.cpu().numpy(), ul.cpu().numpy(), ranges.cpu().numpy()
    with torch.no_grad():
        c_pl = Rn.rnnt_loss_from_planes_modified(blank_lp, label_lp, tl, ul).double().cpu().numpy()
        c_pr = Rn.rnnt_loss_pruned_modified_from_logits(band.detach(), labels, ranges, tl, ul).double().cpu().numpy()
    pb64, pl64 = blank_lp.double().cpu().numpy(), label_lp.double().cpu().numpy()
    c64, ob64, ol64 = M.planes_loss_ref(pb64, pl64, tl_n, ul_n)
    valid = all(M.is_valid_modified(r_n[n], int(tl_n[n]), int(ul_n[n]), S) for n in range(B))
    s = M.clamp_ranges(r_n, ul_n, S)
    with torch.no_grad():                                # the band's two columns in float64, (B, T, S) each
        lp64 = torch.log_softmax(band.detach().double(), -1)
        cols = torch.from_numpy(s).to(dev)[:, :, None] + torch.arange(S, device=dev)
        yb = torch.gather(labels.long(), 1, cols.clamp_max(U - 1).reshape(B, T * S)).reshape(B, T, S)
        band_b = lp64[..., 0].cpu().numpy()
        band_l = torch.gather(lp64, 3, yb[..., None])[..., 0].cpu().numpy()
        del lp64
    bb, bl = np.full((B, T, U + 1), -np.inf), np.full((B, T, U + 1), -np.inf)
    tt = np.arange(T)
    for b in range(B):
        for j in range(S):
            u = s[b] + j
            t = tt[u <= ul_n[b]]
            bb[b, t, u[t]] = band_b[b, t, j]
            t = tt[u < ul_n[b]]
            bl[b, t, u[t]] = band_l[b, t, j]
    cb64 = M.planes_loss_ref(bb, bl, tl_n, ul_n)[0]
    plines = [
        "tools/rnnt_modified_time.py parity: B=%d T=%d U=%d V=%d S=%d against float64" % (B, T, U, V, S),
        "planes loss   cost max rel err %.3g   occupancy max abs err blank %.3g label %.3g" % (
            float(np.max(np.abs(c_pl - c64) / np.abs(c64))), float(np.abs(ob.double().cpu().numpy() - ob64).max()),
            float(np.abs(ol.double().cpu().numpy() - ol64).max())),
        "pruned loss   cost max rel err %.3g (from logits, on the band of rnnt_prune_ranges_modified)" % (
            float(np.max(np.abs(c_pr - cb64) / np.abs(cb64)))),
        "ranges valid: %s; mean cost full lattice %.3f, band %.3f (band >= full: %s)" % (
            valid, float(c64.mean()), float(cb64.mean()), bool((c_pr >= c_pl - 1e-5 * np.abs(c_pl)).all())),
    ]
    ptext = "\n".join(plines) + "\n"
    print(ptext, end="")
    with open(args.parity, "w") as f:
        f.write(ptext)


if __name__ == "__main__":
    main()
