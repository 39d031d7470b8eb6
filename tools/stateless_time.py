"""HIP-event times of the stateless prediction network (include/pika_stateless.h, pika_amd/model/stateless.py).

    python tools/stateless_time.py [--runs 10] [--warmup 3] [--out profiles/stateless_time.txt]

* the search's step, `StatelessContext.follow`, at (B, K, D, ctx) = (64, 4, 512, 2) and (64, 16, 512, 2), V = 5000: the
  kernel next to its torch spelling (gather, shift, where, embedding, grouped conv, ReLU: the CPU path of the same class
  on the device), 50 calls per bracket on fixed random (parent, token);
* one whole frame step of `modified_beam_search` at (B, beam, V) = (64, 4, 5000), H = 512, with the stateless network
  next to the LSTM one (decoder_type 'rnn', one layer), eager and as the captured graph: the call on 60 frames minus the
  call on 10 frames, over 50 -- the encoder and the set-up cancel;
* training forward + backward at (B, U, D, V) = (32, 51, 512, 5000): the kernels next to `nn.Embedding` + `nn.Conv1d`
  autograd (`stateless_reference`), gradients of E and w for a fixed d(out).
The variants alternate inside one loop, every one is warmed up, medians of `runs` with minimum and maximum.  Reported,
not gated: nothing here is asserted anywhere.  Needs a GPU.
"""
import argparse
import os
import statistics
import sys

import torch

from ctc_timing import measure  # (first: it puts the repository on sys.path)
from pika_amd import StatelessContext, StatelessPredNet, modified_beam_search
from pika_amd.model import transducer
from pika_amd.model.stateless import stateless_reference

CALLS, V = 50, 5000


def search_model(decoder_type, dev):
    opt = argparse.Namespace(rnn_size=512, local_rank=0, decoder_type=decoder_type, brnn=False, encoder_type='rnn',
                             dropout=0.0, enc_layers=1, dec_layers=1, embd_dim=512, padding_idx=None)
    torch.manual_seed(0)
    return transducer.Net(opt, 40, V).eval().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "stateless_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stateless_time.py: no HIP device")
    dev = torch.device("cuda")
    lines = ["device: %s   runs %d, warm-up %d; times in ms: median [min, max]" % (
        torch.cuda.get_device_name(0), args.runs, args.warmup)]
    variants, per = [], {}

    # ---- the step
    torch.manual_seed(1)
    for B, K, D, ctx in ((64, 4, 512, 2), (64, 16, 512, 2)):
        net = StatelessPredNet(V, D, ctx).to(dev)
        g = torch.Generator().manual_seed(K)
        parent = torch.randint(0, K, (B, K), generator=g).to(dev)
        token = (torch.randint(0, V, (B, K), generator=g) * (torch.rand(B, K, generator=g) < 0.5)).to(dev)
        for name, native in (("kernel", True), ("torch", False)):
            c = StatelessContext(net, B, K)
            assert c.native
            c.native = native

            def run(c=c, parent=parent, token=token):
                for _ in range(CALLS):
                    c.follow(parent, token)
            name = "follow, %s, %d calls, (B,K,D,ctx) = (%d,%d,%d,%d)" % (name, CALLS, B, K, D, ctx)
            variants.append((name, run))
            per[name] = CALLS

    # ---- training forward + backward
    B, U, D = 32, 51, 512
    net = StatelessPredNet(V, D, 2).to(dev)
    y = torch.randint(0, V, (B, U), device=dev)
    y[:, 0] = 0
    dout = torch.randn(B, U, D, device=dev)
    params = [net.embedding.weight, net.conv.weight]
    for name, fn in (("kernels", net), ("nn.Embedding + nn.Conv1d", lambda y_: stateless_reference(y_, *params))):
        name = "forward + backward, %s, (B,U,D,V) = (%d,%d,%d,%d)" % (name, B, U, D, V)
        variants.append((name, lambda fn=fn: torch.autograd.grad(fn(y), params, dout)))
        per[name] = 1

    # ---- the whole frame step
    searches = {}
    for dec in ("stateless", "rnn"):
        model = search_model(dec, dev)
        x = torch.randn(64, 60, 40, device=dev)
        for graph in (False, True):
            for T in (10, 60):
                name = "modified_beam_search, %s, %s, %d frames, (B,beam,V) = (64,4,%d)" % (
                    dec, "graph" if graph else "eager", T, V)
                x_len = torch.full((64,), T, dtype=torch.int64)
                variants.append((name, lambda model=model, x=x[:, :T].contiguous(), x_len=x_len, graph=graph:
                                 modified_beam_search(model, x, x_len, beam=4, use_graph=graph)))
                per[name] = 1
                searches[(dec, graph, T)] = name

    times = measure(variants, args.warmup, args.runs)
    for name, _ in variants:
        t = times[name]
        lines.append("  %-86s %8.3f [%8.3f, %8.3f]   %7.1f us per call" % (
            name, statistics.median(t), min(t), max(t), 1e3 * statistics.median(t) / per[name]))
    lines.append("one frame step = (60 frames - 10 frames) / 50, from the medians:")
    for dec in ("stateless", "rnn"):
        for graph in (False, True):
            a, b = (statistics.median(times[searches[(dec, graph, T)]]) for T in (60, 10))
            lines.append("  %-9s %-5s %8.1f us per step" % (dec, "graph" if graph else "eager", 1e3 * (a - b) / 50))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
