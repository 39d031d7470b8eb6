"""The stateless prediction network's kernels on the device (include/pika_stateless.h, csrc/stateless.hip) against the
float64 numpy definition (tests/stateless_common.py) within the derived bound gamma(n + 2) * sum|terms| of that module:
forward, backward (with the ReLU mask taken from the kernel's own forward where |z_ref| lies below the forward bound),
forward + backward in one captured graph, and the search's step kernel behind a `ModifiedBeamState`."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stateless_common as SC  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, U, V, D, cpg, ctx): the smallest there is; D no multiple of 64; a single group and U < ctx; depthwise, ctx = 1; more
# than one workgroup per row and per launch, D no multiple of the d_w tile
CASES = [(1, 1, 5, 4, 4, 2), (3, 5, 9, 20, 4, 2), (2, 2, 7, 8, 8, 3), (2, 7, 11, 64, 1, 1), (3, 6, 300, 516, 4, 2)]
ONE_TOKEN = (3, 5, 9, 20, 4, 2, "one token")        # all B U positions hold ONE token: the longest group of d_E


@functools.lru_cache(maxsize=None)
def reference(case):
    B, U, V, D, cpg, ctx = case[:6]
    seed = CASES.index(case) if case in CASES else 99
    y = SC.labels(B, U, V, seed)
    if len(case) > 6:
        y[:] = 2
    E, w = SC.weights(V, D, cpg, ctx, seed)
    z, a = SC.forward(y, E, w)
    dout = np.random.RandomState(77 + seed).standard_normal(z.shape).astype(np.float32)
    for t in (y, E, w, z, a, dout):
        t.setflags(write=False)
    return y, E, w, z, a, dout


def ptr(t):
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_forward(y, E, w, ld=None):
    """pika_stateless_forward itself -> the (B U, ld) buffer, NaN where the kernel did not write."""
    from pika_amd import _lib
    (B, U), (V, D), (_, cpg, ctx) = y.shape, E.shape, w.shape
    ld = D if ld is None else ld
    buf = torch.full((B * U, ld), float("nan"), device=y.device)
    _lib.check(_lib.lib().pika_stateless_forward(ptr(y), y.stride(0), ptr(E), ptr(w), B, U, V, D, cpg, ctx, ptr(buf), ld,
                                                 stream()), "pika_stateless_forward")
    return buf


def run_backward(y, E, w, out, dout):
    """pika_stateless_backward itself on NaN-filled d_E, d_w."""
    from pika_amd import _lib
    lib = _lib.lib()
    (B, U), (V, D), (_, cpg, ctx) = y.shape, E.shape, w.shape
    sorted_tok, order = torch.sort(y.reshape(-1), stable=True)
    d_E = torch.full((V, D), float("nan"), device=y.device)
    d_w = torch.full((D, cpg, ctx), float("nan"), device=y.device)
    nbytes = lib.pika_stateless_backward_workspace_bytes(B, U, D, cpg, ctx)
    assert nbytes > 0
    work = torch.full((nbytes // 4,), float("nan"), device=y.device)
    _lib.check(lib.pika_stateless_backward(ptr(y), y.stride(0), ptr(sorted_tok), ptr(order), ptr(E), ptr(w), ptr(out),
                                           out.stride(0), ptr(dout), dout.stride(0), B, U, V, D, cpg, ctx, ptr(d_E),
                                           ptr(d_w), ptr(work), stream()), "pika_stateless_backward")
    return d_E, d_w


def on_device(case, dev):
    y, E, w, z, a, dout = reference(case)
    return [torch.from_numpy(np.array(t)).to(dev) for t in (y, E, w, dout)]


def module_for(case, dev):
    from pika_amd import StatelessPredNet
    B, U, V, D, cpg, ctx = case[:6]
    y, E, w = reference(case)[:3]
    net = StatelessPredNet(V, D, ctx, groups=D // cpg)
    with torch.no_grad():
        net.embedding.weight.copy_(torch.from_numpy(np.array(E)))
        net.conv.weight.copy_(torch.from_numpy(np.array(w)))
    return net.to(dev)


@pytest.mark.parametrize("case", CASES)
def test_forward_against_float64(hip_device, case):
    B, U, V, D, cpg, ctx = case
    y, E, w, z, a, _ = reference(case)
    yd, Ed, wd, _ = on_device(case, hip_device)
    buf = run_forward(yd, Ed, wd, ld=D + 3)                           # an output view with ld > D
    assert bool(torch.isnan(buf[:, D:]).all())                       # nothing beyond the row's width
    got = buf[:, :D].cpu().numpy().reshape(B, U, D)
    ok, worst = SC.within(got, np.maximum(z, 0.0), a, cpg * ctx)      # (ReLU is 1-Lipschitz: z's bound holds for out)
    print("forward %s: worst error / bound = %.3f" % (case, worst))
    assert ok, worst
    assert (got >= 0).all()
    # the same bits through a contiguous output, through the module, and from a MISALIGNED E (scalar loads)
    assert torch.equal(run_forward(yd, Ed, wd), buf[:, :D])
    assert torch.equal(module_for(case, hip_device)(yd).reshape(B * U, D), buf[:, :D])
    flat = torch.empty(V * D + 1, device=hip_device)
    shifted = flat[1:].view(V, D)
    shifted.copy_(Ed)
    assert Ed.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    assert torch.equal(run_forward(yd, shifted, wd), buf[:, :D])
    # a padded y (row stride > U) reads the same rows
    wide = torch.full((B, U + 2), V - 1, dtype=torch.int64, device=hip_device)
    wide[:, :U] = yd
    assert torch.equal(run_forward(wide[:, :U], Ed, wd), buf[:, :D])


@pytest.mark.parametrize("case", CASES + [ONE_TOKEN], ids=str)
def test_backward_against_float64(hip_device, case):
    B, U, V, D, cpg, ctx = case[:6]
    y, E, w, z, a, dout = reference(case)
    yd, Ed, wd, doutd = on_device(case, hip_device)
    out = run_forward(yd, Ed, wd)
    mask = out.cpu().numpy().reshape(B, U, D) > 0
    near = np.abs(z) <= SC.out_bound(a, w)                            # only there may the kernel's sign differ from z's
    assert ((mask == (z > 0)) | near).all()
    go = dout.astype(np.float64) * np.where(near, mask, z > 0)
    (d_E, a_E, n_E), (d_w, a_w, n_w) = SC.backward(y, E, w, go)
    got_E, got_w = run_backward(yd, Ed, wd, out, doutd.reshape(B * U, D))
    ok_E, worst_E = SC.within(got_E.cpu().numpy(), d_E, a_E, n_E)
    ok_w, worst_w = SC.within(got_w.cpu().numpy(), d_w, a_w, n_w)
    print("backward %s: worst error / bound d_E %.3f, d_w %.3f" % (case, worst_E, worst_w))
    assert ok_E and ok_w, (worst_E, worst_w)                          # (a NaN left in a buffer fails here: written in full)
    unseen = sorted(set(range(V)) - set(int(t) for t in np.asarray(y).reshape(-1)))
    assert unseen
    assert bool((got_E[unseen] == 0).all()) and not bool(torch.signbit(got_E[unseen]).any())
    # a second run on fresh NaN-filled buffers and a fresh workspace: the same bits
    again_E, again_w = run_backward(yd, Ed, wd, out, doutd.reshape(B * U, D))
    assert torch.equal(got_E, again_E) and torch.equal(got_w, again_w)
    # and the module's autograd is this call
    net = module_for(case, hip_device)
    net(yd).backward(doutd)
    assert torch.equal(net.embedding.weight.grad, got_E) and torch.equal(net.conv.weight.grad, got_w)


def test_forward_and_backward_in_one_graph(hip_device):
    case = CASES[1]
    B, U, V, D, cpg, ctx = case
    net = module_for(case, hip_device)
    params = [net.embedding.weight, net.conv.weight]
    yd, _, _, doutd = on_device(case, hip_device)
    y_in, dout_in = yd.clone(), doutd.clone()

    def run():
        out = net(y_in)
        return (out,) + torch.autograd.grad(out, params, dout_in)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                       # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = run()
    rng = np.random.RandomState(4)
    for _ in range(2):                                              # fresh input values, same buffers
        y_new = SC.labels(B, U, V, seed=int(rng.randint(1000)))
        y_in.copy_(torch.from_numpy(y_new))
        dout_in.copy_(torch.from_numpy(rng.standard_normal((B, U, D)).astype(np.float32)))
        graph.replay()
        eager = run()
        for a, b in zip(held, eager):
            assert torch.equal(a, b)
        assert bool((eager[1] != 0).any())


def expected_follow(old, parent, token, blank):
    B, K, ctx = old.shape
    new = np.empty_like(old)
    for b in range(B):
        for j in range(K):
            c = list(old[b, min(max(int(parent[b, j]), 0), K - 1)])
            if token[b, j] != blank:
                c = c[1:] + [int(token[b, j])]
            new[b, j] = c
    return new


@pytest.mark.parametrize("B,K,ctx,D", [(1, 1, 1, 8), (3, 4, 2, 20), (2, 64, 3, 64)])
def test_step_kernel_behind_a_search(hip_device, B, K, ctx, D):
    from pika_amd import ModifiedBeamState, StatelessContext, StatelessPredNet
    dev, V, T = hip_device, 7, 12
    torch.manual_seed(B * 100 + K)
    net = StatelessPredNet(V, D, ctx, groups=D // 4).to(dev)
    context = StatelessContext(net, B, K)
    assert context.native
    state = ModifiedBeamState(B, T, K, 0, dev)
    num_frames = torch.tensor([T, 7, 0][:B] if B != 2 else [5, T], device=dev)
    gen = torch.Generator().manual_seed(K)

    def check(live_hyps):
        tok = context.tokens.cpu().numpy()
        # rows: pika_stateless_forward on the contexts (label rows of length ctx, last position), bit for bit
        want = net(context.tokens.view(B * K, ctx).long())[:, -1, :]
        assert torch.equal(context.rows, want)
        if live_hyps:
            hyp, ln = (t.cpu().numpy() for t in state.hyps())
            live = (state.scores > -float("inf")).cpu().numpy()
            for b in range(B):
                for j in range(K):
                    if live[b, j]:
                        assert list(tok[b, j]) == SC.context_of(hyp[b, j, :ln[b, j]], ctx), (b, j)
        return tok

    old = check(True)
    assert (old == np.array(SC.context_of([], ctx))).all()
    grown = 0
    for t in range(T):
        logits = (3.0 * torch.randn(B * K, V, generator=gen)).to(dev)
        parent, token = state.advance(logits, num_frames)
        context.follow(parent, token)
        tok = check(True)
        assert (tok == expected_follow(old, parent.cpu().numpy(), token.cpu().numpy(), 0)).all()       # dead slots too
        for b, n in enumerate(num_frames.tolist()):
            if t >= n:                                              # inactive: parent identity, token blank
                assert (tok[b] == old[b]).all()
        grown += int((token != 0).sum())
        old = tok
    assert grown > 0 and state.frames.tolist() == num_frames.clamp(max=T).tolist()
    if K >= 2:
        # the in-place hazard, hand-made: slots 0 and 1 name the same parent, and slot 0's parent has a higher index than
        # itself; the last slot reads slot 0, which has been rewritten by then if the kernel works in place
        parent = torch.arange(K, device=dev).repeat(B, 1)
        parent[:, 0], parent[:, 1], parent[:, K - 1] = 1, 1, 0
        token = torch.zeros((B, K), dtype=torch.int64, device=dev)
        token[:, 0], token[:, K - 1] = 3, 4
        context.follow(parent, token)
        tok = check(False)
        want = expected_follow(old, parent.cpu().numpy(), token.cpu().numpy(), 0)
        assert (tok == want).all()
        assert (old[:, 0] != old[:, 1]).any()                        # the case is one: the two old contexts differ
    context.reset(which=[True] + [False] * (B - 1))
    tok = check(False)
    assert (tok[0] == np.array(SC.context_of([], ctx))).all()
    if B > 1:
        assert (tok[1:] == (want if K >= 2 else old)[1:]).all()
