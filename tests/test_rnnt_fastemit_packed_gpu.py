"""FastEmit and the packed (compact) lattice layout of the RNN-T loss against the fp64 oracle and the padded routes.

FastEmit (Yu et al. 2021): the costs are -log P(y|x) as before; the expected gradient w.r.t. log_probs is the oracle's
with every label-emission entry (n, t, u, y_{u+1}), u < U_n, multiplied by 1 + lambda (blank entries and the zeros
outside the sub-lattice unchanged), times autograd's grad_output.  d(logits) routes: scale * (g~ - p * sum g~) with that
scaled g~, within the bound tests/test_rnnt_routes_gpu.py carries through it.

Packed layout: row off_n + t (U_n + 1) + u of a (N, V) tensor holds cell (n, t, u).  The same batch padded to exactly
(T_max, U1_max) runs the same lattice planes, so costs and every live gradient row must be bit-equal.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import log_softmax, make_case
from test_rnnt_routes_gpu import (_check_dlogits, _gemm_f16, _joint_case, _labels, _lse, _tol)

pytestmark = pytest.mark.gpu


def _L():
    from pika_amd import _lib
    return _lib.lib()


def _ok(rc, what):
    from pika_amd import _lib
    _lib.check(rc, what)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _fe(g64, y, tl, ul, lam):
    """The FastEmit gradient: each (n, t, u, y[n, u]) entry with t < T_n, u < U_n times 1 + lam."""
    g = g64.copy()
    for n in range(g.shape[0]):
        if ul[n] == 0:
            continue
        u = np.arange(ul[n])
        g[n, :tl[n], u, y[n, u]] *= 1.0 + lam
    return g


def _pack(a, tl, ul):
    """(B, T, U1, ...) -> (sum T_n (U_n + 1), ...): utterance-major, then t, then u."""
    return np.concatenate([a[n, :tl[n], :ul[n] + 1].reshape((-1,) + a.shape[3:]) for n in range(a.shape[0])])


def _pack_labels(y, ul):
    return np.concatenate([y[n, :ul[n]] for n in range(y.shape[0])]).astype(np.int32)


def _offsets(tl, ul):
    r = tl.astype(np.int64) * (ul + 1)
    return (np.cumsum(r) - r).astype(np.int32), (np.cumsum(ul) - ul).astype(np.int32), int(r.sum())


def _check(g, ref, D, what):
    rel, abs_ = _tol(D)
    err = np.abs(g.astype(np.float64) - ref)
    assert np.all(err <= rel * np.abs(ref) + abs_), (what, float((err - rel * np.abs(ref) - abs_).max()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. FastEmit on the dense route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-3, 0.5])
@pytest.mark.parametrize("B,T,U,V,blank", [(5, 20, 12, 30, 0), (4, 8, 64, 20, 19), (3, 6, 299, 12, 0)],
                         ids=["U1=13", "U1=65", "U1=300"])
def test_fastemit_dense_route_against_fp64(hip_device, B, T, U, V, blank, lam):
    from pika_amd.rnnt import rnnt_loss
    dev = hip_device
    lp, y, tl, ul = make_case(B, T, U, V, seed=U * 7 + V, ragged=True, blank=blank)
    assert tl.min() == 1 and ul.min() == 0
    c64, g64 = O.rnnt_loss(lp, y, tl, ul, blank=blank)
    args = [_d(a, dev) for a in (y, tl, ul)]
    x = _d(lp, dev).requires_grad_(True)
    loss = rnnt_loss(x, *args, average_frames=True, reduction="mean", blank=blank, fastemit_lambda=lam)
    loss.backward()
    costs = rnnt_loss(_d(lp, dev), *args, blank=blank, fastemit_lambda=lam)
    torch.cuda.synchronize()
    c = costs.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(c - c64) <= 1e-5 * np.abs(c64)), (c, c64)
    w = 1.0 / (B * tl.astype(np.float64))                          # grad_output of mean(costs / T_n)
    ref = _fe(g64, y, tl, ul, lam) * w[:, None, None, None]
    _check(x.grad.cpu().numpy(), ref, T + U, "fastemit lam=%g" % lam)
    if lam >= 0.1:      # the gradient is not the plain one (lambda = 1e-3 moves entries by less than the bound)
        plain = g64 * w[:, None, None, None]
        with pytest.raises(AssertionError):
            _check(x.grad.cpu().numpy(), plain, T + U, "plain")

    # lambda = 0 and no keyword: bit-identical
    grads = []
    for kw in ({}, {"fastemit_lambda": 0.0}):
        x0 = _d(lp, dev).requires_grad_(True)
        c0 = rnnt_loss(x0, *args, average_frames=True, reduction="mean", blank=blank, **kw)
        c0.backward()
        grads.append((c0.detach(), x0.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. FastEmit on the d(logits) routes: fused forward / backward (f32 via rnnt_loss_from_logits, bf16 at the C ABI), and
#    the lazy joint route -- loss_backward_fe(grads = NULL), then the compact d(logits) kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_fastemit_dlogits_routes(hip_device):
    from pika_amd.rnnt import rnnt_loss_from_logits
    dev = hip_device
    lam = 0.5
    V, blank, scale, B, T, U = 5000, 0, 0.75, 4, 6, 5
    U1 = U + 1
    R = B * T * U1
    rng = np.random.default_rng(5)
    tl = np.array([T, 1, T - 1, 1], np.int32)
    ul = np.array([U, 0, U - 2, U], np.int32)
    y = _labels(B, U, V, blank, ul, rng)
    A, Wt, bias, X, _, live = _joint_case(B, T, U1, V, blank, 77, tl, ul, boost=set(y[y < V].tolist()) | {blank})
    lse64 = _lse(X)
    lp = (X - lse64).astype(np.float32)
    w = (rng.random(B) + 0.5).astype(np.float32)
    _, g64 = O.rnnt_loss(lp.reshape(B, T, U1, V), y, tl, ul, blank=blank)
    g = (_fe(g64, y, tl, ul, lam) * w[:, None, None, None]).reshape(R, V)
    del g64
    rel, abs_ = _tol(T + U1 - 1)
    L = _L()
    y_d, tl_d, ul_d, w_d = (_d(a, dev) for a in (y, tl, ul, w))
    x32 = X.astype(np.float32)
    x64 = x32.astype(np.float64)
    p_raw = np.exp(x64 - _lse(x64))
    worst = {}

    # rnnt_loss_from_logits (f32 out)
    xl = _d(x32.reshape(B, T, U1, V), dev).requires_grad_(True)
    rnnt_loss_from_logits(xl, y_d, tl_d, ul_d, blank=blank, fastemit_lambda=lam).backward(w_d)
    torch.cuda.synchronize()
    _check_dlogits(xl.grad.reshape(R, V).cpu().numpy(), V, V, g, p_raw, 1.0, rel, abs_, False, live, "from_logits f32",
                   worst)

    # fused backward, bf16 out
    xin = _d(x32, dev)
    ws = torch.empty(L.pika_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    c = torch.empty(B, dtype=torch.float32, device=dev)
    lse = torch.empty(R, dtype=torch.float32, device=dev)
    _ok(L.pika_rnnt_fused_forward(_p(xin), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(c), _p(lse), _p(ws), _s()),
        "fused_forward")
    out = torch.full((R, V), float("nan"), dtype=torch.bfloat16, device=dev)
    _ok(L.pika_rnnt_fused_backward_fe(_p(xin), _p(lse), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(w_d), _p(ws),
                                      _p(out), 1, V, lam, _s()), "fused_backward_fe")
    torch.cuda.synchronize()
    _check_dlogits(out.float().cpu().numpy(), V, V, g, p_raw, 1.0, rel, abs_, True, live, "fused bf16", worst)

    # lazy joint route on log-probs: metadata with lambda, then pika_rnnt_dlogits_compact_bf16 (8-column kernel, colsum)
    lpd = _d(lp, dev)
    ws = torch.empty(L.pika_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    _ok(L.pika_rnnt_loss_forward(_p(lpd), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(c), _p(ws), _s()),
        "loss_forward")
    _ok(L.pika_rnnt_loss_backward_fe(_p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(w_d), _p(ws), None, lam, _s()),
        "loss_backward_fe (metadata)")
    out = torch.full((R, V), float("nan"), dtype=torch.bfloat16, device=dev)
    cs = torch.full((V,), float("nan"), dtype=torch.float32, device=dev)
    _ok(L.pika_rnnt_dlogits_compact_bf16(_p(lpd), None, _p(ws), B, T, U1, V, blank, _p(out), V, scale, _p(cs), _s()),
        "dlogits_compact_bf16")
    torch.cuda.synchronize()
    _check_dlogits(out.float().cpu().numpy(), V, V, g, np.exp(lp.astype(np.float64)), scale, rel, abs_, True, live,
                   "lazy compact", worst, colsum=cs.cpu().numpy())
    # ... and the dense tensor written later from the same metadata
    gd = torch.full((B, T, U1, V), float("nan"), dtype=torch.float32, device=dev)
    _ok(L.pika_rnnt_loss_dense_grads(_p(ws), B, T, U1, V, blank, _p(gd), _s()), "loss_dense_grads")
    torch.cuda.synchronize()
    _check(gd.cpu().numpy().reshape(R, V), g, T + U1 - 1, "lazy dense")

    # the 16-bit joint: gathered forward, metadata with lambda, _f16in compact8 with `gathered`
    A_d, W_d, bias_d = A.to(dev), Wt.to(dev), _d(bias, dev)
    out16, pm, ps, gat, n_part = _gemm_f16(dev, A_d, W_d, bias_d, R, V, V, y_d, T, U1, blank)
    ws = torch.empty(L.pika_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    _ok(L.pika_rnnt_fused_forward_gathered(_p(out16), V, _p(gat), _p(y_d), blank, _p(pm), _p(ps), n_part, _p(y_d), _p(tl_d),
                                           _p(ul_d), B, T, U1, V, blank, _p(c), _p(lse), _p(ws), _s()),
        "fused_forward_gathered")
    _ok(L.pika_rnnt_loss_backward_fe(_p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(w_d), _p(ws), None, lam, _s()),
        "loss_backward_fe (metadata)")
    out = torch.full((R, V), float("nan"), dtype=torch.bfloat16, device=dev)
    cs = torch.full((V,), float("nan"), dtype=torch.float32, device=dev)
    _ok(L.pika_rnnt_dlogits_compact_bf16_f16in(_p(out16), V, _p(lse), _p(ws), B, T, U1, V, blank, _p(out), V, scale,
                                               _p(cs), _p(gat), _p(y_d), blank, _s()), "dlogits_compact_f16in")
    torch.cuda.synchronize()
    xin = out16[:, :V].float().cpu().numpy().astype(np.float64)
    rr = np.arange(R)
    u, t, bb = rr % U1, (rr // U1) % T, rr // (T * U1)
    em = (t < tl[bb]) & (u < ul[bb])
    ye = y[bb[em], u[em]]
    xin[:, blank] = X[:, blank]
    xin[em, ye] = X[em, ye]
    _check_dlogits(out.float().cpu().numpy(), V, V, g, np.exp(xin - lse64), scale, rel, abs_, True, live, "f16in compact8",
                   worst, colsum=cs.cpu().numpy())
    print("\n[fastemit d(logits)] worst:", worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. packed vs padded, log-probs: all three dense writers, lattice widths NW = 1, 2, 16
# ---------------------------------------------------------------------------------------------------------------------
PACKED_CASES = [
    dict(B=5, T=12, U=6, V=5000),      # rnnt_grad_kernel<true, 2>
    dict(B=5, T=20, U=12, V=36),       # rnnt_grad_kernel<false, 4>
    dict(B=4, T=9, U=7, V=4999),       # rnnt_grad_scalar_kernel
    dict(B=3, T=10, U=100, V=36),      # NW = 2
    dict(B=2, T=3, U=1023, V=8),       # NW = 16: one utterance with U_n + 1 = 1024
]


@pytest.mark.parametrize("case", PACKED_CASES, ids=["V%d-U1=%d" % (c["V"], c["U"] + 1) for c in PACKED_CASES])
def test_packed_equals_padded_and_fp64(hip_device, case):
    from pika_amd.rnnt import rnnt_loss
    dev = hip_device
    B, T, U, V = case["B"], case["T"], case["U"], case["V"]
    lp, y, tl, ul = make_case(B, T, U, V, seed=B * 1000 + U + V, ragged=True)
    assert tl.max() == T and ul.max() == U          # the padded tensor is exactly (T_max, U1_max)
    args = [_d(a, dev) for a in (y, tl, ul)]
    xp = _d(lp, dev).requires_grad_(True)
    cp = rnnt_loss(xp, *args)
    cp.sum().backward()
    lpk, yk = _pack(lp, tl, ul), _pack_labels(y, ul)
    xk = _d(lpk, dev).requires_grad_(True)
    ck = rnnt_loss(xk, _d(yk, dev), args[1], args[2], compact=True)
    ck.sum().backward()
    torch.cuda.synchronize()
    assert ck.shape == (B,) and xk.grad.shape == (lpk.shape[0], V)
    assert torch.equal(ck.detach(), cp.detach())
    gp = xp.grad.cpu().numpy()
    gk = xk.grad.cpu().numpy()
    assert np.array_equal(gk, _pack(gp, tl, ul))
    # fp64
    c64, g64 = O.rnnt_loss(lp, y, tl, ul)
    c = ck.detach().cpu().numpy().astype(np.float64)
    assert np.all(np.abs(c - c64) <= 1e-5 * np.abs(c64))
    _check(gk, _pack(g64, tl, ul), T + U, "packed vs fp64")

    # at the C ABI: every element of a NaN-prefilled gradient is written
    L = _L()
    roff, loff, N = _offsets(tl, ul)
    roff_d, loff_d = _d(roff, dev), _d(loff, dev)
    ws = torch.empty(L.pika_rnnt_workspace_bytes(B, T, U + 1), dtype=torch.uint8, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    x = _d(lpk, dev)
    yk_d = _d(yk, dev)
    _ok(L.pika_rnnt_packed_forward(_p(x), _p(yk_d), _p(args[1]), _p(args[2]), _p(roff_d), _p(loff_d), B, T, U + 1, N, V, 0,
                                   _p(costs), _p(ws), _s()), "packed_forward")
    g = torch.full((N, V), float("nan"), dtype=torch.float32, device=dev)
    _ok(L.pika_rnnt_packed_backward(_p(yk_d), _p(args[1]), _p(args[2]), _p(roff_d), _p(loff_d), B, T, U + 1, N, V, 0, None,
                                    _p(ws), _p(g), 0.0, _s()), "packed_backward")
    torch.cuda.synchronize()
    assert not torch.isnan(g).any()
    assert torch.equal(costs, cp.detach()) and np.array_equal(g.cpu().numpy(), gk)


# ---------------------------------------------------------------------------------------------------------------------
# 4. packed from logits: costs and d(logits) rows equal the padded fused route's live rows (f32 and bf16)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [40, 5000, 6268])
def test_packed_from_logits_equals_padded(hip_device, V):
    from pika_amd.rnnt import rnnt_loss_from_logits
    dev = hip_device
    B, T, U = 4, 14, 9
    _, y, tl, ul = make_case(B, T, U, 4, seed=V, ragged=True)
    rng = np.random.default_rng(V + 1)
    y = _labels(B, U, V, 0, ul, rng)
    x = (rng.standard_normal((B, T, U + 1, V)) * 2).astype(np.float32)
    args = [_d(a, dev) for a in (y, tl, ul)]
    xp = _d(x, dev).requires_grad_(True)
    cp = rnnt_loss_from_logits(xp, *args)
    cp.sum().backward()
    xk_np, yk = _pack(x, tl, ul), _pack_labels(y, ul)
    xk = _d(xk_np, dev).requires_grad_(True)
    ck = rnnt_loss_from_logits(xk, _d(yk, dev), args[1], args[2], compact=True)
    ck.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(ck.detach(), cp.detach())
    assert np.array_equal(xk.grad.cpu().numpy(), _pack(xp.grad.cpu().numpy(), tl, ul))
    # bf16 d(logits) at the C ABI, padded and packed
    L = _L()
    U1, R = U + 1, B * T * (U + 1)
    roff, loff, N = _offsets(tl, ul)
    roff_d, loff_d, yk_d = _d(roff, dev), _d(loff, dev), _d(yk, dev)
    outs = []
    for packed in (False, True):
        xin = _d(xk_np if packed else x, dev)
        rows = N if packed else R
        ws = torch.empty(L.pika_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
        c = torch.empty(B, dtype=torch.float32, device=dev)
        lse = torch.empty(rows, dtype=torch.float32, device=dev)
        out = torch.full((rows, V), float("nan"), dtype=torch.bfloat16, device=dev)
        if packed:
            _ok(L.pika_rnnt_packed_fused_forward(_p(xin), _p(yk_d), _p(args[1]), _p(args[2]), _p(roff_d), _p(loff_d), B, T,
                                                 U1, N, V, 0, _p(c), _p(lse), _p(ws), _s()), "packed_fused_forward")
            _ok(L.pika_rnnt_packed_fused_backward(_p(xin), _p(lse), _p(yk_d), _p(args[1]), _p(args[2]), _p(roff_d),
                                                  _p(loff_d), B, T, U1, N, V, 0, None, _p(ws), _p(out), 1, V, 0.0, _s()),
                "packed_fused_backward")
        else:
            _ok(L.pika_rnnt_fused_forward(_p(xin), _p(args[0]), _p(args[1]), _p(args[2]), B, T, U1, V, 0, _p(c), _p(lse),
                                          _p(ws), _s()), "fused_forward")
            _ok(L.pika_rnnt_fused_backward(_p(xin), _p(lse), _p(args[0]), _p(args[1]), _p(args[2]), B, T, U1, V, 0, None,
                                           _p(ws), _p(out), 1, V, _s()), "fused_backward")
        torch.cuda.synchronize()
        outs.append((c.cpu(), out.float().cpu().numpy()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert not np.isnan(outs[1][1]).any()
    assert np.array_equal(outs[1][1], _pack(outs[0][1].reshape(B, T, U1, V), tl, ul))


# ---------------------------------------------------------------------------------------------------------------------
# 5. packed + FastEmit, through autograd with reduction="mean"
# ---------------------------------------------------------------------------------------------------------------------
def test_packed_with_fastemit_mean_reduction(hip_device):
    from pika_amd.rnnt import rnnt_loss, rnnt_loss_from_logits
    dev = hip_device
    B, T, U, V, lam = 4, 16, 10, 48, 0.25
    lp, y, tl, ul = make_case(B, T, U, V, seed=31, ragged=True)
    args = [_d(a, dev) for a in (y, tl, ul)]
    lpk, yk = _pack(lp, tl, ul), _pack_labels(y, ul)
    xk = _d(lpk, dev).requires_grad_(True)
    rnnt_loss(xk, _d(yk, dev), args[1], args[2], reduction="mean", fastemit_lambda=lam, compact=True).backward()
    xs = _d(lp, dev).requires_grad_(True)
    rnnt_loss(xs, *args, reduction="sum", fastemit_lambda=lam).backward()
    xm = _d(lp, dev).requires_grad_(True)
    rnnt_loss(xm, *args, reduction="mean", fastemit_lambda=lam).backward()
    torch.cuda.synchronize()
    gk = xk.grad.cpu().numpy()
    assert np.array_equal(gk, _pack(xm.grad.cpu().numpy(), tl, ul))          # bit-equal to the padded mean
    np.testing.assert_allclose(gk, _pack(xs.grad.cpu().numpy(), tl, ul) / B, rtol=1e-6, atol=1e-38)
    c64, g64 = O.rnnt_loss(lp, y, tl, ul)
    _check(gk, _pack(_fe(g64, y, tl, ul, lam), tl, ul) / B, T + U, "packed fastemit mean")
    # from logits (packed, FastEmit) against the softmax backward of the same gradient
    x = (np.random.default_rng(3).standard_normal((B, T, U + 1, V))).astype(np.float32)
    xk = _d(_pack(x, tl, ul), dev).requires_grad_(True)
    rnnt_loss_from_logits(xk, _d(yk, dev), args[1], args[2], fastemit_lambda=lam, compact=True).sum().backward()
    torch.cuda.synchronize()
    _, g64 = O.rnnt_loss(log_softmax(x.astype(np.float64)).astype(np.float32), y, tl, ul)
    g = _pack(_fe(g64, y, tl, ul, lam), tl, ul)
    x64 = _pack(x, tl, ul).astype(np.float64)
    p = np.exp(x64 - _lse(x64))
    ref = g - p * g.sum(1, keepdims=True)
    rel, abs_ = _tol(T + U)
    bound = rel * (np.abs(g) + p * np.abs(g).sum(1, keepdims=True)) + abs_ * ((g != 0) + 2.0 * p)
    assert np.all(np.abs(xk.grad.cpu().numpy() - ref) <= bound)


# ---------------------------------------------------------------------------------------------------------------------
# 6. validation
# ---------------------------------------------------------------------------------------------------------------------
def test_packed_validation(hip_device):
    from pika_amd.rnnt import rnnt_loss, rnnt_loss_from_logits
    dev = hip_device
    V = 8
    tl = torch.tensor([3, 2], dtype=torch.int32, device=dev)
    ul = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    N = 3 * 3 + 2 * 1
    lp = torch.log_softmax(torch.randn(N, V, device=dev), -1)
    y = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    assert torch.isfinite(rnnt_loss(lp, y, tl, ul, compact=True)).all()
    bad = [
        ("rows", dict(log_probs=lp[:-1])),
        ("labels has", dict(labels=y[:1])),
        ("frames_lengths", dict(frames_lengths=torch.tensor([3, 0], dtype=torch.int32, device=dev))),
        ("1024", dict(labels_lengths=torch.tensor([1024, 0], dtype=torch.int32, device=dev))),
        ("fastemit_lambda", dict(fastemit_lambda=-0.5)),
        ("fastemit_lambda", dict(fastemit_lambda=float("nan"))),
    ]
    for match, kw in bad:
        a = dict(log_probs=lp, labels=y, frames_lengths=tl, labels_lengths=ul, compact=True)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            rnnt_loss(**a)
    with pytest.raises(ValueError, match="rows"):
        rnnt_loss_from_logits(torch.randn(N + 1, V, device=dev), y, tl, ul, compact=True)
    torch.cuda.synchronize()
    # under stream capture: a clear error, nothing captured
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with pytest.raises(RuntimeError, match="stream capture"):
            with torch.cuda.graph(g, stream=s):
                rnnt_loss(lp, y, tl, ul, compact=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the graphed train step carries lambda (the loss' eager backward writes the metadata the replay reads)
# ---------------------------------------------------------------------------------------------------------------------
def _step_grads(model, loss_fn, batch):
    model.zero_grad(set_to_none=True)
    out = model(batch[0], batch[1].long(), batch[2], True)
    loss_fn(out, batch[1].int(), batch[2], batch[3]).sum().backward()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("V", [500, 512], ids=["dense", "lazy"])
def test_graphed_train_step_carries_fastemit(hip_device, V):
    from pika_amd import gemm as G
    from pika_amd.rnnt import RNNTLoss
    from pika_amd.train_graph import GraphedTrainStep
    from test_train_step_gpu import _small_step_harness
    model, _, batches, fused_optim = _small_step_harness(hip_device, 0.0, V=V)
    loss_fe = RNNTLoss(blank=0, fastemit_lambda=0.5).apply
    ref = copy.deepcopy(model)
    old = G.PRECISION
    G.PRECISION = "mixed"
    fused_optim.install()
    try:
        # eager gradients of the first batch: lambda = 0.5 against lambda = 0
        g_fe = _step_grads(ref, loss_fe, batches[0])
        g_0 = _step_grads(ref, RNNTLoss(blank=0).apply, batches[0])
        num = sum(float((g_fe[n] - g_0[n]).double().norm() ** 2) for n in g_fe) ** 0.5
        den = sum(float(g_0[n].double().norm() ** 2) for n in g_0) ** 0.5
        assert num > 0.01 * den, (num, den)       # (the untrained encoder's gradient dominates the norm)
        # replays (lr 0: the parameters stay put) give the eager lambda = 0.5 gradients of the same batch
        gs = GraphedTrainStep(model, loss_fe, lambda: torch.optim.SGD(model.parameters(), 0.0, momentum=0.9, nesterov=True),
                              clip=0.0, warmup=2)
        for b in batches[1:3]:
            gs(*b)
        for _ in range(2):
            gs(*batches[0])
            got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        assert len(gs.graphs) == 1
        gs.close()
    finally:
        fused_optim.uninstall()
        G.PRECISION = old
    assert set(got) == set(g_fe)
    worst = []
    for n in g_fe:
        a, b = got[n].double(), g_fe[n].double()
        nb = b.norm().item()
        if nb < 1e-3 * den:
            continue
        worst.append(((a - b).norm().item() / nb, (a - g_0[n].double()).norm().item() / nb, n))
    worst.sort(reverse=True)
    print("largest relative gradient differences (replay vs eager FastEmit, replay vs eager plain):", worst[:5])
    assert worst[0][0] < 0.1, worst[:5]
    # the replay is the FastEmit gradient, not the plain one: far nearer the first in the parameters FastEmit moves most
    assert max(w[1] for w in worst) > 5 * worst[0][0], worst
    assert all(w[0] < w[1] for w in worst if w[1] > 0.1), worst
