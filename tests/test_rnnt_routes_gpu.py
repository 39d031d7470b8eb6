"""Every shape-selected instantiation of the RNN-T loss (pika_amd/csrc/rnnt_loss.hip) against the fp64 oracle.

The host code picks template instantiations by shape: the alpha/beta workgroup width NW = lattice_width(U1) / 64, the
register depth CQ of the row-per-wave kernels (by V or ld_out), the 8-column d(logits) kernel and its NIT (by V,
ld_out, ld_in), and the gathered / partials variants of the log-sum-exp gather.  ROUTES below names, per row, the
instantiations a row's calls reach and the arguments that select them; tests/test_rnnt_route_table.py restates the
host's selection rules and checks the table against them and against the set of instantiations in the source.

Calls go straight to the C ABI (pika_amd._lib) with workspaces from pika_rnnt_workspace_bytes.  Tolerances:
  costs      1e-5 relative: the fp64-offset lattice of the kernels (as in test_rnnt_loss_gpu.py);
  gradients  (of the loss w.r.t. log-probs, and the two row non-zeros inside d(logits)) 1e-4 relative + 1e-5 absolute
             up to ~320 diagonals, 1e-3 + 2e-5 beyond (test_full_size_lattice_properties_and_sampled_parity);
  d(logits)  derived from that: scale * (g - p * sum g) is off by at most
             |scale| * (rel * (|g| + p * sum |g|) + abs * ([g != 0] + 2 p)), then bf16 rounds to nearest: 2^-8 of the value.
"""
import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import log_softmax

pytestmark = pytest.mark.gpu

PIKA_EINVAL, PIKA_ETOOBIG = -1, -2


def AB(nw):
    return "rnnt_alpha_beta_kernel<%d>" % nw


def LG(cq):
    return "rnnt_lse_gather_kernel<%d>" % cq


MG, MGG = "rnnt_lse_merge_gather_kernel<false>", "rnnt_lse_merge_gather_kernel<true>"


def CK(colsum, ti, cq):
    return "rnnt_dlogits_compact_kernel<%s, %s, %d>" % ("true" if colsum else "false", ti, cq)


def C8(nit, ti):
    return "rnnt_dlogits_compact8_kernel<%d, %s>" % (nit, ti)


def FK(to, cq):
    return "rnnt_dlogits_fused_kernel<%s, %d>" % (to, cq)


F32, F16, BF16 = "float", "_Float16", "__bf16"

# ---------------------------------------------------------------------------------------------------------------------
# Route table.  kind "lattice": RNNTLoss on log-probs, pika_rnnt_fused_forward + _backward (f32 out, ld_out = V) and
# pika_rnnt_fused_forward_partials on one ragged batch of width U1 (utterances: one filling the width, Tn = 1 / Un = 0,
# Un = 64k - 1 and 64k on a wave boundary, one with Tn - 1 < Un).  kind "gathered": pika_gemm_bf16_nt_lse_f16 ->
# pika_rnnt_fused_forward_gathered.  kind "dlogits": one lattice, d(logits) through each route of `routes`:
#   ("lp", colsum, ld_out)              pika_rnnt_dlogits_compact_bf16 on log-probs (forward: pika_rnnt_loss_forward)
#   ("raw", colsum, ld_out)             the same on raw fp32 logits + lse of pika_rnnt_fused_forward (scale 1)
#   ("f16", colsum, ld_out, ld_in, g)   pika_rnnt_dlogits_compact_bf16_f16in after the gathered forward, `gathered` or NULL
#   ("fused", out_dtype, ld_out)        pika_rnnt_fused_forward + pika_rnnt_fused_backward
# "kernels" lists every shape-selected instantiation the row launches, nothing else.
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = [
    # alpha/beta widths: NW = 1, 2, 3, 6 once, NW = 4, 8, 12, 16 at both edges of their U1 range
    dict(kind="lattice", U1=64, T=48, V=40, kernels=(AB(1), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=128, T=48, V=40, kernels=(AB(2), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=129, T=48, V=40, kernels=(AB(3), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=384, T=24, V=16, kernels=(AB(6), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=193, T=48, V=40, kernels=(AB(4), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=256, T=300, V=8, kernels=(AB(4), LG(20), MG, FK(F32, 20))),   # Tn - 1 >= Un at full width
    dict(kind="lattice", U1=385, T=32, V=40, kernels=(AB(8), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=512, T=32, V=16, kernels=(AB(8), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=513, T=24, V=16, kernels=(AB(12), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=768, T=24, V=16, kernels=(AB(12), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=769, T=24, V=16, kernels=(AB(16), LG(20), MG, FK(F32, 20))),
    dict(kind="lattice", U1=1024, T=24, V=16, kernels=(AB(16), LG(20), MG, FK(F32, 20))),
    # the gathered forward: (b, t, u) carried across 16-row blocks of the product's epilogue
    dict(kind="gathered", U1=1, T=1, V=264, blank=0, ld16=264, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=1, T=20, V=264, blank=263, ld16=264, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=2, T=3, V=264, blank=0, ld16=272, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=15, T=3, V=300, blank=299, ld16=300, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=16, T=1, V=264, blank=0, ld16=264, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=16, T=20, V=264, blank=263, ld16=264, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=17, T=3, V=264, blank=0, ld16=264, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=17, T=20, V=300, blank=299, ld16=304, kernels=(AB(1), MGG)),
    dict(kind="gathered", U1=65, T=3, V=264, blank=263, ld16=264, kernels=(AB(2), MGG)),
    dict(kind="gathered", U1=65, T=20, V=264, blank=0, ld16=264, kernels=(AB(2), MGG)),
    dict(kind="gathered", U1=1024, T=1, V=264, blank=0, ld16=264, kernels=(AB(16), MGG)),
    dict(kind="gathered", U1=1024, T=3, V=264, blank=263, ld16=264, kernels=(AB(16), MGG)),
    # d(logits): both sides of CQ (ld_out 5120), of the 8-column kernel (V > 4608, V % 8, pitches) and of NIT
    # (ld_out 5120 / 6656); blank 0 and V - 1, ld_out > V, ld_in > V, scale != 1
    dict(kind="dlogits", V=4608, blank=0, scale=0.75, B=4, T=6, U=5,
         routes=[("lp", False, 4608), ("lp", True, 4608), ("f16", True, 4608, 4608, True), ("f16", False, 4608, 4608, True),
                 ("fused", 0, 4608)],
         kernels=(AB(1), LG(20), MGG, CK(0, F32, 20), CK(1, F32, 20), CK(1, F16, 20), CK(0, F16, 20), FK(F32, 20))),
    dict(kind="dlogits", V=4616, blank=4615, scale=1.5, B=4, T=6, U=5,
         routes=[("lp", True, 4616), ("f16", True, 4616, 4616, True), ("fused", 1, 4616)],
         kernels=(AB(1), LG(20), MGG, C8(10, F32), C8(10, F16), FK(BF16, 20))),
    dict(kind="dlogits", V=5000, blank=0, scale=1.0, B=4, T=6, U=5,
         routes=[("lp", True, 5008), ("f16", True, 5008, 5000, False), ("raw", True, 5000)],
         kernels=(AB(1), LG(20), MGG, C8(10, F32), C8(10, F16))),
    dict(kind="dlogits", V=5120, blank=0, scale=0.75, B=4, T=6, U=5,
         routes=[("lp", True, 5128), ("lp", False, 5120), ("lp", False, 5124), ("f16", True, 5120, 5120, True),
                 ("fused", 0, 5124)],
         kernels=(AB(1), LG(20), MGG, C8(13, F32), CK(0, F32, 20), CK(0, F32, 32), C8(10, F16), FK(F32, 32))),
    dict(kind="dlogits", V=5124, blank=5123, scale=0.75, B=4, T=6, U=5,
         routes=[("lp", True, 5124), ("f16", True, 5128, 5128, True), ("f16", True, 5124, 5124, True), ("fused", 1, 5124)],
         kernels=(AB(1), LG(32), MGG, CK(1, F32, 32), C8(13, F16), CK(1, F16, 32), FK(BF16, 32))),
    dict(kind="dlogits", V=6268, blank=0, scale=1.0, B=4, T=6, U=5,
         routes=[("f16", True, 6272, 6272, True), ("lp", False, 6268), ("f16", False, 6268, 6268, True), ("raw", True, 6268)],
         kernels=(AB(1), LG(32), MGG, C8(13, F16), CK(0, F32, 32), CK(0, F16, 32), CK(1, F32, 32))),
    dict(kind="dlogits", V=6656, blank=6655, scale=0.75, B=4, T=6, U=5,
         routes=[("lp", True, 6656), ("f16", True, 6656, 6656, True), ("fused", 0, 6656)],
         kernels=(AB(1), LG(32), MGG, C8(13, F32), C8(13, F16), FK(F32, 32))),
    dict(kind="dlogits", V=6664, blank=0, scale=1.5, B=4, T=6, U=5,
         routes=[("lp", True, 6664), ("f16", True, 6664, 6664, True), ("fused", 1, 6664)],
         kernels=(AB(1), LG(32), MGG, C8(16, F32), C8(16, F16), FK(BF16, 32))),
    dict(kind="dlogits", V=8192, blank=8191, scale=1.0, B=4, T=6, U=5,
         routes=[("lp", True, 8192), ("f16", True, 8192, 8192, True), ("raw", True, 8192), ("fused", 0, 8192),
                 ("fused", 1, 8192)],
         kernels=(AB(1), LG(32), MGG, C8(16, F32), C8(16, F16), FK(F32, 32), FK(BF16, 32))),
    # a multi-wave lattice (U1 = 70: NW = 2) under the d(logits) kernels
    dict(kind="dlogits", V=5000, blank=0, scale=0.75, B=2, T=4, U=69,
         routes=[("lp", True, 5000), ("f16", True, 5000, 5000, True), ("fused", 1, 5000)],
         kernels=(AB(2), LG(20), MGG, C8(10, F32), C8(10, F16), FK(BF16, 20))),
    # column sums with 5 rows per wave (10302 rows) and a last, partly filled block (10302 % 20 = 2): both kernels, both
    # input types (ld_out / ld_in 4620 push V = 4616 off the 8-column kernel)
    dict(kind="dlogits", V=4616, blank=0, scale=0.75, B=2, T=101, U=50,
         routes=[("lp", True, 4616), ("lp", True, 4620), ("f16", True, 4616, 4616, True), ("f16", True, 4616, 4620, True)],
         kernels=(AB(1), MGG, C8(10, F32), CK(1, F32, 20), C8(10, F16), CK(1, F16, 20))),
]


def _rows(kind):
    rows = [r for r in ROUTES if r["kind"] == kind]
    return pytest.mark.parametrize("row", rows, ids=["%s-%d" % (kind, i) for i in range(len(rows))])


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _L():
    from pika_amd import _lib
    return _lib.lib()


def _ok(rc, what):
    from pika_amd import _lib
    _lib.check(rc, what)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _ws(B, T, U1, dev):
    n = _L().pika_rnnt_workspace_bytes(B, T, U1)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=dev)


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _tol(D):
    """(rel, abs) of a gradient entry after D diagonals (module docstring)."""
    return (1e-4, 1e-5) if D <= 320 else (1e-3, 2e-5)


def _lengths(B, T, U1, rng):
    """Ragged (Tn, Un): one utterance filling the width, Tn = 1 / Un = 0, Un = 64k - 1 and 64k, one with Tn - 1 < Un."""
    U = U1 - 1
    k = max(1, U // 64)
    tl = [T, 1, T, max(1, T - 1), max(1, T // 2)]
    ul = [U, 0, min(U, 64 * k - 1), min(U, 64 * k), U // 3 + (1 if U else 0)]
    ul[4] = min(U, max(ul[4], tl[4]))        # Tn - 1 < Un where the width allows it
    tl, ul = np.array(tl[:B], np.int32), np.array(ul[:B], np.int32)
    perm = rng.permutation(B)
    return tl[perm], ul[perm]


def _labels(B, U, V, blank, ul, rng):
    y = rng.integers(0, V - 1, (B, U)).astype(np.int32)
    y[y >= blank] += 1                        # never the blank
    for n in range(B):
        y[n, ul[n]:] = V                      # padding (never read)
    return y


def _live(tl, ul, T, U1):
    t = np.arange(T)[None, :, None]
    u = np.arange(U1)[None, None, :]
    return (t < tl[:, None, None]) & (u <= ul[:, None, None])


def _check_costs(c, c64, what, worst):
    rel = np.abs(c.astype(np.float64) - c64) / np.maximum(np.abs(c64), 1e-30)
    worst[what + " cost rel"] = max(worst.get(what + " cost rel", 0.0), float(rel.max()))
    assert np.all(rel <= 1e-5), (what, c, c64)


def _check_grads(g, g64, rel, abs_, what, worst):
    err = np.abs(g.astype(np.float64) - g64)
    bound = rel * np.abs(g64) + abs_
    worst[what + " grad err/bound"] = max(worst.get(what + " grad err/bound", 0.0), float((err / bound).max()))
    assert np.all(err <= bound), (what, float((err - bound).max()))


def _check_lattice(a, b, a64, b64, what):
    """The assertions of test_matches_fp64_oracle on exported alpha / beta; cells outside a sub-lattice hold -1e30."""
    valid = np.isfinite(a64)
    assert np.abs(a[valid] - a64[valid]).max() < 1e-3 * max(1.0, np.abs(a64[valid]).max() * 1e-2), what
    assert np.abs(b[valid] - b64[valid]).max() < 1e-3 * max(1.0, np.abs(b64[valid]).max() * 1e-2), what
    assert np.all(a[~valid] <= -1e29) and np.all(b[~valid] <= -1e29), what


def _check_structure(g, tl, ul, what):
    nz = g != 0
    assert nz.sum() <= int((tl.astype(np.int64) * (ul + 1) * 2).sum()), what
    for n in range(g.shape[0]):
        assert not nz[n, tl[n]:].any() and not nz[n, :, ul[n] + 1:].any(), what


def _report(name, worst):
    print("\n[%s] worst: %s" % (name, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def _export(ws, tl_d, ul_d, B, T, U1, dev):
    a = torch.empty((B, T, U1), dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    _ok(_L().pika_rnnt_export_lattice(_p(ws), _p(tl_d), _p(ul_d), B, T, U1, _p(a), _p(b), _s()), "export")
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy()


def _host_partials(x, V):
    """Per-row (max, sum exp) over blocks of two columns plus three empty blocks (-inf, 0): n_part = V/2 + 3 > 16
    for V = 40, so the 16 lanes of a row merge more than one pair each."""
    R = x.shape[0]
    xb = x.reshape(R, V // 2, 2).astype(np.float64)
    pm = xb.max(-1)
    ps = np.exp(xb - pm[..., None]).sum(-1)
    pm = np.concatenate([pm, np.full((R, 3), -np.inf)], 1).astype(np.float32)
    ps = np.concatenate([ps, np.zeros((R, 3))], 1).astype(np.float32)
    return pm, ps


def _dlogits_bound(g, p, scale, rel, abs_, bf16):
    """scale * (g - p * sum g) from fp64 g, p (R, V); the bound e1 of the kernel's fp32 value (module docstring) and the
    bound of the stored value (e1, plus the bf16 rounding of a value within e1 of the reference)."""
    A = np.abs(g).sum(1, keepdims=True)
    e1 = abs(scale) * (rel * (np.abs(g) + p * A) + abs_ * ((g != 0) + 2.0 * p))
    ref = scale * (g - p * g.sum(1, keepdims=True))
    e = e1 + 2.0 ** -8 * (np.abs(ref) + e1) if bf16 else e1
    return ref, e1, e


def _check_dlogits(out, ld_out, V, g, p, scale, rel, abs_, bf16, live_rows, what, worst, colsum=None):
    """out (R, ld_out) as float; g the fp64 gradient w.r.t. log-probs (R, V), p the softmax the route reads.
    colsum: sum_r of the fp32 values before rounding, so within sum_r e1 of the reference's column sum, plus the fp32
    additions in any order: (R - 1) 2^-24 of sum_r |value|."""
    R = g.shape[0]
    assert np.all(out[:, V:] == 0), what + ": columns [V, ld_out) not zero"
    assert np.all(out[~live_rows] == 0), what + ": a row outside its lattice is not zero"
    cs_ref = np.zeros(V)
    cs_bound = np.zeros(V)
    w = 0.0
    for r0 in range(0, R, 2048):
        sl = slice(r0, min(R, r0 + 2048))
        ref, e1, e = _dlogits_bound(g[sl], p[sl], scale, rel, abs_, bf16)
        err = np.abs(out[sl, :V].astype(np.float64) - ref)
        w = max(w, float((err / np.maximum(e, 1e-300)).max()))
        if not np.all(err <= e):
            bad = np.argsort((err - e).ravel())[-5:]
            for i in bad:
                r, c = np.unravel_index(i, err.shape)
                print("%s: row %d col %d: out %.6g ref %.6g bound %.3g p %.4g row g non-zeros %s" % (
                    what, r0 + r, c, out[r0 + r, c], ref[r, c], e[r, c], p[r0 + r, c],
                    [(int(j), float(g[r0 + r, j])) for j in np.nonzero(g[r0 + r])[0]]))
        assert np.all(err <= e), "%s: excess %g at %s" % (what, float((err - e).max()),
                                                       np.unravel_index(np.argmax(err - e), err.shape))
        cs_ref += ref.sum(0)
        cs_bound += e1.sum(0) + (R - 1) * 2.0 ** -24 * (np.abs(ref) + e1).sum(0)
    worst[what + " err/bound"] = max(worst.get(what + " err/bound", 0.0), w)
    if colsum is not None:
        cerr = np.abs(colsum.astype(np.float64) - cs_ref)
        worst[what + " colsum err/bound"] = max(worst.get(what + " colsum err/bound", 0.0),
                                                float((cerr / cs_bound).max()))
        assert np.all(cerr <= cs_bound), "%s: colsum excess %g at column %d" % (what, float((cerr - cs_bound).max()),
                                                                               int(np.argmax(cerr - cs_bound)))


# ---------------------------------------------------------------------------------------------------------------------
# 1a. lattice widths: RNNTLoss (log-probs), fused forward + backward, forward from partials
# ---------------------------------------------------------------------------------------------------------------------
@_rows("lattice")
def test_lattice_width_routes(hip_device, row):
    """Costs 1e-5 rel; dense gradient and the non-zeros inside d(logits) at the gradient bound of D = T + U1 - 1
    diagonals; exported alpha / beta as in test_matches_fp64_oracle; exact zeros outside every sub-lattice."""
    from pika_amd.rnnt import RNNTLoss
    dev = hip_device
    U1, T, V = row["U1"], row["T"], row["V"]
    B = 5
    rng = np.random.default_rng(U1 * 1000 + T)
    tl, ul = _lengths(B, T, U1, rng)
    y = _labels(B, U1 - 1, V, 0, ul, rng)
    x = (rng.standard_normal((B, T, U1, V)) * 2).astype(np.float32)
    lp = log_softmax(x.astype(np.float64)).astype(np.float32)
    w = (rng.random(B) + 0.5).astype(np.float32)
    c64, g64, a64, b64 = O.rnnt_loss(lp, y, tl, ul, want_lattice=True)
    g64 = g64 * w[:, None, None, None]
    rel, abs_ = _tol(T + U1 - 1)
    worst = {}
    y_d, tl_d, ul_d, w_d = (_d(a, dev) for a in (y, tl, ul, w))
    L = _L()

    # RNNTLoss on log-probs
    xl = _d(lp, dev).requires_grad_(True)
    costs = RNNTLoss(blank=0, reduction="sum").apply(xl, y_d, tl_d, ul_d)
    a, b = _export(costs.grad_fn.saved_tensors[3], tl_d, ul_d, B, T, U1, dev)
    costs.backward(w_d)
    torch.cuda.synchronize()
    g = xl.grad.cpu().numpy()
    _check_costs(costs.detach().cpu().numpy(), c64, "log-probs", worst)
    _check_lattice(a, b, a64, b64, "log-probs")
    _check_grads(g, g64, rel, abs_, "log-probs", worst)
    _check_structure(g, tl, ul, "log-probs")

    # fused forward + backward on raw logits (f32 out, ld_out = V)
    R = B * T * U1
    x_d = _d(x, dev)
    ws = _ws(B, T, U1, dev)
    c_d = torch.empty(B, dtype=torch.float32, device=dev)
    lse_d = torch.empty(R, dtype=torch.float32, device=dev)
    _ok(L.pika_rnnt_fused_forward(_p(x_d), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, 0, _p(c_d), _p(lse_d), _p(ws), _s()),
        "fused_forward")
    a, b = _export(ws, tl_d, ul_d, B, T, U1, dev)
    out = _nan((R, V), torch.float32, dev)
    _ok(L.pika_rnnt_fused_backward(_p(x_d), _p(lse_d), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, 0, _p(w_d), _p(ws),
                                   _p(out), 0, V, _s()), "fused_backward")
    torch.cuda.synchronize()
    _check_costs(c_d.cpu().numpy(), c64, "fused", worst)
    _check_lattice(a, b, a64, b64, "fused")
    x64 = x.reshape(R, V).astype(np.float64)
    p = np.exp(x64 - _lse(x64))
    live = _live(tl, ul, T, U1).reshape(R)
    _check_dlogits(out.cpu().numpy(), V, V, g64.reshape(R, V), p, 1.0, rel, abs_, False, live, "fused d(logits)", worst)

    # forward from partial (max, sum exp) statistics, then the dense gradient from its lattice
    pm, ps = _host_partials(x.reshape(R, V), V)
    pm_d, ps_d = _d(pm, dev), _d(ps, dev)
    ws = _ws(B, T, U1, dev)
    _ok(L.pika_rnnt_fused_forward_partials(_p(x_d), _p(pm_d), _p(ps_d), pm.shape[1], _p(y_d), _p(tl_d), _p(ul_d), B, T,
                                           U1, V, 0, _p(c_d), _p(lse_d), _p(ws), _s()), "fused_forward_partials")
    a, b = _export(ws, tl_d, ul_d, B, T, U1, dev)
    gd = _nan((B, T, U1, V), torch.float32, dev)
    _ok(L.pika_rnnt_loss_backward(_p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, 0, _p(w_d), _p(ws), _p(gd), _s()),
        "loss_backward")
    torch.cuda.synchronize()
    g = gd.cpu().numpy()
    _check_costs(c_d.cpu().numpy(), c64, "partials", worst)
    _check_lattice(a, b, a64, b64, "partials")
    _check_grads(g, g64, rel, abs_, "partials", worst)
    _check_structure(g, tl, ul, "partials")
    _report("lattice U1=%d T=%d V=%d" % (U1, T, V), worst)


# ---------------------------------------------------------------------------------------------------------------------
# 1b / 1c shared: a joint-like product A W^T + bias from bf16 operands, exact in fp64
# ---------------------------------------------------------------------------------------------------------------------
K_JOINT = 64


def _lse(x):
    m = x.max(1, keepdims=True)
    return m + np.log(np.exp(x - m).sum(1, keepdims=True))


def _joint_case(B, T, U1, V, blank, seed, tl, ul, boost=(), want_mag=False):
    """bf16 A (B*T*U1, K), bf16 W (V, K), f32 bias -> exact logits X (fp64).  Rows outside every sub-lattice get
    logits of |x| ~ 100 (exp overflows fp32 there: such rows must never reach an exp).  Columns in `boost` get 20 more
    bias: logits where the fp16 copy is 2^-7 off, while the log-probs of the lattice stay O(1)."""
    rng = np.random.default_rng(seed)
    R = B * T * U1
    A = torch.from_numpy(rng.standard_normal((R, K_JOINT)).astype(np.float32)).bfloat16()
    live = _live(tl, ul, T, U1).reshape(R)
    A[torch.from_numpy(~live)] = 30.0
    Wt = torch.from_numpy((rng.standard_normal((V, K_JOINT)) * 0.15).astype(np.float32)).bfloat16()
    bias = (rng.standard_normal(V)).astype(np.float32)
    bias[list(boost)] += 20.0
    A64, W64 = A.float().numpy().astype(np.float64), Wt.float().numpy().astype(np.float64)
    X = A64 @ W64.T + bias.astype(np.float64)
    # sum_k |a_k w_k| + |bias|: scale of the fp32 accumulation error of every logit
    mag = np.abs(A64) @ np.abs(W64).T + np.abs(bias.astype(np.float64)) if want_mag else None
    return A, Wt, bias, X, mag, live


def _gemm_f16(dev, A_d, W_d, bias_d, R, V, ld16, y_d, T, U1, blank, gathered=True):
    n_part = ((V + 255) // 256) * 4
    out16 = _nan((R, ld16), torch.float16, dev)
    pm = torch.empty((R, n_part), dtype=torch.float32, device=dev)
    ps = torch.empty_like(pm)
    gat = _nan((R, 2), torch.float32, dev) if gathered else None
    _ok(_L().pika_gemm_bf16_nt_lse_f16(_p(A_d), K_JOINT, _p(W_d), K_JOINT, _p(out16), ld16, R, V, K_JOINT, _p(bias_d),
                                       _p(pm), _p(ps), n_part, _p(y_d) if U1 > 1 else None, T, U1, blank, _p(gat), _s()),
        "gemm_bf16_nt_lse_f16")
    return out16, pm, ps, gat, n_part


# ---------------------------------------------------------------------------------------------------------------------
# 1b. the gathered forward and the lattice-position carry of the product's epilogue
# ---------------------------------------------------------------------------------------------------------------------
@_rows("gathered")
def test_gathered_forward_and_epilogue_carry(hip_device, row):
    """gathered[m] = (X[m, blank], X[m, label]) within the fp32 accumulation bound (K + 2) 2^-24 (sum_k |a_k w_k| +
    |bias|) (every row's blank, padding rows included; the label where u < U1 - 1 and the label is below V); lse within
    that plus 16 ulp of max(1, |lse|) (exp / log / sum of n_part partials / the final add); costs 1e-5 rel of the
    oracle on the fp64 log-softmax.  The same product with gathered = NULL writes the same fp16 logits and partials."""
    dev = hip_device
    U1, T, V, blank, ld16 = row["U1"], row["T"], row["V"], row["blank"], row["ld16"]
    B = 3
    rng = np.random.default_rng(U1 * 31 + T * 7 + blank)
    tl = np.array([T, max(1, T - 2), 1], np.int32)
    ul = np.array([U1 - 1, max(0, U1 // 2 - 1), 0], np.int32)
    y = _labels(B, U1 - 1, V, blank, ul, rng)
    R = B * T * U1
    A, Wt, bias, X, mag, live = _joint_case(B, T, U1, V, blank, 1000 + U1 + T, tl, ul, want_mag=True)
    A_d, W_d, bias_d = A.to(dev), Wt.to(dev), _d(bias, dev)
    y_d, tl_d, ul_d = (_d(a, dev) for a in (y, tl, ul))
    out16, pm, ps, gat, n_part = _gemm_f16(dev, A_d, W_d, bias_d, R, V, ld16, y_d, T, U1, blank)
    ws = _ws(B, T, U1, dev)
    c_d = torch.empty(B, dtype=torch.float32, device=dev)
    lse_d = _nan((R,), torch.float32, dev)
    _ok(_L().pika_rnnt_fused_forward_gathered(_p(out16), ld16, _p(gat), _p(y_d) if U1 > 1 else None, blank, _p(pm), _p(ps),
                                              n_part, _p(y_d) if U1 > 1 else None, _p(tl_d), _p(ul_d), B, T, U1, V, blank,
                                              _p(c_d), _p(lse_d), _p(ws), _s()), "fused_forward_gathered")
    out16n, pmn, psn, _, _ = _gemm_f16(dev, A_d, W_d, bias_d, R, V, ld16, y_d, T, U1, blank, gathered=False)
    torch.cuda.synchronize()
    worst = {}
    acc = (K_JOINT + 2) * 2.0 ** -24 * mag                       # (R, V)
    G = gat.cpu().numpy().astype(np.float64)
    rows = np.arange(R)
    eb = np.abs(G[:, 0] - X[:, blank])
    worst["blank err/bound"] = float((eb / acc[:, blank]).max())
    assert np.all(eb <= acc[:, blank]), float((eb - acc[:, blank]).max())
    u = rows % U1
    bb = rows // (T * U1)
    lab = np.full(R, V)
    has = u < U1 - 1
    lab[has] = y[bb[has], u[has]]
    has &= lab < V
    el = np.abs(G[has, 1] - X[rows[has], lab[has]])
    if has.any():
        worst["label err/bound"] = float((el / acc[rows[has], lab[has]]).max())
        assert np.all(el <= acc[rows[has], lab[has]]), float((el - acc[rows[has], lab[has]]).max())
    x16 = out16[:, :V].float().cpu().numpy().astype(np.float64)
    e16 = np.abs(x16 - np.clip(X, -65504, 65504))
    assert np.all(e16 <= 2.0 ** -11 * np.abs(X) + 2 * acc), float((e16 - 2.0 ** -11 * np.abs(X) - 2 * acc).max())
    lse64 = _lse(X)[:, 0]
    lse = lse_d.cpu().numpy().astype(np.float64)
    lb = acc.max(1) + (64 + n_part + 16) * 2.0 ** -24 * np.maximum(1.0, np.abs(lse64))
    el = np.abs(lse - lse64)[live]
    worst["lse err/bound"] = float((el / lb[live]).max())
    assert np.all(el <= lb[live]), float((el - lb[live]).max())
    assert np.all(lse[~live] == 0)
    lp = log_softmax(X).astype(np.float32).reshape(B, T, U1, V)
    c64, _ = O.rnnt_loss(lp, y, tl, ul, blank=blank, want_grads=False)
    _check_costs(c_d.cpu().numpy(), c64, "gathered", worst)
    # gathered = NULL: the same product otherwise
    assert torch.equal(out16n[:, :V], out16[:, :V]) and torch.equal(pmn, pm) and torch.equal(psn, ps)
    _report("gathered U1=%d T=%d V=%d blank=%d" % (U1, T, V, blank), worst)


# ---------------------------------------------------------------------------------------------------------------------
# 1c. d(logits) against fp64
# ---------------------------------------------------------------------------------------------------------------------
@_rows("dlogits")
def test_dlogits_routes(hip_device, row):
    """Every element within the bf16 rounding (2^-8) of the fp64 d(logits), plus the gradient bound carried through
    scale * (g - p * sum g) (module docstring); columns [V, ld_out) and rows outside every sub-lattice exactly zero (their
    logits are ~100: exp overflows there); colsum against the fp64 column sums of the unrounded reference, within the
    sum of the per-element bounds before rounding plus fp32 summation (_check_dlogits).  fp16-input route: softmax of the fp16 logits read back from the product, of the exact
    logits for the blank and label columns when `gathered` is passed."""
    dev = hip_device
    V, blank, scale, B, T, U = (row[k] for k in ("V", "blank", "scale", "B", "T", "U"))
    U1 = U + 1
    R = B * T * U1
    rng = np.random.default_rng(V * 7 + U)
    if B == 4:             # (Tn = 1, Un = U): every label leaves from the last frame, where blank has no gradient term
        tl = np.array([T, 1, T - 1, 1], np.int32)
        ul = np.array([U, 0, U - 2, U], np.int32)
    else:
        tl = np.array([T, T - 3], np.int32)
        ul = np.array([U, U - 7], np.int32)
    y = _labels(B, U, V, blank, ul, rng)
    A, Wt, bias, X, mag, live = _joint_case(B, T, U1, V, blank, V + U, tl, ul, boost=set(y[y < V].tolist()) | {blank})
    lse64 = _lse(X)
    lp = (X - lse64).astype(np.float32)
    w = (rng.random(B) + 0.5).astype(np.float32)
    _, g64 = O.rnnt_loss(lp.reshape(B, T, U1, V), y, tl, ul, blank=blank)
    g = (g64 * w[:, None, None, None]).reshape(R, V)
    del g64
    rel, abs_ = _tol(T + U1 - 1)
    L = _L()
    y_d, tl_d, ul_d, w_d = (_d(a, dev) for a in (y, tl, ul, w))
    x32 = X.astype(np.float32)
    worst = {}
    # the row's label column (ye of the row metadata): u < Un, t < Tn
    rr = np.arange(R)
    u, t, bb = rr % U1, (rr // U1) % T, rr // (T * U1)
    ye = np.full(R, -1)
    em = (t < tl[bb]) & (u < ul[bb])
    ye[em] = y[bb[em], u[em]]

    def meta(fwd_ws):          # row metadata of the loss (scaled by w) in fwd_ws
        _ok(L.pika_rnnt_loss_backward(_p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(w_d), _p(fwd_ws), None, _s()),
            "loss_backward (metadata)")

    def fused_fwd(xd):
        ws = _ws(B, T, U1, dev)
        c = torch.empty(B, dtype=torch.float32, device=dev)
        lse = torch.empty(R, dtype=torch.float32, device=dev)
        _ok(L.pika_rnnt_fused_forward(_p(xd), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(c), _p(lse), _p(ws),
                                      _s()), "fused_forward")
        return ws, lse

    for route in row["routes"]:
        kind = route[0]
        what = "%s V=%d %s" % (kind, V, route[1:])
        if kind == "lp":
            colsum, ld_out = route[1], route[2]
            xin = _d(lp, dev)
            ws = _ws(B, T, U1, dev)
            c = torch.empty(B, dtype=torch.float32, device=dev)
            _ok(L.pika_rnnt_loss_forward(_p(xin), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(c), _p(ws), _s()),
                "loss_forward")
            meta(ws)
            out = _nan((R, ld_out), torch.bfloat16, dev)
            cs = _nan((V,), torch.float32, dev) if colsum else None
            _ok(L.pika_rnnt_dlogits_compact_bf16(_p(xin), None, _p(ws), B, T, U1, V, blank, _p(out), ld_out, scale, _p(cs),
                                                 _s()), "dlogits_compact_bf16")
            p = np.exp(lp.astype(np.float64))
            sc, bf = scale, True
        elif kind == "raw":
            colsum, ld_out = route[1], route[2]
            xin = _d(x32, dev)
            ws, lse = fused_fwd(xin)
            meta(ws)
            out = _nan((R, ld_out), torch.bfloat16, dev)
            cs = _nan((V,), torch.float32, dev) if colsum else None
            _ok(L.pika_rnnt_dlogits_compact_bf16(_p(xin), _p(lse), _p(ws), B, T, U1, V, blank, _p(out), ld_out, 1.0, _p(cs),
                                                 _s()), "dlogits_compact_bf16 (raw logits)")
            x64 = x32.astype(np.float64)
            p = np.exp(x64 - _lse(x64))
            sc, bf = 1.0, True
        elif kind == "f16":
            colsum, ld_out, ld_in, use_g = route[1:]
            A_d, W_d, bias_d = A.to(dev), Wt.to(dev), _d(bias, dev)
            out16, pm, ps, gat, n_part = _gemm_f16(dev, A_d, W_d, bias_d, R, V, ld_in, y_d, T, U1, blank)
            ws = _ws(B, T, U1, dev)
            c = torch.empty(B, dtype=torch.float32, device=dev)
            lse = torch.empty(R, dtype=torch.float32, device=dev)
            _ok(L.pika_rnnt_fused_forward_gathered(_p(out16), ld_in, _p(gat), _p(y_d), blank, _p(pm), _p(ps), n_part,
                                                   _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(c), _p(lse), _p(ws),
                                                   _s()), "fused_forward_gathered")
            meta(ws)
            out = _nan((R, ld_out), torch.bfloat16, dev)
            cs = _nan((V,), torch.float32, dev) if colsum else None
            _ok(L.pika_rnnt_dlogits_compact_bf16_f16in(_p(out16), ld_in, _p(lse), _p(ws), B, T, U1, V, blank, _p(out), ld_out,
                                                       scale, _p(cs), _p(gat) if use_g else None,
                                                       _p(y_d) if use_g else None, blank, _s()), "dlogits_compact_f16in")
            torch.cuda.synchronize()
            xin = out16[:, :V].float().cpu().numpy().astype(np.float64)
            if use_g:                  # blank and label columns from the exact logits
                xin[:, blank] = X[:, blank]
                xin[em, ye[em]] = X[em, ye[em]]
            p = np.exp(xin - lse64)
            sc, bf = scale, True
        else:
            out_dtype, ld_out = route[1], route[2]
            colsum = False
            xin = _d(x32, dev)
            ws, lse = fused_fwd(xin)
            out = _nan((R, ld_out), torch.float32 if out_dtype == 0 else torch.bfloat16, dev)
            _ok(L.pika_rnnt_fused_backward(_p(xin), _p(lse), _p(y_d), _p(tl_d), _p(ul_d), B, T, U1, V, blank, _p(w_d),
                                           _p(ws), _p(out), out_dtype, ld_out, _s()), "fused_backward")
            x64 = x32.astype(np.float64)
            p = np.exp(x64 - _lse(x64))
            sc, bf = 1.0, out_dtype == 1
        torch.cuda.synchronize()
        o = out.float().cpu().numpy()
        _check_dlogits(o, ld_out, V, g, p, sc, rel, abs_, bf, live, what, worst,
                       colsum=cs.cpu().numpy() if colsum else None)
        del p
    _report("dlogits V=%d B=%d T=%d U1=%d" % (V, B, T, U1), worst)


# ---------------------------------------------------------------------------------------------------------------------
# 1d. rejections: before any launch (the buffers below are far too small for a launch)
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections(hip_device):
    """U1 = 1025: PIKA_ETOOBIG from the check_dims entries, PIKA_EINVAL from the compact and export entries (their own
    U1 test), a zero workspace size.  V = 8196 or V % 4 != 0: PIKA_EINVAL from the V-limited entries."""
    L = _L()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=hip_device)
    q = _p(buf)
    s = _s()
    B, T = 1, 2
    assert L.pika_rnnt_workspace_bytes(B, T, 1025) == 0
    for U1, V, want in ((1025, 8, PIKA_ETOOBIG),):
        assert L.pika_rnnt_loss_forward(q, q, q, q, B, T, U1, V, 0, q, q, s) == want
        assert L.pika_rnnt_loss_backward(q, q, q, B, T, U1, V, 0, None, q, q, s) == want
        assert L.pika_rnnt_loss_dense_grads(q, B, T, U1, V, 0, q, s) == want
        assert L.pika_rnnt_loss_fwd_bwd(q, q, q, q, B, T, U1, V, 0, q, q, q, s) == want
        assert L.pika_rnnt_fused_forward(q, q, q, q, B, T, U1, V, 0, q, q, q, s) == want
        assert L.pika_rnnt_fused_forward_partials(q, q, q, 4, q, q, q, B, T, U1, V, 0, q, q, q, s) == want
        assert L.pika_rnnt_fused_forward_gathered(q, V, q, q, 0, q, q, 4, q, q, q, B, T, U1, V, 0, q, q, q, s) == want
        assert L.pika_rnnt_fused_backward(q, q, q, q, q, B, T, U1, V, 0, None, q, q, 0, V, s) == want
        assert L.pika_rnnt_dlogits_compact_bf16(q, None, q, B, T, U1, V, 0, q, V, 1.0, q, s) == PIKA_EINVAL
        assert L.pika_rnnt_dlogits_compact_bf16_f16in(q, V, q, q, B, T, U1, V, 0, q, V, 1.0, q, None, None, 0, s) == PIKA_EINVAL
        assert L.pika_rnnt_export_lattice(q, q, q, B, T, U1, q, q, s) == PIKA_EINVAL
    for V in (8196, 6):
        U1 = 2
        assert L.pika_rnnt_fused_forward(q, q, q, q, B, T, U1, V, 0, q, q, q, s) == PIKA_EINVAL
        assert L.pika_rnnt_fused_backward(q, q, q, q, q, B, T, U1, V, 0, None, q, q, 0, V, s) == PIKA_EINVAL
        assert L.pika_rnnt_fused_backward(q, q, q, q, q, B, T, U1, V, 0, None, q, q, 1, V, s) == PIKA_EINVAL
        assert L.pika_rnnt_dlogits_compact_bf16(q, None, q, B, T, U1, V, 0, q, V, 1.0, q, s) == PIKA_EINVAL
        assert L.pika_rnnt_dlogits_compact_bf16_f16in(q, V, q, q, B, T, U1, V, 0, q, V, 1.0, q, None, None, 0, s) == PIKA_EINVAL
    torch.cuda.synchronize()
    assert torch.count_nonzero(buf).item() == 0
