"""The kernels of pika_amd/csrc/joint.hip through the C ABI (include/pika_joint.h) against the float64 restatements and the
case tables of tests/joint_common.py: the gate forward / backward in every dtype combination, at every thread count, at
the saturation clamps and on non-finite inputs; the three log-softmax routes (wave-per-row with 20 and with 32 float4 per
lane, the 256-thread block kernel) on both sides of their boundaries, with padded pitches and a misaligned base; the bf16
log-softmax backward with its zero fill; the MBR risk gradient; and every argument refusal.

Tolerances are those of the autograd-level tests of the same kernels (tests/test_joint_gpu.py, tests/test_mbr.py).  Every
measured error is printed (`JOINTPARITY ...`) before it is asserted; profiles/joint_parity.txt keeps the largest per group.

Measured on the MI355X: gate h 3.8e-7 (of 2e-6), gate gradients 9.5e-7 (of 1e-5), log-softmax forward 1.8e-6 / 1.9e-6 /
1.7e-6 on the three routes (of 1e-5), backward 5.0e-6 at most, risk gradient 4.1e-8.  The non-finite gate cases fail on the
kernel as it was before its clamps let a NaN through (fminf / fmaxf returned -15 or -50 for it).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_common as J  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from pika_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(group, case, what, err, tol):
    print("JOINTPARITY %-12s %-28s %-8s err %.3g  tol %.3g" % (group, case, what, err, tol))


def _max_err(got, want, where=None):
    d = (got.double().cpu() - want).abs()
    if where is not None:
        d = d[where]
    return float(d.max()) if d.numel() else 0.0


# ---- gate ----------------------------------------------------------------------------------------------------------
def _gate_fwd(c, dev, out_dtype):
    B, T, U, H = c["shape"]
    ins = [c[k].to(dev) for k in J.INPUT_NAMES]
    h = torch.empty(B, T, U, H, device=dev, dtype=torch.float32 if out_dtype == J.F32 else torch.bfloat16)
    rc = _lib().pika_joint_gate_fwd(*[t.data_ptr() for t in ins], h.data_ptr(), out_dtype, B, T, U, H, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return h


def _gate_bwd(c, dev, dh):
    B, T, U, H = c["shape"]
    ins = [c[k].to(dev) for k in J.INPUT_NAMES]
    dh = dh.to(dev)
    outs = [torch.full((B, n, H), -7.0, device=dev) for n in (T, U, T, U)]          # de1, dp1, deg, dpg
    rc = _lib().pika_joint_gate_bwd(dh.data_ptr(), J.F32 if dh.dtype == torch.float32 else J.BF16,
                                    *[t.data_ptr() for t in ins], *[t.data_ptr() for t in outs], B, T, U, H, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return outs


def _check_gate(c, dev, out_dtype, dh_dtype):
    """One forward in `out_dtype` and one backward from a `dh_dtype` upstream gradient against float64; NaN positions as a
    set, everything else within tolerance; bf16 results bit for bit against the fp32 results of the same call."""
    name = c["name"]
    h32 = _gate_fwd(c, dev, J.F32)
    nan_want = torch.isnan(c["h"])
    assert torch.equal(torch.isnan(h32).cpu(), nan_want), "%s: NaN positions of h" % name
    assert not bool(torch.isinf(h32).any())
    err = _max_err(h32, c["h"], ~nan_want)
    _report("gate_fwd", name, "h", err, J.GATE_H_TOL)
    assert err < J.GATE_H_TOL
    if out_dtype == J.BF16:
        h16 = _gate_fwd(c, dev, J.BF16)
        assert torch.equal(h16.view(torch.int16)[~nan_want.to(dev)], h32.bfloat16().view(torch.int16)[~nan_want.to(dev)])
        assert torch.equal(torch.isnan(h16).cpu(), nan_want)
    # backward: from the fp32 dh, or from the bf16 dh -- then also from its upcast, which must give the same bits
    if dh_dtype == J.F32:
        got, want = _gate_bwd(c, dev, c["dh"]), c["grads"]
    else:
        got, want = _gate_bwd(c, dev, c["dh16"]), c["grads16"]
        up = _gate_bwd(c, dev, c["dh16"].float())
        for a, b in zip(got, up):
            assert torch.equal(a.view(torch.int32)[~torch.isnan(b)], b.view(torch.int32)[~torch.isnan(b)])
            assert torch.equal(torch.isnan(a), torch.isnan(b))
    for what, a, w in zip(("de1", "dp1", "deg", "dpg"), got, want):
        nan_w = torch.isnan(w)
        assert torch.equal(torch.isnan(a).cpu(), nan_w), "%s: NaN positions of %s" % (name, what)
        assert not bool(torch.isinf(a).any())
        scale = float(w[~nan_w].abs().max()) if bool((~nan_w).any()) else 0.0
        tol = J.GRAD_REL_TOL * max(1.0, scale)
        err = _max_err(a, w, ~nan_w)
        _report("gate_bwd", name, what, err, tol)
        assert err < tol, (name, what, err, tol)


@pytest.mark.parametrize("dh_dtype", [J.F32, J.BF16], ids=["dh_f32", "dh_bf16"])
@pytest.mark.parametrize("out_dtype", [J.F32, J.BF16], ids=["out_f32", "out_bf16"])
@pytest.mark.parametrize("shape", J.GATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gate_shapes_against_float64(hip_device, shape, out_dtype, dh_dtype):
    _check_gate(J.gate_case("shape_%dx%dx%dx%d" % shape), hip_device, out_dtype, dh_dtype)


@pytest.mark.parametrize("dh_dtype", [J.F32, J.BF16], ids=["dh_f32", "dh_bf16"])
@pytest.mark.parametrize("out_dtype", [J.F32, J.BF16], ids=["out_f32", "out_bf16"])
def test_gate_at_the_saturation_clamps(hip_device, out_dtype, dh_dtype):
    """Chosen z1 around +-15 and zg around -50 (and far beyond): h and the four gradients within the usual absolute
    tolerances of float64, nothing NaN or inf (asserted inside: the reference is finite everywhere)."""
    c = J.gate_case("saturation")
    assert c["finite"]
    _check_gate(c, hip_device, out_dtype, dh_dtype)


@pytest.mark.parametrize("dh_dtype", [J.F32, J.BF16], ids=["dh_f32", "dh_bf16"])
@pytest.mark.parametrize("name", sorted(J.GATE_NONFINITE))
def test_gate_on_non_finite_inputs(hip_device, name, dh_dtype):
    """A NaN input element (or +inf and -inf meeting in one sum) makes exactly the outputs NaN that read it, as in the
    reference; a lone +-inf gives the limits (tanh -> +-1, sigmoid -> 1 or 0) within tolerance."""
    _check_gate(J.gate_case(name), hip_device, J.BF16, dh_dtype)


# ---- log-softmax ---------------------------------------------------------------------------------------------------
def _padded_on_device(p, dev):
    t = torch.from_numpy(p.bits.view(np.int32 if p.itemsize == 4 else np.int16).copy()).to(dev)
    assert t.data_ptr() % 256 == 0
    return t, t.data_ptr() + p.byte_offset()


def _fetch(p, t):
    """(the operand as float32 / int16 bits, allocation intact outside it) after the call."""
    torch.cuda.synchronize()
    bits = t.cpu().numpy().view(p.utype)
    win = np.ascontiguousarray(p.window(bits))
    return (torch.from_numpy(win.view(np.float32)) if p.itemsize == 4 else win), p.padding_intact(bits)


def _run_lsm_fwd(c, d, dev):
    p = J.Padded(c["rows"], c["cols"], c["ld"], c["offset"], data=d["x"].numpy())
    t, ptr = _padded_on_device(p, dev)
    assert ptr % 16 == (4 if c["offset"] else 0)
    assert _lib().pika_log_softmax_rows(ptr, c["rows"], c["cols"], c["ld"], c["scale"], _stream()) == 0
    got, intact = _fetch(p, t)
    assert intact, "%s: forward wrote outside [0, cols) x rows" % c["name"]
    return got


def _run_lsm_bwd(c, d, dev):
    pl = J.Padded(c["rows"], c["cols"], c["ld"], c["offset"], data=d["lp"].numpy())
    pg = J.Padded(c["rows"], c["cols"], c["ld"], c["offset"], data=d["g"].numpy())
    (tl, lptr), (tg, gptr) = _padded_on_device(pl, dev), _padded_on_device(pg, dev)
    assert _lib().pika_log_softmax_bwd_rows(lptr, gptr, c["rows"], c["cols"], c["ld"], c["scale"], _stream()) == 0
    got, intact = _fetch(pg, tg)
    lp_after, lp_intact = _fetch(pl, tl)
    assert intact and lp_intact, "%s: backward wrote outside [0, cols) x rows" % c["name"]
    assert np.array_equal(lp_after.numpy().view(np.uint32), d["lp"].numpy().view(np.uint32)), "lp is an input"
    return got


def _check_lsm(c, dev):
    d = J.lsm_data(c["name"])
    good = [r for r in range(c["rows"]) if r not in d["bad_rows"]]
    got = _run_lsm_fwd(c, d, dev)
    for r in d["bad_rows"]:
        assert bool(torch.isnan(got[r]).all()), "%s: row %d must be all NaN" % (c["name"], r)
    assert bool((got[d["neginf"]] == -J.INF).all())
    fin = ~d["neginf"][good]
    assert bool(torch.isfinite(got[good][fin]).all())
    err = _max_err(got[good], d["want"][good], fin)
    _report("lsm_fwd", c["name"], c["route"], err, J.LSM_FWD_TOL)
    assert err < J.LSM_FWD_TOL
    if d["bad_rows"]:
        return err, None
    got_b = _run_lsm_bwd(c, d, dev)
    assert bool(torch.isfinite(got_b).all())
    tol = J.GRAD_REL_TOL * max(1.0, d["gsum"])
    err_b = _max_err(got_b, d["want_bwd"])
    _report("lsm_bwd", c["name"], c["route"], err_b, tol)
    assert err_b < tol
    return err, err_b


@pytest.mark.parametrize("name", [c["name"] for c in J.LSM_CASES if c["kind"] == "finite"])
def test_log_softmax_rows_forward_and_backward_against_float64(hip_device, name):
    _check_lsm(J.LSM_BY_NAME[name], hip_device)


@pytest.mark.parametrize("cols", J.ROUTE_COLS)
def test_log_softmax_routes_agree_on_the_same_data(hip_device, cols):
    """The same rows through the aligned layout (wave kernel up to 8192 columns) and through ld = cols + 1 (block kernel):
    both within the float64 tolerance, on either side of 5120 and of 8192."""
    a, b = J.LSM_BY_NAME["c%d_eq" % cols], J.LSM_BY_NAME["c%d_pad1" % cols]
    assert b["route"] == "block" and a["route"] == {5120: "wave20", 5124: "wave32", 8192: "wave32", 8196: "block"}[cols]
    assert J.lsm_data(a["name"])["x"] is not None and torch.equal(J.lsm_data(a["name"])["x"], J.lsm_data(b["name"])["x"])
    for c in (a, b):
        _check_lsm(c, hip_device)


@pytest.mark.parametrize("name", [c["name"] for c in J.LSM_CASES if c["kind"] != "finite"])
def test_log_softmax_rows_masked_entries_and_non_finite_rows(hip_device, name):
    """-inf entries come out exactly -inf with the rest of the row finite (and a finite backward where g is 0 there); a row
    that is all -inf or holds one NaN comes out all NaN, its neighbours in the same 4-row workgroup unaffected."""
    _check_lsm(J.LSM_BY_NAME[name], hip_device)


@pytest.mark.parametrize("pad", [0, 4], ids=["ld_eq_cols", "ld_padded"])
@pytest.mark.parametrize("cols,ld_out,rows", J.BF16_BWD_CASES)
def test_log_softmax_bwd_rows_bf16(hip_device, cols, ld_out, rows, pad):
    """[0, cols) equals the in-place fp32 backward of the same inputs cast to bf16, bit for bit; [cols, ld_out) is +0; the
    rows behind and the inputs are untouched."""
    d = J.bf16_bwd_data(cols, rows)
    ld = cols + pad
    pl, pg = J.Padded(rows, cols, ld, data=d["lp"].numpy()), J.Padded(rows, cols, ld, data=d["g"].numpy())
    po = J.Padded(rows, ld_out, ld_out, itemsize=2)                # the kernel owns all ld_out columns of a row
    (tl, lptr), (tg, gptr), (to, optr) = (_padded_on_device(p, hip_device) for p in (pl, pg, po))
    assert optr % 8 == 0
    rc = _lib().pika_log_softmax_bwd_rows_bf16(lptr, gptr, optr, rows, cols, ld, ld_out, d["scale"], _stream())
    assert rc == 0
    out, out_intact = _fetch(po, to)
    (g_after, g_intact), (_, l_intact) = _fetch(pg, tg), _fetch(pl, tl)
    assert out_intact and g_intact and l_intact
    assert np.array_equal(g_after.numpy().view(np.uint32), d["g"].numpy().view(np.uint32)), "g is an input here"
    assert not (out[:, cols:] != 0).any(), "columns [cols, ld_out) must be +0"
    # the in-place fp32 kernel on the same inputs
    assert _lib().pika_log_softmax_bwd_rows(lptr, gptr, rows, cols, ld, d["scale"], _stream()) == 0
    g32, g_intact = _fetch(pg, tg)
    assert g_intact
    err = _max_err(g32, d["want"])
    tol = J.GRAD_REL_TOL * max(1.0, d["gsum"])
    _report("lsm_bwd_bf16", "c%d_o%d_r%d_ld%d" % (cols, ld_out, rows, ld), "fp32", err, tol)
    assert err < tol
    want16 = g32.bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(out[:, :cols], want16)


# ---- MBR risk gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ld", J.RISK_SHAPES)
def test_mbr_risk_grad_rows(hip_device, rows, cols, ld):
    d = J.risk_data(rows, cols)
    p = J.Padded(rows, cols, ld, data=d["lp"].numpy())
    t, ptr = _padded_on_device(p, hip_device)
    sym, val = d["sym"].to(hip_device), d["val"].to(hip_device)
    rc = _lib().pika_mbr_risk_grad_rows(ptr, sym.data_ptr(), val.data_ptr(), rows, cols, ld, J.RISK_SCALE, _stream())
    assert rc == 0
    got, intact = _fetch(p, t)
    assert intact, "padding overwritten"
    assert bool(torch.isfinite(got).all())
    for r in d["zero_rows"]:
        assert not bool((got[r].view(torch.int32) != 0).any()), "a val == 0 row must be exact +0 whatever lp holds"
    for r, v in d["neginf_at"]:
        assert float(got[r, v]) == 0.0
    err = _max_err(got, d["want"])
    _report("risk_grad", "%dx%d_ld%d" % (rows, cols, ld), "", err, J.RISK_TOL)
    assert err < J.RISK_TOL


# ---- refusals: host-side checks that return before any launch (dummy non-null pointers) ------------------------------
P = 4096              # a non-null, 16-byte aligned address that is never dereferenced


def test_gate_refusals():
    lib = _lib()

    def fwd(e1=P, p1=P, eg=P, pg=P, h=P, dt=J.F32, B=2, T=3, U=2, H=8):
        return lib.pika_joint_gate_fwd(e1, p1, eg, pg, h, dt, B, T, U, H, None)

    def bwd(dh=P, dt=J.F32, e1=P, p1=P, eg=P, pg=P, de1=P, dp1=P, deg=P, dpg=P, B=2, T=3, U=2, H=8):
        return lib.pika_joint_gate_bwd(dh, dt, e1, p1, eg, pg, de1, dp1, deg, dpg, B, T, U, H, None)
    for k in ("e1", "p1", "eg", "pg", "h"):
        assert fwd(**{k: None}) == J.EINVAL, k
    for k in ("dh", "e1", "p1", "eg", "pg", "de1", "dp1", "deg", "dpg"):
        assert bwd(**{k: None}) == J.EINVAL, k
    for f in (fwd, bwd):
        for k in ("B", "T", "U", "H"):
            assert f(**{k: 0}) == J.EINVAL and f(**{k: -1}) == J.EINVAL, k
        for H in (2, 6, 9, 4099):
            assert f(H=H) == J.EINVAL
        for dt in (2, -1, 7):
            assert f(dt=dt) == J.EINVAL
        assert f(B=65536) == J.ETOOBIG
        assert f(B=65536, H=6) == J.EINVAL


def test_row_kernel_refusals():
    lib = _lib()
    assert lib.pika_log_softmax_rows(None, 2, 8, 8, 1.0, None) == J.EINVAL
    assert lib.pika_log_softmax_bwd_rows(None, P, 2, 8, 8, 1.0, None) == J.EINVAL
    assert lib.pika_log_softmax_bwd_rows(P, None, 2, 8, 8, 1.0, None) == J.EINVAL
    for a in ((None, P, P), (P, None, P), (P, P, None)):
        assert lib.pika_mbr_risk_grad_rows(*a, 2, 8, 8, 1.0, None) == J.EINVAL
        assert lib.pika_log_softmax_bwd_rows_bf16(*a, 2, 8, 8, 64, 1.0, None) == J.EINVAL
    for rows, cols, ld in ((0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, -4, 8), (2, 8, 7), (2, 8, 4), (2, 8, 0)):
        assert lib.pika_log_softmax_rows(P, rows, cols, ld, 1.0, None) == J.EINVAL, (rows, cols, ld)
        assert lib.pika_log_softmax_bwd_rows(P, P, rows, cols, ld, 1.0, None) == J.EINVAL, (rows, cols, ld)
        assert lib.pika_mbr_risk_grad_rows(P, P, P, rows, cols, ld, 1.0, None) == J.EINVAL, (rows, cols, ld)
        assert lib.pika_log_softmax_bwd_rows_bf16(P, P, P, rows, cols, ld, 64, 1.0, None) == J.EINVAL, (rows, cols, ld)
    big = 1 << 31
    assert lib.pika_log_softmax_rows(P, big, 8, 8, 1.0, None) == J.ETOOBIG
    assert lib.pika_log_softmax_bwd_rows(P, P, big, 8, 8, 1.0, None) == J.ETOOBIG
    assert lib.pika_mbr_risk_grad_rows(P, P, P, big, 8, 8, 1.0, None) == J.ETOOBIG
    assert lib.pika_log_softmax_bwd_rows_bf16(P, P, P, big, 8, 8, 64, 1.0, None) == J.ETOOBIG

    def b16(lp=P, g=P, out=P, rows=2, cols=8, ld=8, ld_out=64):
        return lib.pika_log_softmax_bwd_rows_bf16(lp, g, out, rows, cols, ld, ld_out, 1.0, None)
    assert b16(ld_out=4) == J.EINVAL                       # ld_out < cols
    assert b16(ld_out=66) == J.EINVAL and b16(ld_out=9) == J.EINVAL      # ld_out % 4
    assert b16(cols=8192, ld=8192, ld_out=8196) == J.EINVAL             # ld_out > 8192
    assert b16(cols=8196, ld=8196, ld_out=8196) == J.EINVAL
    assert b16(cols=6, ld=8) == J.EINVAL and b16(cols=5, ld=8) == J.EINVAL     # cols % 4
    assert b16(ld=9) == J.EINVAL and b16(ld=10) == J.EINVAL               # ld % 4
    assert b16(out=P + 4) == J.EINVAL and b16(out=P + 2) == J.EINVAL      # out not 8-byte aligned
    assert b16(lp=P + 4) == J.EINVAL and b16(g=P + 8) == J.EINVAL         # lp / g not 16-byte aligned
