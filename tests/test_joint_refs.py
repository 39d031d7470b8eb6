"""The float64 restatements and the case tables of tests/joint_common.py on their own (no GPU): the restatements against
torch autograd in float64, and what every table promises the GPU tests of tests/test_joint_kernels_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_common as J  # noqa: E402


@pytest.mark.parametrize("B,T,U,H", [(1, 1, 1, 4), (2, 3, 2, 8), (2, 5, 3, 20)])
def test_gate_restatements_equal_autograd_in_float64(B, T, U, H):
    g = torch.Generator().manual_seed(B + T + H)
    ins = [torch.randn(B, n, H, generator=g, dtype=torch.float64).requires_grad_(True) for n in (T, U, T, U)]
    dh = torch.randn(B, T, U, H, generator=g, dtype=torch.float64)
    e1, p1, eg, pg = ins
    h = torch.tanh(e1.unsqueeze(2) + p1.unsqueeze(1)) * torch.sigmoid(eg.unsqueeze(2) + pg.unsqueeze(1))
    want = torch.autograd.grad(h, ins, grad_outputs=dh)
    det = [t.detach() for t in ins]
    assert (J.gate_ref(*det) - h.detach()).abs().max() < 1e-14
    for got, w in zip(J.gate_bwd_ref(dh, *det), want):
        assert got.shape == w.shape and (got - w).abs().max() < 1e-13


@pytest.mark.parametrize("rows,cols,scale", [(1, 4, 1.0), (5, 13, 0.7), (3, 300, 0.8)])
def test_log_softmax_restatements_equal_autograd_in_float64(rows, cols, scale):
    g = torch.Generator().manual_seed(rows + cols)
    x = (torch.randn(rows, cols, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    w = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    s = float(np.float32(scale))
    lp = torch.log_softmax(s * x, dim=-1)
    dx, = torch.autograd.grad(lp, [x], grad_outputs=w, retain_graph=True)
    assert (J.log_softmax_ref(x.detach(), scale) - lp.detach()).abs().max() < 1e-13
    assert (J.log_softmax_bwd_ref(lp.detach(), w, scale) - dx).abs().max() < 1e-13
    # the risk gradient: d/dlogits of sum_r val[r] * lp[r, sym[r]]
    sym = torch.randint(0, cols, (rows,), generator=g)
    val = torch.randn(rows, generator=g, dtype=torch.float64)
    val[0] = 0.0
    dr, = torch.autograd.grad((lp.gather(1, sym.unsqueeze(1)).squeeze(1) * val).sum(), [x])
    got = J.risk_grad_ref(lp.detach(), sym, val, scale)
    assert (got - dr).abs().max() < 1e-13 and bool((got[0] == 0).all())


def test_log_softmax_restatement_on_masked_and_non_finite_rows_equals_torch():
    x = torch.randn(4, 9, dtype=torch.float64)
    x[0, 2] = -J.INF
    x[1] = -J.INF
    x[2, 5] = J.NAN
    got, want = J.log_softmax_ref(x, 1.0), torch.log_softmax(x, dim=-1)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(got[2]).all()) and not bool(torch.isnan(got[[0, 3]]).any())
    assert float(got[0, 2]) == -J.INF
    ok = ~torch.isnan(want) & ~torch.isinf(want)
    assert (got[ok] - want[ok]).abs().max() < 1e-13


def test_padded_buffer_builder():
    data = np.arange(6, dtype=np.float32).reshape(2, 3)
    p = J.Padded(2, 3, 5, offset=1, data=data)
    assert p.byte_offset() % 16 == 4 and J.Padded(2, 3, 5).byte_offset() % 256 == 0
    assert np.array_equal(p.window(p.bits).view(np.float32), data)
    assert int(p.pad_mask().sum()) == p.bits.size - 6 and bool((p.bits[p.pad_mask()] == J.SENT32).all())
    assert p.padding_intact(p.bits.copy())
    for at in (0, p.start - 1, p.start + 3, p.start + 2 * 5, p.bits.size - 1):      # front, row padding, rows behind
        b = p.bits.copy()
        b[at] ^= 1
        assert not p.padding_intact(b)
    b = p.bits.copy()
    p.window(b)[...] = 0
    assert p.padding_intact(b)
    assert np.isnan(np.array([J.SENT32]).view(np.float32)[0])
    assert J.Padded(1, 4, 8, itemsize=2).bits.dtype == np.uint16


# ---- gate table ----------------------------------------------------------------------------------------------------
def test_gate_table_covers_the_thread_counts_and_clamps():
    assert [s[3] // 4 for s in J.GATE_SHAPES] == [1, 64, 65, 256, 1024, 1025]
    assert all(s[3] % 4 == 0 for s in J.GATE_SHAPES)
    for v in (-15.5, -15.0, 15.0, 15.5, -40.0, 40.0):
        assert v in J.SAT_Z1
    for v in (-50.5, -50.0, -100.0, 100.0):
        assert v in J.SAT_ZG
    c = J.gate_case("saturation")
    z1 = (c["e1"].double()[:, :, None] + c["p1"].double()[:, None])
    zg = (c["eg"].double()[:, :, None] + c["pg"].double()[:, None])
    n = len(J.SAT_Z1)
    for t in range(c["shape"][1]):
        for u in range(c["shape"][2]):
            assert z1[0, t, u, :n].tolist() == J.SAT_Z1 and zg[0, t, u, n:].tolist() == J.SAT_ZG
            assert set(zg[0, t, u, :n].tolist()) == {J.SAT_MODERATE_ZG} and set(z1[0, t, u, n:].tolist()) == {J.SAT_MODERATE_Z1}


@pytest.mark.parametrize("name", J.gate_case_names())
def test_gate_cases_are_finite_exactly_where_they_say(name):
    c = J.gate_case(name)
    ins = [c[k] for k in J.INPUT_NAMES]
    assert bool(torch.isfinite(c["dh"]).all()) and bool(torch.isfinite(c["dh16"].float()).all())
    bad = sum(int((~torch.isfinite(t)).sum()) for t in ins)
    if c["finite"]:
        assert name.startswith("shape_") or name == "saturation"
        assert bad == 0
        for t in (c["h"],) + tuple(c["grads"]) + tuple(c["grads16"]):
            assert bool(torch.isfinite(t).all())
        return
    # non-finite cases: exactly the named elements, each holding exactly the named value
    assert name in J.GATE_NONFINITE and bad == len(c["named"])
    assert len(c["named"]) == (2 if name.startswith("inf_meet") else 1)
    for which, idx, value in c["named"]:
        got = float(c[which][idx])
        assert (np.isnan(got) and np.isnan(value)) or got == value
    # ... and where the reference is NaN: the lattice positions whose sum holds a NaN (a lone inf gives a limit, not NaN)
    B, T, U, H = c["shape"]
    z = [c["e1"][:, :, None] + c["p1"][:, None], c["eg"][:, :, None] + c["pg"][:, None]]
    nan_pos = torch.isnan(z[0]) | torch.isnan(z[1])
    assert torch.equal(torch.isnan(c["h"]), nan_pos)
    if name.startswith("nan_") or name.startswith("inf_meet"):
        assert int(nan_pos.sum()) == {"nan_e1": U, "nan_eg": U, "nan_p1": T, "nan_pg": T}.get(name, 1)
    else:
        assert int(nan_pos.sum()) == 0 and bool(torch.isfinite(c["h"]).all())
        which, idx, value = c["named"][0]
        b, n, ch = idx
        col = c["h"][b, n, :, ch] if which[0] == "e" else c["h"][b, :, n, ch]
        lim = gate_limit(c, which, idx, value)
        assert (col - lim).abs().max() < 1e-12
    for grads in (c["grads"], c["grads16"]):
        for gr, nan_want in zip(grads, (nan_pos.any(2), nan_pos.any(1), nan_pos.any(2), nan_pos.any(1))):
            assert torch.equal(torch.isnan(gr), nan_want) and bool(torch.isfinite(gr[~nan_want]).all())


def gate_limit(c, which, idx, value):
    """h along the named element of a lone +-inf: tanh -> +-1 times the finite sigmoid, sigmoid -> 1 or 0 times the finite tanh."""
    b, n, ch = idx
    other = {"e1": ("eg", "pg"), "p1": ("eg", "pg"), "eg": ("e1", "p1"), "pg": ("e1", "p1")}[which]
    e, p = c[other[0]].double(), c[other[1]].double()
    z = e[b, n, ch] + p[b, :, ch] if which[0] == "e" else e[b, :, ch] + p[b, n, ch]
    if which in ("e1", "p1"):
        return np.sign(value) * torch.sigmoid(z)
    return (1.0 if value > 0 else 0.0) * torch.tanh(z)


# ---- log-softmax table ---------------------------------------------------------------------------------------------
def test_log_softmax_table_covers_every_route_boundary_and_layout():
    by = {}
    for c in J.LSM_CASES:
        if c["kind"] == "finite":
            by[(c["cols"], c["layout"])] = c
    assert sorted({c for c, _ in by}) == sorted(J.LSM_COLS) == [4, 8, 13, 252, 256, 260, 5116, 5120, 5124, 8188, 8192, 8196, 8197]
    for cols in J.LSM_COLS:
        want = {"eq", "pad4", "pad1"} | ({"off1"} if cols % 4 == 0 else set())
        assert {l for c, l in by if c == cols} == want
        assert by[(cols, "eq")]["ld"] == cols and by[(cols, "pad4")]["ld"] == cols + 4 and by[(cols, "pad1")]["ld"] == cols + 1
        assert by[(cols, "pad1")]["route"] == "block"
        if cols % 4 == 0:
            o = by[(cols, "off1")]
            assert o["offset"] == 1 and o["ld"] % 4 == 0 and o["route"] == "block"
        assert len({by[k]["rows"] for k in by if k[0] == cols}) == 1         # one data set per cols
    # the aligned layouts sit on both sides of both boundaries
    assert [by[(c, "eq")]["route"] for c in (5116, 5120, 5124, 8188, 8192, 8196, 8197)] == \
        ["wave20", "wave20", "wave32", "wave32", "wave32", "block", "block"]
    assert [by[(c, "pad4")]["route"] for c in (5120, 5124, 8192, 8196)] == ["wave20", "wave32", "wave32", "block"]
    assert by[(13, "eq")]["route"] == "block" and by[(4, "eq")]["route"] == "wave20"
    for route in ("wave20", "wave32", "block"):
        assert {c["rows"] for c in J.LSM_CASES if c["route"] == route} >= {3, 5}, route
    assert {c["rows"] for c in J.LSM_CASES if c["kind"] == "finite"} == {1, 2, 3, 4, 5, 9}
    assert {c["scale"] for c in J.LSM_CASES} == {1.0, 0.7}
    assert {c["scale"] for c in J.LSM_CASES if c["route"] == "wave32"} == {1.0, 0.7}
    assert set(J.ROUTE_COLS) <= set(J.LSM_COLS)
    # masking / NaN cases: once on a wave route and once on the block route, inside the first 4-row workgroup
    for kind in ("mask", "neginf_row", "nan_row"):
        assert sorted(c["route"] for c in J.LSM_CASES if c["kind"] == kind) == ["block", "wave20"]


@pytest.mark.parametrize("name", [c["name"] for c in J.LSM_CASES])
def test_log_softmax_cases_are_finite_exactly_where_they_say(name):
    c, d = J.LSM_BY_NAME[name], J.lsm_data(name)
    rows = c["rows"]
    all_neginf = [r for r in range(rows) if bool((d["x"][r] == -J.INF).all())]
    has_nan = [r for r in range(rows) if bool(torch.isnan(d["x"][r]).any())]
    assert len(all_neginf) <= 1 and len(has_nan) <= 1
    assert sorted(all_neginf + has_nan) == d["bad_rows"]
    assert (c["kind"] == "neginf_row") == bool(all_neginf) and (c["kind"] == "nan_row") == bool(has_nan)
    for r in range(rows):
        if r in d["bad_rows"]:
            assert bool(torch.isnan(d["want"][r]).all())
            assert 0 < r < 3 and rows > 4          # next to finite rows inside one 4-row workgroup, and a second workgroup
        else:
            w = d["want"][r]
            assert bool(torch.isfinite(w[~d["neginf"][r]]).all()) and bool((w[d["neginf"][r]] == -J.INF).all())
            assert bool(torch.isfinite(d["want_bwd"][r]).all())
    assert (c["kind"] == "mask") == bool(d["neginf"].any())
    if c["kind"] == "mask":
        assert bool((d["g"][d["neginf"]] == 0).all()) and int(d["neginf"].any(1).sum()) == 2
    assert d["lp"].dtype == torch.float32 and d["gsum"] > 0
    ok = torch.isfinite(d["want"])
    assert (torch.exp(d["want"]) * ok).sum(1)[[r for r in range(rows) if r not in d["bad_rows"]]].sub(1).abs().max() < 1e-12


def test_bf16_backward_table():
    assert [(c, o) for c, o, _ in J.BF16_BWD_CASES] == [(8, 64), (5000, 5056), (5000, 5184), (5120, 5120), (6268, 6272), (8192, 8192)]
    for cols, ld_out, rows in J.BF16_BWD_CASES:
        assert cols % 4 == 0 and ld_out % 4 == 0 and cols <= ld_out <= J.WAVE_MAX and rows % 4 != 0
        d = J.bf16_bwd_data(cols, rows)
        assert bool(torch.isfinite(d["want"]).all()) and d["lp"].shape == (rows, cols)
    assert any(cols <= J.WQ20_MAX < ld_out for cols, ld_out, _ in J.BF16_BWD_CASES)     # WQ picked by ld_out, not cols
    assert any(cols < ld_out <= J.WQ20_MAX for cols, ld_out, _ in J.BF16_BWD_CASES)
    assert any(J.WQ20_MAX < cols < ld_out for cols, ld_out, _ in J.BF16_BWD_CASES)


def test_risk_table():
    assert J.RISK_SHAPES == [(1, 4, 4), (5, 13, 16), (3, 300, 301), (4, 5000, 5000)]
    seen_zero = seen_neginf = False
    for rows, cols, ld in J.RISK_SHAPES:
        d = J.risk_data(rows, cols)
        assert int(d["sym"][0]) == 0 and (rows == 1 or int(d["sym"][-1]) == cols - 1)
        assert bool(((0 <= d["sym"]) & (d["sym"] < cols)).all())
        assert bool(torch.isfinite(d["want"]).all())
        for r in d["zero_rows"]:
            assert float(d["val"][r]) == 0.0 and bool((d["want"][r] == 0).all())
            seen_zero |= bool(torch.isnan(d["lp"][r]).any()) and bool((d["lp"][r] == -J.INF).any())
        for r, v in d["neginf_at"]:
            assert float(d["val"][r]) != 0.0 and int(d["sym"][r]) != v and float(d["lp"][r, v]) == -J.INF
            assert float(d["want"][r, v]) == 0.0
            seen_neginf = True
        live = [r for r in range(rows) if r not in d["zero_rows"]]
        assert live and bool((d["want"][live].abs().sum(1) > 0).all())
        nonfinite_rows = {int(r) for r in (~torch.isfinite(d["lp"])).any(1).nonzero().flatten()}
        assert nonfinite_rows == set(d["zero_rows"] if rows == 5 else []) | {r for r, _ in d["neginf_at"]}
    assert seen_zero and seen_neginf
