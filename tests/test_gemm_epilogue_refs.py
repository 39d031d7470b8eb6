"""tests/gemm_epilogue_common.py on its own (no GPU): the float64 reference against an independent form, the derived
accumulation bound against torch's fp32 CPU product (so the bound is known not to be too tight before it meets a kernel),
the condition the zero-pattern checks rest on, the bf16 ulp helper on hand-picked values, and the checkers themselves on
round-to-nearest-even casts made by torch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_epilogue_common as E  # noqa: E402

ALL_CASES = [("plain",) + s for s in E.SHAPES] + [("td",) + t for t in E.TD_CASES]


def _case(kind, *args):
    return E.case(*args) if kind == "plain" else E.td_case(*args)


def _lhs(c):
    return c["a"].double() if "a" in c else c["cols"]


@pytest.mark.parametrize("spec", ALL_CASES, ids=lambda s: "-".join(map(str, s)))
def test_reference_agrees_with_einsum_form(spec):
    c = _case(*spec)
    A, B = _lhs(c), c["b"].double()
    v = torch.einsum("mk,nk->mn", A, B) + c["bias"].double()[None, :]
    S = torch.einsum("mk,nk->mn", A.abs(), B.abs()) + c["bias"].double().abs()[None, :]
    # two float64 summation orders of exact products: a few float64 ulps of S apart
    assert ((v - c["v"]).abs() <= 2.0 ** -45 * c["S"]).all()
    assert ((S - c["S"]).abs() <= 2.0 ** -45 * c["S"]).all()
    assert c["v"].shape == (c["M"], c["N"])
    # the operands are what they claim: bf16 values, asymmetric (the transposed product is somewhere else entirely)
    assert c["b"].dtype == torch.bfloat16 and c["bias"].dtype == torch.float32
    if c["M"] == c["N"]:
        assert not torch.allclose(c["v"], c["v"].t())


@pytest.mark.parametrize("spec", ALL_CASES, ids=lambda s: "-".join(map(str, s)))
def test_fp32_cpu_product_lies_inside_acc_bound(spec):
    c = _case(*spec)
    got = _lhs(c).float() @ c["b"].float().t() + c["bias"]
    r = E.f32_error_ratio(got, c["v"], E.acc_bound(c["K"], c["S"]))
    assert r <= 1.0, r
    # ... and the bound is not vacuous: a relative error of 2^-14 of S (a product accumulated in anything shorter than
    # fp32) is outside it at every K of the tables
    assert E.acc_bound(c["K"], 1.0) < 2.0 ** -14


@pytest.mark.parametrize("spec", ALL_CASES, ids=lambda s: "-".join(map(str, s)))
def test_decided_elements_are_99_percent(spec):
    c = _case(*spec)
    frac = E.decided(c).double().mean().item()
    assert frac >= 0.99, frac


def test_shapes_sit_on_the_tile_edges():
    assert (E.TILE_M, E.TILE_N, E.TILE_K) == (256, 256, 64)
    for M, N, K in E.SHAPES:
        assert K % E.TILE_K == 0
    Ms, Ns = {s[0] for s in E.SHAPES}, {s[1] for s in E.SHAPES}
    assert 1 in Ms and E.TILE_M - 1 in Ms and E.TILE_M + 1 in Ms and 2 * E.TILE_M + 1 in Ms
    assert any(n % 4 for n in Ns) and any(E.TILE_N < n < E.TILE_N + 8 for n in Ns) and any(n > 2 * E.TILE_N for n in Ns)
    for _, N, _ in E.STORE_PATH_SHAPES:
        assert E.ldo_for(N, 0) % 8 == 0 and E.ldo_for(N, 4) % 8 == 4
        assert {E.ldo_for(N, 0), E.ldo_for(N, 4)} == {E.round_up(N, 4) + 4, E.round_up(N, 4) + 8}
    for dil, stride, pad, T in E.TD_CASES:
        assert E.TD_BATCH * E.td_out_len(T, dil, stride, pad) > E.TILE_M > 2 * E.td_out_len(T, dil, stride, pad)


def test_aux_holds_every_special_where_it_matters():
    for M, N, K in E.SHAPES:
        aux = E.case(M, N, K)["aux"]
        bits = aux.view(torch.int16)
        assert (bits == 0).any() and (bits == -32768).any()                  # +0 and -0
        assert (aux.double() == E.TINY_BF16).any() and (aux > 0).any()
        assert M * N <= 4 or ((aux < 0).any() and (aux.double() > 1e-3).any())       # (the 1 x 4 case holds specials only)
        # corners of the matrix are +0 / -0 / tiny: the three values `>= 0` or a flushed comparison would get wrong
        for r, c_ in ((0, 0), (M - 1, 0)):
            assert abs(float(aux[r, c_])) <= E.TINY_BF16
        want = E.expect_mask(E.case(M, N, K), 1.25)
        assert (want[aux.double() == 0] == 0).all()
        assert (want[aux.double() == E.TINY_BF16] != 0).any()


def test_bf16_ulp_on_hand_picked_values():
    cases = {1.0: 2.0 ** -7, 2.0: 2.0 ** -6, 0.5: 2.0 ** -8, 1.9921875: 2.0 ** -7,      # 1.9921875 = 2 - 2^-7: just below 2
             0.99609375: 2.0 ** -8, 3.0: 2.0 ** -6, -3.0: 2.0 ** -6, 256.0: 2.0, 255.0: 1.0,
             2.0 ** -100: 2.0 ** -107, 2.0 ** -126: 2.0 ** -133, 1.5 * 2.0 ** -126: 2.0 ** -133, 0.0: 2.0 ** -133}
    xs = torch.tensor(list(cases), dtype=torch.float64)
    assert torch.equal(E.bf16_ulp(xs), torch.tensor(list(cases.values()), dtype=torch.float64))
    # against the format itself: the next bf16 above x is x + ulp(x)
    x = torch.tensor([1.0, 1.9921875, 0.0078125, 100.0], dtype=torch.bfloat16)
    nxt = (x.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - x.double()), E.bf16_ulp(x.double()))


def test_dropout_constants():
    assert E.thr_of(0.0) == 0 and E.sc_of(0.0) == 1.0
    assert E.thr_of(0.5) == 32768 and E.sc_of(0.5) == 2.0
    assert E.thr_of(1.0 / 65536) == 1 and E.sc_of(1.0 / 65536) == 65536.0 / 65535
    assert E.thr_of(0.2) == 13107 and E.sc_of(0.2) != 1.0 / (1.0 - 0.2)
    # 0.999 is where 1 / (1 - p) and the realised scale differ by 0.7 %: more than a bf16 half ulp
    assert E.thr_of(0.999) == 65470 and abs(E.sc_of(0.999) / 1000.0 - 1.0) > 2.0 ** -8


def test_bf16_checker_on_torch_rne_casts():
    """Round-to-nearest-even of an fp32 value passes the bf16 check with a zero accumulation allowance and the two-term
    check as well; one bf16 ulp off fails; and a flat 2^-9 |x| is less than RNE itself needs."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(4096, generator=g) * torch.logspace(-3, 3, 4096)
    w[:3] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 2.0 - 2.0 ** -9])
    x = w.double()
    hi = w.bfloat16()
    zero = torch.zeros_like(x)
    assert E.bf16_error_ratio(hi, x, zero) <= 1.0
    lo = (w - hi.float()).bfloat16()
    assert E.two_term_error_ratio(hi, lo, x, zero) <= 1.0
    assert (lo.double().abs() <= 0.5 * E.bf16_ulp(hi.double())).all()
    off = (hi.view(torch.int16) + 1).view(torch.bfloat16)
    assert E.bf16_error_ratio(off, x, zero) > 1.0
    assert E.two_term_error_ratio(off, lo, x, zero) > 1.0
    # truncation instead of rounding is caught too
    trunc = (w.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    assert E.bf16_error_ratio(trunc, x, zero) > 1.0
    # the flat relative form: 1 + 2^-8 ties to 1.0, an error of 2^-8 -- twice 2^-9 |x|
    err = (hi.double() - x).abs()
    assert float(hi[0]) == 1.0 and err[0] == 2.0 ** -8
    assert (err > 2.0 ** -9 * x.abs()).any() and (err <= 2.0 ** -8 * x.abs()).all()


def test_expected_values_by_hand():
    c = E.case(1, 4, 64)
    keep = torch.tensor([[1, 0, 1, 0]], dtype=torch.uint8)
    x = E.expect_dropout(c, keep, 0.5, relu=True)
    assert x[0, 1] == 0 and x[0, 3] == 0
    assert x[0, 0] == 2.0 * max(float(c["v"][0, 0]), 0.0)
    r = E.expect_residual(c, keep, 0.5)
    assert r[0, 1] == c["res"][0, 1].double() and r[0, 2] == 2.0 * c["v"][0, 2] + c["res"][0, 2].double()
    m = E.expect_mask(c, -0.5)
    assert ((m == 0) | (m == -0.5 * c["v0"])).all()


def test_padded_buffer_bookkeeping():
    p = E.Padded(3, 5, torch.float32, 8, "cpu", base_off=4)
    assert p.view.shape == (3, 5) and p.view.stride(0) == 8 and p.intact() and p.untouched()
    p.view.fill_(1.0)
    assert p.intact() and not p.untouched()
    p.buf[4 + 5] = 0.0                       # first pad cell of row 0
    assert not p.intact()
    q = E.Padded(3, 5, torch.float32, 8, "cpu")
    q.buf[3 * 8] = 0.0                       # the extra row behind the view
    assert not q.intact()
