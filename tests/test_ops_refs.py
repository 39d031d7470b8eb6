"""The definitions of tests/ops_common.py without a GPU, each against a second formulation of the same operation, so that
the yardsticks of tests/test_ops_kernels_gpu.py cannot be wrong together with the kernels: the time-delay operand as a
concatenation of shifted slices, col2im as the float64 autograd adjoint of that operand, the float32 tap-ordered sum
inside its derived distance from float64, the fp16 split's reconstruction, its segment pairing and its saturation; and
the argument checks of the C entries, by return code, before any launch."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ops_common as OC  # noqa: E402

ALL_VIEWS = [c + (OC.t_out_of(c[5], *c[:4]),) for c in OC.COL2IM_CASES] + [OC.OVERRUN_CASE]


def shifted_slices(x, taps, dil, stride, pad, rows_per_batch):
    """The operand as model code writes it: left pad (and as many zero frames on the right as the last row asks for),
    one strided slice per tap, concatenated along the channels."""
    B, T, C = x.shape
    need = (rows_per_batch - 1) * stride + (taps - 1) * dil + 1
    xp = F.pad(x, (0, 0, pad, max(0, need - (T + pad))))
    cols = [xp[:, j * dil: j * dil + (rows_per_batch - 1) * stride + 1: stride, :] for j in range(taps)]
    return torch.cat(cols, -1).reshape(B * rows_per_batch, taps * C)


@pytest.mark.parametrize("taps,dil,stride,pad,B,T,C,rpb", ALL_VIEWS)
def test_time_delay_is_the_concatenation_of_shifted_slices(taps, dil, stride, pad, B, T, C, rpb):
    _, x = OC.strided_source(B, T, C, seed=taps + 10 * dil + 100 * stride)
    got = OC.ref_time_delay(x, taps, dil, stride, pad, rpb)
    assert got.shape == (B * rpb, taps * C) and not got.isnan().any()          # nothing outside the view was read
    assert torch.equal(got, shifted_slices(x, taps, dil, stride, pad, rpb))
    if (taps, dil, stride, pad, B, T, C, rpb) == OC.OVERRUN_CASE:
        assert (got.view(B, rpb, taps, C)[:, -1, -1] == 0).all()                 # the case does run past t_in


@pytest.mark.parametrize("rows,K", OC.PLAIN_SHAPES)
def test_plain_matrix_is_the_one_tap_view_and_transpose_cast_pads_with_zeros(rows, K):
    _, x = OC.strided_source(1, rows, K, seed=rows * K)
    assert torch.equal(OC.ref_time_delay(x, 1, 1, 1, 0, rows), x[0])
    ld = (rows + 3) & ~3
    for dt in (torch.float32, torch.bfloat16):
        out = OC.ref_transpose_cast(x, 1, 1, 1, 0, rows, rows, ld + 8, dt)
        assert out.shape == (K, ld + 8) and out.dtype == dt
        assert torch.equal(out[:, :rows], x[0].t().to(dt)) and (out[:, rows:] == 0).all()


@pytest.mark.parametrize("taps,dil,stride,pad,B,T,C", OC.COL2IM_CASES)
def test_col2im_is_the_adjoint_of_the_time_delay_operand(taps, dil, stride, pad, B, T, C):
    t_out = OC.t_out_of(T, taps, dil, stride, pad)
    g = torch.Generator().manual_seed(T)
    dcol = torch.randn(B * t_out, taps * C, generator=g, dtype=torch.float64)
    x = torch.randn(B, T, C, generator=g, dtype=torch.float64, requires_grad=True)
    (OC.ref_time_delay(x, taps, dil, stride, pad, t_out) * dcol).sum().backward()
    ref64 = OC.ref_col2im(dcol, B, t_out, T, C, taps, stride, dil, pad, torch.float64)
    sum_abs = OC.ref_col2im(dcol.abs(), B, t_out, T, C, taps, stride, dil, pad, torch.float64)
    # two float64 sums of the same <= taps terms in two orders
    assert ((x.grad - ref64).abs() <= taps * 2.0 ** -53 * sum_abs).all()
    # the float32 tap-ordered form: `taps` additions, each within 2^-24 of a partial sum bounded by sum |terms|
    d32 = dcol.float()
    ref32 = OC.ref_col2im(d32, B, t_out, T, C, taps, stride, dil, pad)
    assert ref32.dtype == torch.float32
    bound = OC.col2im_bound(d32, B, t_out, T, C, taps, stride, dil, pad)
    exact = OC.ref_col2im(d32, B, t_out, T, C, taps, stride, dil, pad, torch.float64)
    assert ((ref32.double() - exact).abs() <= bound).all()
    # frames that no (t, tap) reaches are exact zeros in both, and the stride-4 case has some
    unreached = sum_abs == 0
    assert (ref32[unreached] == 0).all() and bool(unreached.any()) == (stride == 4)


def test_fp16_split_reconstructs_x_to_22_bits():
    g = torch.Generator().manual_seed(1)
    x = torch.exp2(torch.rand(4096, generator=g) * 29.99 - 14.0) * (torch.randint(0, 2, (4096,), generator=g) * 2.0 - 1.0)
    x[:3] = torch.tensor([2.0 ** -14, OC.F16_MAX, -OC.F16_MAX])
    assert x.abs().min() >= 2.0 ** -14 and x.abs().max() <= OC.F16_MAX         # fp16's normal range
    hi, lo_p = OC.ref_split_f16(x, "pair")
    assert hi.dtype == torch.float16 and lo_p.dtype == torch.float16
    back = hi.double() + lo_p.double() / 2048.0
    assert ((back - x.double()).abs() <= 2.0 ** -22 * x.double().abs()).all()
    # and hi alone does not: the second term is what carries bits 12 .. 22
    assert ((hi.double() - x.double()).abs() > 2.0 ** -13 * x.double().abs()).any()
    # the A and B sides carry the same two terms under their own factors
    for role, (i_lo, f_lo, i_hi, f_hi) in ((0, (1, 32.0, 2, 1 / 64.0)), (1, (2, 64.0, 1, 1 / 32.0))):
        segs = OC.ref_split_f16(x, role)
        assert torch.equal(segs[0], hi)
        big = x.abs() >= 2.0 ** -3            # above it neither scaled term is subnormal unless lo is tiny
        assert torch.equal(segs[i_hi].double()[big], hi.double()[big] * f_hi)
        lo = x.double() - hi.double()
        normal = big & (lo.abs() * 32.0 >= 2.0 ** -14)
        assert ((segs[i_lo].double()[normal] / f_lo - lo[normal]).abs() <= 2.0 ** -11 * lo[normal].abs()).all()


def round_to_11_bits(v):
    """v (float64) rounded to nearest even at 11 significant bits, unbounded exponent: fp16's rounding without its range."""
    m, e = torch.frexp(v)
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)


def test_fp16_split_segments_pair_up_to_the_three_kept_products():
    a = OC.f16_split_inputs(1024, seed=2)
    b = OC.f16_split_inputs(1024, seed=3).flip(0)
    A, B = OC.ref_split_f16(a, 0), OC.ref_split_f16(b, 1)
    total = sum(sa.double() * sb.double() for sa, sb in zip(A, B))            # what the K-concatenated product adds up

    def terms(x):
        x_ = x.double().clamp(-OC.F16_MAX, OC.F16_MAX)
        hi = round_to_11_bits(x_)
        return hi, round_to_11_bits(x_ - hi)
    (ha, la), (hb, lb) = terms(a), terms(b)
    assert torch.equal(ha, A[0].double()) and torch.equal(hb, B[0].double())
    # fp16 x fp16 products are exact in float64 and the power-of-two factors cancel exactly in each, so both sides add
    # the same three numbers in the same order -- unless two segments of one side are swapped or a factor is off
    assert torch.equal(total, ha * hb + la * hb + ha * lb)
    assert bool((la != 0).any()) and bool((la == 0).any())


def test_fp16_split_saturates_at_the_largest_fp16():
    x = torch.tensor([1e5, -1e5, float("inf"), -float("inf"), OC.F16_MAX, 65520.0])
    sign = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, 1.0], dtype=torch.float64)
    hi, lo_p = OC.ref_split_f16(x, "pair")
    assert torch.equal(hi.double(), sign * OC.F16_MAX) and (lo_p == 0).all()
    a, b = OC.ref_split_f16(x, 0), OC.ref_split_f16(x, 1)
    assert (a[1] == 0).all() and (b[2] == 0).all()
    assert torch.equal(a[2].double(), sign * 1023.5) and torch.equal(b[1].double(), sign * 2047.0)


def test_bf16_pair_is_the_first_two_of_three_exact_terms():
    x = OC.f16_split_inputs(1024, seed=4)
    t0, t1 = OC.ref_split_pair_bf16(x)
    assert t0.dtype == torch.bfloat16 and t1.dtype == torch.bfloat16
    rest = x.double() - t0.double() - t1.double()
    assert (rest.abs() <= 2.0 ** -16 * x.double().abs()).all()               # 8 + 8 bits taken
    assert torch.equal(rest.float().bfloat16().double(), rest)                # and the rest fits a third bf16 term


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from pika_amd import _lib
    from pika_amd import gemm as G
    lib = _lib.lib()
    EINVAL = -1
    CONCAT, STACK, PAIR = 0, 1, 2
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15                                     # a 16-byte aligned host address

    def split(C=8, Cp=8, role=0, n_terms=2, layout=CONCAT, dst=p, x=p, ld=8, bs=0):
        return lib.pika_split_bf16_terms(x, 1, 1, C, bs, ld, role, n_terms, layout, Cp, dst, None)

    assert split(x=None) == EINVAL and split(dst=None) == EINVAL
    assert split(n_terms=4, layout=STACK) == EINVAL                            # the fp16 split has no stacked form
    assert split(n_terms=3, layout=PAIR) == EINVAL and split(n_terms=5) == EINVAL
    assert split(layout=3) == EINVAL and split(role=2) == EINVAL
    assert split(C=16, Cp=8) == EINVAL and split(C=8, Cp=12) == EINVAL         # Cp < C; Cp % 8
    assert split(C=8, Cp=16, layout=STACK) == EINVAL                           # the stacked layout has no pad columns
    assert split(C=12, Cp=16) == EINVAL and split(ld=6) == EINVAL and split(bs=2) == EINVAL
    assert split(dst=p + 2) == EINVAL and split(dst=p + 8) == EINVAL and split(x=p + 4) == EINVAL     # misaligned

    def job(**kw):
        a = dict(x=p, n_batch=1, t_in=1, C=8, batch_stride=0, ld=8, role=0, n_terms=2, layout=CONCAT, Cp=8, dst=p)
        a.update(kw)
        return G.SplitJob(*[a[name] for name, _ in G.SplitJob._fields_])

    def two(ja, jb):
        return lib.pika_split_bf16_terms2(None if ja is None else ctypes.byref(ja), None if jb is None else ctypes.byref(jb),
                                          None)

    assert two(None, job()) == EINVAL and two(job(), None) == EINVAL
    assert two(job(n_terms=2), job(n_terms=3)) == EINVAL and two(job(n_terms=4), job(n_terms=2)) == EINVAL
    assert two(job(layout=CONCAT), job(layout=STACK)) == EINVAL and two(job(layout=PAIR), job(layout=CONCAT)) == EINVAL
    assert two(job(), job(dst=p + 2)) == EINVAL and two(job(Cp=4), job()) == EINVAL      # either job's own checks
    assert two(job(n_terms=4, layout=STACK), job(n_terms=4, layout=STACK)) == EINVAL

    def tcast(rows=4, K=8, ld_out=4, out_dtype=G.PIKA_F32, out=p, **kw):
        f = dict(ptr=p, dtype=G.PIKA_F32, rows_per_batch=4, t_in=4, batch_stride=0, ld=8, C=8, stride=1, dil=1, pad=0)
        f.update(kw)
        op = G.Operand(f["ptr"], f["dtype"], f["rows_per_batch"], f["t_in"], f["batch_stride"], f["ld"], f["C"], f["stride"],
                       f["dil"], f["pad"], 0, 0)
        return lib.pika_transpose_cast(ctypes.byref(op), rows, K, out, ld_out, out_dtype, None)

    assert tcast(ld_out=3) == EINVAL                                           # ld_out < rows
    assert tcast(stride=0) == EINVAL and tcast(stride=-1) == EINVAL
    assert tcast(rows_per_batch=0) == EINVAL and tcast(C=0) == EINVAL
    assert tcast(rows=0) == EINVAL and tcast(K=0) == EINVAL and tcast(out=None) == EINVAL and tcast(ptr=None) == EINVAL
    assert tcast(out_dtype=2) == EINVAL                                        # neither f32 nor bf16
    assert lib.pika_transpose_cast(None, 4, 8, p, 4, G.PIKA_F32, None) == EINVAL

    def col2im(dcol=p, dx=p, B=1, t_out=1, t_in=1, C=8, taps=1, stride=1):
        return lib.pika_col2im(dcol, dx, B, t_out, t_in, C, taps, stride, 1, 0, None)

    assert col2im(stride=0) == EINVAL and col2im(taps=0) == EINVAL and col2im(B=0) == EINVAL
    assert col2im(t_out=0) == EINVAL and col2im(t_in=0) == EINVAL and col2im(C=0) == EINVAL
    assert col2im(dcol=None) == EINVAL and col2im(dx=None) == EINVAL
