"""The data-movement entries of include/pika_ops.h called one by one through the C ABI, bit for bit against the plain
definitions of tests/ops_common.py: pika_transpose_cast (plain, bf16-source and time-delay operands around the 64 x 64
tile, the zero-filled columns up to ld_out), pika_col2im (float32 tap order, the derived distance from float64, the adjoint
identity with pika_transpose_cast's own view), the fp16 split (n_terms = 4: both CONCAT roles and the PAIR form,
saturation, the subnormal range), the bf16 hi / lo planes (PIKA_SPLIT_PAIR, n_terms = 2) and the two-job launch
pika_split_bf16_terms2.  Every output is NaN before the call and lies between NaN guards that must stay NaN; none of the
entries takes an output pitch, so the guards are the elements before and after the output, and the pad columns inside it
are part of what is compared."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ops_common as OC  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                     # elements on either side: 128 bytes at least, so the output keeps its 16-byte alignment
CONCAT, STACK, PAIR = 0, 1, 2


class Guarded(object):
    """`n` elements of `dtype` on the device, NaN, between two NaN guards."""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        assert self.ptr % 16 == 0

    def read(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool(host[:GUARD].isnan().all()) and bool(host[GUARD + self.n:].isnan().all()), "a guard was overwritten"
        return host[GUARD:GUARD + self.n]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from pika_amd import _lib as L
    return L, L.lib()


def same_bits(a, b):
    """Equal as bit patterns (16-bit types): what two runs of one kernel must be."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- pika_transpose_cast ----

def transpose_cast(op, rows, K, ld_out, out_dtype, dev):
    from pika_amd import gemm as G
    L, lib = _lib()
    out = Guarded(K * ld_out, out_dtype, dev)
    L.check(lib.pika_transpose_cast(ctypes.byref(op), rows, K, out.ptr, ld_out,
                                    G.PIKA_F32 if out_dtype == torch.float32 else G.PIKA_BF16, _st()), "pika_transpose_cast")
    return out.read().view(K, ld_out)


def check_plain(rows, K, ld_out, src_dtype, dev):
    from pika_amd import gemm as G
    src, x = OC.strided_source(1, rows, K, seed=rows * 1000 + K, dtype=src_dtype)
    d = src.to(dev)
    op, r_, k_ = G.matrix(d[0, :rows, :K])                      # pitch K + 8
    assert (r_, k_) == (rows, K) and op.ld == K + 8
    for out_dtype in (torch.float32, torch.bfloat16):
        got = transpose_cast(op, rows, K, ld_out, out_dtype, dev)
        want = OC.ref_transpose_cast(x, 1, 1, 1, 0, rows, rows, ld_out, out_dtype)
        assert torch.equal(got, want), (rows, K, ld_out, src_dtype, out_dtype)


@pytest.mark.parametrize("rows,K", OC.PLAIN_SHAPES)
def test_transpose_cast_plain(hip_device, rows, K):
    check_plain(rows, K, (rows + 3) & ~3, torch.float32, hip_device)


def test_transpose_cast_zero_fills_whole_tiles_beyond_the_rows(hip_device):
    """rows = 64, ld_out = 132: the zero columns are all of a second 64-row tile and part of a third -- the grid follows
    ld_out, not rows."""
    check_plain(64, 65, 132, torch.float32, hip_device)


@pytest.mark.parametrize("rows,K", [(65, 63), (130, 200)])
def test_transpose_cast_bf16_source(hip_device, rows, K):
    check_plain(rows, K, (rows + 3) & ~3, torch.bfloat16, hip_device)


def check_view(op, x, taps, dil, stride, pad, rpb, B, C, dev):
    rows, K = B * rpb, taps * C
    ld_out = ((rows + 3) & ~3) + 4                              # a few zero columns whatever rows is
    for out_dtype in (torch.float32, torch.bfloat16):
        got = transpose_cast(op, rows, K, ld_out, out_dtype, dev)
        want = OC.ref_transpose_cast(x, taps, dil, stride, pad, rpb, rows, ld_out, out_dtype)
        assert torch.equal(got, want), (taps, dil, stride, pad, out_dtype)


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("taps,dil,stride,pad,B,T,C", OC.TD_CASES)
def test_transpose_cast_time_delay_view(hip_device, taps, dil, stride, pad, B, T, C, src_dtype):
    from pika_amd import gemm as G
    src, x = OC.strided_source(B, T, C, seed=taps + 10 * dil + 100 * stride, dtype=src_dtype)
    d = src.to(hip_device)
    op, M, K, t_out = G.time_delay(d[:, :T, :C], taps, dil, stride, pad)
    assert t_out == OC.t_out_of(T, taps, dil, stride, pad) and (M, K) == (B * t_out, taps * C)
    assert t_out % 64 and K % 64 and op.ld == C + 8 and op.batch_stride == (T + 2) * (C + 8)
    check_view(op, x, taps, dil, stride, pad, t_out, B, C, hip_device)


def test_transpose_cast_taps_past_the_last_frame_read_zero(hip_device):
    from pika_amd import gemm as G
    taps, dil, stride, pad, B, T, C, rpb = OC.OVERRUN_CASE
    src, x = OC.strided_source(B, T, C, seed=8)
    d = src.to(hip_device)
    # t_in is the true length: (rpb - 1) * stride + (taps - 1) * dil >= T, and those elements are zero by definition
    assert (rpb - 1) * stride + (taps - 1) * dil >= T
    op = G.Operand(d.data_ptr(), G.PIKA_F32, rpb, T, d.stride(0), d.stride(1), C, stride, dil, pad, 0, 0)
    check_view(op, x, taps, dil, stride, pad, rpb, B, C, hip_device)


# ---- pika_col2im ----

def col2im(dcol_dev, B, t_out, T, C, taps, stride, dil, pad, dev):
    L, lib = _lib()
    assert dcol_dev.is_contiguous() and dcol_dev.dtype == torch.float32 and dcol_dev.numel() == B * t_out * taps * C
    dx = Guarded(B * T * C, torch.float32, dev)
    L.check(lib.pika_col2im(dcol_dev.data_ptr(), dx.ptr, B, t_out, T, C, taps, stride, dil, pad, _st()), "pika_col2im")
    return dx.read().view(B, T, C)


@pytest.mark.parametrize("taps,dil,stride,pad,B,T,C", OC.COL2IM_CASES)
def test_col2im(hip_device, taps, dil, stride, pad, B, T, C):
    from pika_amd import gemm as G
    t_out = OC.t_out_of(T, taps, dil, stride, pad)
    args = (B, t_out, T, C, taps, stride, dil, pad)
    g = torch.Generator().manual_seed(T * 7 + taps)
    dcol = torch.randn(B * t_out, taps * C, generator=g)
    got = col2im(dcol.to(hip_device), *args, hip_device)
    assert torch.equal(got, OC.ref_col2im(dcol, *args)), args                  # the kernel's own order: its bits
    ref64 = OC.ref_col2im(dcol, *args, torch.float64)
    bound = OC.col2im_bound(dcol, *args)
    assert bool(((got.double() - ref64).abs() <= bound).all()), args
    unreached = bound == 0                                                     # randn: no term is zero
    assert bool((got[unreached] == 0).all()) and bool(unreached.any()) == (stride == 4)
    if (taps, stride) == (1, 1):
        assert torch.equal(got, dcol.view(B, T, C))                            # the identity

    # one definition of the operand for both kernels: <X, dcol> == <x, col2im(dcol)> with dcol = X as
    # pika_transpose_cast sees a random x, both sides in float64 from the two device outputs.  The right side inherits
    # the float32 sums' distance from their exact values, |x| times the bound above, summed (the float64 dot products
    # themselves are 2^-29 of that)
    src, x = OC.strided_source(B, T, C, seed=T)
    d = src.to(hip_device)
    op, M, K, _ = G.time_delay(d[:, :T, :C], taps, dil, stride, pad)
    ld = (M + 3) & ~3
    X = transpose_cast(op, M, K, ld, torch.float32, hip_device)[:, :M].t().contiguous()
    dx = col2im(X.to(hip_device), *args, hip_device)
    lhs = (X.double() * X.double()).sum()
    rhs = (x.double() * dx.double()).sum()
    allow = (x.double().abs() * OC.col2im_bound(X, *args)).sum()
    assert abs(lhs.item() - rhs.item()) <= allow.item(), (lhs.item(), rhs.item(), allow.item())


# ---- pika_split_bf16_terms ----

def split(x_dev, nb, t_in, C, role, n_terms, layout, Cp, dev):
    """One split of the (nb, t_in, C) view x_dev (unit inner stride); the output as a flat bf16 tensor on the host."""
    L, lib = _lib()
    nseg = 2 if layout == PAIR else (6 if n_terms == 3 else 3)
    dst = Guarded(nseg * nb * t_in * Cp, torch.bfloat16, dev)
    L.check(lib.pika_split_bf16_terms(x_dev.data_ptr(), nb, t_in, C, x_dev.stride(0), x_dev.stride(1), role, n_terms, layout,
                                      Cp, dst.ptr, _st()), "pika_split_bf16_terms")
    return dst.read()


def batched_source(x_flat, nb, t_in, C, dev):
    """x_flat's values as an (nb, t_in, C) view with pitch C + 16 and a batch stride of t_in + 2 rows, NaN around it."""
    src = torch.full((nb, t_in + 2, C + 16), float("nan"))
    src[:, :t_in, :C] = x_flat.view(nb, t_in, C)
    return src.to(dev)[:, :t_in, :C]


def check_f16_split(x_flat, nb, t_in, C, Cp_pad, dev):
    x = x_flat.view(nb, t_in, C)
    xd = batched_source(x_flat, nb, t_in, C, dev)
    for role in (0, 1):                                                        # CONCAT, Cp > C
        got = split(xd, nb, t_in, C, role, 4, CONCAT, Cp_pad, dev).view(torch.float16).view(nb, t_in, 3, Cp_pad)
        for s_, want in enumerate(OC.ref_split_f16(x, role)):
            assert torch.equal(got[:, :, s_, :C], want), (role, s_)
            assert bool((got[:, :, s_, C:] == 0).all()), (role, s_)
    for Cp in (C, Cp_pad):                                                     # PAIR: planes (2, nb, t_in, Cp)
        got = split(xd, nb, t_in, C, 0, 4, PAIR, Cp, dev).view(torch.float16).view(2, nb, t_in, Cp)
        for s_, want in enumerate(OC.ref_split_f16(x, "pair")):
            assert torch.equal(got[s_, :, :, :C], want), (Cp, s_)
            assert bool((got[s_, :, :, C:] == 0).all()), (Cp, s_)


def test_fp16_split(hip_device):
    nb, t_in, C = 3, 7, 24
    x = OC.f16_split_inputs(nb * t_in * C, seed=11)
    lo32 = OC.ref_split_f16(x, 0)[1].float().abs()
    assert bool(((lo32 == 0) | (lo32 >= 2.0 ** -14)).all())                    # this set stays out of the subnormal range
    check_f16_split(x, nb, t_in, C, 64, hip_device)


def test_fp16_split_in_the_subnormal_range(hip_device):
    """Scaled residuals, hi / 32, hi / 64 and hi itself below 2^-14: the yardstick converts as IEEE 754 does, to nearest
    even with gradual underflow, and so does the device (v_cvt_f16_f32 under the kernels' default mode, which keeps fp16
    subnormals)."""
    x = OC.f16_subnormal_inputs()
    segs = [s.float().abs() for role in (0, 1, "pair") for s in OC.ref_split_f16(x, role)]
    assert all(bool(((s > 0) & (s < 2.0 ** -14)).any()) for s in segs)          # every segment does go subnormal
    check_f16_split(x, 1, 2, 16, 24, hip_device)


def test_bf16_pair_planes(hip_device):
    """PIKA_SPLIT_PAIR with n_terms = 2: plane 0 = bf16(x), plane 1 = bf16(x - t0) at n_batch * t_in * Cp elements, pad
    columns zero."""
    nb, t_in, C = 3, 7, 24
    g = torch.Generator().manual_seed(12)
    x_flat = torch.randn(nb * t_in * C, generator=g) * torch.exp2(torch.randint(-6, 7, (nb * t_in * C,), generator=g).float())
    x_flat[::41] = 0.0
    x = x_flat.view(nb, t_in, C)
    xd = batched_source(x_flat, nb, t_in, C, hip_device)
    t0, t1 = OC.ref_split_pair_bf16(x)
    for Cp in (C, 64):
        flat = split(xd, nb, t_in, C, 0, 2, PAIR, Cp, hip_device)
        lo_off = nb * t_in * Cp
        for off, want in ((0, t0), (lo_off, t1)):
            plane = flat[off:off + lo_off].view(nb, t_in, Cp)
            assert torch.equal(plane[:, :, :C], want), (Cp, off)
            assert bool((plane[:, :, C:] == 0).all()), (Cp, off)


# ---- pika_split_bf16_terms2 ----

@pytest.mark.parametrize("n_terms,layout", [(2, CONCAT), (3, STACK), (4, PAIR)])
def test_two_jobs_in_one_launch(hip_device, n_terms, layout):
    """A job of more than 256 granules (two workgroups) and one of fewer in one launch, in both orders: each destination
    holds the bits of the same job done alone, and its guards stay NaN."""
    from pika_amd import gemm as G
    L, lib = _lib()
    nseg = 2 if layout == PAIR else (6 if n_terms == 3 else 3)
    big = dict(nb=3, t_in=30, C=32, Cp=32 if layout == STACK else 40, role=0)     # 360 / 450 granules
    small = dict(nb=2, t_in=5, C=8, Cp=8 if layout == STACK else 16, role=1)      # 10 / 20 granules
    for j, seed in ((big, 21), (small, 22)):
        j["gran"] = j["nb"] * j["t_in"] * (j["Cp"] // 8)
        g = torch.Generator().manual_seed(seed)
        n = j["nb"] * j["t_in"] * j["C"]
        flat = OC.f16_split_inputs(n, seed) if n >= 600 else torch.randn(n, generator=g) * 8.0
        j["x"] = batched_source(flat, j["nb"], j["t_in"], j["C"], hip_device)
        j["alone"] = split(j["x"], j["nb"], j["t_in"], j["C"], j["role"], n_terms, layout, j["Cp"], hip_device)
        assert not bool(j["alone"].view(torch.float16 if n_terms == 4 else torch.bfloat16).isnan().any())
    assert big["gran"] > 256 and small["gran"] < 256
    for first, second in ((big, small), (small, big)):
        dsts, jobs = [], []
        for j in (first, second):
            dst = Guarded(nseg * j["nb"] * j["t_in"] * j["Cp"], torch.bfloat16, hip_device)
            dsts.append(dst)
            jobs.append(G.SplitJob(j["x"].data_ptr(), j["nb"], j["t_in"], j["C"], j["x"].stride(0), j["x"].stride(1), j["role"],
                                   n_terms, layout, j["Cp"], dst.ptr))
        L.check(lib.pika_split_bf16_terms2(ctypes.byref(jobs[0]), ctypes.byref(jobs[1]), _st()), "pika_split_bf16_terms2")
        for j, dst in zip((first, second), dsts):
            assert same_bits(dst.read(), j["alone"]), (n_terms, layout, j["gran"])
