"""Plain definitions of the data-movement entries of include/pika_ops.h, torch on the CPU and no project kernel:
the virtual time-delay operand X(r, k) of include/pika_gemm.h, its transposed zero-padded copy (pika_transpose_cast), its
adjoint (pika_col2im), the two-term fp16 split (pika_split_bf16_terms, n_terms = 4) and the hi / lo bf16 planes
(PIKA_SPLIT_PAIR, n_terms = 2).  Every one of these is exact or a fixed-order float32 sum of at most `taps` terms, so the
GPU tests (tests/test_ops_kernels_gpu.py) compare bit for bit; tests/test_ops_refs.py checks each definition here against
a second formulation.  The shapes of both files live here, so that the two cover the same cases."""
import torch

F16_MAX = 65504.0

# pika_transpose_cast of a plain matrix: rows x K around the 64 x 64 tile
PLAIN_SHAPES = [(1, 4), (63, 64), (64, 65), (65, 63), (130, 200)]
# time-delay views (taps, dil, stride, pad, B, T, C): rows_per_batch and taps * C are no multiples of 64, so one 64-row
# tile crosses a batch boundary and the last tile of the reduction is partial; the last one is causal (ti < 0 reads zero)
TD_CASES = [(3, 1, 1, 0, 3, 25, 24), (3, 3, 1, 0, 3, 30, 20), (3, 3, 4, 0, 2, 61, 8), (5, 1, 1, 4, 3, 23, 12)]
# pika_col2im on top of those: the identity, and stride 2 under 3 taps (input frames hit by 1 or 2 taps alternately)
COL2IM_CASES = TD_CASES + [(1, 1, 1, 0, 2, 9, 8), (3, 1, 2, 0, 2, 17, 8)]
# a view with as many rows per batch as input frames: the last taps of the last rows run past t_in and read zero
# (taps, dil, stride, pad, B, T, C, rows_per_batch)
OVERRUN_CASE = (3, 2, 1, 0, 3, 21, 12, 21)


def t_out_of(T, taps, dil, stride, pad):
    """Output frames of a time-delay layer (pika_amd.gemm.time_delay): causal layers (pad > 0) keep T."""
    return T if pad else (T - dil * (taps - 1) - 1) // stride + 1


def strided_source(B, T, C, seed, dtype=torch.float32):
    """(source, view): a (B, T, C) view with unit inner stride into a source whose row pitch (C + 8) and batch stride
    ((T + 2) rows) are larger than the view needs; what lies outside the view is NaN."""
    g = torch.Generator().manual_seed(seed)
    src = torch.full((B, T + 2, C + 8), float("nan"))
    src[:, :T, :C] = torch.randn(B, T, C, generator=g) * (1.0 + torch.arange(C) / C)
    src = src.to(dtype)
    return src, src[:, :T, :C]


def ref_time_delay(x, taps, dil, stride, pad, rows_per_batch):
    """X(r, k) of include/pika_gemm.h as a (B * rows_per_batch, taps * C) matrix over x (B, t_in, C), by explicit indexing:
    b = r // rows_per_batch, t = r % rows_per_batch, tap = k // C, c = k % C, ti = t * stride + tap * dil - pad, zero outside
    [0, t_in)."""
    B, t_in, C = x.shape
    r = torch.arange(B * rows_per_batch).unsqueeze(1)
    k = torch.arange(taps * C).unsqueeze(0)
    b, t = r // rows_per_batch, r % rows_per_batch
    tap, c = k // C, k % C
    ti = t * stride + tap * dil - pad
    inside = (ti >= 0) & (ti < t_in)
    val = x[b, ti.clamp(0, t_in - 1), c]
    return torch.where(inside, val, torch.zeros((), dtype=x.dtype))


def ref_transpose_cast(x, taps, dil, stride, pad, rows_per_batch, rows, ld_out, out_dtype):
    """X^T as a (taps * C, ld_out) matrix of out_dtype with zeros in columns [rows, ld_out); the bf16 cast rounds to
    nearest even."""
    X = ref_time_delay(x.float(), taps, dil, stride, pad, rows_per_batch)[:rows]
    out = torch.zeros(X.shape[1], ld_out, dtype=torch.float32)
    out[:, :rows] = X.t()
    return out.to(out_dtype)


def ref_col2im(dcol, B, t_out, t_in, C, taps, stride, dil, pad, dtype=torch.float32):
    """dx[b, ti, c] = sum over tap = 0 .. taps - 1, in that order and from 0.0, of dcol[(b, t)][tap * C + c] where
    t * stride + tap * dil - pad == ti and t < t_out; in `dtype` (float32: the kernel's own order, hence its bits)."""
    d = dcol.to(dtype).reshape(B, t_out, taps, C)
    dx = torch.zeros(B, t_in, C, dtype=dtype)
    ti = torch.arange(t_in)
    for tap in range(taps):
        num = ti + pad - tap * dil
        hit = (num >= 0) & (num % stride == 0) & (num // stride < t_out)
        dx[:, ti[hit]] = dx[:, ti[hit]] + d[:, num[hit] // stride, tap]
    return dx


def col2im_bound(dcol, B, t_out, t_in, C, taps, stride, dil, pad):
    """taps * 2^-24 * sum |terms| per element of dx, float64: `taps` float32 additions, each within 2^-24 of a partial
    sum that never exceeds the sum of the magnitudes."""
    return taps * 2.0 ** -24 * ref_col2im(dcol.double().abs(), B, t_out, t_in, C, taps, stride, dil, pad, torch.float64)


def ref_split_f16(x, role):
    """The fp16 split of include/pika_ops.h (n_terms = 4).  role 0 (A side): (hi, 32 lo, hi / 64); role 1 (B side):
    (hi, hi / 32, 64 lo); "pair": (hi, 2^11 lo).  Conversions are IEEE round-to-nearest-even with subnormals."""
    x_ = x.float().clamp(-F16_MAX, F16_MAX)
    hi = x_.half()
    lo = x_ - hi.float()
    if role == "pair":
        return hi, (lo * 2048.0).half()
    if role == 0:
        return hi, (lo * 32.0).half(), (hi.float() / 64.0).half()
    if role == 1:
        return hi, (hi.float() / 32.0).half(), (lo * 64.0).half()
    raise ValueError(role)


def ref_split_pair_bf16(x):
    """t0 = bf16(x), t1 = bf16(x - t0): the hi / lo planes of PIKA_SPLIT_PAIR with n_terms = 2."""
    t0 = x.bfloat16()
    return t0, (x - t0.float()).bfloat16()


F16_EXACT = [1.0, -0.375, 1000.0, 0.125, 1023.5, -3.0, 512.0, 0.1669921875]       # lo = 0


def f16_split_inputs(n, seed):
    """n float32 values for the fp16 split: |x| log-uniform in [2^-3, 2^10) with random signs, every residual either zero
    or large enough that 32 lo is a normal fp16 number (the subnormal range has a case of its own), and, spread over the
    set: exact zeros, +-65504, 1e5, -1e5 (saturation) and values that fp16 holds exactly."""
    g = torch.Generator().manual_seed(seed)
    x = torch.exp2(torch.rand(n, generator=g) * 13.0 - 3.0) * (torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0)
    hi = x.half().float()
    lo = x - hi
    x = torch.where((lo != 0) & (lo.abs() * 32.0 < 2.0 ** -14), hi, x)
    special = [0.0, 0.0, F16_MAX, -F16_MAX, 1e5, -1e5] + F16_EXACT
    assert n > 31 * len(special)
    for i, v in enumerate(special):
        x[31 * i + 5] = v
    return x


def f16_subnormal_inputs():
    """32 values whose scaled residuals, hi / 32 and hi / 64, or hi itself, fall into fp16's subnormal range: hand-picked
    ties and boundaries and a log-uniform fill of [2^-27, 2^-2)."""
    picked = [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -14, 2.0 ** -14 * (1 + 2.0 ** -11),
              0.125 + 2.0 ** -26, -(0.125 + 2.0 ** -21), 2.0 ** -9, 2.0 ** -9 * (1 + 2.0 ** -10), 3.0 * 2.0 ** -20, -1e-5]
    g = torch.Generator().manual_seed(77)
    fill = torch.exp2(torch.rand(32 - len(picked), generator=g) * 25.0 - 27.0)
    fill = fill * (torch.randint(0, 2, fill.shape, generator=g) * 2.0 - 1.0)
    return torch.cat([torch.tensor(picked, dtype=torch.float32), fill])
