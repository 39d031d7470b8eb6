"""The fused epilogues of the direct-to-LDS bf16 GEMM (include/pika_gemm.h: pika_gemm_bf16_epilogue,
pika_gemm_bf16_dropout_residual, pika_gemm_bf16_ex, pika_dropout_mask_cast_bf16) as plain float64 formulas, the element-wise
error bounds they are held to, and the tables of shapes.  Nothing here needs a GPU: tests/test_gemm_epilogue_refs.py checks
the formulas, the bounds and the tables on their own, tests/test_gemm_epilogue_gpu.py runs the kernels against them.

Why the bounds are element-wise and derived: the operands are bf16 values, so every product a*b is exact in fp32 (8 x 8
significand bits) and A B^T + bias in float64 is exact up to float64 rounding.  What the kernel adds before its final
rounding is the fp32 accumulation alone (`acc_bound`), then one documented rounding per output format.  No max-norm
tolerance appears anywhere.
"""
import functools
import math

import numpy as np
import torch

EINVAL = -1
EPI_F32, EPI_DROPOUT_BF16, EPI_MASK_BF16, EPI_DROPOUT_RESIDUAL = 0, 1, 2, 3

# output tile and K-tile of gemm_pp (pika_amd/csrc/gemm_glds.hip: "256 x 256 x 64"); the shapes below sit on their edges
TILE_M, TILE_N, TILE_K = 256, 256, 64
#   (1, 4, 64)      one row, one group of four columns, one K-tile
#   (255, 252, 64)  one tile, one short of full in both directions
#   (257, 260, 128) an interior tile, a 4-column edge tile, a 1-row tile
#   (300, 258, 192) N % 4 != 0: the last group of four columns is half outside
#   (513, 520, 64)  three row tiles, two interior column tiles and an 8-column edge
SHAPES = [(1, 4, 64), (255, 252, 64), (257, 260, 128), (300, 258, 192), (513, 520, 64)]
STORE_PATH_SHAPES = [(257, 260, 128), (513, 520, 64)]
# time-delay A operands: (dil, stride, pad, T) with C = 64, taps = 3, batch 3; 3 * t_out = 270 rows cross a tile edge and the
# first tile holds rows of all three batches
TD_C, TD_TAPS, TD_BATCH, TD_N = 64, 3, 3, 260
TD_CASES = [(2, 1, 0, 94), (1, 2, 0, 181), (1, 1, 2, 90)]
MASK_CAST_SHAPES = [(1, 4), (257, 260), (33, 1024)]

U32 = 2.0 ** -23          # one whole fp32 ulp (relative), see acc_bound
TINY_BF16 = 2.0 ** -126   # smallest positive normal bf16


def round_up(n, k):
    return (n + k - 1) // k * k


# ---- dropout constants ---------------------------------------------------------------------------------------------
def thr_of(p):
    """The 16-bit drop threshold round(p * 65536) of the float32 argument p_drop (ties to even, as lrintf)."""
    return int(np.rint(np.float32(p) * np.float32(65536.0)))


def sc_of(p):
    """The scale of kept values, 65536 / (65536 - thr): 1 / (1 - p) for the p the 16-bit threshold realises, not for p."""
    return 65536.0 / (65536 - thr_of(p))


# ---- bounds ----------------------------------------------------------------------------------------------------------
def acc_bound(K, S):
    """Element-wise bound on |fp32-accumulated (A B^T + bias) - exact| for ANY order of the additions.

    Each of the K products of two bf16 values is exact in fp32.  Summing K exact terms and the bias takes K additions;
    allow K + 2 roundings (two spare: the kernel's 1/(1-p) is itself a rounded fp32 number and the multiplication by it
    rounds once more, both relative to a value of at most S).  By the standard inductive argument (Higham, Accuracy and
    Stability of Numerical Algorithms, Lemma 3.1) the result is sum_k t_k (1 + theta_k) with |theta_k| <= gamma =
    n u / (1 - n u), n = K + 2, whatever the order or the tree, so the error is at most gamma * S with
    S = sum_k |a_k b_k| + |bias|.
    u is taken as 2^-23, a WHOLE ulp per operation instead of the half ulp of round-to-nearest: an MFMA accumulator is not
    documented to round every partial sum to nearest (it may truncate or keep a wider intermediate), and a whole ulp
    covers either.  Nothing here is measured on the kernel."""
    n = (K + 2) * U32
    return n / (1.0 - n) * S


def bf16_ulp(x):
    """Spacing of the bf16 numbers in the binade of |x| (float64 tensor): 2^(floor(log2 |x|) - 7); below the smallest
    normal, and at 0, the subnormal spacing 2^-133."""
    x = torch.as_tensor(x, dtype=torch.float64).abs()
    _, e = torch.frexp(x)                      # |x| = m 2^e, m in [0.5, 1)
    e = torch.clamp(e - 1, min=-126)           # (frexp(0) gives e = 0, which clamps nowhere wrong: see below)
    ulp = torch.ldexp(torch.ones_like(x), e - 7)
    return torch.where(x < TINY_BF16, torch.full_like(x, 2.0 ** -133), ulp)


def ratio(err, bound):
    """Largest err / bound (element-wise; bound > 0 everywhere)."""
    return float((err / bound).max()) if err.numel() else 0.0


def f32_error_ratio(got, x, bound):
    """fp32 outputs: |got - x| <= bound, element by element.  Returns the largest error / bound."""
    return ratio((got.double() - x).abs(), bound)


def bf16_error_ratio(out, x, bound):
    """bf16 outputs: |float(out) - x| <= half a bf16 ulp of out + bound: round-to-nearest-even of an fp32 value that lies
    within `bound` of x.

    The rounding term is the half ulp of the binade `out` lies in, between 2^-9 |out| (significand just under 2) and
    2^-8 |out| (significand 1).  A flat 2^-9 |x| is NOT a property of bf16: x = 1 + 2^-8 rounds to 1.0, an error of
    2^-8 > 2^-9 x, in any correct implementation (tests/test_gemm_epilogue_refs.py shows it on torch's own cast)."""
    o = out.double()
    return ratio((o - x).abs(), 0.5 * bf16_ulp(o) + bound)


def two_term_error_ratio(out, out_lo, x, bound):
    """Two-term bf16 outputs: |float(out) + float(out_lo) - x| <= 2^-17 |x| + bound (the remainder v - out is at most
    half an ulp of out, a power of two or a number of a lower binade, and is itself rounded to 8 bits)."""
    return ratio((out.double() + out_lo.double() - x).abs(), 2.0 ** -17 * x.abs() + bound)


def is_pos_zero(t):
    """Element-wise: the bit pattern is +0 (bf16 or fp32 tensor)."""
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) == 0


# ---- operands and exact values ---------------------------------------------------------------------------------------
def _bf16_values(t):
    return t.bfloat16()


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """Operands and exact values of one shape; cached and shared by every test (treat as read-only).

    a (M, K), b (N, K): bf16.  Asymmetric on purpose -- a ramp along K on a, a gain per row on b, a mean on a's rows --
    so that a transposed, row-swapped or K-reversed product cannot pass.  bias (N,) fp32, res (M, N) fp32, aux (M, N) bf16.
    v = a b^T + bias, v0 = a b^T, S = |a| |b|^T + |bias|, S0 = |a| |b|^T, all float64."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    ramp = torch.linspace(0.25, 1.75, K)
    rowmean = 0.1 * ((torch.arange(M) % 3).float() - 1.0)[:, None]
    a = _bf16_values((torch.randn(M, K, generator=g) + rowmean) * ramp)
    gain = 0.5 + 0.375 * (torch.arange(N) % 5).float()
    b = _bf16_values(torch.randn(N, K, generator=g) * gain[:, None] / math.sqrt(K))
    bias = 0.5 * torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    ad, bd = a.double(), b.double()
    v0 = ad @ bd.t()
    S0 = ad.abs() @ bd.abs().t()
    c = dict(M=M, N=N, K=K, a=a, b=b, bias=bias, res=res, v0=v0, S0=S0, v=v0 + bias.double(), S=S0 + bias.double().abs())
    c["aux"] = aux_for(M, N, g)
    return c


AUX_SPECIALS = [0.0, -0.0, TINY_BF16, -1.0, 2.0, -TINY_BF16]


def aux_for(M, N, g):
    """The mask operand of PIKA_EPI_MASK_BF16: normal values of both signs with +0, -0 and the smallest positive (and
    negative) normal sprinkled in, and placed on purpose on every tile corner, the first and last row and column."""
    aux = torch.randn(M, N, generator=g).bfloat16()
    flat = aux.view(-1)
    for k, s in enumerate(AUX_SPECIALS):
        flat[k::len(AUX_SPECIALS) + 1 + k] = s
    rows = sorted({r for r in (0, 1, TILE_M - 1, TILE_M, 2 * TILE_M - 1, 2 * TILE_M, M - 2, M - 1) if 0 <= r < M})
    cols = sorted({c for c in (0, 3, 4, TILE_N - 1, TILE_N, TILE_N + 3, 2 * TILE_N - 1, 2 * TILE_N, N - 5, N - 4, N - 2, N - 1)
                   if 0 <= c < N})
    k = 0
    for r in rows:
        for c in cols:
            aux[r, c] = AUX_SPECIALS[k % 3]        # +0, -0, tiny in turn
            k += 1
    # the whole last row and last column walk through all specials
    for c in range(N):
        aux[M - 1, c] = AUX_SPECIALS[c % len(AUX_SPECIALS)]
    for r in range(M):
        aux[r, N - 1] = AUX_SPECIALS[(r + 1) % len(AUX_SPECIALS)]
    return aux


def expect_f32(c, relu):
    return c["v"].clamp(min=0) if relu else c["v"]


def expect_dropout(c, keep, p, relu):
    """x = keep * sc * relu?(v)"""
    return keep.double() * sc_of(p) * expect_f32(c, relu)


def expect_mask(c, scale):
    """x = scale * (a b^T) where aux > 0, else 0 (no bias, no ReLU); -0 and +0 are not > 0, the smallest normal is."""
    return torch.where(c["aux"].double() > 0, float(np.float32(scale)) * c["v0"], torch.zeros_like(c["v0"]))


def expect_residual(c, keep, p):
    """x = keep * sc * v + residual"""
    return keep.double() * sc_of(p) * c["v"] + c["res"].double()


def decided(c):
    """Elements whose sign / zero-ness the kernel must agree on: |v| > acc_bound."""
    return c["v"].abs() > acc_bound(c["K"], c["S"])


# ---- time-delay operands -----------------------------------------------------------------------------------------------
def td_out_len(T, dil, stride, pad):
    return T if pad else (T - dil * (TD_TAPS - 1) - 1) // stride + 1


@functools.lru_cache(maxsize=None)
def td_case(dil, stride, pad, T):
    """x (batch, T, C) bf16, w (N, taps * C) bf16, bias; the explicit im2col matrix (zeros outside [0, T)) and its exact
    product.  Row (b, t), column (tap, c) reads x[b, t * stride + tap * dil - pad, c]."""
    g = torch.Generator().manual_seed(7000 + 100 * dil + 10 * stride + pad)
    C, taps, Bn, N = TD_C, TD_TAPS, TD_BATCH, TD_N
    K = taps * C
    ramp = torch.linspace(0.5, 1.5, C)
    x = _bf16_values(torch.randn(Bn, T, C, generator=g) * ramp + 0.2 * torch.arange(Bn).float()[:, None, None])
    gain = 0.5 + 0.375 * (torch.arange(N) % 5).float()
    w = _bf16_values(torch.randn(N, K, generator=g) * gain[:, None] / math.sqrt(K))
    bias = 0.5 * torch.randn(N, generator=g)
    t_out = td_out_len(T, dil, stride, pad)
    cols = torch.zeros(Bn, t_out, taps, C, dtype=torch.float64)
    for t in range(t_out):
        for j in range(taps):
            ti = t * stride + j * dil - pad
            if 0 <= ti < T:
                cols[:, t, j, :] = x[:, ti, :].double()
    cols = cols.view(Bn * t_out, K)
    wd = w.double()
    v0 = cols @ wd.t()
    S0 = cols.abs() @ wd.abs().t()
    return dict(M=Bn * t_out, N=N, K=K, t_out=t_out, T=T, dil=dil, stride=stride, pad=pad, x=x, b=w, bias=bias, cols=cols,
                v0=v0, S0=S0, v=v0 + bias.double(), S=S0 + bias.double().abs())


# ---- output buffers with sentinels -------------------------------------------------------------------------------------
SENTINEL = -32768.0        # exact in bf16 and fp32, far from every result


def ldo_for(N, mod8):
    """N rounded up to 4, plus 4 or plus 8 -- whichever makes ldo % 8 == mod8 (0 or 4)."""
    n4 = round_up(N, 4)
    return n4 + 4 if (n4 + 4) % 8 == mod8 else n4 + 8


class Padded:
    """An (M, N) view with pitch `ld` inside a larger buffer filled with a sentinel: `base_off` elements in front, M + 1
    rows.  `intact()` tells whether every cell outside the view still holds the sentinel."""

    def __init__(self, M, N, dtype, ld, device, base_off=0, fill=SENTINEL):
        self.buf = torch.full((base_off + (M + 1) * ld + 8,), fill, dtype=dtype, device=device)
        self.view = self.buf[base_off: base_off + (M + 1) * ld].view(M + 1, ld)[:M, :N]
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside[base_off: base_off + (M + 1) * ld].view(M + 1, ld)[:M, :N] = True
        self.outside = ~inside
        self.before = self.buf.clone()

    def intact(self):
        return torch.equal(self.buf[self.outside], self.before[self.outside])

    def untouched(self):
        return torch.equal(self.buf, self.before)

    def cpu(self):
        return self.view.cpu()
