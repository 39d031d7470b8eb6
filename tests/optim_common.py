"""Yardsticks for the optimizer kernels (pika_amd/csrc/optim.hip) and the BMUF block-update kernels
(pika_amd/csrc/bmuf.hip), numpy only.

Two forms of every operation:

* float32, ONE numpy operation per rounding, in the order the kernel documents (which is the order of the separate
  torch ops of the training script / of trainer/bmuf.py:83-98, :291-313).  IEEE-754 `+ - * /` are correctly rounded on
  both sides and the kernels switch FMA contraction off, so a kernel equals its float32 yardstick bit for bit
  (`same()` below; NaN positions included).
* float64 with a running error bound (`_E`), which is what validates the float32 form on the CPU
  (tests/test_optim_refs.py) and what bounds two float32 evaluations that round their scalars differently.

The bound.  With u = 2**-24 every correctly rounded float32 operation returns fl(x) = x (1 + d), |d| <= u, so it adds
u |x| to the error of its result (`_E._r`; 2**-149 covers a subnormal result, whose error is absolute).  The errors
of the operands propagate to first order:  e(a +- b) = e(a) + e(b);  e(a b) = |b| e(a) + |a| e(b);
e(a / b) = (e(a) + |a / b| e(b)) / |b|.  A Python scalar handed to a kernel is rounded to float32 first: error
u |s|.  The result is "a few u times the magnitudes entering each sum", e.g. for the momentum buffer
b' = b m + g:  e = u (|b m| [m rounded] + |b m| [product] + |b m + g| [sum]).  Second-order terms (products of two
errors, and u |x| taken at the exact x instead of the computed one) are below u times the first-order bound; SLACK
covers them.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -149
SLACK = 1.0 + 2.0 ** -10
CHUNK = 16384

# lengths per tensor: empty, shorter than the scalar head, around the 4-wide body, the 256-thread trip, a chunk, two chunks
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 32768 + 1]
SIZE_LISTS = {
    "edges": LENGTHS,
    "empty_between": [5, 0, 16385, 0, 0, 3],
    "model": [1024 * 240, 1024, 7, 3 * 5 * 11, 4096 * 1024, 1, 513],       # the shapes of tests/test_optim_gpu.py
}
SCALARS = [(0.9, 0.003), (0.5, 0.25)]                                        # (momentum, lr)


def tensors(sizes, seed, scale=1.0):
    r = np.random.RandomState(seed)
    return [(r.standard_normal(n) * scale).astype(F) for n in sizes]


def same(a, b):
    """Equality of two float32 arrays as values, a NaN equal to a NaN in the same place."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- float32 ---------------------------------------------------------------------------------------------------------
def absmax(grads):
    """max |g| over all tensors (0 for none); NaN if any element is NaN."""
    m = F(0)
    for g in grads:
        if g.size:
            if np.isnan(g).any():
                return F(np.nan)
            m = max(m, np.abs(g).max())
    return F(m)


def clip_coef(norm, max_norm):
    with np.errstate(all="ignore"):
        return F(max_norm) / (F(norm) + F(1e-6))


def clip(grads, max_norm, norm=None):
    """clip_grad_norm_(.., max_norm, inf): (norm, gradients); scaled only when coef < 1 or coef is NaN."""
    norm = absmax(grads) if norm is None else F(norm)
    coef = clip_coef(norm, max_norm)
    if coef < 1 or coef != coef:
        with np.errstate(all="ignore"):
            return norm, [g * coef for g in grads]
    return norm, [g.copy() for g in grads]


def threshold_norms(max_norm):
    """Three norms next to the clip threshold: the smallest with coef < 1, one with coef == 1, the largest with
    coef > 1, found by stepping down from max_norm one float32 at a time."""
    n = F(max_norm)
    assert clip_coef(n, max_norm) < 1
    while clip_coef(np.nextafter(n, F(0)), max_norm) < 1:
        n = np.nextafter(n, F(0))
    below, n = n, np.nextafter(n, F(0))
    assert clip_coef(n, max_norm) == 1, "no float32 norm gives coef == 1 for this max_norm"
    exact = n
    while clip_coef(n, max_norm) == 1:
        n = np.nextafter(n, F(0))
    return below, exact, n


def nesterov(p, g, b, lr, m, first):
    """torch.optim.SGD(nesterov=True, dampening=0): (p', b').  `b` is ignored on the first step."""
    lr, m = F(lr), F(m)
    with np.errstate(all="ignore"):
        b2 = g.copy() if first else b * m + g
        t = b2 * m
        t = g + t
        t = t * lr
        return p - t, b2


def bmuf_update(d, dp, g, world, bm, blr):
    """upd() of bmuf.hip == trainer/bmuf.py:93-96: (delta_prev', global'); local' = global'."""
    world, bm, blr = F(world), F(bm), F(blr)
    with np.errstate(all="ignore"):
        avg = d / world
        c = blr * (F(1) - bm)
        t1 = dp * bm
        t2 = avg * c
        dp2 = t1 + t2
        t3 = dp2 * (F(1) + bm)
        return dp2, g - t3


def adam_coefficients(betas, sync_period, rho, bm):
    """The six coefficients of one block, float64 on the host as the trainer forms them."""
    out = []
    for beta in betas:
        bt, br = beta ** sync_period, beta ** (rho * bm)
        out.append((bt * (br - 1), 1 - bt * br, 1 - bt))
    return out


def adam_moments(x, blk, world, c1, c2, c3):
    """One moment of bmuf_adam_moments_kernel == trainer/bmuf.py:276, :288-291: the new block moment (x' = blk')."""
    world, c1, c2, c3 = F(world), F(c1), F(c2), F(c3)
    with np.errstate(all="ignore"):
        m = x / world
        a = c1 * blk
        a = a + c2 * m
        return a / c3


# ---- float64 with a running first-order error bound ------------------------------------------------------------------
class _E(object):
    """A float64 value `v` that stands for a float32 computation, and the bound `e` of their difference."""

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)

    @staticmethod
    def scalar(s):                      # a host scalar rounded to float32 on its way into the kernel
        return _E(float(s), U * abs(float(s)))

    @staticmethod
    def _r(v, e):                       # one correctly rounded float32 operation
        return _E(v, e + U * np.abs(v) + TINY)

    def __add__(self, o):
        return _E._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return _E._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return _E._r(self.v * o.v, np.abs(o.v) * self.e + np.abs(self.v) * o.e)

    def __truediv__(self, o):
        q = self.v / o.v
        return _E._r(q, (self.e + np.abs(q) * o.e) / np.abs(o.v))

    def out(self):
        return self.v, self.e * SLACK


def clip64(grads, max_norm):
    """(norm, values, bounds).  The bound is that of the scaled gradient on either side of the threshold: where the two
    precisions decide `coef < 1` differently, coef is within its own error of 1 and g (1 - coef) is within the bound."""
    norm = float(absmax(grads))         # a maximum of absolute values: no rounding
    coef = _E.scalar(max_norm) / (_E(norm) + _E(float(F(1e-6))))
    vals, bounds = [], []
    for g in grads:
        s = _E(g) * coef
        v, e = s.out()
        vals.append(v if coef.v < 1 else g.astype(np.float64))
        bounds.append(e)
    return norm, vals, bounds


def nesterov64(p, g, b, lr, m, first):
    """(p', b', bound of p', bound of b')"""
    lr, m, p, g = _E.scalar(lr), _E.scalar(m), _E(p), _E(g)
    b2 = g if first else _E(b) * m + g
    p2 = p - (g + b2 * m) * lr
    (pv, pe), (bv, be) = p2.out(), b2.out()
    return pv, bv, pe, be


def bmuf_update64(d, dp, g, world, bm, blr):
    """(delta_prev', global', bound of delta_prev', bound of global')"""
    world, bm, blr, one = _E(float(world)), _E.scalar(bm), _E.scalar(blr), _E(1.0)
    avg = _E(d) / world
    dp2 = _E(dp) * bm + avg * (blr * (one - bm))
    g2 = _E(g) - dp2 * (one + bm)
    (dv, de), (gv, ge) = dp2.out(), g2.out()
    return dv, gv, de, ge


def adam_moments64(x, blk, world, c1, c2, c3):
    """(block moment, its bound)"""
    c1, c2, c3 = _E.scalar(c1), _E.scalar(c2), _E.scalar(c3)
    a = c1 * _E(blk) + c2 * (_E(x) / _E(float(world)))
    return (a / c3).out()


def worst_ratio(got32, want64, bound):
    """max |got - want| / bound over the elements with a non-zero bound (0 for none); every other must be equal."""
    err = np.abs(got32.astype(np.float64) - want64)
    bound = np.broadcast_to(bound, err.shape)
    nz = bound > 0
    assert np.all(err[~nz] == 0)
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
