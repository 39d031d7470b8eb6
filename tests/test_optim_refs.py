"""The yardsticks of tests/optim_common.py, validated on the CPU before anything on a GPU is compared with them: the
float32 restatements stay within their derived float64 bounds on the inputs the GPU tests use, agree with the stock
torch calls within the tolerances tests/test_optim_gpu.py uses, and the chunk tables of pika_amd.optim cover every
element of every tensor exactly once."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_common as Y  # noqa: E402

F = np.float32


@pytest.mark.parametrize("name", sorted(Y.SIZE_LISTS))
def test_chunk_tables_cover_every_element_exactly_once(name):
    from pika_amd import optim as O
    assert O.CHUNK == Y.CHUNK
    sizes = Y.SIZE_LISTS[name]
    ct, co, cl = O.chunk_lists(sizes)
    assert len(ct) == len(co) == len(cl) == sum((n + Y.CHUNK - 1) // Y.CHUNK for n in sizes)
    seen = [np.zeros(n, dtype=np.int32) for n in sizes]
    for t, off, ln in zip(ct, co, cl):
        assert 0 < ln <= Y.CHUNK and off >= 0 and off + ln <= sizes[t]
        seen[t][off:off + ln] += 1
    assert all((s == 1).all() for s in seen)
    assert ct == sorted(ct)
    assert O.chunk_lists([0, 0]) == ([], [], [])


@pytest.mark.parametrize("m,lr", Y.SCALARS)
@pytest.mark.parametrize("first", [True, False])
def test_nesterov_within_its_float64_bound(m, lr, first):
    sizes = Y.SIZE_LISTS["edges"]
    worst = 0.0
    for p, g, b in zip(Y.tensors(sizes, 1), Y.tensors(sizes, 2, 3.0), Y.tensors(sizes, 3, 0.5)):
        p2, b2 = Y.nesterov(p, g, b, lr, m, first)
        assert p2.dtype == b2.dtype == F
        p64, b64, ep, eb = Y.nesterov64(p, g, b, lr, m, first)
        worst = max(worst, Y.worst_ratio(p2, p64, ep), Y.worst_ratio(b2, b64, eb))
    assert 0 < worst <= 1.0, worst


@pytest.mark.parametrize("scale", [0.01, 40.0])
def test_clip_within_its_float64_bound(scale):
    grads = Y.tensors(Y.SIZE_LISTS["edges"], 5, scale)
    norm, out = Y.clip(grads, 3.0)
    n64, v64, e64 = Y.clip64(grads, 3.0)
    assert float(norm) == n64 == max(float(np.abs(g).max()) for g in grads if g.size)
    for g, o, v, e in zip(grads, out, v64, e64):
        if scale < 1:
            assert Y.same_bits(o, g)
        assert Y.worst_ratio(o, v, e) <= 1.0


@pytest.mark.parametrize("world", [1, 6, 8])
def test_bmuf_update_and_adam_moments_within_their_float64_bounds(world):
    worst_u = worst_a = 0.0
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 2048 * 256 + 3):
        d, dp, g, blk = (t for t in Y.tensors([n] * 4, n))
        dp2, g2 = Y.bmuf_update(d, dp * F(0.1), g, world, 0.9, 1.0)
        dp64, g64, edp, eg = Y.bmuf_update64(d, dp * F(0.1), g, world, 0.9, 1.0)
        worst_u = max(worst_u, Y.worst_ratio(dp2, dp64, edp), Y.worst_ratio(g2, g64, eg))
        for c in Y.adam_coefficients((0.9, 0.999), 5, 7.3, 0.9):
            a = Y.adam_moments(d, blk, world, *c)
            a64, ea = Y.adam_moments64(d, blk, world, *c)
            worst_a = max(worst_a, Y.worst_ratio(a, a64, ea))
    assert 0 < worst_u <= 1.0 and 0 < worst_a <= 1.0, (worst_u, worst_a)


def test_scalar_product_of_the_block_update_is_formed_in_float32():
    # 1 - 0.9f is exact in float32 and is NOT float32(0.1): the kernel's coefficient, not the double one
    c = F(1.0) * (F(1) - F(0.9))
    assert c != F(1.0 * (1 - 0.9))
    d = np.array([3.0], dtype=F)
    dp2, _ = Y.bmuf_update(d, np.zeros(1, dtype=F), np.zeros(1, dtype=F), 1, 0.9, 1.0)
    assert dp2[0] == d[0] * c


@pytest.mark.parametrize("scale", [0.01, 40.0])
def test_yardsticks_agree_with_stock_torch_on_the_cpu(scale):
    """clip_grad_norm_(inf) + SGD(nesterov=True) of torch on CPU tensors, four steps, on the parameters and gradients
    of tests/test_optim_gpu.py and within the tolerances it uses between torch and the kernels.

    torch forms the clip coefficient as `(norm + 1e-6).reciprocal() * max_norm` (Tensor.__rtruediv__), two roundings
    where the kernel and the yardstick divide once; the two coefficients are equal or one float32 apart.  The 2e-7 on
    the gradients is the file's tolerance for equal coefficients (x * clamp(c) against x * c), which is what these
    inputs give; one float32 apart would show as up to 2.4e-7."""
    g = torch.Generator().manual_seed(12)
    shapes = [(1024, 240), (1024,), (7,), (3, 5, 11), (4096, 1024), (1,), (513,)]
    assert [int(np.prod(s)) for s in shapes] == Y.SIZE_LISTS["model"]
    tp = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    ps = [t.detach().numpy().copy() for t in tp]
    opt = torch.optim.SGD(tp, 0.003, momentum=0.9, nesterov=True)
    bs = [None] * len(ps)
    g = torch.Generator().manual_seed(3)
    for step in range(4):
        gs = []
        for t in tp:
            t.grad = torch.randn(t.shape, generator=g) * scale
            gs.append(t.grad.numpy().copy())
        tn = torch.nn.utils.clip_grad_norm_(tp, 3.0, norm_type=float("inf"))
        norm, gs = Y.clip(gs, 3.0)
        assert float(tn) == float(norm)
        for t, gg in zip(tp, gs):
            assert np.allclose(t.grad.numpy(), gg, rtol=2e-7, atol=0), step
        opt.step()
        for i, (t, gg) in enumerate(zip(tp, gs)):
            ps[i], bs[i] = Y.nesterov(ps[i], gg, bs[i], 0.003, 0.9, step == 0)
            assert np.allclose(t.detach().numpy(), ps[i], rtol=0, atol=1e-7 * float(np.abs(ps[i]).max())), step
            mb = opt.state[t]["momentum_buffer"].numpy()
            assert np.allclose(mb, bs[i], rtol=0, atol=3e-7 * float(np.abs(mb).max())), step


def test_absmax_and_clip_edges():
    z = np.zeros(5, dtype=F)
    assert Y.same_bits(Y.absmax([z, np.array([-0.0], dtype=F)]), F(0.0))
    assert np.isnan(Y.absmax([z, np.array([1.0, np.nan], dtype=F)]))
    assert Y.absmax([]) == 0 and Y.absmax([np.zeros(0, dtype=F)]) == 0
    sub = np.array([0, 1e-45, -3e-45, 0], dtype=F)
    assert Y.absmax([sub]) == F(3e-45) and Y.absmax([sub]) > 0
    _, (g,) = Y.clip([np.array([1.0, -2.0, np.inf, 0.0], dtype=F)], 3.0)
    assert np.isnan(g[2]) and not g[[0, 1, 3]].any()
    _, (g, h) = Y.clip([np.array([1.0, np.nan], dtype=F), np.ones(3, dtype=F)], 3.0)
    assert np.isnan(g).all() and np.isnan(h).all()
    # the three sides of the threshold exist next to each other
    lo, eq, hi = Y.threshold_norms(3.0)
    assert Y.clip_coef(lo, 3.0) < 1 and Y.clip_coef(eq, 3.0) == 1 and Y.clip_coef(hi, 3.0) > 1
    assert lo > eq > hi
