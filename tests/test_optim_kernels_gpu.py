"""The three entry points of include/pika_optim.h called directly, with hand-built pointer and chunk tables, against the
float32 yardsticks of tests/optim_common.py: EQUAL (NaN positions included) at every alignment of parameter, gradient
and momentum buffer, at every length around the scalar head, the 4-wide body, the 256-thread trip and the chunk, with
the maximum / an infinity / a NaN in a head, a body and a tail, and on the three sides of the clip threshold.  Every
tensor is carved out of a larger allocation between guard elements, which must come back unchanged."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_common as Y  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 8                       # a multiple of 4: a tensor's element offset decides its alignment
SENTINEL = F(7.5e37)            # finite and above every test value: a read of a guard would win the maximum
PIKA_EINVAL = -1


class Arena(object):
    """Tensors carved out of ONE device allocation (256-byte aligned) at chosen element offsets mod 4."""

    def __init__(self, arrays, offsets, dev):
        pos, self.starts, self.sizes = 0, [], [a.size for a in arrays]
        for a, o in zip(arrays, offsets):
            pos += GUARD
            pos += (o - pos) % 4
            self.starts.append(pos)
            pos += a.size
        self.host = np.full(pos + GUARD, SENTINEL, dtype=F)
        for a, s in zip(arrays, self.starts):
            self.host[s:s + a.size] = a
        self.dev = torch.from_numpy(self.host).to(dev)
        assert self.dev.data_ptr() % 16 == 0
        for s, o in zip(self.starts, offsets):
            assert (self.dev.data_ptr() + 4 * s) % 16 == 4 * o
        self.ptrs = torch.tensor([self.dev.data_ptr() + 4 * s for s in self.starts], dtype=torch.int64, device=dev)

    def read(self):
        """The tensors as they are now; asserts that nothing outside them was written."""
        got = self.dev.cpu().numpy()
        mask = np.ones(got.size, dtype=bool)
        out = []
        for s, n in zip(self.starts, self.sizes):
            mask[s:s + n] = False
            out.append(got[s:s + n].copy())
        assert Y.same_bits(got[mask], self.host[mask]), "a guard element was overwritten"
        return out


class Chunks(object):
    def __init__(self, sizes, dev):
        from pika_amd import optim as O
        ct, co, cl = O.chunk_lists(sizes)
        self.n = len(ct)
        self.ct = torch.tensor(ct, dtype=torch.int32, device=dev)
        self.co = torch.tensor(co, dtype=torch.int64, device=dev)
        self.cl = torch.tensor(cl, dtype=torch.int32, device=dev)

    def args(self):
        return self.ct.data_ptr(), self.co.data_ptr(), self.cl.data_ptr(), self.n


def _st():
    return torch.cuda.current_stream().cuda_stream


def gpu_clip(grads, offsets, max_norm, dev, norm=None):
    """absmax (unless a norm is given) + scale_by_clip on carved gradients: (norm, gradients)."""
    from pika_amd import _lib
    lib = _lib.lib()
    a, ch = Arena(grads, offsets, dev), Chunks([g.size for g in grads], dev)
    out = torch.full((3,), 123.0, device=dev)            # the norm between two words that must stay
    if norm is None:
        _lib.check(lib.pika_multi_absmax(a.ptrs.data_ptr(), *ch.args(), out[1:].data_ptr(), _st()), "absmax")
        assert all(Y.same_bits(x, y) for x, y in zip(a.read(), grads)), "absmax wrote to a gradient"
    else:
        out[1] = float(norm)
    _lib.check(lib.pika_multi_scale_by_clip(a.ptrs.data_ptr(), *ch.args(), out[1:].data_ptr(), float(max_norm), _st()),
               "scale")
    o = out.cpu().numpy()
    assert o[0] == 123.0 and o[2] == 123.0
    return o[1], a.read()


def gpu_sgd(ps, gs, bs, offsets, lr, m, first, dev):
    """offsets: one (op, og, ob) per tensor.  Returns (parameters, buffers); the gradients must stay as they were."""
    from pika_amd import _lib
    lib = _lib.lib()
    ap, ag, ab = (Arena(x, [o[k] for o in offsets], dev) for k, x in enumerate((ps, gs, bs)))
    ch = Chunks([p.size for p in ps], dev)
    _lib.check(lib.pika_multi_sgd_nesterov(ap.ptrs.data_ptr(), ag.ptrs.data_ptr(), ab.ptrs.data_ptr(), *ch.args(),
                                           float(lr), float(m), int(first), _st()), "sgd")
    assert all(Y.same_bits(x, y) for x, y in zip(ag.read(), gs)), "the step wrote to a gradient"
    return ap.read(), ab.read()


def check_sgd(sizes, offsets, lr, m, first, dev, seed):
    ps, gs, bs = Y.tensors(sizes, seed), Y.tensors(sizes, seed + 1, 3.0), Y.tensors(sizes, seed + 2, 0.5)
    got_p, got_b = gpu_sgd(ps, gs, bs, offsets, lr, m, first, dev)
    for i, (p, g, b) in enumerate(zip(ps, gs, bs)):
        want_p, want_b = Y.nesterov(p, g, b, lr, m, first)
        bad_p, bad_b = np.flatnonzero(got_p[i] != want_p), np.flatnonzero(got_b[i] != want_b)
        assert Y.same(got_p[i], want_p) and Y.same(got_b[i], want_b), \
            (i, sizes[i], offsets[i], bad_p[:8], bad_b[:8])


ALL_OFFSETS = list(itertools.product(range(4), repeat=3))        # every (op, og, ob): the 16 with <= 1 off, 48 mixed


@pytest.mark.parametrize("m,lr", Y.SCALARS)
@pytest.mark.parametrize("first", [1, 0])
def test_sgd_alignment_matrix(hip_device, first, m, lr):
    """One tensor per (op, og, ob) in {0..3}^3, lengths cycling so that every alignment meets several: the vector
    route with every head length where the three agree mod 4, the scalar route everywhere else."""
    lengths = [1029, 6, 255, 1, 2050, 3, 16385, 5, 257, 2, 1024]     # 11 is coprime to 64: four launches cover more
    for rot in range(2):
        sizes = [lengths[(i + 5 * rot) % len(lengths)] for i in range(len(ALL_OFFSETS))]
        check_sgd(sizes, ALL_OFFSETS, lr, m, first, hip_device, seed=10 + rot)


@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3), (0, 0, 1), (3, 0, 0), (2, 1, 2)])
@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("name", ["edges", "empty_between"])
def test_sgd_lengths(hip_device, name, first, offs):
    sizes = Y.SIZE_LISTS[name]
    m, lr = Y.SCALARS[(first + sum(offs)) % 2]
    check_sgd(sizes, [offs] * len(sizes), lr, m, first, hip_device, seed=20)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("scale", [0.01, 40.0])
@pytest.mark.parametrize("name", ["edges", "empty_between"])
def test_clip_lengths_and_alignments(hip_device, name, scale, off):
    sizes = Y.SIZE_LISTS[name]
    grads = Y.tensors(sizes, 30 + off, scale)
    offsets = [(off + (i if name == "edges" else 0)) % 4 for i in range(len(sizes))]
    norm, got = gpu_clip(grads, offsets, 3.0, hip_device)
    want_norm, want = Y.clip(grads, 3.0)
    assert Y.same_bits(norm, want_norm)
    for i, (a, b) in enumerate(zip(got, want)):
        assert Y.same(a, b), (i, sizes[i], offsets[i], np.flatnonzero(a != b)[:8])
        if scale < 1:
            assert Y.same_bits(a, grads[i])


def test_only_empty_tensors_are_a_bad_argument(hip_device):
    """n_chunks <= 0 is PIKA_EINVAL (include/pika_optim.h) from all three entry points, before any launch."""
    from pika_amd import _lib, optim as O
    lib = _lib.lib()
    assert O.chunk_lists([0, 0, 0]) == ([], [], [])
    a = Arena([np.zeros(0, dtype=F)] * 3, [0, 1, 2], hip_device)
    t = torch.zeros(4, dtype=torch.int64, device=hip_device)
    out = torch.full((1,), 5.0, device=hip_device)
    p, tp = a.ptrs.data_ptr(), t.data_ptr()
    for n_chunks in (0, -1):
        assert lib.pika_multi_absmax(p, tp, tp, tp, n_chunks, out.data_ptr(), _st()) == PIKA_EINVAL
        assert lib.pika_multi_scale_by_clip(p, tp, tp, tp, n_chunks, out.data_ptr(), 3.0, _st()) == PIKA_EINVAL
        assert lib.pika_multi_sgd_nesterov(p, p, p, tp, tp, tp, n_chunks, 0.1, 0.9, 1, _st()) == PIKA_EINVAL
    assert float(out) == 5.0            # not even the memset of the norm ran
    a.read()


# ---- where the maximum sits ------------------------------------------------------------------------------------------
POS_SIZES = [7, 16384 + 6, 32768 + 3]
# (tensor, index): the first head element; inside a 4-wide body; the first element of a second chunk; the last tail
# element of the last chunk of the last tensor
POSITIONS = {"head": (0, 0), "body": (1, 4 * 777 + 6), "chunk2": (1, 16384), "tail": (2, POS_SIZES[2] - 1)}
POS_OFFSETS = [[1, 2, 3], [3, 0, 1], [2, 3, 0], [0, 1, 2]]


def _clip_case(grads, offsets, dev):
    norm, got = gpu_clip(grads, offsets, 3.0, dev)
    want_norm, want = Y.clip(grads, 3.0)
    assert Y.same_bits(norm, want_norm) or (np.isnan(norm) and np.isnan(want_norm)), (norm, want_norm)
    for i, (a, b) in enumerate(zip(got, want)):
        assert Y.same(a, b), (i, offsets[i], np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[:8])
    return norm, got


@pytest.mark.parametrize("where", sorted(POSITIONS))
@pytest.mark.parametrize("offsets", POS_OFFSETS[:2])
def test_maximum_in_a_head_a_second_chunk_and_a_tail(hip_device, where, offsets):
    t, i = POSITIONS[where]
    grads = Y.tensors(POS_SIZES, 40)                 # |N(0, 1)| over 5e4 samples stays below 6
    grads[t][i] = F(-9.25)
    norm, got = _clip_case(grads, offsets, hip_device)
    assert norm == F(9.25) and got[t][i] == F(-9.25) * Y.clip_coef(9.25, 3.0)
    # -0.0 against all zeros: the norm is +0.0 and nothing is scaled, bit for bit
    zeros = [np.zeros(n, dtype=F) for n in POS_SIZES]
    zeros[t][i] = F(-0.0)
    norm, got = _clip_case(zeros, offsets, hip_device)
    assert Y.same_bits(norm, F(0.0)) and all(Y.same_bits(a, b) for a, b in zip(got, zeros))


@pytest.mark.parametrize("where", sorted(POSITIONS))
@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
def test_infinity_and_nan_as_the_maximum(hip_device, where, value):
    t, i = POSITIONS[where]
    offsets = POS_OFFSETS[(t + 2) % 4]
    grads = Y.tensors(POS_SIZES, 41)
    grads[t][i] = F(value)
    norm, got = _clip_case(grads, offsets, hip_device)
    if np.isnan(value):
        # a NaN norm: every element of every tensor, the tensors whose own chunks held no NaN included
        assert np.isnan(norm) and all(np.isnan(g).all() for g in got)
    else:
        assert norm == F(np.inf)
        for k, g in enumerate(got):
            nan = np.isnan(g)
            assert nan.sum() == (k == t) and (not nan.any() or nan[i]) and not g[~nan].any()


def test_nan_norm_from_the_host_reaches_tensors_without_one(hip_device):
    grads = Y.tensors(POS_SIZES, 42)
    _, got = gpu_clip(grads, [1, 2, 3], 3.0, hip_device, norm=np.nan)
    assert all(np.isnan(g).all() for g in got)


@pytest.mark.parametrize("where", sorted(POSITIONS))
def test_absmax_of_subnormals_is_exact(hip_device, where):
    t, i = POSITIONS[where]
    grads = [np.zeros(n, dtype=F) for n in POS_SIZES]
    tiny = np.array([1, 5, 3], dtype=np.uint32).view(F)          # the three smallest odd multiples of 2**-149
    grads[0][3], grads[1][100], grads[2][16384 * 2] = tiny[0], -tiny[2], tiny[0]
    grads[t][i] = -tiny[1]
    from pika_amd import _lib
    a, ch = Arena(grads, POS_OFFSETS[0], hip_device), Chunks(POS_SIZES, hip_device)
    out = torch.zeros(1, device=hip_device)
    _lib.check(_lib.lib().pika_multi_absmax(a.ptrs.data_ptr(), *ch.args(), out.data_ptr(), _st()), "absmax")
    assert Y.same_bits(out.cpu().numpy()[0], tiny[1]) and Y.same_bits(Y.absmax(grads), tiny[1])
    a.read()


@pytest.mark.parametrize("off", [0, 3])
def test_clip_threshold_below_at_and_above_one(hip_device, off):
    below, exact, above = Y.threshold_norms(3.0)
    for k, norm in enumerate((below, exact, above)):
        grads = [g * F(0.3) for g in Y.tensors([5, 16385, 1027], 50 + k)]
        assert max(np.abs(g).max() for g in grads) < norm
        grads[1][16384] = -norm
        got_norm, got = gpu_clip(grads, [off, (off + 1) % 4, off], 3.0, hip_device)
        want_norm, want = Y.clip(grads, 3.0)
        assert Y.same_bits(got_norm, norm) and Y.same_bits(want_norm, norm)
        coef = Y.clip_coef(norm, 3.0)
        assert (coef < 1, coef == 1, coef > 1)[k]
        for a, b, g in zip(got, want, grads):
            assert Y.same(a, b)
            if k == 0:
                assert not Y.same_bits(a, g)
            else:
                assert Y.same_bits(a, g), "coef >= 1: the gradients stay untouched, bit for bit"
