"""The entry points of include/pika_bmuf.h called directly against the float32 yardsticks of tests/optim_common.py:
EQUAL for `delta`, `update` and `adam_moments` at every length around the 4-wide body, at the sizes where the
grid-stride loops take a second trip, with every vector aligned and not; the NaN flag at every position that a loop
edge could miss; the skip flag; and BmufAdamTrainer on the device against a CPU / gloo worker of the same class."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bmuf_common as C  # noqa: E402
import optim_common as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 8
SENTINEL = F(7.5e37)
STRIDE = 2048 * 256                     # threads of the full grid
N_VEC2 = STRIDE * 4 + 5                 # the vector loop's second trip, with a scalar tail (8 MB per vector)
N_SCALAR2 = STRIDE + 3                  # the scalar loop's second trip
SMALL = [1, 3, 4, 5, 1023, 1024, 1025]


class Carved(object):
    """A vector at element offset `off` (mod 4) of its own allocation, between guards."""

    def __init__(self, a, off, dev):
        self.n, self.start = a.size, GUARD + off
        self.host = np.full(a.size + 2 * GUARD + 4, SENTINEL, dtype=F)
        self.host[self.start:self.start + a.size] = a
        self.dev = torch.from_numpy(self.host).to(dev)
        self.ptr = self.dev.data_ptr() + 4 * self.start
        assert self.ptr % 16 == 4 * off

    def view(self):
        return self.dev[self.start:self.start + self.n]

    def read(self):
        got = self.dev.cpu().numpy()
        s, e = self.start, self.start + self.n
        assert Y.same_bits(got[:s], self.host[:s]) and Y.same_bits(got[e:], self.host[e:]), "a guard was overwritten"
        return got[s:e].copy()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from pika_amd import _lib as L
    return L, L.lib()


def _flag(dev, v=0):
    return torch.full((1,), v, dtype=torch.int32, device=dev)


def check_delta(n, offs, dev):
    L, lib = _lib()
    g, l = Y.tensors([n, n], 1000 + n % 997)
    cg, cl, cd = Carved(g, offs[0], dev), Carved(l, offs[1], dev), Carved(np.zeros(n, dtype=F), offs[2], dev)
    L.check(lib.pika_bmuf_delta(cg.ptr, cl.ptr, cd.ptr, n, _st()), "delta")
    assert Y.same(cd.read(), g - l), (n, offs)
    assert Y.same_bits(cg.read(), g) and Y.same_bits(cl.read(), l)


def check_update(n, offs, world, dev, bm=0.9, blr=1.0, skip=None):
    """offs: (delta, delta_prev, global, local).  skip: None (no flag), 0 or 1 (a flag word with that value)."""
    L, lib = _lib()
    d, dp, g, l = Y.tensors([n] * 4, 2000 + n % 997)
    dp = dp * F(0.1)
    cd, cdp, cg, cl = (Carved(a, o, dev) for a, o in zip((d, dp, g, l), offs))
    flag = None if skip is None else _flag(dev, skip)
    L.check(lib.pika_bmuf_update(cd.ptr, cdp.ptr, cg.ptr, cl.ptr, n, float(world), bm, blr,
                                 None if flag is None else flag.data_ptr(), _st()), "update")
    got_dp, got_g, got_l = cdp.read(), cg.read(), cl.read()
    assert Y.same_bits(cd.read(), d)
    if skip:
        assert Y.same_bits(got_dp, dp) and Y.same_bits(got_g, g) and Y.same_bits(got_l, l), (n, offs)
        assert int(flag.item()) == 1
        return
    want_dp, want_g = Y.bmuf_update(d, dp, g, world, bm, blr)
    assert Y.same(got_dp, want_dp), (n, offs, world, np.flatnonzero(got_dp != want_dp)[:8])
    assert Y.same(got_g, want_g), (n, offs, world, np.flatnonzero(got_g != want_g)[:8])
    assert Y.same_bits(got_l, got_g)


def check_adam(n, offs, world, dev, skip=0, rho=7.3):
    L, lib = _lib()
    x1, b1, x2, b2 = Y.tensors([n] * 4, 3000 + n % 997)
    x1, x2, b2 = x1 * F(3), np.abs(x2) * F(5), np.abs(b2)
    c = Y.adam_coefficients((0.9, 0.999), 5, rho, 0.9)
    cs = [Carved(a, o, dev) for a, o in zip((x1, b1, x2, b2), offs)]
    flag = _flag(dev, skip)
    L.check(lib.pika_bmuf_adam_moments(cs[0].ptr, cs[1].ptr, cs[2].ptr, cs[3].ptr, n, float(world), *c[0], *c[1],
                                       flag.data_ptr(), _st()), "adam_moments")
    got = [x.read() for x in cs]
    if skip:
        assert all(Y.same_bits(a, b) for a, b in zip(got, (x1, b1, x2, b2))), (n, offs)
        return
    w1, w2 = Y.adam_moments(x1, b1, world, *c[0]), Y.adam_moments(x2, b2, world, *c[1])
    for a, w in ((got[0], w1), (got[1], w1), (got[2], w2), (got[3], w2)):
        assert Y.same(a, w), (n, offs, world, np.flatnonzero(a != w)[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 6, 8])
def test_small_lengths_equal_the_yardstick(hip_device, world):
    for n in SMALL:
        check_delta(n, (0, 0, 0), hip_device)
        check_update(n, (0, 0, 0, 0), world, hip_device, skip=0)
        check_update(n, (0, 0, 0, 0), world, hip_device, bm=0.5, blr=0.75)
        check_adam(n, (0, 0, 0, 0), world, hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 6, 8])
@pytest.mark.parametrize("n,off", [(N_VEC2, 0), (N_SCALAR2, 1)])
def test_second_trip_of_the_grid_stride_loops(hip_device, n, off, world):
    check_update(n, (off, 0, 0, 0), world, hip_device, skip=0)
    check_adam(N_SCALAR2, (0, off, 0, 0), world, hip_device)
    if world == 6:
        check_delta(n, (0, off, 0), hip_device)


UPDATE_OFFSETS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 2, 3, 0), (3, 1, 2, 1),
                  (2, 2, 2, 2)]
DELTA_OFFSETS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3), (3, 3, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("offs", UPDATE_OFFSETS)
def test_update_alignments(hip_device, offs):
    for n in (1029, 4099):
        check_update(n, offs, 6, hip_device, skip=0)
        check_adam(n, offs, 6, hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("offs", DELTA_OFFSETS)
def test_delta_alignments(hip_device, offs):
    for n in (5, 1029, 4099):
        check_delta(n, offs, hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (0, 0, 3, 0), (1, 2, 3, 2)])
def test_set_skip_flag_leaves_every_vector_bit_identical(hip_device, offs):
    for n in (5, 1029, N_SCALAR2):
        check_update(n, offs, 6, hip_device, skip=1)
        check_adam(n, offs, 6, hip_device, skip=1)


@pytest.mark.gpu
@pytest.mark.parametrize("n,off", [(7, 0), (7, 1), (1, 0), (N_SCALAR2, 0), (N_SCALAR2, 3), (N_VEC2, 0)])
def test_nan_flag_positions(hip_device, n, off):
    """One flag word per probe, all read back at once.  A NaN in element 0, in element n-1, in each position of the
    1-3 element tail and in the second grid-stride trip sets the flag; so does a negative NaN bit pattern.  An
    infinity does not; a clear flag stays 0 and a set flag stays 1 on clean input."""
    L, lib = _lib()
    clean = Y.tensors([n], 7)[0]
    c = Carved(clean, off, hip_device)
    v = c.view()
    positions = sorted({0, n - 1, n - 2, n - 3, (n >> 2) << 2, STRIDE, STRIDE + 1, n // 2} & set(range(n)))
    specials = torch.from_numpy(np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000],
                                         dtype=np.uint32).view(F)).to(hip_device)
    probes = [(p, 0) for p in positions] + [(n - 1, 1), (0, 2), (n - 1, 3), (0, 4)]
    flags = torch.zeros(len(probes) + 2, dtype=torch.int32, device=hip_device)
    flags[-1] = 1
    want = []
    keep = torch.from_numpy(clean).to(hip_device)
    for k, (pos, s) in enumerate(probes):
        v[pos:pos + 1].copy_(specials[s:s + 1])
        L.check(lib.pika_bmuf_nan_flag(c.ptr, n, flags[k:].data_ptr(), _st()), "nan_flag")
        v[pos:pos + 1].copy_(keep[pos:pos + 1])
        want.append(1 if s < 3 else 0)
    for k in (len(probes), len(probes) + 1):                   # clean input: 0 stays 0, 1 stays 1
        L.check(lib.pika_bmuf_nan_flag(c.ptr, n, flags[k:].data_ptr(), _st()), "nan_flag")
    got = flags.cpu().numpy().tolist()
    assert got == want + [0, 1], list(zip(probes, got))
    assert Y.same_bits(c.read(), clean)


# ---- BmufAdamTrainer on the device ------------------------------------------------------------------------------------
def _adam_cpu_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "pika_amd", "dropin"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from trainer.bmuf import BmufAdamTrainer
    model = C.make_model(0)
    optim = C.make_adam(model)
    tr = BmufAdamTrainer(0, rank, world, model, C.BM, C.BLR, C.SYNC_PERIOD, optim)
    rec = {}
    try:
        for rnd in range(C.ROUNDS):
            C.local_adam_steps(model, optim, 0, rnd)
            for when in ("before", "after"):
                if when == "after":
                    assert tr.update_and_sync() == 1
                p, m, v, steps = C.adam_state(model, optim)
                rec.update({"%s%d_%s" % (when, rnd, k): a for k, a in
                            (("local", p), ("m", m), ("v", v), ("steps", steps), ("rho", np.float64(tr.rho)),
                             ("global", tr.param.numpy().copy()), ("delta_prev", tr.delta_prev.numpy().copy()),
                             ("blk_m", tr.exp_avg.numpy().copy()), ("blk_v", tr.exp_avg_sq.numpy().copy()))})
        np.savez(out, **rec)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.gpu
def test_bmuf_adam_trainer_on_hip_single_rank(hip_device, tmp_path):
    """world_size 1: every block of a CPU / gloo BmufAdamTrainer, replayed on the device from the recorded state before
    the sync (local parameters, both moments, the steps; and the trainer's own block state: global model, delta_prev,
    block moments, rho), compared with the recorded state after it.

    * Both moments, the block moments, the step counters and rho: EQUAL.  The CPU branch runs the kernel's float32
      operations in the kernel's order (x / world, c1 * blk, + c2 * m, / c3; torch rounds a Python scalar to float32 on
      use as the C call does), and the steps / rho are host arithmetic on both sides.
    * Parameters (local == global) and delta_prev: within TWO derived bounds of optim_common.bmuf_update64.  The CPU
      branch multiplies by float32(blr * (1 - bm)) formed in float64 as the reference does (trainer/bmuf.py:277-279);
      the kernel forms float32(blr) * (1 - float32(bm)) in float32, three roundings instead of one (with bm = 0.9:
      0.100000024 against 0.1).  Each side is within the bound of the float64 form, which counts the kernel's
      roundings, the CPU branch's being a subset of them."""
    out = str(tmp_path / "adam_cpu.npz")
    mp.spawn(_adam_cpu_worker, args=(1, C.free_port(), out), nprocs=1, join=True)
    z = np.load(out)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(C.free_port()), RANK="0", WORLD_SIZE="1")
    from pika_amd.bmuf import BmufAdamTrainer
    model = C.make_model(0).to(hip_device)
    optim = C.make_adam(model)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)    # noqa: E731
    worst = 0.0
    try:
        tr = BmufAdamTrainer(0, 0, 1, model, C.BM, C.BLR, C.SYNC_PERIOD, optim)
        assert tr.is_hip and next(model.parameters()).data_ptr() == tr.local.data_ptr()
        for rnd in range(C.ROUNDS):
            b = lambda k: z["before%d_%s" % (rnd, k)]       # noqa: E731
            a = lambda k: z["after%d_%s" % (rnd, k)]        # noqa: E731
            off = 0
            tr.local.copy_(dev(b("local")))
            tr.param.copy_(dev(b("global")))
            tr.delta_prev.copy_(dev(b("delta_prev")))
            tr.exp_avg.copy_(dev(b("blk_m")))
            tr.exp_avg_sq.copy_(dev(b("blk_v")))
            tr.rho = float(b("rho"))
            for i, p in enumerate(model.parameters()):
                k = p.numel()
                st = optim.state[p]
                if "exp_avg" not in st:         # what Adam's first step creates
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                st["step"].fill_(float(b("steps")[i]))
                st["exp_avg"].copy_(dev(b("m")[off:off + k]).view_as(p))
                st["exp_avg_sq"].copy_(dev(b("v")[off:off + k]).view_as(p))
                off += k
            assert tr.update_and_sync() == 1
            p, m, v, steps = C.adam_state(model, optim)
            assert Y.same(m, a("m")) and Y.same(v, a("v")), rnd
            assert Y.same(tr.exp_avg.cpu().numpy(), a("blk_m")) and Y.same(tr.exp_avg_sq.cpu().numpy(), a("blk_v")), rnd
            assert np.array_equal(steps, a("steps")) and tr.rho == float(a("rho")), rnd
            # the moments live in the exchange buffer the kernels wrote
            st0 = optim.state[next(model.parameters())]
            assert st0["exp_avg"].data_ptr() == tr.xch.data_ptr() + 4 * tr.num_param
            d = b("global") - b("local")
            dp64, g64, edp, eg = Y.bmuf_update64(d, b("delta_prev"), b("global"), 1, C.BM, C.BLR)
            want_dp, want_g = Y.bmuf_update(d, b("delta_prev"), b("global"), 1, C.BM, C.BLR)
            got_dp, got_g = tr.delta_prev.cpu().numpy(), tr.param.cpu().numpy()
            assert Y.same(got_dp, want_dp) and Y.same(got_g, want_g) and Y.same(p, want_g), rnd   # the kernel's yardstick
            for got, cpu, w64, e in ((got_dp, a("delta_prev"), dp64, edp), (got_g, a("global"), g64, eg),
                                     (p, a("local"), g64, eg)):
                assert Y.worst_ratio(got, w64, e) <= 1.0 and Y.worst_ratio(cpu, w64, e) <= 1.0, rnd
                r = float((np.abs(got.astype(np.float64) - cpu) / (2 * e)).max())
                worst = max(worst, r)
                assert r <= 1.0, (rnd, r)
        print("BmufAdamTrainer device vs CPU: worst |difference| / (2 bound) = %.3f" % worst)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
