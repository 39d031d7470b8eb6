"""The joint network on a pruned (banded) lattice without a GPU: the two C entry points are declared, exported and bound
and refuse bad arguments before any launch; `joint_pruned` and `rnnt_pruned_joint_loss` resolve from the package;
`joint_pruned` on CPU tensors is the formula on `rnnt_prune_lm`'s rows; and the two statements of the prediction-side sum
that tests/test_joint_banded_gpu.py relies on (a loop over t with the membership test; gather, then index_add) agree."""
import ctypes
import inspect
import os
import re

import numpy as np
import torch

import joint_banded_common as JB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIKA_EINVAL, PIKA_ETOOBIG = -1, -2
ENTRIES = {
    "pika_joint_gate_banded_fwd": "e1 p1 eg pg ranges h out_dtype B T U S H stream",
    "pika_joint_gate_banded_bwd": "dh dh_dtype e1 p1 eg pg ranges de1 dp1 deg dpg B T U S H stream",
}


def test_entries_are_declared_exported_and_bound_and_the_abi_is_25():
    from pika_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pika_joint.h")).read(), flags=re.S)
    L = _lib.lib()
    assert _lib.ABI_VERSION == 25 and L.pika_amd_abi_version() == 25
    for name, params in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/pika_joint.h" % name
        declared = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert declared == params.split()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(L, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(declared)


def test_entries_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    L = _lib.lib()
    q = ctypes.c_void_p(256)               # never dereferenced: every call below returns before a launch
    for fn, params in ENTRIES.items():
        names = params.split()
        ints = dict(out_dtype=0, dh_dtype=1, B=2, T=5, U=4, S=2, H=8, stream=None)
        ok = {n: ints.get(n, q) for n in names}

        def call(**kw):
            a = dict(ok, **kw)
            return getattr(L, fn)(*[a[n] for n in names])
        for n in names:
            if n not in ints:
                assert call(**{n: None}) == PIKA_EINVAL, (fn, n)
        for n in ("B", "T", "U", "S", "H"):
            assert call(**{n: 0}) == PIKA_EINVAL and call(**{n: -3}) == PIKA_EINVAL, (fn, n)
        assert call(H=6) == PIKA_EINVAL and call(H=2) == PIKA_EINVAL
        assert call(S=5) == PIKA_EINVAL                                   # S > U
        dt = "out_dtype" if "out_dtype" in names else "dh_dtype"
        assert call(**{dt: 2}) == PIKA_EINVAL and call(**{dt: -1}) == PIKA_EINVAL
        assert call(B=65536) == PIKA_ETOOBIG
        assert call(B=65536, H=6) == PIKA_EINVAL                          # a bad argument comes before the size


def test_python_entry_points_resolve_from_the_package():
    import pika_amd
    from pika_amd import rnnt
    from pika_amd.model import hipops, ops
    assert pika_amd.joint_pruned is ops.joint_pruned and "joint_pruned" in dir(pika_amd)
    assert pika_amd.rnnt_pruned_joint_loss is rnnt.rnnt_pruned_joint_loss and "rnnt_pruned_joint_loss" in dir(pika_amd)
    assert issubclass(hipops.BandedGateFn, torch.autograd.Function)
    sig = inspect.signature(ops.joint_pruned)
    assert list(sig.parameters) == ["enc", "pred", "ranges", "s_range", "fc1", "fc_gate", "fc2", "log_softmax", "scale"]
    assert sig.parameters["log_softmax"].default is False and sig.parameters["scale"].default == 1.0
    sig = inspect.signature(rnnt.rnnt_pruned_joint_loss)
    assert list(sig.parameters) == ["enc", "pred", "labels", "frames_lengths", "labels_lengths", "fc1", "fc_gate", "fc2",
                                    "simple_am", "simple_lm", "s_range", "blank", "fastemit_lambda", "reduction"]
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == dict(
        s_range=5, blank=0, fastemit_lambda=0.0, reduction="sum")


def test_joint_pruned_on_cpu_is_the_formula_on_the_band_rows():
    from pika_amd import joint_pruned
    from pika_amd.rnnt import rnnt_prune_lm
    B, T, U1, H, Jw, V, S = 2, 6, 5, 8, 12, 7, 3
    g = torch.Generator().manual_seed(3)
    enc, pred = torch.randn(B, T, H, generator=g), torch.randn(B, U1, H, generator=g)
    torch.manual_seed(4)
    fc1, fcg, fc2 = torch.nn.Linear(2 * H, Jw), torch.nn.Linear(2 * H, Jw), torch.nn.Linear(Jw, V)
    ranges = torch.tensor([[0, 1, 2, 2, 9, -4], [2, 0, 1, -1, 7, 2]], dtype=torch.int32)     # 9, 7 -> 2; -4, -1 -> 0
    d = lambda t: t.detach().double()   # noqa: E731
    e1 = d(enc) @ d(fc1.weight)[:, :H].T + d(fc1.bias)
    eg = d(enc) @ d(fcg.weight)[:, :H].T + d(fcg.bias)
    p1 = rnnt_prune_lm(d(pred) @ d(fc1.weight)[:, H:].T, ranges, S)
    pg = rnnt_prune_lm(d(pred) @ d(fcg.weight)[:, H:].T, ranges, S)
    assert torch.equal(p1[0, 4], (d(pred) @ d(fc1.weight)[:, H:].T)[0, 2:5])                 # the clamp of 9
    assert torch.equal(p1[1, 3], (d(pred) @ d(fc1.weight)[:, H:].T)[1, 0:3])                 # the clamp of -1
    h = torch.tanh(e1[:, :, None] + p1) * torch.sigmoid(eg[:, :, None] + pg)
    want = h @ d(fc2.weight).T + d(fc2.bias)
    got = joint_pruned(enc, pred, ranges, S, fc1, fcg, fc2).detach()
    assert got.shape == (B, T, S, V) and got.dtype == torch.float32
    assert float((got.double() - want).abs().max()) < 1e-6
    got = joint_pruned(enc, pred, ranges, S, fc1, fcg, fc2, log_softmax=True, scale=0.7).detach()
    assert float((got.double() - torch.log_softmax(0.7 * want, -1)).abs().max()) < 1e-6
    # the band that is the lattice is ops.joint
    from pika_amd.model.ops import joint
    full = joint_pruned(enc, pred, torch.zeros(B, T, dtype=torch.int32), U1, fc1, fcg, fc2).detach()
    assert float((full - joint(enc, pred, fc1, fcg, fc2, log_softmax=False).detach()).abs().max()) < 1e-6


def test_the_two_statements_of_the_prediction_side_sum_agree():
    """On a non-monotone `ranges` with clamped entries, in float64: the loop over t with the membership test (the
    definition in include/pika_joint.h) equals gathering the rows and adding dz back with index_add_ (the oracle of the GPU
    test).  A row outside every band is exactly zero in both."""
    B, T, U, S, H = 2, 9, 7, 3, 4
    g = torch.Generator().manual_seed(0)
    e1, eg = torch.randn(B, T, H, generator=g), torch.randn(B, T, H, generator=g)
    p1, pg = torch.randn(B, U, H, generator=g), torch.randn(B, U, H, generator=g)
    dh = torch.randn(B, T, S, H, generator=g)
    ranges = np.array([[4, 0, 3, 1, 11, -2, 4, 0, 2], [0, 4, 0, 4, 0, 4, 9, -5, 4]], np.int32)
    assert (np.diff(ranges, axis=1) < 0).any()
    rows = JB.band_rows(ranges, U, S)
    assert int(rows.min()) == 0 and int(rows.max()) == U - 1
    cov = JB.covered(ranges, U, S)
    assert cov[0].all() and cov[1].tolist() == [True, True, True, False, True, True, True]
    de1, dp1, deg, dpg = JB.banded_gate_bwd_ref(dh, e1, p1, eg, pg, ranges, S)
    # dz of every band row, straight from the formulas
    bidx = torch.arange(B)[:, None, None].expand(B, T, S)
    z1 = e1.double()[:, :, None] + p1.double()[bidx, rows]
    zg = eg.double()[:, :, None] + pg.double()[bidx, rows]
    th, sg = torch.tanh(z1), torch.sigmoid(zg)
    dz1 = dh.double() * sg * (1 - th * th)
    dzg = dh.double() * th * sg * (1 - sg)
    for dz, dp, de in ((dz1, dp1, de1), (dzg, dpg, deg)):
        loop = JB.pred_side_loop_ref(dz, ranges, U)
        assert float((loop - dp).abs().max()) < 1e-12
        assert (loop[1, 3] == 0).all() and (dp[1, 3] == 0).all()
        assert float((dz.sum(2) - de).abs().max()) < 1e-12
    h = JB.banded_gate_ref(e1, p1, eg, pg, ranges, S)
    assert float((h - th * sg).abs().max()) < 1e-12


def test_the_test_ranges_are_what_they_claim():
    for shape in JB.SHAPES:
        B, T, U, S, H = shape
        for kind in JB.KINDS:
            r = JB.make_ranges(shape, kind)
            assert r.shape == (B, T) and r.dtype == np.int32
            if kind != "clamped":
                assert r.min() >= 0 and r.max() <= U - S
        c = JB.make_ranges(shape, "clamped")
        assert (c == -3).any() and (T * B < 2 or (c == U + 7).any())
    assert not JB.covered(JB.make_ranges(JB.UNCOVERED_SHAPE, "nonmonotone"), 9, 4)[0, 4]
