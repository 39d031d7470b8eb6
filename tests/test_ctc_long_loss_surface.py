"""CPU-side checks of the long-form loss's surface: exports and signatures, docstrings, the header against the ctypes
table, the workspace formula, every refusal of the C ABI entries (no launch, no GPU), and the Python exceptions."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOBIG = -1, -2
SYMBOLS = (("pika_ctc_long_loss_workspace_bytes", "size_t", ctypes.c_size_t, 3),
           ("pika_ctc_long_loss_forward", "int", ctypes.c_int, 15), ("pika_ctc_long_loss_backward", "int", ctypes.c_int, 15))


def test_exports_signatures_and_docstrings():
    import pika_amd
    from pika_amd import ctc
    want = [(p.name, p.default) for p in inspect.signature(ctc.ctc_loss).parameters.values()]
    for name, first in (("ctc_long_loss", "log_probs"), ("ctc_long_loss_from_logits", "logits")):
        fn = getattr(ctc, name)
        assert getattr(pika_amd, name) is fn and name in pika_amd._CTC_EXPORTS and name in dir(pika_amd)
        got = [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
        assert got[1:] == want[1:] and got[0] == (first, inspect.Parameter.empty), name
        assert name in ctc.__doc__
    assert ctc.LONG_LOSS_TILE > 0 and ctc.LONG_LOSS_FRAMES > 0 and ctc.LONG_LOSS_FRAMES % 8 == 0
    assert ctc.LONG_LOSS_TILE + 2 * ctc.LONG_LOSS_FRAMES <= 1024       # a tile and what it recomputes: one workgroup
    doc = ctc.ctc_long_loss.__doc__
    for word in ("8 * B * T", "LONG_LOSS_TILE", "LONG_LOSS_FRAMES", "torch.cuda.graph", "bit-identical", "zero_infinity"):
        assert word in doc, word
    assert "ctc_long_loss" in ctc.ctc_long_loss_from_logits.__doc__ and "ctc_long_loss" in ctc.ctc_loss.__doc__
    assert "ctc_long_align" in ctc.ctc_align.__doc__                # the alignment keeps its limit and says where to go
    for text in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ctc_long_loss" in open(os.path.join(ROOT, text)).read(), text


def test_header_and_ctypes_table_declare_the_symbols():
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25                       # new symbols only
    header = open(os.path.join(ROOT, "include", "pika_ctc.h")).read()
    lib = _lib.lib()
    assert lib.pika_amd_abi_version() == 25
    for sym, res_c, res, count in SYMBOLS:
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        decl = re.search(r"\b%s %s\((.*?)\);" % (res_c, sym), header, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        got_res, args = _lib.SIGNATURES[sym]
        assert got_res is res and len(args) == len(params) == count, sym
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_longlong if p.startswith("long long ") else ctypes.c_int
            assert a is want, (sym, p, a)
    assert "8 B T Sp" in header and "U_max <= 2^28" in header


def test_workspace_formula_and_refused_shapes():
    from pika_amd import _lib, ctc
    lib = _lib.lib()
    W = ctc.LONG_LOSS_TILE

    def formula(B, T, U):
        Sp = -(-(2 * U + 1) // W) * W
        return 8 * B * T * Sp + 16 * B * T + 8 * B + 16 * B * Sp + 16 * B * (Sp // W) + 4 * B * T + 8 * B * U
    for B, T, U in ((1, 1, 0), (1, 7, 3), (2, 64, W // 2), (3, 65, W // 2 + 1), (8, 3000, 1500), (32, 1500, 600),
                    (2, 130, W + 1), (1, 90000, 20000)):
        assert lib.pika_ctc_long_loss_workspace_bytes(B, T, U) == formula(B, T, U) > 0, (B, T, U)
    for B, T, U in ((0, 5, 1), (-1, 5, 1), (1, 0, 1), (1, -3, 1), (1, 5, -1), (65536, 5, 1), (1, 5, 2 ** 28 + 1),
                    (1, 5, 2 ** 31 - 1), (65535, 2 ** 31 - 1, 2 ** 28)):
        assert lib.pika_ctc_long_loss_workspace_bytes(B, T, U) == 0, (B, T, U)
    # the one-workgroup entry points keep their limit
    assert lib.pika_ctc_workspace_bytes(1, 5, 512) == 0 and lib.pika_ctc_long_loss_workspace_bytes(1, 5, 512) > 0


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)     # never dereferenced: every call below is refused
    good = dict(B=2, T=9, C=5, blank=0, U=3)

    # q: x, lse, input_lengths, targets, target_lengths, costs / grads, workspace, grad_costs
    def forward(q, B, T, C, blank, U):
        return lib.pika_ctc_long_loss_forward(q[0], 10, 5, q[1], q[2], q[3], q[4], B, T, C, blank, U, q[5], q[6], None)

    def backward(q, B, T, C, blank, U):
        return lib.pika_ctc_long_loss_backward(q[0], 10, 5, q[1], q[2], q[4], B, T, C, blank, U, q[7], q[6], q[5], None)
    full = [p] * 8
    for call, optional in ((forward, (1, 7)), (backward, (1, 3, 7))):      # optional, or not an argument of the call
        for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-2 ** 31), dict(C=0), dict(C=-4), dict(U=-1), dict(blank=-1),
                   dict(blank=5), dict(blank=2 ** 31 - 1)):
            assert call(full, **dict(good, **kw)) == EINVAL, kw
        for kw in (dict(B=65536), dict(U=2 ** 28 + 1), dict(U=2 ** 31 - 1), dict(B=65535, T=2 ** 31 - 1, U=2 ** 28)):
            assert call(full, **dict(good, **kw)) == ETOOBIG, kw
        assert call(full, **dict(good, U=2 ** 31 - 1, B=-1)) == EINVAL          # a negative size first
        assert call(full, **dict(good, B=65536, blank=7)) == EINVAL
        assert call([None] * 8, **dict(good, B=65536)) == ETOOBIG              # sizes before pointers
        for i in range(8):
            if i in optional:
                continue
            assert call([None if j == i else p for j in range(8)], **good) == EINVAL, (call.__name__, i)
            if i == 3:
                continue            # targets: required only with U_max > 0, which the line above covered
            # with every optional pointer missing as well (targets too, at U_max == 0), this one still makes the call refuse
            q = [None if j == i or j in optional or j == 3 else p for j in range(8)]
            assert call(q, **dict(good, U=0 if call is forward else 3)) == EINVAL, (call.__name__, i)
    q = [p] * 8
    q[3] = None
    assert forward(q, **good) == EINVAL                                         # targets missing with U_max > 0


def test_python_exceptions():
    from pika_amd import ctc
    lp = torch.zeros(6, 2, 4).log_softmax(-1)
    tg = torch.ones(2, 3, dtype=torch.int64)
    il, tl = torch.tensor([6, 6]), torch.tensor([3, 2])
    for fn in (ctc.ctc_long_loss, ctc.ctc_long_loss_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp, tg, il, tl)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp[:, 0], tg[0], il[:1], tl[:1])
        with pytest.raises(ValueError, match="not a valid value for reduction"):
            fn(lp, tg, il, tl, reduction="median")
    # a long transcript on the CPU is refused for the device, not for its length: the routing comes after the checks
    long_tg = torch.ones(2, 600, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ctc.ctc_loss(lp, long_tg, il, torch.tensor([600, 600]))
