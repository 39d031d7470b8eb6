"""CPU-side checks of the long-form alignment's surface: exports and signatures, docstrings, the header against the ctypes
table, the scratch formula, every refusal of the C ABI entry (no launch, no GPU), and the CPU-tensor refusal."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty
SIGNATURES = {
    "ctc_long_align": [("log_probs", E), ("targets", E), ("input_lengths", None), ("target_lengths", None), ("blank", 0)],
    "ctc_long_align_from_logits": [("logits", E), ("targets", E), ("input_lengths", None), ("target_lengths", None),
                                   ("blank", 0)],
    "ctc_segment_scores": [("starts", E), ("ends", E), ("token_scores", E), ("segment_offsets", E)],
}
EINVAL, ETOOBIG = -1, -2


def test_exports_signatures_and_docstrings():
    import pika_amd
    from pika_amd import ctc
    for name, want in SIGNATURES.items():
        fn = getattr(ctc, name)
        assert getattr(pika_amd, name) is fn and name in pika_amd._CTC_EXPORTS and name in dir(pika_amd)
        assert [(p.name, p.default) for p in inspect.signature(fn).parameters.values()] == want, name
        assert name in ctc.__doc__
    assert ctc.LONG_ALIGN_TILE > 0 and ctc.LONG_ALIGN_FRAMES > 0 and ctc.LONG_ALIGN_FRAMES % 4 == 0
    assert ctc.LONG_ALIGN_TILE + 2 * ctc.LONG_ALIGN_FRAMES <= 1024      # a tile and what it recomputes: one workgroup
    doc = ctc.ctc_long_align.__doc__
    for word in ("wildcard", "no host synchronisation", "bit-identical", "LONG_ALIGN_TILE", "ctc_segment_scores"):
        assert word in doc, word
    assert "ctc_long_align" in ctc.ctc_long_align_from_logits.__doc__
    assert "NaN" in ctc.ctc_segment_scores.__doc__
    for text in ("README.md", "DESIGN.md"):
        assert "ctc_long_align" in open(os.path.join(ROOT, text)).read(), text


def test_header_and_ctypes_table_declare_the_symbols():
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25                       # new symbols only
    header = open(os.path.join(ROOT, "include", "pika_ctc.h")).read()
    lib = _lib.lib()
    assert lib.pika_amd_abi_version() == 25
    for sym, res_c, res, count in (("pika_ctc_long_align", "int", ctypes.c_int, 18),
                                   ("pika_ctc_long_align_scratch_bytes", "size_t", ctypes.c_size_t, 3)):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        decl = re.search(r"\b%s %s\((.*?)\);" % (res_c, sym), header, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        got_res, args = _lib.SIGNATURES[sym]
        assert got_res is res and len(args) == len(params) == count, sym
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_longlong if p.startswith("long long ") else ctypes.c_int
            assert a is want, (sym, p, a)
    assert "U_max <= 2^28" in header                    # the limit on U_max is stated


def test_scratch_formula_and_refused_shapes():
    from pika_amd import _lib, ctc
    lib = _lib.lib()
    W = ctc.LONG_ALIGN_TILE

    def formula(B, T, U):
        Sp = -(-(2 * U + 1) // W) * W
        G = -(-T // 4)
        return B * G * Sp + 8 * B * Sp + 4 * B * 4 * G + 4 * B * 4 * G + 16 * B
    for B, T, U in ((1, 1, 0), (1, 7, 3), (2, 64, W // 2), (3, 65, W // 2 + 1), (1, 4000, 511), (1, 90000, 15000),
                    (2, 130, W + 1)):
        assert lib.pika_ctc_long_align_scratch_bytes(B, T, U) == formula(B, T, U), (B, T, U)
    # an hour against its transcript: two bits per cell, not three fp32 planes
    assert lib.pika_ctc_long_align_scratch_bytes(1, 90000, 15000) < 90000 * 30001 * 0.26
    for B, T, U in ((0, 5, 1), (-1, 5, 1), (1, 0, 1), (1, -3, 1), (1, 5, -1), (65536, 5, 1), (1, 5, 2 ** 28 + 1),
                    (1, 5, 2 ** 31 - 1), (65535, 2 ** 31 - 1, 2 ** 28)):
        assert lib.pika_ctc_long_align_scratch_bytes(B, T, U) == 0, (B, T, U)


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)     # never dereferenced: every call below is refused
    good = dict(B=2, T=9, C=5, blank=0, U=3)
    # q: x, lse, input_lengths, targets, target_lengths, scores, starts, ends, token_scores, scratch

    def call(q, B, T, C, blank, U):
        return lib.pika_ctc_long_align(q[0], 5 * 2, 5, q[1], q[2], q[3], q[4], B, T, C, blank, U, q[5], q[6], q[7], q[8],
                                       q[9], None)
    full = [p] * 10
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-2 ** 31), dict(C=0), dict(C=-4), dict(U=-1), dict(blank=-1),
               dict(blank=5), dict(blank=2 ** 31 - 1)):
        assert call(full, **dict(good, **kw)) == EINVAL, kw
    for kw in (dict(B=65536), dict(U=2 ** 28 + 1), dict(U=2 ** 31 - 1), dict(B=65535, T=2 ** 31 - 1, U=2 ** 28)):
        assert call(full, **dict(good, **kw)) == ETOOBIG, kw
    assert call(full, **dict(good, U=2 ** 31 - 1, B=-1)) == EINVAL          # a negative size first
    assert call(full, **dict(good, B=65536, blank=7)) == EINVAL
    assert call([None] * 10, **dict(good, B=65536)) == ETOOBIG              # sizes before pointers
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9):                                  # every pointer but lse (index 1)
        assert call([None if j == i else p for j in range(10)], **good) == EINVAL, i
    # lse NULL, and targets NULL with U_max == 0, are no refusals: only another missing pointer makes these calls refuse
    for i in (0, 2, 4, 5, 6, 7, 8, 9):
        q = [None if j in (i, 1) else p for j in range(10)]
        assert call(q, **good) == EINVAL, i
        q[3] = None
        assert call(q, **dict(good, U=0)) == EINVAL, i
    q = [p] * 10
    q[3] = None
    assert call(q, **good) == EINVAL                                        # targets missing with U_max > 0


def test_cpu_tensors_and_bad_arguments_are_refused():
    from pika_amd import ctc
    lp = torch.zeros(6, 2, 4).log_softmax(-1)
    tg = torch.ones(2, 3, dtype=torch.int64)
    for fn in (ctc.ctc_long_align, ctc.ctc_long_align_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp, tg)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp[:, 0], tg[0], [6], [3])
    with pytest.raises(ValueError, match="must share one shape"):
        ctc.ctc_segment_scores(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32),
                               torch.zeros(2, 3), torch.tensor([0, 3]))
    with pytest.raises(TypeError, match="segment_offsets must be int32 or int64"):
        ctc.ctc_segment_scores(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32),
                               torch.zeros(2, 3), torch.tensor([0.0, 3.0]))
    with pytest.raises(ValueError, match="segment_offsets must be"):
        ctc.ctc_segment_scores(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32),
                               torch.zeros(2, 3), torch.zeros(3, 2, dtype=torch.int64))
