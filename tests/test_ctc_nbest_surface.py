"""CPU-side checks of the n-best alignment's surface: exports, signatures, the header and the ctypes table, the size
formula and the argument refusals of the C ABI (no launch, no GPU), and the exceptions the Python wrapper documents."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ctc_nbest_align", "ctc_nbest_align_from_logits")
SYMBOLS = ("pika_ctc_nbest_align_scratch_bytes", "pika_ctc_nbest_align")


def test_exports_and_signatures():
    import pika_amd
    from pika_amd import ctc
    for name, first in zip(NAMES, ("log_probs", "logits")):
        fn = getattr(ctc, name)
        assert getattr(pika_amd, name) is fn and name in pika_amd._CTC_EXPORTS and name in dir(pika_amd)
        got = [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
        e = inspect.Parameter.empty
        assert got == [(first, e), ("input_lengths", e), ("tokens", e), ("lengths", e), ("blank", 0), ("max_len", None)]
    assert "geometric mean" in ctc.ctc_nbest_align.__doc__ and "committed + tail" in ctc.ctc_nbest_align.__doc__


def test_header_and_ctypes_table_declare_the_symbols():
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25
    header = open(os.path.join(ROOT, "include", "pika_ctc.h")).read()
    lib = _lib.lib()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
    # the declared parameter list against the ctypes one: as many arguments, integers where the header says int
    decl = re.search(r"int pika_ctc_nbest_align\((.*?)\);", header, re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    res, args = _lib.SIGNATURES["pika_ctc_nbest_align"]
    assert res is ctypes.c_int and len(args) == len(params) == 21
    for p, a in zip(params, args):
        want = ctypes.c_int if p.startswith("int ") and "*" not in p else (
            ctypes.c_longlong if p.startswith("long long ") else ctypes.c_void_p)
        assert a is want, (p, a)
    assert _lib.SIGNATURES["pika_ctc_nbest_align_scratch_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)


def test_scratch_bytes_follow_the_header():
    from pika_amd import _lib
    lib = _lib.lib()
    for B, N, T, U in [(32, 16, 240, 240), (1, 1, 1, 0), (3, 4, 9, 31), (3, 4, 9, 32), (2, 64, 1000, 511), (1, 2, 5, 7)]:
        Wp = (2 * U + 1 + 63) // 64 * 64
        assert lib.pika_ctc_nbest_align_scratch_bytes(B, N, T, U) == B * N * ((T + 3) // 4) * Wp > 0
    for dims in [(0, 1, 5, 1), (1, 0, 5, 1), (1, 1, 0, 1), (1, 1, 5, -1), (-1, 1, 5, 1), (1, -2, 5, 1), (1, 1, 5, 512),
                 (65536, 1, 5, 1), (1, 65536, 5, 1)]:
        assert lib.pika_ctc_nbest_align_scratch_bytes(*dims) == 0, dims


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2
    p = ctypes.c_void_p(0x1000)     # never dereferenced: EVERY call below is refused before any launch
    good = dict(B=2, N=3, L=6, T=5, C=4, blank=0, U=3)

    def call(q, B, N, L, T, C, blank, U):
        # q: x, lse, input_lengths, tokens, lengths, full, best, starts, ends, token_scores, scratch
        return lib.pika_ctc_nbest_align(q[0], 20, 4, q[1], q[2], q[3], q[4], B, N, L, T, C, blank, U, q[5], q[6], q[7],
                                        q[8], q[9], q[10], None)
    full = [p] * 11
    for kw in (dict(B=0), dict(N=0), dict(L=0), dict(T=0), dict(C=0), dict(B=-1), dict(N=-1), dict(L=-2), dict(T=-3),
               dict(U=-1), dict(blank=-1), dict(blank=4)):
        assert call(full, **dict(good, **kw)) == EINVAL, kw
    for kw in (dict(U=512), dict(B=65536), dict(N=65536)):
        assert call(full, **dict(good, **kw)) == ETOOBIG, kw
    assert call(full, **dict(good, U=512, blank=7)) == EINVAL       # dimensions first
    for i in range(11):
        if i == 1:
            continue                # lse may be NULL: x then holds log-probs (not called: it would launch)
        assert call([None if j == i else p for j in range(11)], **good) == EINVAL, i


def test_python_wrapper_raises_the_documented_exceptions():
    from pika_amd import ctc
    lp, il = torch.zeros(5, 2, 4), torch.tensor([5, 5])
    tokens, lengths = torch.ones(2, 3, 6, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32)
    for fn in (ctc.ctc_nbest_align, ctc.ctc_nbest_align_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp, il, tokens, lengths)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp[:, 0], il[:1], tokens[0], lengths[0])
        with pytest.raises(TypeError, match="tokens must be int32 or int64"):
            fn(lp, il, tokens.float(), lengths)
        with pytest.raises(TypeError, match="lengths must be int32 or int64"):
            fn(lp, il, tokens, lengths.to(torch.int16))
        for bad in (torch.ones(2, 4, dtype=torch.int32), torch.ones(3, dtype=torch.int32),
                    torch.ones(2, 3, 6, dtype=torch.int32)):
            with pytest.raises(ValueError, match="tokens must be"):
                fn(lp, il, tokens, bad)
        with pytest.raises(ValueError, match="empty dimension"):
            fn(lp, il, tokens[:, :, :0], lengths)
        for max_len in (512, 1000, -1):
            with pytest.raises(ValueError, match="max_len"):
                fn(lp, il, tokens, lengths, max_len=max_len)
        with pytest.raises(ValueError, match="max_len"):            # L itself may be wide: the default stops at 511
            fn(lp, il, torch.ones(2, 3, 600, dtype=torch.int64), lengths, max_len=600)
