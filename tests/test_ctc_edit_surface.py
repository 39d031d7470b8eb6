"""CPU-side checks of the n-best edit distances' surface: exports and signatures, the header and the ctypes table, the
refusals of both C ABI entries (no launch, no GPU), and the exceptions the Python wrappers raise."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty
SIGNATURES = {
    "ctc_nbest_edit_distance": [("tokens", E), ("lengths", E), ("targets", E), ("target_lengths", E)],
    "ctc_nbest_pairwise_distance": [("tokens", E), ("lengths", E)],
    "ctc_nbest_mbr_decode": [("tokens", E), ("lengths", E), ("scores", E), ("scale", 1.0)],
}
SYMBOLS = ("pika_ctc_edit_distance", "pika_ctc_edit_distance_host")


def test_exports_and_signatures():
    import pika_amd
    from pika_amd import ctc
    for name, want in SIGNATURES.items():
        fn = getattr(ctc, name)
        assert getattr(pika_amd, name) is fn and name in pika_amd._CTC_EXPORTS and name in dir(pika_amd)
        assert [(p.name, p.default) for p in inspect.signature(fn).parameters.values()] == want, name
        assert name in ctc.__doc__
    # the host route keeps its signature and its warning; the new one promises the opposite
    assert [p for p in inspect.signature(ctc.ctc_nbest_errors).parameters] == [
        p for p in inspect.signature(ctc.ctc_nbest_edit_distance).parameters]
    assert "SYNCHRONISES" in ctc.ctc_nbest_errors.__doc__
    assert "no host synchronisation" in ctc.ctc_nbest_edit_distance.__doc__


def test_header_and_ctypes_table_declare_the_symbols():
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25                       # new symbols only
    header = open(os.path.join(ROOT, "include", "pika_ctc.h")).read()
    lib = _lib.lib()
    assert lib.pika_amd_abi_version() == 25
    for sym, count in zip(SYMBOLS, (11, 10)):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        decl = re.search(r"\bint %s\((.*?)\);" % sym, header, re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        res, args = _lib.SIGNATURES[sym]
        assert res is ctypes.c_int and len(args) == len(params) == count, sym
        for p, a in zip(params, args):
            assert a is (ctypes.c_int if p.startswith("int ") and "*" not in p else ctypes.c_void_p), (sym, p, a)
    # the shared recurrence is one function in one header, called by the kernel and by the host entry
    source = open(os.path.join(ROOT, "pika_amd", "csrc", "ctc_edit.hip")).read()
    core = open(os.path.join(ROOT, "pika_amd", "csrc", "ctc_edit_core.h")).read()
    assert len(re.findall(r"inline void ctc_edit_step\(", core)) == 1 and source.count("ctc_edit_step(") == 2
    assert "PIKA_EDIT_MAX_REF 4096" in core


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    from pika_amd.ctc import MAX_EDIT_REF
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2
    assert MAX_EDIT_REF == 4096
    p = ctypes.c_void_p(0x1000)     # never dereferenced: every call with it below is refused, or has no pair to work on
    good = dict(Na=3, La=6, Nr=2, Lr=5, B=2)

    def device(q, Na, La, Nr, Lr, B):
        # q: a_tokens, a_lengths, r_tokens, r_lengths, out
        return lib.pika_ctc_edit_distance(q[0], q[1], Na, La, q[2], q[3], Nr, Lr, B, q[4], None)

    def host(q, Na, La, Nr, Lr, B):
        return lib.pika_ctc_edit_distance_host(q[0], q[1], Na, La, q[2], q[3], Nr, Lr, B, q[4])
    for call in (device, host):
        full = [p] * 5
        for kw in (dict(Na=-1), dict(La=-1), dict(Nr=-1), dict(Lr=-1), dict(B=-1), dict(B=-2 ** 31), dict(La=-2 ** 31)):
            assert call(full, **dict(good, **kw)) == EINVAL, (call.__name__, kw)
        for kw in (dict(Lr=4097), dict(Lr=2 ** 31 - 1), dict(B=65536, Na=65536, Nr=1), dict(B=2 ** 16, Na=2 ** 14, Nr=2),
                   dict(B=2 ** 31 - 1, Na=2 ** 31 - 1, Nr=2 ** 31 - 1)):
            assert call(full, **dict(good, **kw)) == ETOOBIG, (call.__name__, kw)
        assert call(full, **dict(good, Lr=4097, B=-1)) == EINVAL        # a negative size first
        assert call([None] * 5, **dict(good, Lr=4097)) == ETOOBIG       # sizes before pointers
        for i in range(5):
            assert call([None if j == i else p for j in range(5)], **good) == EINVAL, (call.__name__, i)
        # no pair: success, nothing is touched, whatever the pointers; a wide hypothesis side is no limit
        for kw in (dict(B=0), dict(Na=0), dict(Nr=0), dict(B=0, La=10 ** 6, Lr=4096)):
            assert call(full, **dict(good, **kw)) == 0 and call([None] * 5, **dict(good, **kw)) == 0, (call.__name__, kw)
    # with a width of 0 that side's token pointer may be NULL (host entry: it runs)
    lengths = np.array([[2, 0, -1]], dtype=np.int32)
    r_tokens, r_lengths = np.array([[[4, 5, 6]]], dtype=np.int32), np.array([[3]], dtype=np.int32)
    out = np.zeros((1, 3, 1), dtype=np.int32)
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)      # noqa: E731
    assert lib.pika_ctc_edit_distance_host(None, ptr(lengths), 3, 0, ptr(r_tokens), ptr(r_lengths), 1, 3, 1,
                                           ptr(out)) == 0 and out.reshape(-1).tolist() == [3, 3, -1]
    out = np.zeros((1, 1, 3), dtype=np.int32)
    assert lib.pika_ctc_edit_distance_host(ptr(r_tokens), ptr(r_lengths), 1, 3, None, ptr(lengths), 3, 0, 1,
                                           ptr(out)) == 0 and out.reshape(-1).tolist() == [3, 3, -1]


def test_python_wrappers_raise_the_documented_exceptions():
    from pika_amd import ctc
    tokens, lengths = torch.ones(2, 3, 6, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32)
    targets, tl, scores = torch.ones(2, 4, dtype=torch.int64), torch.tensor([4, 2]), torch.zeros(2, 3)
    calls = ((ctc.ctc_nbest_edit_distance, (targets, tl)), (ctc.ctc_nbest_pairwise_distance, ()),
             (ctc.ctc_nbest_mbr_decode, (scores,)))
    for fn, extra in calls:
        fn(tokens, lengths, *extra)
        with pytest.raises(TypeError, match="tokens must be int32 or int64"):
            fn(tokens.float(), lengths, *extra)
        with pytest.raises(TypeError, match="lengths must be int32 or int64"):
            fn(tokens, lengths.to(torch.int16), *extra)
        for bad in (torch.ones(2, 4, dtype=torch.int32), torch.ones(3, dtype=torch.int32),
                    torch.ones(2, 3, 6, dtype=torch.int32)):
            with pytest.raises(ValueError, match="tokens must be"):
                fn(tokens, bad, *extra)
        with pytest.raises(ValueError, match="tokens must be"):
            fn(tokens[0, 0], lengths[0, 0], *extra)
    # what the reference side adds: `ctc_nbest_errors`'s exceptions, and the width limit
    with pytest.raises(TypeError, match="targets must be int32 or int64"):
        ctc.ctc_nbest_edit_distance(tokens, lengths, targets.float(), tl)
    with pytest.raises(TypeError, match="target_lengths must be int32 or int64"):
        ctc.ctc_nbest_edit_distance(tokens, lengths, targets, tl.float())
    for bad_targets, bad_tl in ((targets[:1], tl), (targets, tl[:1]), (targets[0], tl), (targets, torch.tensor(4))):
        with pytest.raises(ValueError, match="targets must be"):
            ctc.ctc_nbest_edit_distance(tokens, lengths, bad_targets, bad_tl)
    wide = torch.ones(2, 4097, dtype=torch.int64)
    assert ctc.ctc_nbest_edit_distance(tokens, lengths, wide[:, :4096], tl).tolist() == [[3.0] * 3, [1.0] * 3]
    with pytest.raises(ValueError, match="at most 4096"):
        ctc.ctc_nbest_edit_distance(tokens, lengths, wide, tl)
    # the list on both sides: its own width is the limit
    assert ctc.ctc_nbest_pairwise_distance(wide[:, None, :4096], torch.tensor([[4096], [7]])).tolist() == [[[0.0]], [[0.0]]]
    for fn, extra in ((ctc.ctc_nbest_pairwise_distance, ()), (ctc.ctc_nbest_mbr_decode, (torch.zeros(2, 1),))):
        with pytest.raises(ValueError, match="at most 4096"):
            fn(wide[:, None], torch.tensor([[5], [7]]), *extra)
    with pytest.raises(TypeError, match="scores must be a float tensor"):
        ctc.ctc_nbest_mbr_decode(tokens, lengths, scores.long())
    for bad in (scores[:, :2], scores[0], torch.zeros(2, 3, 1)):
        with pytest.raises(ValueError, match="scores must be"):
            ctc.ctc_nbest_mbr_decode(tokens, lengths, bad)
