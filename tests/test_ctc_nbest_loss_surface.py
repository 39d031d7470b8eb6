"""CPU-side checks of the n-best loss's surface: exports, signatures, the header and the ctypes table, the workspace
formula and the argument refusals of the C ABI (no launch, no GPU), the exceptions the Python wrappers raise, and
`ctc_nbest_errors` on a hand-checked list."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty
LIST = [("input_lengths", E), ("tokens", E), ("lengths", E)]
TAIL = [("blank", 0), ("max_len", None)]
SIGNATURES = {
    "ctc_nbest_loss": [("log_probs", E)] + LIST + TAIL,
    "ctc_nbest_loss_from_logits": [("logits", E)] + LIST + TAIL,
    "ctc_mwer_loss": [("log_probs", E)] + LIST + [("errors", E)] + TAIL + [("reduction", "mean")],
    "ctc_mwer_loss_from_logits": [("logits", E)] + LIST + [("errors", E)] + TAIL + [("reduction", "mean")],
    "ctc_nbest_errors": [("tokens", E), ("lengths", E), ("targets", E), ("target_lengths", E)],
}
SYMBOLS = ("pika_ctc_nbest_loss_workspace_bytes", "pika_ctc_nbest_loss_forward", "pika_ctc_nbest_loss_backward")


def test_exports_and_signatures():
    import pika_amd
    from pika_amd import ctc
    for name, want in SIGNATURES.items():
        fn = getattr(ctc, name)
        assert getattr(pika_amd, name) is fn and name in pika_amd._CTC_EXPORTS and name in dir(pika_amd)
        assert [(p.name, p.default) for p in inspect.signature(fn).parameters.values()] == want, name
    assert "ctc_nbest_loss" in ctc.ctc_nbest_align.__doc__ and "No autograd, no host" not in ctc.ctc_nbest_align.__doc__
    assert "SYNCHRONISES" in ctc.ctc_nbest_errors.__doc__


def test_header_and_ctypes_table_declare_the_symbols():
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25
    header = open(os.path.join(ROOT, "include", "pika_ctc.h")).read()
    lib = _lib.lib()
    assert lib.pika_amd_abi_version() == 25
    for sym, count in zip(SYMBOLS, (4, 17, 15)):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        decl = re.search(r"\b%s\((.*?)\);" % sym, header, re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        res, args = _lib.SIGNATURES[sym]
        assert len(args) == len(params) == count, sym
        for p, a in zip(params, args):
            want = ctypes.c_int if p.startswith("int ") and "*" not in p else (
                ctypes.c_longlong if p.startswith("long long ") else ctypes.c_void_p)
            assert a is want, (sym, p, a)
    assert _lib.SIGNATURES[SYMBOLS[0]][0] is ctypes.c_size_t
    assert _lib.SIGNATURES[SYMBOLS[1]][0] is ctypes.c_int and _lib.SIGNATURES[SYMBOLS[2]][0] is ctypes.c_int


def test_workspace_bytes_follow_the_header():
    from pika_amd import _lib
    lib = _lib.lib()
    for B, N, T, U in [(32, 16, 240, 63), (1, 1, 1, 0), (3, 4, 9, 31), (3, 4, 9, 32), (2, 64, 1000, 511)]:
        Wp = (2 * U + 1 + 63) // 64 * 64
        want = 8 * B * N * T * Wp + 16 * B * N * T + 8 * B * N + 12 * B * N * Wp
        assert lib.pika_ctc_nbest_loss_workspace_bytes(B, N, T, U) == want > 0
    for dims in [(0, 1, 5, 1), (1, 0, 5, 1), (1, 1, 0, 1), (1, 1, 5, -1), (-1, 1, 5, 1), (1, -2, 5, 1), (1, 1, 5, 512),
                 (65536, 1, 5, 1), (1, 65536, 5, 1), (65535, 65535, 2 ** 31 - 1, 511)]:
        assert lib.pika_ctc_nbest_loss_workspace_bytes(*dims) == 0, dims


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2
    p = ctypes.c_void_p(0x1000)     # never dereferenced: EVERY call below is refused before any launch
    good = dict(B=2, N=3, L=6, T=5, C=4, blank=0, U=3)

    def forward(q, B, N, L, T, C, blank, U):
        # q: x, lse, input_lengths, tokens, lengths, full_scores, workspace
        return lib.pika_ctc_nbest_loss_forward(q[0], 20, 4, q[1], q[2], q[3], q[4], B, N, L, T, C, blank, U, q[5], q[6],
                                               None)

    def backward(q, B, N, L, T, C, blank, U):
        # q: x, lse, input_lengths, grad_scores, workspace, grads
        return lib.pika_ctc_nbest_loss_backward(q[0], 20, 4, q[1], q[2], B, N, T, C, blank, U, q[3], q[4], q[5], None)
    for call, n in ((forward, 7), (backward, 6)):
        full = [p] * n
        bad = [dict(B=0), dict(N=0), dict(T=0), dict(C=0), dict(B=-1), dict(N=-1), dict(T=-3), dict(U=-1),
               dict(blank=-1), dict(blank=4)] + ([dict(L=0), dict(L=-2)] if call is forward else [])
        for kw in bad:
            assert call(full, **dict(good, **kw)) == EINVAL, (call.__name__, kw)
        for kw in (dict(U=512), dict(B=65536), dict(N=65536), dict(B=65535, N=65535, T=2 ** 31 - 1, U=511)):
            assert call(full, **dict(good, **kw)) == ETOOBIG, (call.__name__, kw)
        assert call(full, **dict(good, U=512, blank=7)) == EINVAL       # dimensions first
        for i in range(n):
            if i == 1:
                continue                # lse may be NULL: x then holds log-probs (not called: it would launch)
            assert call([None if j == i else p for j in range(n)], **good) == EINVAL, (call.__name__, i)


def test_python_wrappers_raise_the_documented_exceptions():
    from pika_amd import ctc
    lp, il = torch.zeros(5, 2, 4), torch.tensor([5, 5])
    tokens, lengths = torch.ones(2, 3, 6, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32)
    errors = torch.zeros(2, 3)
    for base, extra in ((ctc.ctc_nbest_loss, ()), (ctc.ctc_nbest_loss_from_logits, ()),
                        (ctc.ctc_mwer_loss, (errors,)), (ctc.ctc_mwer_loss_from_logits, (errors,))):
        def fn(x, il, tokens, lengths, **kw):
            return base(x, il, tokens, lengths, *extra, **kw)
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
    # what MWER adds, on scores that need no device
    full = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="reduction"):
        ctc._mwer(full, errors, "median")
    with pytest.raises(TypeError, match="errors must be a float tensor"):
        ctc._mwer(full, errors.long(), "mean")
    with pytest.raises(ValueError, match="errors must be"):
        ctc._mwer(full, errors[:, :2], "mean")


def test_nbest_errors_on_a_hand_checked_list():
    from pika_amd import ctc
    tokens = torch.tensor([[[1, 2, 3, 9], [1, 3, 9, 9], [3, 2, 1, 4], [9, 9, 9, 9], [7, 7, 7, 7]],
                           [[5, 6, 9, 9], [9, 9, 9, 9], [6, 5, 9, 9], [5, 5, 6, 6], [1, 1, 1, 1]]])
    lengths = torch.tensor([[3, 2, 4, 0, -1], [2, 0, 2, 4, -1]])
    targets = torch.tensor([[1, 2, 3], [5, 6, 0]])
    out = ctc.ctc_nbest_errors(tokens, lengths, targets, torch.tensor([3, 2]))
    assert out.dtype == torch.float32 and out.device.type == "cpu"
    #   [1,2,3]: 0   [1,3]: 1 (one deletion)   [3,2,1,4]: 3   []: 3   missing: 0
    #   [5,6]: 0     []: 2                      [6,5]: 2       [5,5,6,6]: 2   missing: 0
    assert out.tolist() == [[0.0, 1.0, 3.0, 3.0, 0.0], [0.0, 2.0, 2.0, 2.0, 0.0]]
    one = ctc.ctc_nbest_errors(tokens[1].to(torch.int32), lengths[1], targets[1, :2], torch.tensor(2))
    assert one.tolist() == [0.0, 2.0, 2.0, 2.0, 0.0]
    with pytest.raises(TypeError, match="targets must be int32 or int64"):
        ctc.ctc_nbest_errors(tokens, lengths, targets.float(), torch.tensor([3, 2]))
    with pytest.raises(ValueError, match="targets must be"):
        ctc.ctc_nbest_errors(tokens, lengths, targets[:1], torch.tensor([3, 2]))
