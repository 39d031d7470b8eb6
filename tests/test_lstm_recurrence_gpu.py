"""The C ABI of the training LSTM recurrence (include/pika_lstm.h: pika_lstm_train_pack -> _fwd -> _bwd, the persistent
launches of pika_amd/csrc/lstm_train.hip) against the float64 oracle of tests/lstm_common.py, on the test's own buffers.

Every width H = 256, 512, 768, 1024 (one kernel instantiation each) meets S in {1, 2, 3, 51, long}, B in {1, 15, 16, 17, 33,
the largest batch the device admits}, both recurrent gains and one saturated input.  Per case and tensor (out, gates,
cells; dgates from the kernel's own gates and cells, so forward error is not counted twice):

    max |kernel - oracle| <= max(4 * e_model, floor)        e_model = max |arithmetic model - oracle| on the same inputs

(tests/test_lstm_oracle.py shows on the CPU that this is inside 2e-5 and that a kernel losing a cross term, a bf16 term of
W_hh, the gate order or the cell carry is ten times outside it.)  Besides: error word 0 after every launch; sentinel bands
around every output untouched and every output element written; same bits from two runs; armed = 0 and armed = 1 alike and
the backward scratch left 0xff; rows of the first row block and steps of the past independent of what else runs.

Measured on an MI355X, the largest  error / e_model  over the cases of a width with S >= 2 (bound: 4):

    H      out    gates  cells  dgates  dgates end to end
    256    1.06   1.06   1.07   1.02    1.02
    512    1.04   1.06   1.04   1.07    0.98
    768    1.10   1.07   1.08   1.16    0.91
    1024   1.04   1.04   1.12   1.04    1.04

The kernels are as far from float64 as their stated arithmetic is, at every width.  Where S = 1 there is no product and
e_model is fp32 rounding (3e-8 .. 2e-7); the kernels' largest error there is 2.5e-7 on every tensor and width, under the
floor of 9.5e-7 that decides those cases."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_common as LC  # noqa: E402

WIDTHS = (256, 512, 768, 1024)
SENTINEL = 0xA5                 # bytes; as fp32 -2.87e-16: never a value of these tensors
HEAD = 1024                     # floats in front of an output
_GAVE_UP = []                   # a launch that reported a non-zero error word: nothing more is launched by this module


def _lib():
    from pika_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """A (B, S, W) fp32 output in the middle of a sentinel-filled buffer; the band behind it holds at least the rows a
    kernel that wrote its padded row block (16 rows) would reach."""

    def __init__(self, B, S, W):
        n = B * S * W
        tail = (-B % 16) * S * W + HEAD
        self.raw = torch.full((4 * (HEAD + n + tail),), SENTINEL, dtype=torch.uint8, device="cuda")
        self.lo, self.hi = 4 * HEAD, 4 * (HEAD + n)
        self.t = self.raw[self.lo:self.hi].view(torch.float32).view(B, S, W)

    def check(self, name):
        assert bool((self.raw[:self.lo] == SENTINEL).all()), "%s: bytes in front of the tensor written" % name
        assert bool((self.raw[self.hi:] == SENTINEL).all()), "%s: bytes behind the (B, S, .) extent written" % name
        words = self.raw[self.lo:self.hi].view(torch.int32)
        assert not bool((words == 0xA5A5A5A5 - (1 << 32)).any()), \
            "%s: elements never written" % name


def _status(work, what):
    word = ctypes.c_int(-1)
    assert _lib().pika_lstm_train_status(work.data_ptr(), ctypes.byref(word), _stream()) == 0
    if word.value != 0:
        _GAVE_UP.append(what)
        pytest.fail("%s: error word %d -- a workgroup gave up waiting; nothing more is launched" % (what, word.value))


def _pack(w):
    assert not _GAVE_UP, _GAVE_UP
    lib = _lib()
    H = w.shape[1]
    packed = torch.empty(lib.pika_lstm_train_packed_bytes(H), dtype=torch.uint8, device="cuda")
    assert lib.pika_lstm_train_pack(w.data_ptr(), H, packed.data_ptr(), _stream()) == 0
    return packed


def _forward(gx, packed):
    """-> out, gates, cells (device), all checks of a forward launch done."""
    assert not _GAVE_UP, _GAVE_UP
    lib = _lib()
    B, S, H4 = gx.shape
    H = H4 // 4
    nbytes = lib.pika_lstm_train_fwd_work_bytes(S, B, H)
    assert nbytes == 256 + 4 * ((B + 15) // 16) * S * 16 * H
    work = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")          # (the forward fills its own scratch)
    out, gates, cells = Guarded(B, S, H), Guarded(B, S, H4), Guarded(B, S, H)
    rc = lib.pika_lstm_train_fwd(gx.data_ptr(), packed.data_ptr(), out.t.data_ptr(), gates.t.data_ptr(), cells.t.data_ptr(),
                                 work.data_ptr(), work.numel(), S, B, H, _stream())
    assert rc == 0, rc
    _status(work, "pika_lstm_train_fwd B=%d S=%d H=%d" % (B, S, H))
    for name, g in (("out", out), ("gates", gates), ("cells", cells)):
        g.check(name)
    return out.t, gates.t, cells.t


def _scratch(S, B, H, fill=0xFF):
    nbytes = _lib().pika_lstm_train_bwd_work_bytes(S, B, H)
    assert nbytes == 256 + 1024 * S * ((B + 15) // 16) * (H // 16) ** 2
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")


def _backward(dy, packed, gates, cells, armed=1, work=None):
    """-> dgates (device); the scratch (fresh and 0xff-filled unless given) is 0xff behind its first 256 bytes afterwards."""
    assert not _GAVE_UP, _GAVE_UP
    lib = _lib()
    B, S, H = dy.shape
    if work is None:
        work = _scratch(S, B, H, 0xFF if armed else 0x5A)
    dg = Guarded(B, S, 4 * H)
    rc = lib.pika_lstm_train_bwd(dy.data_ptr(), packed.data_ptr(), gates.data_ptr(), cells.data_ptr(), dg.t.data_ptr(),
                                 work.data_ptr(), work.numel(), armed, S, B, H, _stream())
    assert rc == 0, rc
    _status(work, "pika_lstm_train_bwd B=%d S=%d H=%d armed=%d" % (B, S, H, armed))
    dg.check("dgates")
    assert bool((work[256:] == 0xFF).all()), "the backward scratch is not left as a memset leaves it"
    return dg.t


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _compare(names, got, want, model, tag):
    """Asserts max |got - want| <= max(4 * e_model, floor) per tensor; prints error / e_model."""
    line, bad = [], []
    for n, g, w, m in zip(names, got, want, model):
        g = g.cpu()
        assert bool(torch.isfinite(g).all()), (tag, n)
        e, e_model = LC.err(g, w), LC.err(m, w)
        line.append("%s %.2e / %.2e = %.2f" % (n, e, e_model, e / max(e_model, 1e-30)))
        if e > LC.bound(e_model, w):
            bad.append((n, e, e_model, LC.bound(e_model, w)))
    print("RATIO %s | %s" % (tag, " | ".join(line)))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_kernels_match_the_float64_oracle(case):
    B, S, H, gain, sat = LC.resolve(case, _cus())
    gx, w, dy = LC.inputs(B, S, H, gain, sat)
    gxd, dyd = gx.cuda(), dy.cuda()
    packed = _pack(w.cuda())
    out, gates, cells = _forward(gxd, packed)
    dg = _backward(dyd, packed, gates, cells)
    # the sums are in a fixed order by design: a second run on fresh scratch gives the same bits
    again = _forward(gxd, packed)
    assert all(_bits(a, b) for a, b in zip((out, gates, cells), again)), "forward: two runs differ"
    assert _bits(dg, _backward(dyd, packed, gates, cells)), "backward: two runs differ"

    tag = "H=%d %s" % (H, LC.case_id(case))
    _compare(("out", "gates", "cells"), (out, gates, cells), LC.forward(gx, w), LC.forward(gx, w, LC.MODEL), tag)
    gk, ck = gates.cpu(), cells.cpu()
    _compare(("dgates",), (dg,), (LC.backward(dy, w, gk, ck),), (LC.backward(dy, w, gk, ck, LC.MODEL),), tag)


@pytest.mark.parametrize("H", WIDTHS)
def test_forward_then_backward_end_to_end(H):
    """dgates of the chain fwd -> bwd against the oracle's own chain (the forward's error enters the gradient)."""
    B, S = 17, 51
    gx, w, dy = LC.inputs(B, S, H, 1, False, seed=1)
    packed = _pack(w.cuda())
    out, gates, cells = _forward(gx.cuda(), packed)
    dg = _backward(dy.cuda(), packed, gates, cells)
    _, g64, c64 = LC.forward(gx, w)
    _, g32, c32 = LC.forward(gx, w, LC.MODEL)
    _compare(("dgates_e2e",), (dg,), (LC.backward(dy, w, g64, c64),), (LC.backward(dy, w, g32, c32, LC.MODEL),),
             "H=%d end-to-end B17-S51" % H)


@pytest.mark.parametrize("H", WIDTHS)
def test_armed_and_unarmed_backward_agree_and_leave_the_scratch_armed(H):
    """armed = 0: the launch fills a scratch full of garbage itself; armed = 1: the caller's 0xff.  Same bits, and either
    leaves every byte behind the first 256 at 0xff, so that the next launch on that scratch -- another (B, S) that fits --
    may be armed."""
    B, S = 17, 9
    gx, w, dy = LC.inputs(B, S, H, 1, False, seed=2)
    packed = _pack(w.cuda())
    _, gates, cells = _forward(gx.cuda(), packed)
    dyd = dy.cuda()
    work0, work1 = _scratch(S, B, H, 0x5A), _scratch(S, B, H, 0xFF)
    d0 = _backward(dyd, packed, gates, cells, armed=0, work=work0)
    d1 = _backward(dyd, packed, gates, cells, armed=1, work=work1)
    assert _bits(d0, d1)
    B2, S2 = 33, 5
    assert _lib().pika_lstm_train_bwd_work_bytes(S2, B2, H) <= work0.numel()
    gx2, _, dy2 = LC.inputs(B2, S2, H, 1, False, seed=3)
    _, gates2, cells2 = _forward(gx2.cuda(), packed)
    fresh = _backward(dy2.cuda(), packed, gates2, cells2)
    for work in (work0, work1):
        assert _bits(_backward(dy2.cuda(), packed, gates2, cells2, armed=1, work=work), fresh)
    # a single step exchanges nothing; the unarmed launch still owes the caller an armed scratch (include/pika_lstm.h)
    _, gates3, cells3 = _forward(gx2[:, :1].contiguous().cuda(), packed)
    _backward(dy2[:, :1].contiguous().cuda(), packed, gates3, cells3, armed=0, work=_scratch(1, B2, H, 0x5A))


@pytest.mark.parametrize("H", WIDTHS)
def test_a_row_block_does_not_depend_on_the_others(H):
    """An MFMA output row depends on its own A row only: rows [0, 16) of a 17- and a 33-row batch have the bits of the
    16-row batch.  A difference means a row block read another's slot."""
    S = 6
    gx, w, dy = LC.inputs(33, S, H, 2, False, seed=4)
    packed = _pack(w.cuda())
    runs = {}
    for B in (16, 17, 33):
        fwd = _forward(gx[:B].contiguous().cuda(), packed)
        runs[B] = fwd + (_backward(dy[:B].contiguous().cuda(), packed, fwd[1], fwd[2]),)
    for B in (17, 33):
        for name, a, b in zip(("out", "gates", "cells", "dgates"), runs[16], runs[B]):
            assert _bits(a, b[:16]), (B, name)
    for name, a, b in zip(("out", "gates", "cells", "dgates"), runs[17], runs[33]):
        assert _bits(a[16:17], b[16:17]), name


@pytest.mark.parametrize("H", WIDTHS)
def test_the_past_does_not_depend_on_the_future(H):
    B, S, S1 = 19, 12, 5
    gx, w, _ = LC.inputs(B, S, H, 2, False, seed=5)
    packed = _pack(w.cuda())
    whole = _forward(gx.cuda(), packed)
    part = _forward(gx[:, :S1].contiguous().cuda(), packed)
    for name, a, b in zip(("out", "gates", "cells"), whole, part):
        assert _bits(a[:, :S1], b), name


@pytest.mark.parametrize("H", WIDTHS)
def test_one_row_more_than_fits_is_refused_without_a_launch(H):
    lib = _lib()
    B, S = LC.max_batch(H, _cus()) + 1, 2
    gx = torch.zeros(B, S, 4 * H, device="cuda")
    packed = _pack(torch.zeros(4 * H, H, device="cuda"))
    out, gates, cells, dg = (torch.full(s, -7.0, device="cuda") for s in ((B, S, H), (B, S, 4 * H), (B, S, H), (B, S, 4 * H)))
    fw = torch.full((lib.pika_lstm_train_fwd_work_bytes(S, B, H),), 0x5A, dtype=torch.uint8, device="cuda")
    bw = torch.full((lib.pika_lstm_train_bwd_work_bytes(S, B, H),), 0x5A, dtype=torch.uint8, device="cuda")
    assert lib.pika_lstm_train_fwd(gx.data_ptr(), packed.data_ptr(), out.data_ptr(), gates.data_ptr(), cells.data_ptr(),
                                   fw.data_ptr(), fw.numel(), S, B, H, _stream()) == -2          # PIKA_ETOOBIG
    assert lib.pika_lstm_train_bwd(out.data_ptr(), packed.data_ptr(), gates.data_ptr(), cells.data_ptr(), dg.data_ptr(),
                                   bw.data_ptr(), bw.numel(), 0, S, B, H, _stream()) == -2
    torch.cuda.synchronize()
    assert bool((fw == 0x5A).all()) and bool((bw == 0x5A).all())          # not even the error word was cleared
    assert all(bool((t == -7.0).all()) for t in (out, gates, cells, dg))
