"""CPU-side checks of `CtcBeamStream.commit`: the Python surface, the new entry points beside an unchanged ABI version,
their size functions, and the argument checks of the C entry points (refused before any launch, so no GPU is needed)."""
import inspect
import os

import pytest


def test_commit_is_part_of_the_class():
    from pika_amd import ctc

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][1:]
    S = ctc.CtcBeamStream
    assert sig(S.commit) == [("which", None), ("max_tail", None)]
    assert isinstance(S.consumed, property) and isinstance(S.room, property)
    assert ctc.STREAM_RETIRED_WORD == 3
    doc = " ".join(S.__doc__.split())
    for word in ("commit(which=None, max_tail=None)", "consumed", "room", "the host-side sum is not enforced"):
        assert word in doc, word


def test_new_symbols_beside_an_unchanged_abi_version():
    from pika_amd import _lib
    lib = _lib.lib()
    assert _lib.ABI_VERSION == 25 and lib.pika_amd_abi_version() == 25
    for prefix in ("pika_ctc_", "pika_ctc_lm_", "pika_ctc_lm2_"):
        for name in ("stream_commit", "stream_commit_scratch_bytes"):
            assert prefix + name in _lib.SIGNATURES and getattr(lib, prefix + name) is not None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pika_ctc_decode.h")).read()
    assert "#define PIKA_CTC_STREAM_RETIRED_OFFSET 12\n" in text
    assert "#define PIKA_CTC_STREAM_RECORD_BYTES 1824\n" in text


def test_scratch_bytes():
    from pika_amd import _lib
    lib = _lib.lib()
    plain = lib.pika_ctc_stream_commit_scratch_bytes

    def fused(B, F, beam):
        return lib.pika_ctc_lm_stream_commit_scratch_bytes(B, F, beam, 32)

    def fused2(B, F, beam):
        return lib.pika_ctc_lm2_stream_commit_scratch_bytes(B, F, beam, 32)
    for fn in (plain, fused, fused2):
        for bad in ((0, 10, 4), (2, 0, 4), (2, 10, 0), (-1, 10, 4), (2, 10, 65), (65536, 10, 4), (1, 2 ** 21 + 1, 64)):
            assert fn(*bad) == 0, bad
        for B, F, beam in ((1, 1, 1), (3, 24, 4), (3, 80, 16), (32, 600, 64), (1, 2 ** 21, 64)):
            got = fn(B, F, beam)
            assert got == 4 * B * F * beam                                  # the labels of one path per slot
            assert 0 < got <= lib.pika_ctc_beam_scratch_bytes(B, F, beam)   # never more than the tables
    assert lib.pika_ctc_lm_stream_commit_scratch_bytes(2, 10, 4, 0) == 0
    assert lib.pika_ctc_lm2_stream_commit_scratch_bytes(2, 10, 4, 129) == 0


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    N, P = None, 256            # P: a non-null pointer that is never followed -- every call below is refused first
    # commit(state, B, max_frames, beam, which, max_tail, L, tokens, lengths, scratch, stream)
    assert lib.pika_ctc_stream_commit(N, 1, 8, 4, N, -1, 8, P, P, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 8, 4, N, -1, 8, N, P, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 8, 4, N, -1, 8, P, N, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 8, 4, N, -1, 8, P, P, N, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 8, 4, N, -1, 0, P, P, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 8, 4, N, 3, -5, P, P, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 0, 8, 4, N, -1, 8, P, P, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 0, 4, N, -1, 8, P, P, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 8, 0, N, -1, 8, P, P, P, N) == -1
    assert lib.pika_ctc_stream_commit(P, 1, 8, 65, N, -1, 8, P, P, P, N) == -2
    assert lib.pika_ctc_stream_commit(P, 65536, 8, 4, N, -1, 8, P, P, P, N) == -2
    assert lib.pika_ctc_stream_commit(P, 1, 2 ** 21 + 1, 64, N, -1, 8, P, P, P, N) == -2
    # the LM forms: (state, B, max_frames, beam, candidates, which, max_tail, L, tokens, lengths, scratch, stream)
    for fn in (lib.pika_ctc_lm_stream_commit, lib.pika_ctc_lm2_stream_commit):
        assert fn(N, 1, 8, 4, 8, N, -1, 8, P, P, P, N) == -1
        assert fn(P, 1, 8, 4, 8, N, -1, 8, P, P, N, N) == -1
        assert fn(P, 1, 8, 4, 8, N, -1, 0, P, P, P, N) == -1
        assert fn(P, 1, 8, 4, 0, N, -1, 8, P, P, P, N) == -1
        assert fn(P, 1, 8, 4, 129, N, -1, 8, P, P, P, N) == -2
        assert fn(P, 1, 8, 65, 8, N, -1, 8, P, P, P, N) == -2


def test_commit_argument_errors():
    from pika_amd import ctc
    stream = object.__new__(ctc.CtcBeamStream)     # the checks come before anything touches the device
    stream.batch, stream.device = 3, "cpu"
    with pytest.raises(ValueError, match="max_tail"):
        stream.commit(max_tail=-1)
    with pytest.raises(ValueError, match="batch = 3"):
        stream.commit(which=[True, False])
    with pytest.raises(TypeError, match="which"):
        stream.commit(which=[0.5, 1.0, 0.0])
