"""CPU-side checks of the streaming one-symbol-per-frame beam search (include/pika_msearch_stream.h): symbols, the ctypes
table, the sizes of the side record and the scratch, the argument checks of the C entry points (refused before any
launch, so no GPU is needed) and the Python surface."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pika_msearch_stream_side_bytes", "pika_msearch_stream_reset", "pika_msearch_commit_scratch_bytes",
         "pika_msearch_commit", "pika_msearch_lm_commit")
N, P = None, 16        # (P: a non-null pointer that is never followed: the checks come before any launch)


def test_symbols_table_and_abi_version():
    from pika_amd import _lib
    lib = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pika_msearch_stream.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pika_[a-z0-9_]+)\s*\(", text))) == sorted(NAMES)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 25 and lib.pika_amd_abi_version() == 25
    # the offsets of the side record are public
    for macro in ("RETIRED_OFFSET", "OFFSET_OFFSET", "BONUS_OFFSET_OFFSET"):
        assert "#define PIKA_MSEARCH_STREAM_%s(B)" % macro in text


def test_sizes():
    from pika_amd import _lib
    lib = _lib.lib()
    side, scratch = lib.pika_msearch_stream_side_bytes, lib.pika_msearch_commit_scratch_bytes
    # i32 retired[B], f64 offset[B], f64 bonus_offset[B], each rounded up to 16 bytes
    assert side(1) == 16 + 16 + 16 and side(3) == 16 + 32 + 32 and side(4) == 16 + 32 + 32
    assert side(5) == 32 + 48 + 48 and side(65535) == 262144 + 2 * 524288
    assert side(0) == 0 and side(-1) == 0 and side(65536) == 0
    assert scratch(3, 4, 8) == 4 * 3 * 4 * 8 and scratch(1, 1, 1) == 4 and scratch(2, 64, 40) == 4 * 2 * 64 * 40
    for bad in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (2, 65, 8), (65536, 4, 8), (1, 64, 2 ** 21 + 1)):
        assert scratch(*bad) == 0, bad


def commit(lib, state=P, side=P, B=1, K=4, mf=8, which=N, max_tail=-1, rebase=0, L=8, outs=(P, P, P), scratch=P):
    return lib.pika_msearch_commit(*((state, side, B, K, mf, which, max_tail, rebase, L) + outs + (scratch, N)))


def lm_commit(lib, state=P, side=P, B=1, K=4, C=8, mf=8, which=N, max_tail=-1, rebase=0, L=8, outs=(P, P, P),
              scratch=P):
    return lib.pika_msearch_lm_commit(*((state, side, B, K, C, mf, which, max_tail, rebase, L) + outs + (scratch, N)))


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    assert lib.pika_msearch_stream_reset(N, 1, N, N) == -1
    assert lib.pika_msearch_stream_reset(P, 0, N, N) == -1 and lib.pika_msearch_stream_reset(P, -3, N, N) == -1
    assert lib.pika_msearch_stream_reset(P, 65536, N, N) == -2
    for fn in (commit, lm_commit):
        for kw in (dict(state=N), dict(side=N), dict(scratch=N), dict(outs=(N, P, P)), dict(outs=(P, N, P)),
                   dict(outs=(P, P, N)), dict(L=0), dict(L=-1), dict(B=0), dict(K=0), dict(mf=0)):
            assert fn(lib, **kw) == -1, (fn.__name__, kw)
        assert fn(lib, B=65536) == -2 and fn(lib, K=65, **({"C": 65} if fn is lm_commit else {})) == -2
    assert commit(lib, K=64, mf=2 ** 21 + 1) == -2
    assert lm_commit(lib, K=9) == -1 and lm_commit(lib, K=65, C=64) == -1            # K > C
    assert lm_commit(lib, C=65) == -2 and lm_commit(lib, C=0) == -1 and lm_commit(lib, C=64, mf=2 ** 21 + 1) == -2


def test_exports_and_signatures():
    import pika_amd
    from pika_amd.decoder import modified_search as S
    for name in ("ModifiedBeamStream", "ModifiedStreamDecoder"):
        assert getattr(pika_amd, name) is getattr(S, name) and name in dir(pika_amd)

    def sig(fn, skip=1):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][skip:]
    E = inspect.Parameter.empty
    C = S.ModifiedBeamStream
    assert sig(C.__init__) == [("batch", E), ("max_frames", E), ("beam", 4), ("blank", 0), ("lm", None),
                               ("lm_weight", 0.5), ("length_bonus", 0.0), ("candidates", None), ("device", None),
                               ("dtype", None)]
    assert sig(C.advance) == [("logits", E), ("num_frames", E), ("sm_scale", 1.0), ("blank_penalty", 0.0)]
    assert sig(C.commit) == [("which", None), ("max_tail", None), ("rebase", False), ("max_len", None)]
    assert sig(C.hyps) == [("max_len", None)] and sig(C.reset) == [("which", None)]
    for p in ("frames", "retired", "consumed", "room", "offset", "bonus_offset", "scores", "overflowed"):
        assert isinstance(getattr(C, p), property), p
    D = S.ModifiedStreamDecoder
    assert sig(D.__init__) == [("model", E), ("batch", E), ("max_frames", E), ("beam", 4), ("lm", None),
                               ("lm_weight", 0.5), ("length_bonus", 0.0), ("candidates", None), ("sm_scale", 1.0),
                               ("blank_penalty", 0.0), ("blank", 0), ("precision", "fp16x2")]
    assert sig(D.advance) == [("enc_chunk", E), ("lengths", None)] and sig(D.reset) == [("which", None)]
    assert sig(D.commit) == [("which", None), ("max_tail", None), ("rebase", False)]


def test_python_argument_checks():
    from pika_amd import ModifiedBeamStream, ModifiedStreamDecoder, ctc
    for kw in (dict(beam=0), dict(beam=65), dict(batch=0), dict(max_frames=0), dict(blank=-1), dict(candidates=8),
               dict(lm_weight=1.0), dict(length_bonus=0.5)):            # (the LM's arguments without an LM)
        with pytest.raises(ValueError):
            ModifiedBeamStream(**dict(dict(batch=2, max_frames=8, device="cpu"), **kw))
    with pytest.raises(TypeError):
        ModifiedBeamStream(2, 8, device="cpu", dtype=torch.float16)
    lm = object.__new__(ctc.CtcNgramLm)            # never reached beyond the type check
    with pytest.raises(TypeError):
        ModifiedBeamStream(2, 8, lm="not an LM")
    with pytest.raises(TypeError, match="float32"):
        ModifiedBeamStream(2, 8, lm=lm, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="HIP device"):
        ModifiedBeamStream(2, 8, lm=lm, device="cpu")          # the LM form is HIP only
    with pytest.raises(ValueError, match="candidates"):
        ModifiedBeamStream(2, 8, lm=lm, beam=8, candidates=7)

    class NotRnn(object):
        decoder_type = "transformer"
    with pytest.raises(NotImplementedError):
        ModifiedStreamDecoder(NotRnn(), 2, 8)
