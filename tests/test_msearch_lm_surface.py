"""CPU-side checks of the fused one-symbol-per-frame beam search (include/pika_msearch_lm.h): symbols, the ctypes table,
the size of the state blob, the argument checks of the C entry points (refused before any launch, so no GPU is needed)
and the Python surface."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pika_msearch_lm_state_bytes", "pika_msearch_lm_reset", "pika_msearch_lm_advance", "pika_msearch_lm_results",
         "pika_msearch_lm_hyps")
N, P = None, 16        # (P: a non-null pointer that is never followed: the checks come before any launch)


def test_symbols_table_and_abi_version():
    from pika_amd import _lib
    lib = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pika_msearch_lm.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pika_[a-z0-9_]+)\s*\(", text))) == sorted(NAMES)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 25 and lib.pika_amd_abi_version() == 25


def test_state_bytes():
    from pika_amd import _lib
    fn = _lib.lib().pika_msearch_lm_state_bytes
    for bad in ((0, 4, 8, 10), (2, 0, 8, 10), (2, 4, 0, 10), (2, 4, 8, 0), (-1, 4, 8, 10), (2, 9, 8, 10), (2, 4, 65, 10),
                (2, 65, 65, 10), (65536, 4, 8, 10), (1, 4, 64, 2 ** 21 + 1)):
        assert fn(*bad) == 0, bad
    assert fn(1, 4, 64, 2 ** 21) > 0
    # the documented layout: 32 B K + 8 B bytes rounded up to 16, then B tables of N 8-byte keys, N from C
    assert fn(3, 4, 8, 24) == 416 + 3 * 8 * 512
    assert fn(1, 1, 1, 1) == 48 + 8 * 64
    assert fn(2, 64, 64, 40) == (32 * 128 + 16) + 2 * 8 * 8192
    assert fn(2, 16, 64, 40) == (32 * 32 + 16) + 2 * 8 * 8192           # the tables follow C, the head K


FST = (P, P, P, P, P, 3, 5)               # five arrays, num_states, num_arcs
NOFST = (N, N, N, N, N, 0, 0)


def advance(lib, state=P, logits=P, ld=5, nf=P, B=1, K=4, C=8, mf=8, V=5, blank=0, sm=1.0, pen=0.0, f1=FST, f2=NOFST,
            w=(0.5, 1.0, 0.0), parent=P, token=P):
    return lib.pika_msearch_lm_advance(*((state, logits, ld, nf, B, K, C, mf, V, blank, sm, pen) + f1 + (6, 1) + f2
                                         + ((6, 1) if f2[5] else (0, 0)) + w + (parent, token, N)))


def results(lib, state=P, B=1, K=4, C=8, mf=8, f1=FST, start=1, f2=NOFST, start2=0, w=(0.5, 1.0), use_final=1, nbest=1,
            L=8, outs=(P, P, P, P)):
    return lib.pika_msearch_lm_results(*((state, B, K, C, mf) + f1 + (start, 6, 1) + f2 + (start2,)
                                         + ((6, 1) if f2[5] else (0, 0)) + w + (use_final, nbest, L) + outs + (N,)))


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    inf, nan = float("inf"), float("nan")
    # reset(state, B, K, C, max_frames, num_states, start, num_states2, start2, which, stream)
    assert lib.pika_msearch_lm_reset(N, 1, 4, 8, 8, 3, 1, 0, 0, N, N) == -1
    assert lib.pika_msearch_lm_reset(P, 0, 4, 8, 8, 3, 1, 0, 0, N, N) == -1
    assert lib.pika_msearch_lm_reset(P, 1, 0, 8, 8, 3, 1, 0, 0, N, N) == -1
    assert lib.pika_msearch_lm_reset(P, 1, 4, 8, 0, 3, 1, 0, 0, N, N) == -1
    assert lib.pika_msearch_lm_reset(P, 1, 9, 8, 8, 3, 1, 0, 0, N, N) == -1          # K > C
    assert lib.pika_msearch_lm_reset(P, 1, 4, 8, 8, 0, 0, 0, 0, N, N) == -1          # no states
    assert lib.pika_msearch_lm_reset(P, 1, 4, 8, 8, 3, 3, 0, 0, N, N) == -1          # start outside [0, S)
    assert lib.pika_msearch_lm_reset(P, 1, 4, 8, 8, 3, -1, 0, 0, N, N) == -1
    assert lib.pika_msearch_lm_reset(P, 1, 4, 8, 8, 3, 1, 2, 2, N, N) == -1          # the second automaton's
    assert lib.pika_msearch_lm_reset(P, 1, 4, 8, 8, 3, 1, -1, 0, N, N) == -1
    assert lib.pika_msearch_lm_reset(P, 1, 4, 65, 8, 3, 1, 0, 0, N, N) == -2
    assert lib.pika_msearch_lm_reset(P, 65536, 4, 8, 8, 3, 1, 0, 0, N, N) == -2
    assert lib.pika_msearch_lm_reset(P, 1, 4, 64, 2 ** 21 + 1, 3, 1, 0, 0, N, N) == -2
    # advance
    for kw in (dict(state=N), dict(logits=N), dict(nf=N), dict(parent=N), dict(token=N)):
        assert advance(lib, **kw) == -1, kw
    for kw in (dict(ld=4), dict(V=1), dict(blank=5), dict(blank=-1), dict(mf=0), dict(B=0), dict(K=0), dict(C=0),
               dict(K=9)):
        assert advance(lib, **kw) == -1, kw
    for bad in (inf, -inf, nan):
        assert advance(lib, sm=bad) == -1 and advance(lib, pen=bad) == -1
        for i in range(3):
            w = [0.5, 1.0, 0.0]
            w[i] = bad
            assert advance(lib, w=tuple(w)) == -1
    # the automata, as pika_ctc_lm.h: a missing array, no states, negative arcs; arcs may be absent when there are none
    for i in range(5):
        miss = FST[:i] + (N,) + FST[i + 1:]
        assert advance(lib, f1=miss) == -1 and advance(lib, f2=miss) == -1, i
    assert advance(lib, f1=(P, P, P, P, P, 0, 5)) == -1 and advance(lib, f1=(P, P, P, P, P, 3, -1)) == -1
    assert advance(lib, f2=(P, P, P, P, P, 3, -1)) == -1 and advance(lib, f2=(P, P, P, P, P, -1, 0)) == -1
    assert advance(lib, f2=(P, N, N, N, N, 0, 0)) == -1                  # "none" is no states, no arcs AND no arrays
    assert advance(lib, f2=(N, N, N, N, N, 0, 3)) == -1
    assert advance(lib, C=65) == -2 and advance(lib, K=65, C=65) == -2
    assert advance(lib, B=65536) == -2 and advance(lib, C=64, mf=2 ** 21 + 1) == -2
    # results
    for i in range(4):
        outs = (P,) * i + (N,) + (P,) * (3 - i)
        assert results(lib, outs=outs) == -1
    assert results(lib, state=N) == -1
    for kw in (dict(nbest=0), dict(L=0), dict(K=9), dict(B=0), dict(start=3), dict(start=-1), dict(f1=NOFST),
               dict(f2=FST, start2=3), dict(w=(nan, 1.0)), dict(w=(0.5, inf))):
        assert results(lib, **kw) == -1, kw
    assert results(lib, nbest=5) == -2 and results(lib, C=65) == -2 and results(lib, B=65536) == -2
    # hyps(state, B, K, C, max_frames, L, tokens, lengths, stream)
    assert lib.pika_msearch_lm_hyps(N, 1, 4, 8, 8, 8, P, P, N) == -1
    assert lib.pika_msearch_lm_hyps(P, 1, 4, 8, 8, 8, N, P, N) == -1
    assert lib.pika_msearch_lm_hyps(P, 1, 4, 8, 8, 8, P, N, N) == -1
    assert lib.pika_msearch_lm_hyps(P, 1, 4, 8, 8, 0, P, P, N) == -1
    assert lib.pika_msearch_lm_hyps(P, 1, 9, 8, 8, 8, P, P, N) == -1
    assert lib.pika_msearch_lm_hyps(P, 1, 4, 65, 8, 8, P, P, N) == -2


def test_exports_and_signatures():
    import pika_amd
    from pika_amd.decoder import modified_search as S
    for name in ("ModifiedLmBeamState", "modified_beam_search_lm", "ModifiedBeamState", "modified_beam_search"):
        assert getattr(pika_amd, name) is getattr(S, name) and name in dir(pika_amd)

    def sig(fn, skip=1):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][skip:]
    E = inspect.Parameter.empty
    C = S.ModifiedLmBeamState
    assert sig(C.__init__) == [("batch", E), ("max_frames", E), ("lm", E), ("beam", 4), ("blank", 0), ("lm_weight", 0.5),
                               ("length_bonus", 0.0), ("candidates", None), ("device", None)]
    assert sig(C.advance) == [("logits", E), ("num_frames", E), ("sm_scale", 1.0), ("blank_penalty", 0.0)]
    assert sig(C.results) == [("nbest", 1), ("max_len", None), ("use_final", True)]
    assert sig(C.hyps) == [("max_len", None)] and sig(C.reset) == [("which", None)]
    assert all(isinstance(getattr(C, p), property) for p in ("frames", "scores", "am_scores", "overflowed"))
    assert sig(S.modified_beam_search_lm, 0) == [
        ("model", E), ("x", E), ("x_len", E), ("lm", E), ("beam", 4), ("nbest", 1), ("sm_scale", 1.0),
        ("blank_penalty", 0.0), ("use_graph", True), ("blank", 0), ("precision", "fp16x2"), ("lm_weight", 0.5),
        ("length_bonus", 0.0), ("candidates", None), ("use_final", True)]
    # the helpers are shared with the plain state, not copied
    for name in ("_which", "_check_logits", "_read"):
        assert getattr(C, name) is getattr(S.ModifiedBeamState, name)


def test_constructor_errors():
    from pika_amd import ModifiedLmBeamState, ctc
    lm = object.__new__(ctc.CtcNgramLm)            # never reached beyond the type check
    for bad in (None, "not an LM", 3):
        with pytest.raises(TypeError):
            ModifiedLmBeamState(2, 8, bad)
    for kw in (dict(beam=0), dict(beam=65), dict(candidates=3), dict(candidates=65), dict(beam=8, candidates=7)):
        with pytest.raises(ValueError):
            ModifiedLmBeamState(2, 8, lm, **kw)
    with pytest.raises(ValueError, match="candidates"):
        ModifiedLmBeamState(2, 8, lm, beam=4, candidates=65)
    for kw in (dict(lm_weight=float("nan")), dict(length_bonus=float("inf"))):
        with pytest.raises(ValueError, match="finite"):
            ModifiedLmBeamState(2, 8, lm, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        ModifiedLmBeamState(2, 8, lm, device="cpu")    # there is no CPU path
    pair = object.__new__(ctc.CtcBiasedLm)
    pair.lm, pair.bias, pair.bias_weight = lm, lm, 1.0
    with pytest.raises(RuntimeError, match="HIP device"):
        ModifiedLmBeamState(2, 8, pair, device="cpu")
