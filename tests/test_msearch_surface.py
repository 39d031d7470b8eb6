"""CPU-side checks of the one-symbol-per-frame beam search: symbols, the ctypes table, the size of the state blob, the
argument checks of the C entry points (refused before any launch, so no GPU is needed) and the Python surface."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pika_msearch_state_bytes", "pika_msearch_reset", "pika_msearch_advance", "pika_msearch_results",
         "pika_msearch_hyps")


def test_symbols_table_and_abi_version():
    from pika_amd import _lib
    lib = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pika_msearch.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pika_[a-z0-9_]+)\s*\(", text))) == sorted(NAMES)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 25 and lib.pika_amd_abi_version() == 25
    assert "#define PIKA_MSEARCH_ROOT 0x7ffffffe\n" in text and "#define PIKA_MSEARCH_MAX_BEAM 64\n" in text


def test_state_bytes():
    from pika_amd import _lib
    fn = _lib.lib().pika_msearch_state_bytes
    for bad in ((0, 4, 10), (2, 0, 10), (2, 4, 0), (-1, 4, 10), (2, 65, 10), (65536, 4, 10), (1, 64, 2 ** 21 + 1)):
        assert fn(*bad) == 0, bad
    assert fn(1, 64, 2 ** 21) > 0
    # the documented layout: 12 B K + 8 B bytes rounded up to 16, then B tables of N 8-byte keys
    assert fn(3, 4, 24) == 176 + 3 * 8 * 256
    assert fn(1, 1, 1) == 32 + 8 * 64
    assert fn(2, 64, 40) == (12 * 128 + 16) + 2 * 8 * 8192


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    N, P = None, 16        # (P: a non-null pointer that is never followed: the checks come before any launch)
    inf, nan = float("inf"), float("nan")
    assert lib.pika_msearch_reset(N, 1, 4, 8, N, N) == -1
    assert lib.pika_msearch_reset(P, 0, 4, 8, N, N) == -1
    assert lib.pika_msearch_reset(P, 1, 65, 8, N, N) == -2
    assert lib.pika_msearch_reset(P, 65536, 4, 8, N, N) == -2
    assert lib.pika_msearch_reset(P, 1, 64, 2 ** 21 + 1, N, N) == -2
    # advance(state, logits, ld, num_frames, B, K, max_frames, V, blank, sm_scale, blank_penalty, parent, token, stream)
    assert lib.pika_msearch_advance(N, P, 5, P, 1, 4, 8, 5, 0, 1.0, 0.0, P, P, N) == -1
    assert lib.pika_msearch_advance(P, N, 5, P, 1, 4, 8, 5, 0, 1.0, 0.0, P, P, N) == -1
    assert lib.pika_msearch_advance(P, P, 5, N, 1, 4, 8, 5, 0, 1.0, 0.0, P, P, N) == -1
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 8, 5, 0, 1.0, 0.0, N, P, N) == -1
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 8, 5, 0, 1.0, 0.0, P, N, N) == -1
    assert lib.pika_msearch_advance(P, P, 4, P, 1, 4, 8, 5, 0, 1.0, 0.0, P, P, N) == -1        # ld < V
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 8, 1, 0, 1.0, 0.0, P, P, N) == -1        # V < 2
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 8, 5, 5, 1.0, 0.0, P, P, N) == -1        # blank outside [0, V)
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 8, 5, -1, 1.0, 0.0, P, P, N) == -1
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 0, 5, 0, 1.0, 0.0, P, P, N) == -1        # max_frames < 1
    for bad in (inf, -inf, nan):
        assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 8, 5, 0, bad, 0.0, P, P, N) == -1
        assert lib.pika_msearch_advance(P, P, 5, P, 1, 4, 8, 5, 0, 1.0, bad, P, P, N) == -1
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 65, 8, 5, 0, 1.0, 0.0, P, P, N) == -2
    assert lib.pika_msearch_advance(P, P, 5, P, 1, 64, 2 ** 21 + 1, 5, 0, 1.0, 0.0, P, P, N) == -2
    # results(state, B, K, max_frames, nbest, L, tokens, lengths, scores, stream)
    assert lib.pika_msearch_results(N, 1, 4, 8, 1, 8, P, P, P, N) == -1
    assert lib.pika_msearch_results(P, 1, 4, 8, 1, 8, P, P, N, N) == -1
    assert lib.pika_msearch_results(P, 1, 4, 8, 0, 8, P, P, P, N) == -1
    assert lib.pika_msearch_results(P, 1, 4, 8, 1, 0, P, P, P, N) == -1
    assert lib.pika_msearch_results(P, 1, 4, 8, 5, 8, P, P, P, N) == -2                        # nbest > K
    assert lib.pika_msearch_results(P, 1, 65, 8, 1, 8, P, P, P, N) == -2
    # hyps(state, B, K, max_frames, L, tokens, lengths, stream)
    assert lib.pika_msearch_hyps(N, 1, 4, 8, 8, P, P, N) == -1
    assert lib.pika_msearch_hyps(P, 1, 4, 8, 8, N, P, N) == -1
    assert lib.pika_msearch_hyps(P, 1, 4, 8, 0, P, P, N) == -1
    assert lib.pika_msearch_hyps(P, 1, 65, 8, 8, P, P, N) == -2


def test_exports_and_signatures():
    import pika_amd
    from pika_amd.decoder import modified_search as S
    for name in ("ModifiedBeamState", "modified_beam_search"):
        assert getattr(pika_amd, name) is getattr(S, name) and name in dir(pika_amd)

    def sig(fn, skip=1):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][skip:]
    E = inspect.Parameter.empty
    C = S.ModifiedBeamState
    assert sig(C.__init__)[:5] == [("batch", E), ("max_frames", E), ("beam", 4), ("blank", 0), ("device", None)]
    assert sig(C.advance) == [("logits", E), ("num_frames", E), ("sm_scale", 1.0), ("blank_penalty", 0.0)]
    assert sig(C.results) == [("nbest", 1), ("max_len", None)]
    assert sig(C.hyps) == [("max_len", None)] and sig(C.reset) == [("which", None)]
    assert all(isinstance(getattr(C, p), property) for p in ("frames", "scores", "overflowed"))
    assert sig(S.modified_beam_search, 0)[:8] == [("model", E), ("x", E), ("x_len", E), ("beam", 4), ("nbest", 1),
                                                  ("sm_scale", 1.0), ("blank_penalty", 0.0), ("use_graph", True)]


def test_constructor_and_input_checks():
    from pika_amd import ModifiedBeamState
    for kw in (dict(beam=0), dict(beam=65), dict(batch=0), dict(max_frames=0), dict(blank=-1)):
        args = dict(batch=2, max_frames=8, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):
            ModifiedBeamState(**args)
    with pytest.raises(TypeError):
        ModifiedBeamState(2, 8, device="cpu", dtype=torch.float16)
    s = ModifiedBeamState(2, 8, beam=3, device="cpu")
    nf = torch.tensor([8, 8])
    good = torch.zeros(6, 5)
    with pytest.raises(TypeError):
        s.advance(good.double(), nf)                               # not the state's dtype
    with pytest.raises(TypeError):
        s.advance(good.half(), nf)
    with pytest.raises(ValueError):
        s.advance(torch.zeros(5, 6).t(), nf)                       # rows are not contiguous
    with pytest.raises(ValueError):
        s.advance(torch.zeros(6, 10)[:, ::2], nf)
    with pytest.raises(ValueError):
        s.advance(torch.zeros(5, 5), nf)                           # not batch * beam rows
    with pytest.raises(ValueError):
        s.advance(good, torch.tensor([8]))
    with pytest.raises(ValueError):
        s.advance(good, nf, sm_scale=float("nan"))
    with pytest.raises(ValueError):
        ModifiedBeamState(2, 8, beam=3, blank=5, device="cpu").advance(good, nf)
    for nbest in (0, 4):
        with pytest.raises(ValueError, match="nbest"):
            s.results(nbest=nbest)
    s.advance(torch.zeros(6, 8)[:, :5], nf)                        # a row stride above V is fine
    assert s.frames.tolist() == [1, 1]
    if torch.cuda.is_available():
        g = ModifiedBeamState(2, 8, beam=3)
        assert g.native
        with pytest.raises(RuntimeError, match="HIP device"):
            g.advance(good, nf)                                    # a CPU tensor for a state on the device
        with pytest.raises(TypeError):
            g.advance(good.double().cuda(), nf)
