"""CPU-side checks of the one-symbol-per-frame beam search with a neural LM (include/pika_msearch_nn.h): symbols, the
ctypes table, the argument checks of the C entry points (refused before any launch, so no GPU is needed) and the Python
surface."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pika_msearch_nn_reset", "pika_msearch_nn_advance", "pika_msearch_nn_results")
N, P = None, 16        # (P: a non-null pointer that is never followed: the checks come before any launch)


def test_symbols_table_and_abi_version():
    from pika_amd import _lib
    lib = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pika_msearch_nn.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pika_[a-z0-9_]+)\s*\(", text))) == sorted(NAMES)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 25 and lib.pika_amd_abi_version() == 25
    # the blob is the fused search's: its size and its slot read-out are reused, not declared again
    assert lib.pika_msearch_lm_state_bytes(3, 4, 8, 24) == 416 + 3 * 8 * 512


FST = (P, P, P, P, P, 3, 5)               # five arrays, num_states, num_arcs
NOFST = (N, N, N, N, N, 0, 0)


def advance(lib, state=P, logits=P, ld=5, nf=P, B=1, K=4, C=8, mf=8, V=5, blank=0, sm=1.0, pen=0.0, f1=NOFST, f2=NOFST,
            w=(0.5, 1.0, 0.0), rows=P, lld=5, VL=5, off=0, ns=1.0, nw=0.3, parent=P, token=P):
    return lib.pika_msearch_nn_advance(*((state, logits, ld, nf, B, K, C, mf, V, blank, sm, pen)
                                         + f1 + ((6, 1) if f1[5] else (0, 0)) + f2 + ((6, 1) if f2[5] else (0, 0)) + w
                                         + (rows, lld, VL, off, ns, nw, parent, token, N)))


def results(lib, state=P, B=1, K=4, C=8, mf=8, f1=NOFST, start=0, f2=NOFST, start2=0, w=(0.5, 1.0), use_final=1, nbest=1,
            L=8, outs=(P, P, P, P)):
    return lib.pika_msearch_nn_results(*((state, B, K, C, mf) + f1 + (start,) + ((6, 1) if f1[5] else (0, 0)) + f2
                                         + (start2,) + ((6, 1) if f2[5] else (0, 0)) + w + (use_final, nbest, L) + outs
                                         + (N,)))


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    inf, nan = float("inf"), float("nan")
    # reset(state, B, K, C, max_frames, num_states, start, num_states2, start2, which, stream)
    reset = lib.pika_msearch_nn_reset
    assert reset(N, 1, 4, 8, 8, 0, 0, 0, 0, N, N) == -1 and reset(N, 1, 4, 8, 8, 3, 1, 0, 0, N, N) == -1
    for bad in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 8, 0), (1, 9, 8, 8)):
        assert reset(*((P,) + bad + (0, 0, 0, 0, N, N))) == -1, bad
    assert reset(P, 1, 4, 8, 8, 0, 0, 2, 0, N, N) == -1              # a second automaton without a first
    assert reset(P, 1, 4, 8, 8, -1, 0, 0, 0, N, N) == -1 and reset(P, 1, 4, 8, 8, 3, 1, -1, 0, N, N) == -1
    assert reset(P, 1, 4, 8, 8, 3, 3, 0, 0, N, N) == -1 and reset(P, 1, 4, 8, 8, 3, -1, 0, 0, N, N) == -1
    assert reset(P, 1, 4, 8, 8, 3, 1, 2, 2, N, N) == -1
    assert reset(P, 1, 4, 65, 8, 0, 0, 0, 0, N, N) == -2 and reset(P, 65536, 4, 8, 8, 0, 0, 0, 0, N, N) == -2
    assert reset(P, 1, 4, 64, 2 ** 21 + 1, 0, 0, 0, 0, N, N) == -2
    # advance: with no automaton, with one, with two
    for fsts in (dict(), dict(f1=FST), dict(f1=FST, f2=FST)):
        for kw in (dict(state=N), dict(logits=N), dict(nf=N), dict(parent=N), dict(token=N), dict(rows=N)):
            assert advance(lib, **dict(fsts, **kw)) == -1, kw
        for kw in (dict(ld=4), dict(V=1), dict(blank=5), dict(blank=-1), dict(mf=0), dict(B=0), dict(K=0), dict(C=0),
                   dict(K=9), dict(lld=4), dict(VL=0), dict(VL=-1), dict(VL=6), dict(ns=inf), dict(ns=nan),
                   dict(nw=-inf), dict(nw=nan), dict(sm=inf), dict(pen=nan)):
            assert advance(lib, **dict(fsts, **kw)) == -1, kw
        for i in range(3):
            w = [0.5, 1.0, 0.0]
            w[i] = nan
            assert advance(lib, **dict(fsts, w=tuple(w))) == -1
        assert advance(lib, **dict(fsts, C=65)) == -2 and advance(lib, **dict(fsts, B=65536)) == -2
        assert advance(lib, **dict(fsts, C=64, mf=2 ** 21 + 1)) == -2
    assert advance(lib, f2=FST) == -1                                 # a second automaton without a first
    for i in range(5):
        miss = FST[:i] + (N,) + FST[i + 1:]
        assert advance(lib, f1=miss) == -1 and advance(lib, f1=FST, f2=miss) == -1, i
    assert advance(lib, f1=(P, P, P, P, P, 3, -1)) == -1 and advance(lib, f1=(P, N, N, N, N, 0, 0)) == -1
    assert advance(lib, f1=(N, N, N, N, N, 0, 3)) == -1
    # results
    for fsts in (dict(), dict(f1=FST, start=1), dict(f1=FST, start=1, f2=FST, start2=2)):
        for i in range(4):
            assert results(lib, **dict(fsts, outs=(P,) * i + (N,) + (P,) * (3 - i))) == -1
        for kw in (dict(state=N), dict(nbest=0), dict(L=0), dict(K=9), dict(B=0), dict(w=(nan, 1.0)), dict(w=(0.5, inf))):
            assert results(lib, **dict(fsts, **kw)) == -1, kw
        assert results(lib, **dict(fsts, nbest=5)) == -2 and results(lib, **dict(fsts, C=65)) == -2
    assert results(lib, f1=FST, start=3) == -1 and results(lib, f1=FST, start=1, f2=FST, start2=3) == -1
    assert results(lib, f2=FST) == -1


def test_exports_and_signatures():
    import pika_amd
    from pika_amd.decoder import modified_search as S
    from pika_amd.model import lm as LM
    for name in ("ModifiedNnLmBeamState", "modified_beam_search_nnlm"):
        assert getattr(pika_amd, name) is getattr(S, name) and name in dir(pika_amd)
    assert pika_amd.LstmLm is LM.LstmLm and "LstmLm" in dir(pika_amd)

    def sig(fn, skip=1):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][skip:]
    E = inspect.Parameter.empty
    C = S.ModifiedNnLmBeamState
    assert issubclass(C, S._BeamState)
    assert sig(C.__init__) == [("batch", E), ("max_frames", E), ("beam", 4), ("blank", 0), ("nn_weight", 0.3),
                               ("nn_scale", 1.0), ("nn_label_offset", 0), ("lm", None), ("lm_weight", 0.5),
                               ("length_bonus", 0.0), ("candidates", None), ("device", None)]
    assert sig(C.advance) == [("logits", E), ("lm_logits", E), ("num_frames", E), ("sm_scale", 1.0),
                              ("blank_penalty", 0.0)]
    assert sig(C.results) == [("nbest", 1), ("max_len", None), ("use_final", True)]
    assert sig(C.hyps) == [("max_len", None)] and sig(C.reset) == [("which", None)]
    assert all(isinstance(getattr(C, p), property) for p in ("frames", "scores", "am_scores", "bonus", "overflowed"))
    assert sig(S.modified_beam_search_nnlm, 0) == [
        ("model", E), ("x", E), ("x_len", E), ("nnlm", E), ("beam", 4), ("nbest", 1), ("sm_scale", 1.0),
        ("blank_penalty", 0.0), ("use_graph", True), ("blank", 0), ("precision", "fp16x2"), ("nn_weight", 0.3),
        ("nn_scale", 1.0), ("nn_label_offset", 0), ("lm", None), ("lm_weight", 0.5), ("length_bonus", 0.0),
        ("candidates", None), ("use_final", True)]
    assert "LODR" in S.modified_beam_search_nnlm.__doc__ and "LODR" in C.__doc__
    assert sig(LM.LstmLm.__init__) == [("vocab", E), ("embed_dim", E), ("hidden", E), ("layers", 1), ("sos", 0)]
    for name in ("start", "step", "logits", "select"):
        assert callable(getattr(LM.LstmLm, name)) and name in LM.__doc__
    for doc, word in (("README.md", "modified_beam_search_nnlm"), ("INTEGRATION.md", "pika_msearch_nn.h"),
                      ("DESIGN.md", "Modified beam search with a neural LM")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_constructor_errors():
    from pika_amd import ModifiedNnLmBeamState
    for bad in ("not an LM", 3):
        with pytest.raises(TypeError):
            ModifiedNnLmBeamState(2, 8, lm=bad)
    for kw in (dict(beam=0), dict(beam=65), dict(candidates=3), dict(candidates=65), dict(beam=8, candidates=7)):
        with pytest.raises(ValueError):
            ModifiedNnLmBeamState(2, 8, **kw)
    for kw in (dict(nn_weight=float("nan")), dict(nn_scale=float("inf")), dict(lm_weight=-float("inf")),
               dict(length_bonus=float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            ModifiedNnLmBeamState(2, 8, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        ModifiedNnLmBeamState(2, 8, device="cpu")      # there is no CPU path


def test_lstm_lm_protocol_on_the_cpu():
    """Stepping token by token is the whole-sentence forward; select re-orders the rows."""
    from pika_amd.model.lm import LstmLm
    torch.manual_seed(0)
    lm = LstmLm(11, 6, 7, layers=2, sos=3).eval()
    for bad in (dict(vocab=0), dict(sos=11), dict(layers=0)):
        with pytest.raises(ValueError):
            LstmLm(**dict(dict(vocab=11, embed_dim=6, hidden=7), **bad))
    tokens = torch.randint(0, 11, (5, 4))
    with torch.no_grad():
        want = lm(tokens)
        out, state = lm.start(5)
        got = [lm.logits(out)]
        for i in range(4):
            out, state = lm.step(tokens[:, i], state)
            got.append(lm.logits(out))
        assert want.shape == (5, 5, 11) and torch.allclose(torch.stack(got, 1), want, atol=1e-6)
        index = torch.tensor([4, 0, 0, 2, 1])
        picked = lm.select(state, index)
        assert all(torch.equal(p, s[:, index]) for p, s in zip(picked, state))
        out2, _ = lm.step(tokens[index, 0], picked)
        ref, _ = lm.step(tokens[:, 0], state)
        assert torch.allclose(out2, ref[index], atol=1e-6)
