"""CPU-side checks of the time stamps of the one-symbol-per-frame beam search (include/pika_msearch_times.h): symbols,
the ctypes table, the size of the record, the argument checks of the C entry points (refused before any launch, so no
GPU is needed) and the Python surface."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pika_msearch_times_bytes", "pika_msearch_times_reset", "pika_msearch_times_step", "pika_msearch_times_hyps",
         "pika_msearch_times_results", "pika_msearch_times_commit")
N, P = None, 16        # (P: a non-null pointer that is never followed: the checks come before any launch)


def header():
    return open(os.path.join(ROOT, "include", "pika_msearch_times.h")).read()


def test_symbols_table_and_abi_version():
    from pika_amd import _lib
    lib = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pika_[a-z0-9_]+)\s*\(", text))) == sorted(NAMES)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        # the header's parameter count is the table's
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 25 and lib.pika_amd_abi_version() == 25
    for macro in ("SEEN_OFFSET", "LOST_OFFSET", "CUR_OFFSET", "PLANES_OFFSET"):
        assert "#define PIKA_MSEARCH_TIMES_%s(B)" % macro in text
    # the older headers are as they were: none of them names the new one
    for other in ("pika_msearch.h", "pika_msearch_lm.h", "pika_msearch_stream.h"):
        assert "times" not in open(os.path.join(ROOT, "include", other)).read()


def test_sizes():
    from pika_amd import _lib
    size = _lib.lib().pika_msearch_times_bytes
    # i32 seen[B], lost[B], cur[B] rounded up to 16 bytes together, then two planes of i32 [B][K][max_frames]
    assert size(1, 1, 1) == 16 + 8 and size(3, 4, 8) == 48 + 8 * 3 * 4 * 8 and size(4, 4, 8) == 48 + 8 * 4 * 4 * 8
    assert size(5, 64, 37) == 64 + 8 * 5 * 64 * 37 and size(65535, 1, 1) == 786432 + 8 * 65535
    assert size(1, 64, 2 ** 21) == 16 + 8 * 64 * 2 ** 21
    for bad in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (2, 65, 8), (65536, 4, 8), (1, 64, 2 ** 21 + 1), (-1, 4, 8)):
        assert size(*bad) == 0, bad


def reset(lib, times=P, B=1, K=4, mf=8, which=N):
    return lib.pika_msearch_times_reset(times, B, K, mf, which, N)


def step(lib, times=P, state=P, side=N, B=1, K=4, C=0, mf=8, parent=P, token=P, blank=0):
    return lib.pika_msearch_times_step(times, state, side, B, K, C, mf, parent, token, blank, N)


def hyps(lib, times=P, state=P, B=1, K=4, C=0, mf=8, L=8, out=P):
    return lib.pika_msearch_times_hyps(times, state, B, K, C, mf, L, out, N)


def results(lib, times=P, state=P, B=1, K=4, C=0, mf=8, n=2, L=8, tokens=P, lengths=P, out=P):
    return lib.pika_msearch_times_results(times, state, B, K, C, mf, n, L, tokens, lengths, out, N)


def commit(lib, times=P, state=P, B=1, K=4, C=0, mf=8, which=N, lengths=P, slot_map=P, L=8, out=P):
    return lib.pika_msearch_times_commit(times, state, B, K, C, mf, which, lengths, slot_map, L, out, N)


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    nulls = {reset: ("times",), step: ("times", "state", "parent", "token"), hyps: ("times", "state", "out"),
             results: ("times", "state", "tokens", "lengths", "out"),
             commit: ("times", "state", "lengths", "slot_map", "out")}
    for fn, names in nulls.items():
        for name in names:
            assert fn(lib, **{name: N}) == -1, (fn.__name__, name)
        for kw in (dict(B=0), dict(B=-2), dict(K=0), dict(mf=0), dict(mf=-1)):
            assert fn(lib, **kw) == -1, (fn.__name__, kw)
        assert fn(lib, B=65536) == -2 and fn(lib, K=65) == -2 and fn(lib, K=64, mf=2 ** 21 + 1) == -2, fn.__name__
        if fn is reset:
            continue
        # C: 0 the plain blob, K <= C <= 64 the fused search's
        assert fn(lib, C=-1) == -1 and fn(lib, C=3) == -1 and fn(lib, K=9, C=8) == -1, fn.__name__
        assert fn(lib, C=65) == -2 and fn(lib, K=4, C=64, mf=2 ** 21 + 1) == -2, fn.__name__
        assert fn(lib, K=65, C=65) == -2, fn.__name__
    assert step(lib, blank=-1) == -1
    for fn in (hyps, results, commit):
        assert fn(lib, L=0) == -1 and fn(lib, L=-3) == -1, fn.__name__
    assert hyps(lib, K=64, L=2 ** 26) == -2
    assert results(lib, n=0) == -1 and results(lib, n=-1) == -1
    assert results(lib, n=5) == -2 and results(lib, K=64, n=64, L=2 ** 26) == -2


def test_exports_signatures_and_docstrings():
    import pika_amd
    from pika_amd.decoder import modified_search as S
    for name in ("ModifiedBeamTimes", "modified_beam_search_timed"):
        assert getattr(pika_amd, name) is getattr(S, name) and name in dir(pika_amd)

    def sig(fn, skip=1):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][skip:]
    E = inspect.Parameter.empty
    C = S.ModifiedBeamTimes
    assert sig(C.__init__) == [("search", E)]
    assert sig(C.step) == [("parent", E), ("token", E)] and sig(C.hyps) == [("max_len", None)]
    assert sig(C.results) == [("tokens", E), ("lengths", E)] and sig(C.reset) == [("which", None)]
    assert sig(C.commit) == [("lengths", E), ("slot_map", E), ("which", None), ("max_len", None)]
    assert isinstance(C.lost, property)
    both = sig(S.modified_beam_search, 0)[3:] + sig(S.modified_beam_search_lm, 0)[11:]
    assert sig(S.modified_beam_search_timed, 0) == [("model", E), ("x", E), ("x_len", E), ("lm", None)] + both
    D = S.ModifiedStreamDecoder
    assert sig(D.track_times) == [] and sig(D.results_timed) == sig(D.results)
    # the old wrappers drive the loop without the hook
    assert sig(S._drive, 0)[-1] == ("hook", None)
    for fn in (S.modified_beam_search, S.modified_beam_search_lm):
        assert "hook" not in inspect.getsource(fn)
    assert "modified_beam_search_timed" in S.modified_beam_search.__doc__
    assert "rnnt_align_modified" not in S.modified_beam_search.__doc__
    for obj in (C, S.modified_beam_search_timed, D):
        assert "times" in obj.__doc__
    for doc, word in (("README.md", "modified_beam_search_timed"), ("INTEGRATION.md", "pika_msearch_times.h"),
                      ("DESIGN.md", "Time stamps of the modified beam search")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_python_argument_checks():
    import torch
    from pika_amd import ModifiedBeamState, ModifiedBeamStream, ModifiedBeamTimes
    with pytest.raises(TypeError):
        ModifiedBeamTimes("a search")
    state = ModifiedBeamState(2, 8, 3, 0, device="cpu")
    times = ModifiedBeamTimes(state)
    assert (times.batch, times.beam, times.max_frames, times.blank) == (2, 3, 8, 0) and not times.native
    assert times.lost.tolist() == [False, False] and (times.hyps() == -1).all() and times.hyps(5).shape == (2, 3, 5)
    good = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(TypeError):
        times.step(good.int(), good)
    with pytest.raises(ValueError):
        times.step(good[:1], good[:1])
    with pytest.raises(ValueError):
        times.hyps(max_len=0)
    with pytest.raises(ValueError):
        times.results(torch.zeros((2, 4, 8), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int64))   # N > beam
    with pytest.raises(ValueError):
        times.commit(torch.zeros(3, dtype=torch.int64), good)
    stream = ModifiedBeamStream(2, 8, 3, device="cpu")
    assert ModifiedBeamTimes(stream).search is stream
    from pika_amd.decoder.modified_search import modified_beam_search_timed
    with pytest.raises(ValueError, match="LM"):
        modified_beam_search_timed(None, None, None, candidates=8)
