"""CPU-side checks of the CTC decoders: the references of tests/ctc_decode_common.py against brute force, the Python
signatures and exports, the C ABI's size formula and argument refusals (no launch, no GPU), and the properties the GPU
test's case list must have -- from the reference alone."""
import ctypes
import inspect
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_decode_common as D  # noqa: E402

# (T, C, blank): the beam of 16 holds every prefix that can exist (at most 15 non-empty ones)
EXHAUSTIVE = [(3, 3, 0), (3, 3, 2), (2, 4, 0), (2, 4, 1), (1, 2, 0), (4, 2, 0), (1, 16, 5), (3, 2, 1)]


def all_prefixes(T, C, blank):
    """Every label sequence some frame labelling of T frames collapses to."""
    return {tuple(R.collapse(fl, blank)) for fl in itertools.product(range(C), repeat=T)}


@pytest.mark.parametrize("T,C,blank", EXHAUSTIVE)
def test_reference_equals_brute_force_when_the_beam_holds_everything(T, C, blank):
    lp = D.case_lp(T, C, 10 * T + C)
    want = all_prefixes(T, C, blank)
    assert len(want) - 1 <= 15
    hyps, margin, reent = D.beam_search(lp, 16, 16, blank)
    assert {l for l, _ in hyps} == want and reent == 0
    for l, s in hyps:
        assert s == pytest.approx(-R.dp_cost(lp.astype(np.float64), list(l), blank), abs=1e-12)
    assert [s for _, s in hyps] == sorted((s for _, s in hyps), reverse=True)
    # T = 3, C = 3: 2 + 4 + 8 = 14 non-empty label sequences at most; those with adjacent repeats need more frames
    if (T, C) == (3, 3):
        assert len(want) == 9


def test_reference_tie_order_and_greedy():
    v = np.log(1.0 / 4.0)
    hyps, _, _ = D.beam_search(np.full((1, 4), v), 3, 3, blank=1)
    assert [l for l, _ in hyps] == [(), (0,), (2,)] and all(s == v for _, s in hyps)
    lp = np.log(np.array([[.1, .6, .3], [.1, .6, .3], [.5, .2, .3], [.2, .2, .6], [.2, .6, .2], [.4, .4, .2]]))
    tokens, frames, score = D.greedy(lp, 0)
    assert (tokens, frames) == ([1, 2, 1], [0, 3, 4])       # the last row's equal maxima go to class 0, the blank
    assert score == pytest.approx(np.log(.6 * .6 * .5 * .6 * .6 * .4))
    assert D.greedy(lp, 1)[:2] == ([0, 2, 0], [2, 3, 5])


def test_signatures_and_exports():
    import pika_amd
    from pika_amd import ctc

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ctc.ctc_greedy_decode) == [("log_probs", E), ("input_lengths", E), ("blank", 0)]
    assert sig(ctc.ctc_greedy_decode_from_logits) == [("logits", E), ("input_lengths", E), ("blank", 0)]
    assert sig(ctc.ctc_beam_search) == [("log_probs", E), ("input_lengths", E), ("beam", 16), ("nbest", 1), ("blank", 0)]
    assert sig(ctc.ctc_beam_search_from_logits) == [("logits", E), ("input_lengths", E), ("beam", 16), ("nbest", 1),
                                                    ("blank", 0)]
    for name in ("ctc_greedy_decode", "ctc_greedy_decode_from_logits", "ctc_beam_search", "ctc_beam_search_from_logits"):
        assert getattr(pika_amd, name) is getattr(ctc, name) and name in dir(pika_amd)
    from pika_amd import _lib
    assert _lib.ABI_VERSION == 25               # new symbols only: no signature changed


def test_cpu_tensors_and_bad_limits_are_refused():
    from pika_amd import ctc
    lp, il = torch.zeros(3, 1, 4), torch.tensor([3])
    for fn in (ctc.ctc_greedy_decode, ctc.ctc_greedy_decode_from_logits, ctc.ctc_beam_search,
               ctc.ctc_beam_search_from_logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(lp, il)
    for fn in (ctc.ctc_beam_search, ctc.ctc_beam_search_from_logits):
        for kw in (dict(beam=65), dict(beam=4, nbest=5), dict(beam=0), dict(beam=4, nbest=0)):
            with pytest.raises(ValueError):
                fn(lp, il, **kw)


def test_scratch_size_follows_the_header():
    from pika_amd import _lib
    lib = _lib.lib()

    def want(B, T, beam):
        n = 64
        while n < 2 * T * beam:
            n *= 2
        return 8 * B * n
    for dims in [(32, 240, 16), (1, 1, 1), (3, 9, 64), (2, 1000, 16), (1, 600, 4), (5, 1, 33), (1, 2 ** 21, 64)]:
        assert lib.pika_ctc_beam_scratch_bytes(*dims) == want(*dims), dims
    for dims in [(0, 5, 4), (1, 0, 4), (1, 5, 0), (-1, 5, 4), (1, 5, 65), (65536, 5, 4), (1, 2 ** 21 + 1, 64)]:
        assert lib.pika_ctc_beam_scratch_bytes(*dims) == 0, dims


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2
    p = ctypes.c_void_p(0x1000)     # never dereferenced: EVERY call below is refused before any launch
    good = dict(B=2, T=5, C=4, blank=0, K=8, beam=4, nbest=2)

    # q: x, input_lengths, blank_lp, top_val, top_idx, lse, tokens, lengths, scores, frames / scratch
    CALLS = {
        "rows": lambda q, B, T, C, blank, K, beam, nbest: lib.pika_ctc_decode_rows(
            q[0], C * B, C, q[1], B, T, C, blank, K, 1, q[2], q[3], q[4], q[5], None),
        "greedy": lambda q, B, T, C, blank, K, beam, nbest: lib.pika_ctc_greedy(
            q[2], q[3], q[4], q[1], B, T, C, blank, q[6], q[7], q[8], q[9], None),
        "search": lambda q, B, T, C, blank, K, beam, nbest: lib.pika_ctc_beam_search(
            q[0], C * B, C, q[5], q[2], q[3], q[4], q[1], B, T, C, blank, beam, nbest, q[6], q[7], q[8], q[9], None),
    }
    full = [p] * 10
    for kw in (dict(B=0), dict(T=0), dict(C=0), dict(B=-1), dict(T=-3), dict(C=-2), dict(blank=-1), dict(blank=4)):
        for name, call in CALLS.items():
            assert call(full, **dict(good, **kw)) == EINVAL, (kw, name)
    for kw, rc in ((dict(K=0), EINVAL), (dict(K=-1), EINVAL), (dict(K=129), ETOOBIG)):
        assert CALLS["rows"](full, **dict(good, **kw)) == rc, kw
    for kw, rc in ((dict(beam=0), EINVAL), (dict(nbest=0), EINVAL), (dict(beam=65, nbest=1), ETOOBIG),
                   (dict(beam=4, nbest=5), ETOOBIG), (dict(beam=64, nbest=65), ETOOBIG)):
        assert CALLS["search"](full, **dict(good, **kw)) == rc, kw
    for name, call in CALLS.items():
        assert call(full, **dict(good, B=65536)) == ETOOBIG, name
    # null pointers: q-index -> the calls that take that pointer as a required one
    needs = {0: ("rows", "search"), 1: tuple(CALLS), 2: tuple(CALLS), 3: tuple(CALLS), 4: tuple(CALLS), 5: ("rows",),
             6: ("greedy", "search"), 7: ("greedy", "search"), 8: ("greedy", "search"), 9: ("greedy", "search")}
    for i, names in needs.items():
        q = [None if j == i else p for j in range(10)]
        for name in names:
            assert CALLS[name](q, **good) == EINVAL, (i, name)


def test_gpu_case_list_is_separated_and_re_enters():
    # properties of tests/test_ctc_decode_gpu.py's search cases (kept in ctc_decode_common), from the float64 reference
    # and the float32 yardstick
    G = D
    refs = [(c.name,) + c.ref() for c in G.ALL_SEARCH]
    for name, h64, bound, separated, reent, margin, err32 in refs:
        print("CTCDECODE %-22s bound %.3g margin %.3g float32 err %.3g re-entries %d %s" % (
            name, bound, margin, err32, reent, "" if separated else "NOT separated"))
        assert bound >= 1e-6 * max(abs(s) for _, s in h64) and bound >= 4 * err32
    unseparated = [r[0] for r in refs if not r[3]]
    assert len(refs) >= 20 and len(unseparated) <= 0.1 * len(refs), unseparated
    assert sum(1 for r in refs if r[4] > 0) >= 3
    # what the issue measured for the re-entry cases
    by_name = {r[0]: r for r in refs}
    for name, reent in (("T12_C3_beam2_s1", 1), ("T30_C4_beam3_s3", 2), ("T24_C4_beam4_s2", 1), ("T24_C4_beam4_s3", 1),
                        ("T60_C8_beam8_s0", 2)):
        assert by_name[name][4] == reent, (name, by_name[name][4])
    # the exhaustive cases of the GPU list do hold every prefix
    for c in G.ALL_SEARCH:
        if c.exhaustive:
            assert len(c.ref()[0]) == len(all_prefixes(c.T, c.C, c.blank)) <= min(c.beam, 16)
    # the cases the issue names are there
    have = {(c.T, c.C, c.beam) for c in G.ALL_SEARCH}
    for want in ((12, 3, 2), (30, 4, 3), (24, 4, 4), (60, 8, 8), (16, 8, 16), (10, 40, 16), (6, 260, 16), (8, 70, 64),
                 (5, 1028, 16), (4, 5003, 4), (600, 6, 4), (1, 2, 4)):
        assert want in have, want
    assert any(c.beam == 1 for c in G.ALL_SEARCH)
