"""CTC beam search with n-gram LM shallow fusion on the MI355X against the reference of tests/ctc_lm_common.py.

The reference is the float64 fused prefix beam search on the SAME fp32 log-probs and the same FST; the yardstick is
the same function run in float32.  Per case the bound is max(4 x the yardstick's largest error of a fused or acoustic
score, 1e-6 * max|score|), and a case is *separated* when its margin exceeds 2 * bound -- the rule of
tests/ctc_decode_common.py.  On separated cases the token lists equal the reference's entry by entry and the scores lie
within the bound.  On every case the entries are distinct and sorted by `scores`, `am_scores` <= -dp_cost + bound (a
beam sums a subset of the paths), and scores - am_scores is within the bound of lm_weight * LM + length_bonus * length
(+ the final term), the LM part recomputed in float64 from the FST.  tests/test_ctc_lm_surface.py checks the properties
of the case list from the reference alone.  Every measured error is printed (`CTCLM ...`) before it is asserted;
profiles/ctc_lm_parity.txt keeps that output.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_decode_common as D  # noqa: E402
import ctc_lm_common as L  # noqa: E402

pytestmark = pytest.mark.gpu

_DEVICE_LMS = {}


def device_lm(lm, dev):
    """One upload per reference LM."""
    from pika_amd import ctc
    if id(lm) not in _DEVICE_LMS:
        _DEVICE_LMS[id(lm)] = (lm, ctc.CtcNgramLm(lm.fst, lm.backoff_id, lm.label_offset, device=dev))
    return _DEVICE_LMS[id(lm)][1]


def unpack(out, T, B, nbest):
    tokens, lengths, scores, am = out
    assert tokens.shape == (B, nbest, T) and tokens.dtype == torch.int32
    assert lengths.shape == (B, nbest) and lengths.dtype == torch.int32
    assert scores.shape == (B, nbest) and scores.dtype == torch.float32
    assert am.shape == (B, nbest) and am.dtype == torch.float32
    tokens, lengths, scores, am = (v.cpu().numpy() for v in (tokens, lengths, scores, am))
    res = []
    for n in range(B):
        hyps = []
        for k in range(nbest):
            ln = int(lengths[n, k])
            if ln < 0:
                assert scores[n, k] == -np.inf and am[n, k] == -np.inf and (tokens[n, k] == -1).all()
                hyps.append((None, -np.inf, -np.inf))
            else:
                assert (tokens[n, k, ln:] == -1).all() and (tokens[n, k, :ln] >= 0).all()
                hyps.append((tuple(int(v) for v in tokens[n, k, :ln]), float(scores[n, k]), float(am[n, k])))
        res.append(hyps)
    return res


def gpu_search(case, lp, ils, nbest, dev, logits=False, candidates=None, **over):
    """lp (T,B,C) numpy -> per utterance [(label tuple, score, am_score)], missing entries as (None, -inf, -inf)."""
    from pika_amd import ctc
    fn = ctc.ctc_beam_search_lm_from_logits if logits else ctc.ctc_beam_search_lm
    kw = dict(beam=case.beam, nbest=nbest, blank=case.blank, lm_weight=case.lm_weight, length_bonus=case.length_bonus,
              candidates=case.candidates if candidates is None else candidates, use_final=case.use_final)
    kw.update(over)
    out = fn(torch.from_numpy(lp).to(dev), torch.tensor(ils), device_lm(case.lm, dev), **kw)
    return unpack(out, lp.shape[0], lp.shape[1], nbest)


def check_hyps(case, got, nbest, lp64=None, tol=None, want=None):
    h64, bound, separated, _, margin, err32 = case.ref()
    if want is None:
        want = h64
    tol = bound if tol is None else tol
    want = want[:nbest]
    real = [h for h in got if h[0] is not None]
    assert len(real) == len(want) and all(h[0] is None for h in got[len(real):]), (case.name, got)
    labels = [h[0] for h in real]
    assert len(set(labels)) == len(labels), (case.name, "two entries denote the same label sequence")
    lp64 = case.lp.astype(np.float64) if lp64 is None else lp64
    over, e_lm = -np.inf, 0.0
    for l, s, am in real:
        over = max(over, am + R.dp_cost(lp64, list(l), case.blank))
        lm64 = case.lm.score(l)
        assert lm64 is not None, (case.name, l, "the LM cannot produce this prefix")
        term = case.lm_weight * lm64[0] + case.length_bonus * len(l)
        if case.use_final:
            fin = case.lm.final(lm64[1])
            assert fin is not None, (case.name, l, "no final state")
            term += case.lm_weight * float(fin)
        e_lm = max(e_lm, abs(s - am - term))
    e_f = max([abs(g[1] - w[1]) for g, w in zip(real, want)] + [0.0]) if separated else float("nan")
    e_a = max([abs(g[2] - w[2]) for g, w in zip(real, want)] + [0.0]) if separated else float("nan")
    print("CTCLM %-28s nbest %2d  fused err %.3g  am err %.3g  am over -dp_cost %.3g  |fused - am - LM64 terms| %.3g  "
          "(bound %.3g, float32 err %.3g, margin %.3g, %s)" % (case.name, nbest, e_f, e_a, over, e_lm, tol, err32, margin,
                                                              "separated" if separated else "NOT separated"))
    for x, y in zip(real, real[1:]):
        assert x[1] >= y[1], (case.name, "not sorted")
    assert over <= tol, (case.name, over, tol)
    assert e_lm <= tol, (case.name, e_lm, tol)
    if separated:
        assert labels == [w[0] for w in want], (case.name, labels, want)
        assert e_f <= tol and e_a <= tol, (case.name, e_f, e_a, tol)


@pytest.mark.parametrize("case", L.LM_CASES, ids=lambda c: c.name)
def test_search_against_float64(hip_device, case):
    got = gpu_search(case, case.lp[:, None], [case.T], case.beam, hip_device)[0]
    check_hyps(case, got, case.beam)
    first = gpu_search(case, case.lp[:, None], [case.T], 1, hip_device)[0]
    assert first == got[:1]                     # nbest = 1 is the head of nbest = beam
    check_hyps(case, first, 1)


def test_search_from_logits(hip_device):
    for case in (L.LM_CASES[3], L.LM_CASES[6], L.LM_CASES[8]):
        logits = np.random.RandomState(1000 + case.seed).randn(case.T, case.C).astype(np.float32)
        lp64 = D.log_softmax64(logits)
        _, bound, _, _, _, _ = case.ref()
        # the same distribution up to the fp32 rounding of the logits and one of logit - lse per entry of a path
        tol = bound + case.T * 2.0 ** -22 * float(np.abs(logits).max() + np.log(case.C))
        want, margin, _ = L.search(lp64, case.lm, case.beam, case.candidates, case.blank, case.lm_weight,
                                   case.length_bonus, case.use_final)
        got = gpu_search(case, logits[:, None], [case.T], case.beam, hip_device, logits=True)[0]
        plain = gpu_search(case, case.lp[:, None], [case.T], case.beam, hip_device)[0]
        e_form = max(abs(g[1] - p[1]) for g, p in zip(got, plain)) if [g[0] for g in got] == [p[0] for p in plain] \
            else float("nan")
        e_ref = max(abs(g[1] - w[1]) for g, w in zip(got, want))
        print("CTCLM %-28s from logits: fused err %.3g (tol %.3g), against the log-prob form %.3g (bound %.3g), margin %.3g"
              % (case.name, e_ref, tol, e_form, bound, margin))
        # the two forms of one search agree within the case's bound; the looser tol is for the comparison with the
        # float64 reference alone, whose input (the float64 log-softmax of the logits) is another rounding of the rows
        if case.ref()[2]:
            assert [g[0] for g in got] == [p[0] for p in plain], case.name
            assert e_form <= bound, (case.name, e_form, bound)
        if margin > 2 * tol:
            assert [g[0] for g in got] == [w[0] for w in want]
            assert e_ref <= tol, (case.name, e_ref, tol)
        assert all(am <= -R.dp_cost(lp64, list(l), case.blank) + tol for l, _, am in got if l is not None)


def test_lm_switched_off_equals_the_plain_search(hip_device):
    from pika_amd import ctc
    n = 0
    for pc in D.SEARCH_CASES:
        h64, bound, separated, _, _, _ = pc.ref()
        if not separated:
            continue
        lm = L.make_lm(pc.C, pc.blank, 300 + pc.seed, order=3)          # reaches every class
        case = L.LmCase(pc.T, pc.C, pc.beam, 2 * pc.beam, pc.seed, blank=pc.blank, lm_weight=0.0, length_bonus=0.0,
                        use_final=False, lp=pc.lp, lm=lm)
        got = gpu_search(case, pc.lp[:, None], [pc.T], pc.beam, hip_device)[0]
        x = torch.from_numpy(pc.lp[:, None].copy()).to(hip_device)
        tokens, lengths, scores = (v.cpu().numpy() for v in ctc.ctc_beam_search(x, torch.tensor([pc.T]), beam=pc.beam,
                                                                               nbest=pc.beam, blank=pc.blank))
        plain = [(tuple(int(v) for v in tokens[0, k, :lengths[0, k]]), float(scores[0, k])) if lengths[0, k] >= 0
                 else (None, -np.inf) for k in range(pc.beam)]
        err = max([abs(g[2] - p[1]) for g, p in zip(got, plain) if p[0] is not None] + [0.0])
        print("CTCLM %-28s LM off: am err against ctc_beam_search %.3g (bound %.3g)" % (pc.name, err, bound))
        assert [g[0] for g in got] == [p[0] for p in plain], pc.name
        assert err <= bound, (pc.name, err, bound)
        assert all(g[1] == g[2] for g in got if g[0] is not None)       # no bonus: the fused score is tot
        n += 1
    assert n >= 10


def test_search_ragged_batch(hip_device):
    from pika_amd import ctc
    dev = hip_device
    lp, ils, c0 = L.RAGGED_LP.copy(), L.RAGGED_ILS, L.RAGGED_CASES[0]
    for nbest in (1, L.RAGGED_BEAM):
        got = gpu_search(c0, lp, ils, nbest, dev)
        for case, hyps in zip(L.RAGGED_CASES, got):
            check_hyps(case, hyps, nbest)
    # frames beyond T_n are never read
    dirty = lp.copy()
    for n, il in enumerate(ils):
        dirty[il:, n] = np.nan
    assert gpu_search(c0, dirty, ils, L.RAGGED_BEAM, dev) == got
    # host / device lengths, int32 / int64; lengths clamp to [1,T]
    lm = device_lm(c0.lm, dev)
    x = torch.from_numpy(lp).to(dev)
    kw = dict(beam=L.RAGGED_BEAM, nbest=2, lm_weight=c0.lm_weight, length_bonus=c0.length_bonus,
              candidates=L.RAGGED_CAND)
    want = ctc.ctc_beam_search_lm(x, torch.tensor(ils), lm, **kw)
    for il in (torch.tensor(ils, dtype=torch.int32), torch.tensor(ils).to(dev),
               torch.tensor(ils, dtype=torch.int32).to(dev)):
        for u, v in zip(want, ctc.ctc_beam_search_lm(x, il, lm, **kw)):
            assert torch.equal(u, v)
    u = ctc.ctc_beam_search_lm(x, torch.tensor([0, 99, 11]), lm, **kw)
    v = ctc.ctc_beam_search_lm(x, torch.tensor([1, L.RAGGED_T, 11]), lm, **kw)
    assert all(torch.equal(p, q) for p, q in zip(u, v))
    # a (B,T,C) tensor seen time-major
    bt = x.transpose(0, 1).contiguous().transpose(0, 1)
    assert not bt.is_contiguous()
    for p, q in zip(want, ctc.ctc_beam_search_lm(bt, torch.tensor(ils), lm, **kw)):
        assert torch.equal(p, q)
    # unbatched (T,C): utterance 0 on its own, no batch axis
    one = ctc.ctc_beam_search_lm(x[:, 0], torch.tensor([ils[0]]), lm, **kw)
    assert one[0].shape == (2, L.RAGGED_T) and all(torch.equal(p, q[0]) for p, q in zip(one, want))


def test_unreachable_classes_are_excluded_at_any_weight(hip_device):
    case = [c for c in L.LM_CASES if c.unreachable][0]
    for lmw in (0.0, case.lm_weight):
        got = gpu_search(case, case.lp[:, None], [case.T], case.beam, hip_device, lm_weight=lmw)[0]
        assert all(l is None or not set(l) & set(case.unreachable) for l, _, _ in got)
    lp = case.lp.copy()                     # the unreachable class made the best of every row: still never emitted
    lp[:, case.unreachable[0]] = 0.0
    got = gpu_search(case, lp[:, None], [case.T], case.beam, hip_device, lm_weight=0.0)[0]
    assert all(l is None or case.unreachable[0] not in l for l, _, _ in got) and got[0][0] is not None


def test_two_runs_are_bit_identical(hip_device):
    for case in (L.LM_CASES[3], L.LM_CASES[9]):
        a = gpu_search(case, case.lp[:, None], [case.T], case.beam, hip_device)
        assert a == gpu_search(case, case.lp[:, None], [case.T], case.beam, hip_device)


def test_graph_capture_equals_eager(hip_device):
    from pika_amd import ctc
    dev = hip_device
    T, B, C = 12, 3, 9
    lm = device_lm(L.make_lm(C, 0, 77, order=3), dev)
    data = [(D.case_lp(T, C, 60 + i, B=B), il) for i, il in enumerate(([12, 9, 10], [5, 12, 12], [12, 1, 7]))]

    def step(x, il):
        return (ctc.ctc_beam_search_lm(x, il, lm, beam=4, nbest=3, lm_weight=0.5, length_bonus=0.25, candidates=5)
                + ctc.ctc_beam_search_lm_from_logits(x, il, lm, beam=4, nbest=3, use_final=False))

    sx = torch.from_numpy(data[0][0]).to(dev)
    sil = torch.tensor(data[0][1], dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up off the default stream, then one linear capture
        step(sx, sil)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sx, sil)
    for lp, il in data[1:]:
        sx.copy_(torch.from_numpy(lp))
        sil.copy_(torch.tensor(il, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = step(torch.from_numpy(lp).to(dev), torch.tensor(il, dtype=torch.int32, device=dev))
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)


def test_adjacent_buffers_keep_their_guards(hip_device):
    from pika_amd import _lib, ctc
    lib, dev = _lib.lib(), hip_device
    T, B, C, beam, nbest, K, GUARD = 10, 2, 37, 8, 5, 12, 256
    ref_lm = L.make_lm(C, 0, 71, order=3)
    lm = device_lm(ref_lm, dev)
    x = torch.from_numpy(D.case_lp(T, C, 70, B=B)).to(dev)
    il = torch.tensor([10, 8], dtype=torch.int32, device=dev)
    sizes = dict(blank_lp=4 * T * B, top_val=4 * T * B * K, top_idx=4 * T * B * K, tokens=4 * B * nbest * T,
                 lengths=4 * B * nbest, scores=4 * B * nbest, am=4 * B * nbest,
                 scratch=lib.pika_ctc_lm_scratch_bytes(B, T, beam, K))
    assert sizes["scratch"] > 0
    offs, total = {}, GUARD
    for name, nbytes in sizes.items():
        offs[name] = total
        total += (nbytes + 15) // 16 * 16 + GUARD
    arena = torch.full((total,), 0xA5, dtype=torch.uint8, device=dev)
    p = {name: arena.data_ptr() + o for name, o in offs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    st, sb = x.stride(0), x.stride(1)
    assert lib.pika_ctc_decode_rows(x.data_ptr(), st, sb, il.data_ptr(), B, T, C, 0, K, 0, p["blank_lp"], p["top_val"],
                                    p["top_idx"], None, stream) == 0
    assert lib.pika_ctc_lm_beam_search(
        x.data_ptr(), st, sb, None, p["blank_lp"], p["top_val"], p["top_idx"], il.data_ptr(), B, T, C, 0, beam, nbest,
        *L.fst_args(lm), K, 0.5, 0.25, 1, p["tokens"], p["lengths"], p["scores"], p["am"], p["scratch"], stream) == 0
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    keep = np.ones(total, dtype=bool)
    for name, nbytes in sizes.items():
        keep[offs[name]:offs[name] + nbytes] = False
    assert (host[keep] == 0xA5).all(), "a kernel wrote outside its buffer"

    def view(name, dtype, shape):
        return np.frombuffer(host[offs[name]:offs[name] + sizes[name]].tobytes(), dtype=dtype).reshape(shape)
    s = ctc.ctc_beam_search_lm(x, il, lm, beam=beam, nbest=nbest, lm_weight=0.5, length_bonus=0.25, candidates=K)
    assert (view("tokens", np.int32, (B, nbest, T)) == s[0].cpu().numpy()).all()
    assert (view("lengths", np.int32, (B, nbest)) == s[1].cpu().numpy()).all()
    assert (view("scores", np.float32, (B, nbest)) == s[2].cpu().numpy()).all()
    assert (view("am", np.float32, (B, nbest)) == s[3].cpu().numpy()).all()


def test_lm_device_forms_are_one_device(hip_device):
    # "cuda", "cuda:0", torch.device("cuda") and None all name the device the tensors report
    from pika_amd import ctc
    case = L.LM_CASES[0]
    x = torch.from_numpy(case.lp[:, None].copy()).to(hip_device)
    outs = []
    for device in (None, "cuda", torch.device("cuda"), "cuda:%d" % x.device.index, x.device):
        lm = ctc.CtcNgramLm(case.lm.fst, case.lm.backoff_id, device=device)
        assert lm.device == x.device and lm.offsets.device == x.device
        outs.append(ctc.ctc_beam_search_lm(x, torch.tensor([case.T]), lm, beam=case.beam, candidates=case.candidates))
    assert all(torch.equal(u, v) for o in outs[1:] for u, v in zip(o, outs[0]))
