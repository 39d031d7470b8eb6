"""`ctc_nbest_align` on the MI355X against the float64 reference of tests/ctc_nbest_common.py.

For every feasible hypothesis of every case: the times are valid (0 <= start <= end < T_b, runs in order, equal
neighbours a frame apart) and the labelling they imply collapses to the hypothesis; its float64 rescore is at least the
float64 best minus 2 * bound; `best_scores` is within bound of that rescore; every token score is within bound of the
float64 sum over the GPU's own run; `full_scores` agrees with -dp_cost to the relative bound tests/test_ctc_gpu.py uses
for costs (4x the error of torch's fp32 CPU ctc_loss on the same hypotheses, floor 1e-6, ceiling 1e-3); and where the
float64 optimum is unique by margin > 2 * bound, starts / ends equal the float64 Viterbi's exactly.  `bound` is
ctc_common.bound: T rounded additions on values no larger than the float64 lattice's own.

The from-logits form reads logit - lse rounded once, behind an fp32 log-sum-exp: every value may differ from the fp32
log-prob by a few ulp of |logit| + |lse| <= 2 (max|logit| + log C), so over the T_b frames of a path its figures get
T_b * 2^-22 * (max|logit| + log C) on top of the bounds above (the allowance test_ctc_gpu.py makes for ctc_align), and
paths are compared where the margin exceeds twice that.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402
import ctc_nbest_common as NB  # noqa: E402

pytestmark = pytest.mark.gpu
GARBAGE = (-2 ** 31, 2 ** 31 - 1, -7, 2 ** 30)     # what stands beyond an entry's length


class Case(object):
    """lp (T,B,C) fp32; hyps[b] a list of label lists (None: missing); the float64 reference, computed once."""

    def __init__(self, name, lp, hyps, ils=None, blank=0):
        self.name, self.lp, self.hyps, self.blank = name, np.ascontiguousarray(lp, dtype=np.float32), hyps, blank
        self.T, self.B, self.C = self.lp.shape
        self.N = len(hyps[0])
        assert len(hyps) == self.B and all(len(h) == self.N for h in hyps)
        self.ils = list(ils) if ils is not None else [self.T] * self.B
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = [(NB.nbest_align(self.lp[:self.ils[b], b], self.hyps[b], self.blank),
                          NB.cost_bound(self.lp[:self.ils[b], b], [
                              h for h in self.hyps[b] if h is not None and NB.feasible(self.ils[b], self.C, h, self.blank)],
                              self.blank)) for b in range(self.B)]
        return self._ref

    def pack(self, L):
        """(tokens (B,N,L) int64 with garbage beyond every length, lengths (B,N) int64 with -1 for a missing entry)."""
        tokens = torch.tensor(GARBAGE, dtype=torch.int64).repeat(self.B, self.N, (L + 3) // 4)[:, :, :L].clone()
        lengths = torch.full((self.B, self.N), -1, dtype=torch.int64)
        for b, hs in enumerate(self.hyps):
            for k, h in enumerate(hs):
                if h is not None:
                    lengths[b, k] = len(h)
                    tokens[b, k, :min(len(h), L)] = torch.tensor(h[:L], dtype=torch.int64)
        return tokens, lengths


def run(case, dev, L, x=None, logits=False, il=None, **kw):
    from pika_amd import ctc
    tokens, lengths = case.pack(L)
    x = torch.from_numpy(case.lp).to(dev) if x is None else x
    fn = ctc.ctc_nbest_align_from_logits if logits else ctc.ctc_nbest_align
    out = fn(x, torch.tensor(case.ils) if il is None else il, tokens, lengths, blank=case.blank, **kw)
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.float32]
    assert [tuple(o.shape) for o in out] == [(case.B, case.N)] * 2 + [(case.B, case.N, L)] * 3
    return [o.cpu().numpy() for o in out]


def check(case, out, extra=0.0, max_len=None):
    """Every criterion of the module docstring; returns (unique by margin, feasible)."""
    full, best, starts, ends, tsc = out
    L = starts.shape[2]
    max_len = min(L, 511) if max_len is None else max_len
    unique = feasible = 0
    for b in range(case.B):
        refs, cb = case.ref()[b]
        Tb, lp64 = case.ils[b], case.lp[:case.ils[b], b].astype(np.float64)
        for k, r in enumerate(refs):
            where = (case.name, b, k)
            U = 0 if r is None else min(len(r.seq), L)
            if r is None or len(r.seq) > max_len or not r.feasible:
                if r is not None and len(r.seq) > max_len:
                    assert np.isnan(full[b, k]) and np.isnan(best[b, k]), where
                else:
                    assert full[b, k] == -np.inf and best[b, k] == -np.inf, where
                assert (starts[b, k] == -1).all() and (ends[b, k] == -1).all() and (tsc[b, k] == -np.inf).all(), where
                continue
            feasible += 1
            st, en = starts[b, k, :U].astype(np.int64), ends[b, k, :U].astype(np.int64)
            assert (starts[b, k, U:] == -1).all() and (ends[b, k, U:] == -1).all() and (tsc[b, k, U:] == -np.inf).all()
            assert (0 <= st).all() and (st <= en).all() and (en < Tb).all(), where
            assert (en[:-1] < st[1:]).all(), where
            for j in range(U - 1):
                if r.seq[j] == r.seq[j + 1]:
                    assert st[j + 1] - en[j] >= 2, where
            fl = NB.labelling(Tb, st, en, r.seq, case.blank)
            assert R.collapse(fl, case.blank) == r.seq, where
            rs = R.rescore(lp64, fl)
            tol = r.bound + extra
            print("NBEST %-22s b%d k%-2d U %3d  full err %.3g (bound %.3g)  best err %.3g  rescore gap %.3g (bound %.3g)" % (
                case.name, b, k, U, abs(full[b, k] + r.cost), cb * abs(r.cost) + extra, abs(best[b, k] - rs),
                r.best - rs, tol))
            assert rs >= r.best - 2 * tol, where
            assert abs(best[b, k] - rs) <= tol + 1e-12, where
            for j in range(U):
                assert abs(tsc[b, k, j] - NB.run_score(lp64, st[j], en[j], r.seq[j])) <= tol + 1e-12, where + (j,)
            assert abs(full[b, k] + r.cost) <= cb * abs(r.cost) + extra + 1e-12, where
            if r.unique and (extra == 0.0 or R.margin(lp64, r.seq, case.blank) > 2 * tol):
                unique += 1
                assert st.tolist() == r.starts.tolist() and en.tolist() == r.ends.tolist(), where
    return unique, feasible


def randn_cases():
    """The beam-search n-bests of the 3 * randn inputs, seeds 0-2 as one batch per shape."""
    out = []
    for T, C, beam in NB.RANDN_SHAPES:
        parts = [NB.randn_case(T, C, beam, seed) for seed in NB.SEEDS]
        out.append(Case("randn_T%d_C%d_N%d" % (T, C, beam), np.stack([p[0] for p in parts], 1), [p[1] for p in parts]))
    return out


RANDN = randn_cases()
ALT = [1, 2] * 256


@pytest.mark.parametrize("case", RANDN, ids=lambda c: c.name)
def test_beam_nbest_against_float64(hip_device, case):
    # L == T, narrower than T (but not than any hypothesis) and wider
    widest = max(len(h) for hs in case.hyps for h in hs)
    total = uniq = 0
    for L in (case.T, max(widest, 1), case.T + 5):
        u, f = check(case, run(case, hip_device, L))
        assert f == case.B * case.N
        total, uniq = total + f, uniq + u
    print("n-best alignment %s: %d of %d paths unique by margin" % (case.name, uniq, total))
    assert uniq >= 0.9 * total


def test_state_axis(hip_device):
    lens = (0, 1, 31, 32, 63, 64, 511)
    case = Case("state_axis", NB.randn_lp(520, 4, 20)[:, None], [[ALT[:U] for U in lens]])
    check(case, run(case, hip_device, 511))                         # Wp = 1024
    for max_len in (31, 32, 63, 64):                                # Wp = 64, 128, 128, 192: longer entries give NaN
        out = run(case, hip_device, 511, max_len=max_len)
        _, f = check(case, out, max_len=max_len)
        assert f == sum(U <= max_len for U in lens)
        assert np.isnan(out[0][0, lens.index(max_len) + 1])         # the entry of length max_len + 1 (or the next)
    short = Case("state_axis_plus1", case.lp, [[ALT[:32], ALT[:33], ALT[:31]]])
    out = run(short, hip_device, 40, max_len=31)
    check(short, out, max_len=31)
    assert np.isnan(out[0][0, 0]) and np.isnan(out[1][0, 1]) and np.isfinite(out[0][0, 2])


def test_time_axis(hip_device):
    one = Case("T1", NB.randn_lp(1, 4, 21)[:, None], [[[], [2], [1, 2]]])
    check(one, run(one, hip_device, 3))
    # T_b = U + repeats exactly: one path, full == best; one frame short: infeasible
    seq = [1, 1, 2, 2, 3]
    lp = np.stack([NB.randn_lp(8, 4, 22), NB.randn_lp(8, 4, 23)], 1)
    exact = Case("T_exact", lp, [[seq, [1, 2]], [seq, [3]]], ils=[7, 6])
    out = run(exact, hip_device, 5)
    check(exact, out)
    r = exact.ref()[0][0][0]
    assert abs(out[0][0, 0] - out[1][0, 0]) <= r.bound + exact.ref()[0][1] * abs(r.cost)
    assert out[0][1, 0] == -np.inf and out[1][1, 0] == -np.inf and (out[2][1, 0] == -1).all() and np.isfinite(out[0][1, 1])


def test_ragged_lengths_never_read_padding(hip_device):
    T, C, ils = 12, 5, [12, 7, 9, 1]
    lp = np.stack([NB.randn_lp(T, C, 30 + b) for b in range(4)], 1)
    hyps = [[[1, 2, 3], [4]], [[], [2, 2]], [[4, 4, 1, 2], [3]], [[1], []]]
    case = Case("ragged", lp, hyps, ils=ils)
    clean = run(case, hip_device, 6)
    check(case, clean)
    x = torch.from_numpy(lp).clone()
    for b, il in enumerate(ils):
        x[il:, b] = float("nan")
    for il_t in (torch.tensor(ils), torch.tensor(ils, dtype=torch.int32, device=hip_device)):
        for logits in (False, True):
            want = clean if not logits else run(case, hip_device, 6, logits=True)
            got = run(case, hip_device, 6, x=x.to(hip_device), il=il_t, logits=logits)
            for a, c in zip(want, got):
                assert np.array_equal(a, c)
    # lengths beyond [1,T] are clamped on the device
    wide = run(case, hip_device, 6, il=torch.tensor([99, 7, 9, -4]))
    for a, c in zip(clean, wide):
        assert np.array_equal(a, c)


def test_long_utterance_from_commit_lp(hip_device):
    # T = 600: a plain fp32 log-space lattice would carry |alpha| ~ 3.5 T here; the fp64 offset keeps the cost bound
    lp = NB.commit_lp(600, 32, 5)
    case = Case("T600_C32_commit_lp", lp[:, None], [NB.beam_hyps(lp, 4, 4)])
    _, f = check(case, run(case, hip_device, 600))
    assert f == 4


def test_repeats(hip_device):
    a = Case("all_one_class", NB.randn_lp(14, 2, 40)[:, None], [[[1] * 6, [1] * 7, [1] * 8]])
    _, f = check(a, run(a, hip_device, 8))
    assert f == 2                                                    # [1] * 8 needs 15 frames
    b = Case("alphabet3", NB.randn_lp(9, 3, 41)[:, None], [[[1, 1, 2, 1], [2, 2], [1, 2, 1, 2, 1]]])
    _, f = check(b, run(b, hip_device, 9))
    assert f == 3


def test_class_axis_and_strides(hip_device):
    dev = hip_device
    c5 = Case("C5_blank4", NB.randn_lp(7, 5, 50)[:, None], [[[0, 1], [3, 3], [2]]], blank=4)
    check(c5, run(c5, dev, 4))
    T, B, C = 6, 3, 1028
    lp = np.stack([NB.randn_lp(T, C, 51 + b) for b in range(B)], 1)
    wide = Case("C1028", lp, [[[1027, 5], [600]], [[1], [1027, 1027]], [[], [513, 2, 1027]]])
    dense = run(wide, dev, 3)
    check(wide, dense)
    batch_major = torch.from_numpy(lp).to(dev).transpose(0, 1).contiguous()          # (B,T,C)
    x = batch_major.transpose(0, 1)
    assert x.shape == (T, B, C) and x.stride() == (C, T * C, 1)
    buf = torch.empty(T * B * C + 1, device=dev)
    buf[1:].copy_(torch.from_numpy(lp).reshape(-1))
    shifted = buf[1:].view(T, B, C)
    assert shifted.data_ptr() % 16 == 4
    sliced = torch.from_numpy(lp).to(dev).repeat_interleave(2, dim=2)[:, :, ::2]     # class stride 2: the one copy
    for other in (x, shifted, sliced):
        for logits in (False, True):
            want = dense if not logits else run(wide, dev, 3, logits=True)
            for a, c in zip(want, run(wide, dev, 3, x=other, logits=logits)):
                assert np.array_equal(a, c)


def test_nbest_axis(hip_device):
    lp, hyps = NB.randn_case(40, 8, 8, 0)
    single = Case("N1", lp[:, None], [hyps[:1]])
    check(single, run(single, hip_device, 40))
    lp2, hyps2 = NB.randn_case(40, 8, 8, 1)
    holes = [[hyps[0], None, hyps[1], hyps[2], None, None, hyps[3], hyps[4]] * 2,
             [None, hyps2[0], hyps2[1], None, hyps2[2], hyps2[3], hyps2[4], None] * 2]
    case = Case("N16_holes", np.stack([lp, lp2], 1), holes)
    _, f = check(case, run(case, hip_device, 40))
    assert f == 20
    # int32 tokens and lengths already on the device; unbatched input
    from pika_amd import ctc
    tokens, lengths = single.pack(40)
    x = torch.from_numpy(lp).to(hip_device)
    out = ctc.ctc_nbest_align(x, torch.tensor([40], device=hip_device), tokens[0].to(hip_device, torch.int32),
                              lengths[0].to(hip_device, torch.int32))
    assert [tuple(o.shape) for o in out] == [(1,), (1,), (1, 40), (1, 40), (1, 40)]
    for a, c in zip(run(single, hip_device, 40), out):
        assert np.array_equal(a[0], c.cpu().numpy())


def test_refused_tokens(hip_device):
    lp, hyps = NB.randn_case(40, 8, 8, 2)
    good = Case("refused_clean", lp[:, None], [hyps[:4]])
    clean = run(good, hip_device, 40)
    h = hyps[1]
    assert len(h) >= 2
    bad = Case("refused", lp[:, None], [[hyps[0], h[:1] + [0] + h[1:], h[:-1] + [8], hyps[3]]])
    out = run(bad, hip_device, 40)
    _, f = check(bad, out)                      # entries 1 and 2: -inf and -1, as an infeasible entry
    assert f == 2
    for a, c in zip(clean, out):
        assert np.array_equal(a[0, 0], c[0, 0]) and np.array_equal(a[0, 3], c[0, 3])
    for logits_out in (run(bad, hip_device, 40, logits=True),):
        assert logits_out[0][0, 1] == -np.inf and logits_out[0][0, 2] == -np.inf


def test_from_logits_against_log_probs(hip_device):
    T, B, C, beam = 40, 3, 8, 8
    logits = 3.0 * torch.randn(T, B, C, generator=torch.Generator().manual_seed(60))
    lp = torch.log_softmax(logits.double(), -1).float().numpy()
    case = Case("forms", lp, [NB.beam_hyps(lp[:, b], beam, beam) for b in range(B)])
    check(case, run(case, hip_device, T))
    extra = T * 2.0 ** -22 * (float(logits.abs().max()) + float(np.log(C)))
    u, f = check(case, run(case, hip_device, T, x=logits.to(hip_device), logits=True), extra=extra)
    print("from_logits: %d of %d paths compared exactly" % (u, f))
    assert f == B * beam and u >= 0.9 * f


def test_search_output_goes_straight_in(hip_device):
    from pika_amd import ctc
    dev, T, B, C = hip_device, 40, 3, 8
    lp = np.stack([NB.randn_lp(T, C, 70 + b) for b in range(B)], 1)
    x, il = torch.from_numpy(lp).to(dev), torch.tensor([40, 33, 40], dtype=torch.int32, device=dev)

    def through(tokens, lengths, scores, ils):
        out = [o.cpu().numpy() for o in ctc.ctc_nbest_align(x, il, tokens, lengths)]
        tokens, lengths, scores = tokens.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()
        hyps = [[None if lengths[b, k] < 0 else tokens[b, k, :lengths[b, k]].tolist() for k in range(lengths.shape[1])]
                for b in range(B)]
        case = Case("search", lp, hyps, ils=ils)
        _, f = check(case, out)
        assert f == int((lengths >= 0).sum()) > 0           # every existing entry is feasible
        for b in range(B):
            for k, r in enumerate(case.ref()[b][0]):
                if r is not None:                           # the beam's tot sums a subset of the alignments
                    assert out[0][b, k] >= scores[b, k] - r.bound, (b, k, out[0][b, k], scores[b, k])
    through(*ctc.ctc_beam_search(x, il, beam=8, nbest=8), ils=[40, 33, 40])
    stream = ctc.CtcBeamStream(B, 64, beam=8, device=dev)   # results are (B,4,64): L wider than T
    for s0, s1 in ((0, 7), (7, 20), (20, 40)):
        stream.advance(x[s0:s1], (il - s0).clamp(0, s1 - s0))
    through(*stream.results(nbest=4), ils=[40, 33, 40])


def test_cross_check_against_align_and_loss(hip_device):
    from pika_amd import ctc
    dev, T, B, C, N = hip_device, 70, 2, 8, 4
    parts = [NB.randn_case(T, C, 16, seed) for seed in (0, 1)]
    case = Case("cross", np.stack([p[0] for p in parts], 1), [p[1][:N] for p in parts])
    full, best, starts, ends, _ = run(case, dev, T)
    tokens, lengths = case.pack(T)
    U = int(lengths.max())
    rep = torch.from_numpy(case.lp).to(dev).repeat_interleave(N, dim=1)
    tg, tl, il = tokens.reshape(B * N, T)[:, :U].clamp(0, C - 1), lengths.reshape(-1), torch.full((B * N,), T)
    scores, fl = ctc.ctc_align(rep, tg, il, tl)
    costs = ctc.ctc_loss(rep, tg, il, tl, reduction="none")
    scores, fl, costs = scores.cpu().numpy(), fl.cpu().numpy(), costs.double().cpu().numpy()
    for b in range(B):
        refs, cb = case.ref()[b]
        for k, r in enumerate(refs):
            n, u = b * N + k, len(r.seq)
            assert abs(full[b, k] + costs[n]) <= cb * abs(r.cost)
            assert abs(best[b, k] - scores[n]) <= r.bound
            if r.unique:
                assert NB.labelling(T, starts[b, k, :u], ends[b, k, :u], r.seq, 0).tolist() == fl[n].tolist()


def test_two_runs_are_bit_identical_and_graph_replay(hip_device):
    from pika_amd import ctc
    dev, T, C, N = hip_device, 40, 8, 8
    data = []
    for pair in ((0, 1), (2, 0), (1, 2)):
        parts = [NB.randn_case(T, C, N, seed) for seed in pair]
        case = Case("graph", np.stack([p[0] for p in parts], 1), [p[1] for p in parts])
        data.append((torch.from_numpy(case.lp), torch.tensor([40, 31 + pair[0]], dtype=torch.int32)) + tuple(
            t.to(torch.int32) for t in case.pack(T)))
    a = ctc.ctc_nbest_align(*[t.to(dev) for t in data[0]])
    b = ctc.ctc_nbest_align(*[t.to(dev) for t in data[0]])
    for p, q in zip(a, b):
        assert torch.equal(p, q)

    def step(x, il, tokens, lengths):
        return ctc.ctc_nbest_align(x, il, tokens, lengths) + ctc.ctc_nbest_align_from_logits(x, il, tokens, lengths)
    static = [t.to(dev) for t in data[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up off the default stream, then one linear capture
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*static)
    for item in data[1:]:
        for dst, src in zip(static, item):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for p, q in zip(outs, step(*[t.to(dev) for t in item])):
            assert torch.equal(p, q)
