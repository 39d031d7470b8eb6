"""`ctc_nbest_loss`, `ctc_mwer_loss` and their from-logits forms on the MI355X against the float64 reference of
tests/ctc_nbest_loss_common.py.

For every case, from log-probs and from logits, through `(full * w).sum().backward()` with random signed weights: every
live hypothesis's score within the relative bound (plus, from logits, the allowance for logit - lse), every dead one's
sentinel (-inf; NaN when longer than max_len), the gradient finite and within the absolute bound of the reference summed
over the live entries only -- the dead entries carry the weights NaN, +inf and 1e30 -- and rows t >= T_b exactly 0.0.
Every figure is printed (`NBLOSS ...`) before it is asserted.  Bounds: tests/ctc_nbest_loss_common.py.

MWER.  The risk is a smooth function of the scores with d risk / d full_k = g_k, so a score error delta_k moves it by
sum_k |g_k| delta_k to first order; the value is compared within twice that, delta_k being the score bound of entry k
(floor 1e-6).  The gradient is compared within the gradient bound that the yardstick gives for the reference's own
weights g.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_nbest_loss_common as NL  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = (float("nan"), float("inf"), 1e30)         # the weights of dead entries


def rand_seq(U, C, blank, seed, repeats=True):
    """U labels != blank; without `repeats` no two neighbours are equal."""
    rng = np.random.RandomState(seed)
    classes = [c for c in range(C) if c != blank]
    out = []
    for i in rng.randint(0, len(classes), size=U):
        c = classes[i]
        if not repeats and out and out[-1] == c:
            c = classes[(i + 1) % len(classes)]
        out.append(int(c))
    return out


class Case(object):
    """Seeded logits (T,B,C), an n-best list per utterance, lengths, signed weights; the reference, computed once."""

    def __init__(self, name, T, C, hyps, ils=None, blank=0, seed=0, scale=1.0, max_len=None, L=None, weights=None):
        self.name, self.T, self.C, self.hyps, self.blank = name, T, C, hyps, blank
        self.B, self.N = len(hyps), len(hyps[0])
        assert all(len(h) == self.N for h in hyps)
        self.ils = list(ils) if ils is not None else [T] * self.B
        g = torch.Generator().manual_seed(2000 + seed)
        self.logits = scale * torch.randn(T, self.B, C, generator=g)
        self.L = max([len(h) for hs in hyps for h in hs if h is not None] + [1]) if L is None else L
        self.max_len = min(self.L, 511) if max_len is None else max_len
        w = torch.randn(self.B, self.N, generator=g) if weights is None else torch.tensor(weights, dtype=torch.float32)
        self.weights = w.numpy().astype(np.float64)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = NL.Ref(self.logits, self.hyps, self.ils, self.weights, self.blank, self.max_len)
        return self._ref

    def lp32(self):
        """The fp32 log-probs the GPU is given: the float64 log_softmax, rounded once."""
        return torch.log_softmax(self.logits.double(), -1).float()

    def poisoned(self):
        """The weights as the GPU gets them: NaN, +inf and 1e30 at the dead entries."""
        w, n = torch.from_numpy(self.weights).float(), 0
        for b, k in zip(*np.nonzero(~self.ref().live)):
            w[b, k] = POISON[n % 3]
            n += 1
        return w


def run(case, dev, logits_form, x=None, il=None):
    """(full (B,N) numpy, gradient as float64 CPU tensor, the gradient as it came) through the public functions."""
    from pika_amd import ctc
    tokens, lengths = NL.pack(case.hyps, case.L)
    x = ((case.logits if logits_form else case.lp32()).to(dev) if x is None else x).detach().requires_grad_(True)
    fn = ctc.ctc_nbest_loss_from_logits if logits_form else ctc.ctc_nbest_loss
    full = fn(x, torch.tensor(case.ils) if il is None else il, tokens, lengths, blank=case.blank, max_len=case.max_len)
    assert full.dtype == torch.float32 and tuple(full.shape) == (case.B, case.N)
    # (autograd.grad hands over the tensor the backward wrote; .grad of a strided leaf would take the leaf's layout)
    (grad,) = torch.autograd.grad((full * case.poisoned().to(dev)).sum(), x)
    assert grad.shape == x.shape and grad.is_contiguous()
    return full.detach().cpu().numpy(), grad.double().cpu(), grad


def check(case, out, logits_form):
    full, grad, _ = out
    r = case.ref()
    worst = 0.0
    for b in range(case.B):
        for k in range(case.N):
            where = (case.name, logits_form, b, k)
            if not r.live[b, k]:
                want = r.full[b, k]
                assert (np.isnan(full[b, k]) if np.isnan(want) else full[b, k] == want), where
                continue
            tol = r.b_score * abs(r.full[b, k]) + (r.extra[b] if logits_form else 0.0)
            err = abs(full[b, k] - r.full[b, k])
            worst = max(worst, err / max(tol, 1e-300))
            assert err <= tol + 1e-12, where + (err, tol)
    gref, b_g = (r.dx, r.b_dx) if logits_form else (r.dlp, r.b_dlp)
    e_grad = float((grad - gref).abs().max())
    print("NBLOSS %-22s %-10s score err / bound %.3g (rel bound %.3g)  grad abs err %.3g (bound %.3g)  live %d of %d" % (
        case.name, "logits" if logits_form else "log_probs", worst, r.b_score, e_grad, b_g, int(r.live.sum()),
        r.live.size))
    assert torch.isfinite(grad).all(), case.name
    assert e_grad <= b_g, (case.name, logits_form, e_grad, b_g)
    dead = torch.arange(case.T)[:, None] >= torch.tensor(case.ils)[None, :]
    assert (grad[dead] == 0).all(), "gradient beyond T_b must be exactly zero"


def both(case, dev):
    for logits_form in (False, True):
        check(case, run(case, dev, logits_form), logits_form)


#   the empty one, adjacent repeats, two that share classes, an exact duplicate pair (entries 2 and 3; entry 1 shares
#   their classes), a missing entry, one infeasible by length (13 frames of 12, 10 of 9)
MIXED = Case("mixed", 12, 5, [[[], [2, 2, 1], [1, 2, 3], [1, 2, 3], None, [1] * 7],
                              [[], [3, 3, 2], [2, 3, 4], [2, 3, 4], None, [4, 4, 4, 4, 4, 1]]], ils=[12, 9], seed=1)
#   a token equal to blank, to C and to -3; an entry longer than max_len (NaN); two live ones
REFUSED = Case("refused", 10, 5, [[[1, 0, 2], [1, 5], [-3, 2], [1, 2, 3, 4], [1, 2], [3]]], seed=2, max_len=3, L=4)
STATE_AXIS = [
    Case("U31_one_wave", 70, 40, [[rand_seq(31, 40, 0, 3), rand_seq(20, 40, 0, 4)]], seed=3, max_len=31),
    Case("U32_two_waves", 70, 40, [[rand_seq(32, 40, 0, 5), rand_seq(31, 40, 0, 3)]], seed=4, max_len=32),
    Case("U511", 530, 600, [[rand_seq(511, 600, 0, 6, repeats=False), rand_seq(200, 600, 0, 7)]], seed=5),
]
FRAMES = [
    Case("Tb_1_7_8_9_17", 17, 6, [[[], [2], [3]]] + [[[], [1, 2, 2], [3, 1, 4, 2]]] * 4, ils=[1, 7, 8, 9, 17], seed=6),
    Case("T600_C8_peaky", 600, 8, [[rand_seq(40, 8, 0, 8), rand_seq(100, 8, 0, 9), []]], seed=7, scale=8.0),
]
CLASSES = [
    Case("C1", 5, 1, [[[], [0], [1]]], seed=8),                                          # only the empty one is live
    Case("C5_blank4", 6, 5, [[[0, 1], [3, 3], []], [[2], [1, 0, 1], [3]]], blank=4, seed=9),
    Case("C7_blank3", 6, 7, [[[0, 6], [5, 5], []], [[2], [1, 0, 1], [4]]], blank=3, seed=10),
    Case("C8_blank0", 6, 8, [[[7, 1], [3, 3], []], [[2], [1, 7, 1], [4]]], blank=0, seed=11),
    Case("C1028", 6, 1028, [[[1027, 5], [600]], [[1], [1027, 1027]]], seed=12),
]
ALL = [MIXED, REFUSED] + STATE_AXIS + FRAMES + CLASSES


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_scores_and_gradients_against_float64(hip_device, case):
    both(case, hip_device)


def test_mixed_list_is_what_it_says(hip_device):
    live = MIXED.ref().live
    assert live.tolist() == [[True, True, True, True, False, False]] * 2
    assert np.isnan(REFUSED.ref().full[0, 3]) and REFUSED.ref().live.tolist() == [[False] * 4 + [True] * 2]
    # the duplicate pair: the gradient of the sum of both weights times the single entry's
    one = Case("single", 12, 5, [[[1, 2, 3]], [[2, 3, 4]]], ils=[12, 9], seed=1, weights=[[1.0], [1.0]])
    pair = Case("pair", 12, 5, [[[1, 2, 3]] * 2, [[2, 3, 4]] * 2], ils=[12, 9], seed=1, weights=[[0.75, -2.0], [3.0, 0.5]])
    for logits_form in (False, True):
        g1, g2 = run(one, hip_device, logits_form)[1], run(pair, hip_device, logits_form)[1]
        r = pair.ref()
        tol = r.b_dx if logits_form else r.b_dlp
        assert float((g2[:, 0] + 1.25 * g1[:, 0]).abs().max()) <= tol
        assert float((g2[:, 1] - 3.5 * g1[:, 1]).abs().max()) <= tol


def test_strided_and_misaligned_views(hip_device):
    dev, case = hip_device, CLASSES[3]                      # C = 8: rows of 32 bytes, so alignment decides the path
    T, B, C = case.T, case.B, case.C
    for logits_form in (False, True):
        dense = (case.logits if logits_form else case.lp32()).to(dev)
        batch_major = dense.transpose(0, 1).contiguous().transpose(0, 1)
        assert batch_major.stride() == (C, T * C, 1)
        buf = torch.empty(T * B * C + 1, device=dev)
        buf[1:].copy_(dense.reshape(-1))
        shifted = buf[1:].view(T, B, C)
        assert shifted.data_ptr() % 16 == 4
        wide = torch.empty(T, B, 2 * C + 4, device=dev)
        wide[:, :, :C] = dense
        padded = wide[:, :, :C]                             # outer strides only: rows stay 16-byte aligned
        want = run(case, dev, logits_form)
        check(case, want, logits_form)
        for other in (batch_major, shifted, padded):
            got = run(case, dev, logits_form, x=other)
            check(case, got, logits_form)
            assert got[2].is_contiguous() and got[2].stride() == (B * C, C, 1)
            assert np.array_equal(got[0], want[0])


def test_from_logits_weights_summing_to_zero_and_not(hip_device):
    hyps = [[[1, 2], [2, 1, 1], [3], []], [[4, 4], [1], [2, 3, 1], [5, 1]]]
    w = np.array([[0.5, -1.25, 2.0, 0.0], [1.5, 0.25, -0.75, 0.0]])
    zero = w.copy()
    zero[:, 3] = -w.sum(1)
    assert (zero.sum(1) == 0).all()
    for name, weights in (("zero_sum", zero), ("nonzero_sum", w + np.array([[0.0, 0.0, 0.0, 0.5]]))):
        case = Case(name, 9, 6, hyps, ils=[9, 8], seed=20, weights=weights.tolist())
        assert case.ref().live.all() and abs(case.weights.sum(1)).max() == (0.0 if name == "zero_sum" else 4.0 - 2.25)
        both(case, hip_device)
    # absent: every row of d/d logits sums to ~0 only through the occupancies; present: the softmax term shows
    g = run(Case("zero_sum", 9, 6, hyps, ils=[9, 8], seed=20, weights=zero.tolist()), hip_device, True)[1]
    assert float(g.sum(-1).abs().max()) < 1e-5


def test_full_scores_equal_nbest_align_and_n1_equals_ctc_loss(hip_device):
    from pika_amd import ctc
    dev = hip_device
    for case in (MIXED, REFUSED, STATE_AXIS[1], FRAMES[1]):
        tokens, lengths = NL.pack(case.hyps, case.L)
        for logits_form in (False, True):
            x = (case.logits if logits_form else case.lp32()).to(dev)
            align = ctc.ctc_nbest_align_from_logits if logits_form else ctc.ctc_nbest_align
            loss = ctc.ctc_nbest_loss_from_logits if logits_form else ctc.ctc_nbest_loss
            a = align(x, torch.tensor(case.ils), tokens, lengths, blank=case.blank, max_len=case.max_len)[0]
            f = loss(x, torch.tensor(case.ils), tokens, lengths, blank=case.blank, max_len=case.max_len)
            r = case.ref()
            d = (a - f).abs().cpu().numpy()
            print("NBLOSS %-22s full_scores vs ctc_nbest_align: max abs diff %.3g" % (
                case.name, d[r.live].max() if r.live.any() else 0.0))
            assert (d[r.live] <= r.b_score * np.abs(r.full[r.live]) + 1e-12).all()
            assert torch.equal(a.isnan(), f.isnan()) and torch.equal(a[~a.isnan()], f[~f.isnan()])    # bit for bit
    # N = 1 against -ctc_loss(reduction='none') and its gradient
    T, B, C = 30, 3, 9
    seqs = [rand_seq(U, C, 0, 30 + U) for U in (6, 0, 11)]
    case = Case("N1", T, C, [[s] for s in seqs], ils=[30, 22, 27], seed=21, L=11)
    r = case.ref()
    tg, tl, il = torch.zeros(B, 11, dtype=torch.int64), torch.tensor([len(s) for s in seqs]), torch.tensor(case.ils)
    for b, s in enumerate(seqs):
        tg[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
    for logits_form in (False, True):
        full, grad, _ = run(case, dev, logits_form)
        x = (case.logits if logits_form else case.lp32()).to(dev).requires_grad_(True)
        costs = (ctc.ctc_loss_from_logits if logits_form else ctc.ctc_loss)(x, tg, il, tl, reduction="none")
        (costs * -torch.from_numpy(case.weights[:, 0]).float().to(dev)).sum().backward()
        assert (np.abs(full[:, 0] + costs.detach().cpu().numpy()) <= r.b_score * np.abs(r.full[:, 0]) + (
            max(r.extra) if logits_form else 0.0)).all()
        assert float((grad - x.grad.double().cpu()).abs().max()) <= (r.b_dx if logits_form else r.b_dlp)


def test_two_runs_are_bit_identical_and_graph_replay(hip_device):
    from pika_amd import ctc
    dev = hip_device
    a, b = run(MIXED, dev, False), run(MIXED, dev, False)
    assert np.array_equal(a[0], b[0], equal_nan=True) and torch.equal(a[2], b[2])
    a, b = run(STATE_AXIS[1], dev, True), run(STATE_AXIS[1], dev, True)
    assert np.array_equal(a[0], b[0]) and torch.equal(a[2], b[2])

    T, C, N, L = 24, 7, 4, 6
    data = []
    for seed, ils in ((0, [24, 17]), (1, [9, 24]), (2, [20, 21])):
        hyps = [[rand_seq(U, C, 0, 100 * seed + 10 * b + U) for U in (0, 3, 5, 6)] for b in range(2)]
        hyps[seed % 2][seed] = None
        g = torch.Generator().manual_seed(3000 + seed)
        tokens, lengths = NL.pack(hyps, L)
        data.append((torch.randn(T, 2, C, generator=g), torch.tensor(ils, dtype=torch.int32), tokens.to(torch.int32),
                     lengths.to(torch.int32), torch.randn(2, N, generator=g)))

    def step(x, il, tokens, lengths, w):
        out = []
        for fn in (ctc.ctc_nbest_loss, ctc.ctc_nbest_loss_from_logits):
            full = fn(x, il, tokens, lengths, max_len=L)
            out += [full.detach(), torch.autograd.grad((torch.nan_to_num(full, neginf=0.0) * w).sum(), x)[0]]
        return out
    static = [t.to(dev) for t in data[0]]
    static[0].requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up off the default stream, then one capture of forward and backward
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*static)
    for item in data[1:]:
        with torch.no_grad():
            for dst, src in zip(static, item):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = [t.to(dev) for t in item]
        eager[0].requires_grad_(True)
        for p, q in zip(outs, step(*eager)):
            assert torch.equal(p, q)
        assert outs[0].isinf().any() and outs[1].abs().max() > 0


def test_unbatched_form(hip_device):
    from pika_amd import ctc
    case = Case("unbatched", 11, 6, [[[1, 2], [], [3, 3, 1], None]], seed=22)
    tokens, lengths = NL.pack(case.hyps, case.L)
    r = case.ref()
    for logits_form in (False, True):
        x = (case.logits if logits_form else case.lp32())[:, 0].to(hip_device).requires_grad_(True)
        fn = ctc.ctc_nbest_loss_from_logits if logits_form else ctc.ctc_nbest_loss
        full = fn(x, torch.tensor([11]), tokens[0], lengths[0])
        assert tuple(full.shape) == (4,)
        (full * case.poisoned()[0].to(hip_device)).sum().backward()
        assert tuple(x.grad.shape) == (11, 6)
        batched = run(case, hip_device, logits_form)
        assert np.array_equal(full.detach().cpu().numpy(), batched[0][0]) and torch.equal(x.grad, batched[2][:, 0])
        assert float((x.grad.double().cpu() - (r.dx if logits_form else r.dlp)[:, 0]).abs().max()) <= (
            r.b_dx if logits_form else r.b_dlp)


def test_mwer_end_to_end(hip_device):
    from pika_amd import ctc
    dev, T, B, C, beam = hip_device, 40, 3, 12, 8
    g = torch.Generator().manual_seed(40)
    logits = 2.0 * torch.randn(T, B, C, generator=g)
    ils = [40, 33, 40]
    il = torch.tensor(ils, dtype=torch.int32, device=dev)
    lp32 = torch.log_softmax(logits.double(), -1).float()
    tokens, lengths, _ = ctc.ctc_beam_search(lp32.to(dev), il, beam=beam, nbest=beam)
    lengths = lengths.clone()
    lengths[2] = -1                                          # an utterance whose list is entirely dead
    refs = [rand_seq(U, C, 0, 50 + U) for U in (9, 7, 8)]
    targets = torch.zeros(B, 9, dtype=torch.int64)
    for b, s in enumerate(refs):
        targets[b, :len(s)] = torch.tensor(s)
    errors = ctc.ctc_nbest_errors(tokens, lengths, targets, torch.tensor([9, 7, 8]))
    assert errors.device == tokens.device and tuple(errors.shape) == (B, beam) and (errors[2] == 0).all()
    tk, ln = tokens.cpu().numpy(), lengths.cpu().numpy()
    hyps = [[None if ln[b, k] < 0 else tk[b, k, :ln[b, k]].tolist() for k in range(beam)] for b in range(B)]
    assert float(errors[:2].max()) > 0 and sum(h is not None for h in hyps[0]) == beam
    scores = NL.Ref(logits, hyps, ils, np.zeros((B, beam)), 0, 511)
    assert scores.live[:2].all() and not scores.live[2].any()
    for reduction in ("none", "sum", "mean"):
        value, gref = NL.mwer(scores.full, errors.cpu().numpy(), reduction)
        ref = NL.Ref(logits, hyps, ils, gref, 0, 511)          # the gradient for the reference's own weights
        for logits_form in (False, True):
            x = (logits if logits_form else lp32).to(dev).requires_grad_(True)
            fn = ctc.ctc_mwer_loss_from_logits if logits_form else ctc.ctc_mwer_loss
            risk = fn(x, il, tokens, lengths, errors, reduction=reduction)
            assert tuple(risk.shape) == ((B,) if reduction == "none" else ())
            risk.sum().backward()
            delta = ref.b_score * np.abs(np.where(ref.live, ref.full, 0.0)) + (
                np.array(ref.extra)[:, None] if logits_form else 0.0)
            tol = max(2.0 * float((np.abs(gref) * delta).sum()), 1e-6)
            err = float(np.abs(risk.detach().cpu().numpy() - value).max())
            e_grad = float((x.grad.double().cpu() - (ref.dx if logits_form else ref.dlp)).abs().max())
            b_g = ref.b_dx if logits_form else ref.b_dlp
            print("NBLOSS mwer %-5s %-10s value err %.3g (bound %.3g)  grad abs err %.3g (bound %.3g)" % (
                reduction, "logits" if logits_form else "log_probs", err, tol, e_grad, b_g))
            assert err <= tol
            assert torch.isfinite(x.grad).all() and e_grad <= b_g
            assert (x.grad[:, 2] == 0).all() and (x.grad[33:, 1] == 0).all()
            if reduction == "none":
                assert float(risk.detach()[2]) == 0.0


def test_no_replicated_input(hip_device):
    from pika_amd import _lib, ctc
    dev, T, B, C, N, U = hip_device, 64, 4, 1000, 8, 10
    g = torch.Generator().manual_seed(60)
    hyps = [[rand_seq(1 + (3 * b + k) % U, C, 0, 61 + 8 * b + k) for k in range(N)] for b in range(B)]
    tokens, lengths = (t.to(dev, torch.int32) for t in NL.pack(hyps, U))
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    ws = _lib.lib().pika_ctc_nbest_loss_workspace_bytes(B, N, T, U)
    limit = 2 * T * B * C * 4 + ws + (1 << 20)
    assert limit < 2 * N * T * B * C * 4                    # what the replicated route needs at the least
    for fn in (ctc.ctc_nbest_loss, ctc.ctc_nbest_loss_from_logits):
        x = torch.randn(T, B, C, generator=g).to(dev).requires_grad_(True)
        w = torch.randn(B, N, generator=g).to(dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        full = fn(x, il, tokens, lengths, max_len=U)
        (full * w).sum().backward()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        print("NBLOSS %s: peak growth %d bytes, limit %d, replicated route >= %d" % (
            fn.__name__, grown, limit, 2 * N * T * B * C * 4))
        assert torch.isfinite(full).all() and x.grad.abs().max() > 0
        assert grown < limit
