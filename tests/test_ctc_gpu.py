"""CTC loss, gradients and forced alignment on the MI355X against the float64 references of tests/ctc_common.py.

Tolerances.  The yardstick is torch's own fp32 CPU `F.ctc_loss` (behind an fp32 `log_softmax`) against the float64
reference on the same inputs: for each shape the HIP path's error may be at most 4x that fp32 error -- both
accumulate in fp32, in a different order -- with a floor of 1e-6 where the fp32 error happens to be (near) zero and,
for costs, the ceiling of the project's stated parity, 1e-3 relative.  Costs are compared relatively, gradients
absolutely (their entries lie in [-grad_cost, grad_cost]).  Every figure is printed (`CTCPARITY ...`) before it is
asserted; profiles/ctc_parity.txt is where that output is kept.

Alignment.  The score is compared with the float64 Viterbi of the SAME fp32 log-probs within ctc_common.bound (T rounded
additions); the returned frame labels must collapse to the transcript and rescore (float64) to the score; they must
equal the float64 path wherever it leads every other path by margin > 2 * bound; the tie cases are pinned exactly.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402

pytestmark = pytest.mark.gpu


def rand_seq(U, C, blank, seed):
    """U labels != blank, repeats allowed."""
    rng = np.random.RandomState(seed)
    classes = [c for c in range(C) if c != blank]
    return [int(classes[i]) for i in rng.randint(0, len(classes), size=U)]


def repeats(seq):
    return sum(1 for a, b in zip(seq, seq[1:]) if a == b)


class Case(object):
    """Seeded randn logits (T,B,C), transcripts, lengths; the float64 reference and the fp32 yardstick, computed once."""

    def __init__(self, name, T, C, seqs, ils=None, blank=0, seed=0, gc=None):
        self.name, self.T, self.C, self.seqs, self.blank = name, T, C, seqs, blank
        self.B = len(seqs)
        self.ils = list(ils) if ils is not None else [T] * self.B
        for s, t in zip(seqs, self.ils):
            assert t >= len(s) + repeats(s), (name, "infeasible")
        g = torch.Generator().manual_seed(1000 + seed)
        self.logits = torch.randn(T, self.B, C, generator=g)
        self.gc = None if gc is None else torch.tensor(gc, dtype=torch.float32)
        self._ref = None

    def ref(self):
        if self._ref is None:
            r64 = R.torch_reference(self.logits, self.seqs, self.ils, self.blank, self.gc, torch.float64)
            r32 = R.torch_reference(self.logits, self.seqs, self.ils, self.blank, self.gc, torch.float32)
            self._ref = (r64, r32)
        return self._ref

    def lp32(self):
        """The fp32 log-probs the GPU is given: the float64 log_softmax, rounded once."""
        return F.log_softmax(self.logits.double(), -1).float()

    def targets(self, fill=0):
        return R.pad_targets(self.seqs, fill=fill)

    def lens(self):
        return torch.tensor(self.ils), torch.tensor([len(s) for s in self.seqs])


def bounds(case):
    """(cost bound, d/d logits bound, d/d log_probs bound) from the fp32 yardstick."""
    (c64, dx64, dl64), (c32, dx32, dl32) = case.ref()
    e_cost = float(((c32 - c64).abs() / c64.abs().clamp(min=1e-30)).max())
    return (min(max(4 * e_cost, 1e-6), 1e-3), max(4 * float((dx32 - dx64).abs().max()), 1e-6),
            max(4 * float((dl32 - dl64).abs().max()), 1e-6))


def run_loss(case, dev, logits_form, x_cpu=None, **kw):
    """(costs, gradient) on the GPU through the public functions, as float64 CPU tensors."""
    from pika_amd import ctc
    x = (case.logits if logits_form else case.lp32()) if x_cpu is None else x_cpu
    x = x.to(dev).requires_grad_(True)
    il, tl = case.lens()
    fn = ctc.ctc_loss_from_logits if logits_form else ctc.ctc_loss
    costs = fn(x, kw.pop("targets", case.targets()), il, tl, blank=case.blank, reduction="none", **kw)
    gc = torch.ones(case.B) if case.gc is None else case.gc
    (costs * gc.to(dev)).sum().backward()
    return costs.detach().double().cpu(), x.grad.double().cpu()


def check_parity(case, dev, **kw):
    (c64, dx64, dl64), _ = case.ref()
    b_cost, b_dx, b_dl = bounds(case)
    for logits_form, gref, b_g in ((False, dl64, b_dl), (True, dx64, b_dx)):
        costs, grad = run_loss(case, dev, logits_form, **kw)
        e_cost = float(((costs - c64).abs() / c64.abs().clamp(min=1e-30)).max())
        e_grad = float((grad - gref).abs().max())
        print("CTCPARITY %-22s %-10s cost rel err %.3g (bound %.3g)  grad abs err %.3g (bound %.3g)" % (
            case.name, "logits" if logits_form else "log_probs", e_cost, b_cost, e_grad, b_g))
        assert torch.isfinite(grad).all()
        assert e_cost <= b_cost, (case.name, logits_form, e_cost, b_cost)
        assert e_grad <= b_g, (case.name, logits_form, e_grad, b_g)
        il = torch.tensor(case.ils)
        dead = torch.arange(case.T)[:, None] >= il[None, :]
        assert (grad[dead] == 0).all(), "gradient beyond T_n must be exactly zero"


def mk(name, T, C, Us, blank=0, seed=0, ils=None, gc=None):
    return Case(name, T, C, [rand_seq(U, C, blank, seed * 31 + i) for i, U in enumerate(Us)], ils, blank, seed, gc)


STATE_AXIS = [mk("U0", 5, 4, [0]), mk("U1", 4, 4, [1]), mk("U31", 70, 8, [31], seed=1), mk("U32", 70, 8, [32], seed=21),
              mk("U64", 140, 8, [64], seed=3), mk("U200_T420", 420, 16, [200], seed=4)]
TIME_AXIS = [Case("T1", 1, 4, [[], [2]], seed=5), Case("T_exact", 7, 4, [[1, 1, 2, 2, 3]], seed=6),
             mk("T600_U40_C32", 600, 32, [40], seed=7)]
REPEATS = [Case("all_one_class", 14, 2, [[1] * 6], seed=8), mk("alphabet2", 24, 3, [10, 7], seed=9),
           Case("alphabet3", 9, 3, [[1, 1, 2, 1], [2, 2]], seed=10)]
CLASS_AXIS = [mk("C%d_blank%d" % (C, bl), 6, C, [2, 1], blank=bl, seed=11 + C, gc=[0.5, 2.0])
              for C, bl in ((3, 0), (5, 4), (7, 3), (8, 7), (260, 100), (1028, 0))]
RAGGED = Case("ragged", 12, 5, [[1, 2, 3], [], [4, 4, 1, 2]], ils=[12, 7, 9], seed=12, gc=[1.0, 0.25, 3.0])
ALL = STATE_AXIS + TIME_AXIS + REPEATS + CLASS_AXIS + [RAGGED]


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_costs_and_gradients_against_float64(hip_device, case):
    check_parity(case, hip_device)


def test_ragged_batch_never_reads_padding(hip_device):
    case = RAGGED
    il, tl = case.lens()
    dead = torch.arange(case.T)[:, None] >= il[None, :]
    tg = case.targets(fill=0)
    for n, s in enumerate(case.seqs):       # labels beyond U_n: out of range on both sides
        tg[n, len(s):] = 999 if n % 2 else -7
    for logits_form in (False, True):
        x = (case.logits if logits_form else case.lp32()).clone()
        clean = run_loss(case, hip_device, logits_form)
        x[dead] = float("nan")
        dirty = run_loss(case, hip_device, logits_form, x_cpu=x, targets=tg)
        assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])
        assert (dirty[1][dead] == 0).all()


def test_unaligned_base_pointer(hip_device):
    from pika_amd import ctc
    case = CLASS_AXIS[3]                    # C = 8: the 16-byte writer when aligned
    il, tl = case.lens()
    for logits_form in (False, True):
        src = case.logits if logits_form else case.lp32()
        want = run_loss(case, hip_device, logits_form)
        flat = torch.zeros(src.numel() + 1, device=hip_device)
        x = flat[1:].view(src.shape)        # contiguous, base 4 bytes off a 16-byte boundary
        x.copy_(src)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
        x.requires_grad_(True)
        fn = ctc.ctc_loss_from_logits if logits_form else ctc.ctc_loss
        costs = fn(x, case.targets(), il, tl, blank=case.blank, reduction="none")
        (costs * case.gc.to(hip_device)).sum().backward()
        assert torch.equal(costs.double().cpu(), want[0]) and torch.equal(x.grad.double().cpu(), want[1])


def test_surface_forms_agree(hip_device):
    from pika_amd import ctc
    case, dev = RAGGED, hip_device
    il, tl = case.lens()
    lp = case.lp32().to(dev)
    want, gwant = run_loss(case, dev, False)
    flat = torch.tensor([c for s in case.seqs for c in s])
    forms = [(case.targets(), il, tl), (case.targets().int(), il.int(), tl.int()),
             (case.targets().to(dev), il.to(dev), tl.to(dev)), (case.targets().int().to(dev), il.int().to(dev), tl.int().to(dev)),
             (flat, il, tl), (flat.int().to(dev), il.to(dev), tl.int().to(dev)), (flat.to(dev), il.int(), tl)]
    for tg, a, b in forms:
        x = lp.clone().requires_grad_(True)
        costs = ctc.ctc_loss(x, tg, a, b, reduction="none")
        (costs * case.gc.to(dev)).sum().backward()
        assert torch.equal(costs.double().cpu(), want) and torch.equal(x.grad.double().cpu(), gwant)
    # non-contiguous log_probs: (B,T,C).transpose(0,1)
    x = lp.transpose(0, 1).contiguous().requires_grad_(True)
    costs = ctc.ctc_loss(x.transpose(0, 1), case.targets(), il, tl, reduction="none")
    assert not x.transpose(0, 1).is_contiguous()
    (costs * case.gc.to(dev)).sum().backward()
    assert torch.equal(costs.double().cpu(), want) and torch.equal(x.grad.transpose(0, 1).double().cpu(), gwant)
    # unbatched (T,C): utterance 0 on its own
    x = lp[:, 0].clone().requires_grad_(True)
    c0 = ctc.ctc_loss(x, torch.tensor(case.seqs[0]), torch.tensor(case.T), torch.tensor(len(case.seqs[0])),
                      reduction="none")
    assert c0.shape == ()
    (c0 * case.gc[0]).backward()
    assert float(c0) == float(want[0]) and torch.equal(x.grad.double().cpu(), gwant[:, 0])


def test_reductions_and_module(hip_device):
    from pika_amd import ctc
    case, dev = RAGGED, hip_device
    il, tl = case.lens()
    lp = case.lp32().to(dev)
    costs, _ = run_loss(case, dev, False)
    (c64, _, _), _ = case.ref()
    want = {"none": costs, "sum": costs.sum(), "mean": (costs / tl.clamp(min=1)).mean()}
    for red, go in (("none", torch.tensor([0.5, -1.0, 2.0])), ("sum", torch.tensor(3.0)), ("mean", torch.tensor(-0.7))):
        x = lp.clone().requires_grad_(True)
        out = ctc.ctc_loss(x, case.targets(), il, tl, reduction=red)
        assert torch.allclose(out.double().cpu(), want[red], rtol=1e-6, atol=0)
        out.backward(go.to(dev))
        # the same reduction through torch's autograd on the float64 reference
        w = {"none": go.double(), "sum": go.double().expand(3), "mean": go.double() / (3.0 * tl.clamp(min=1))}[red]
        _, _, dl = R.torch_reference(case.logits, case.seqs, case.ils, case.blank, w)
        _, _, dl32 = R.torch_reference(case.logits, case.seqs, case.ils, case.blank, w, torch.float32)
        err, bound = float((x.grad.double().cpu() - dl).abs().max()), max(4 * float((dl32 - dl).abs().max()), 1e-6)
        print("CTCPARITY %-22s %-10s grad abs err %.3g (bound %.3g)" % ("ragged/" + red, "log_probs", err, bound))
        assert err <= bound
        # module == function
        y = lp.clone().requires_grad_(True)
        out2 = ctc.CTCLoss(reduction=red)(y, case.targets(), il, tl)
        out2.backward(go.to(dev))
        assert torch.equal(out2, out) and torch.equal(y.grad, x.grad)
    ref_mean = F.ctc_loss(F.log_softmax(case.logits.double(), -1), case.targets(), il, tl, reduction="mean")
    assert float(want["mean"]) == pytest.approx(float(ref_mean), rel=1e-5)


def test_infeasible_rows(hip_device):
    from pika_amd import ctc
    dev = hip_device
    # row 0 feasible; row 1 too short for its repeats (T_n = 3 < 2 + 1 + ... ); row 2 carries a label >= C
    seqs, ils, T, C = [[1, 2], [1, 1, 2], [1, 7, 2]], [6, 3, 6], 6, 4
    good = Case("feasible_row", T, C, [seqs[0]], [6], seed=13)
    logits = torch.randn(T, 3, C, generator=torch.Generator().manual_seed(77))
    logits[:, 0] = good.logits[:, 0]
    il, tl = torch.tensor(ils), torch.tensor([2, 3, 3])
    (c64, dx64, dl64), _ = good.ref()
    for logits_form in (False, True):
        fn = ctc.ctc_loss_from_logits if logits_form else ctc.ctc_loss
        src = logits if logits_form else F.log_softmax(logits.double(), -1).float()
        for zi in (False, True):
            x = src.to(dev).requires_grad_(True)
            costs = fn(x, R.pad_targets(seqs), il, tl, reduction="none", zero_infinity=zi)
            costs.sum().backward()
            c = costs.double().cpu()
            assert (c[1:] == (0.0 if zi else float("inf"))).all(), c
            assert (x.grad[:, 1:] == 0).all() and torch.isfinite(x.grad).all()
            assert abs(float(c[0]) - float(c64[0])) <= bounds(good)[0] * float(c64[0])
            gref = dx64 if logits_form else dl64
            assert float((x.grad[:, 0].double().cpu() - gref[:, 0]).abs().max()) <= bounds(good)[1 if logits_form else 2]
    scores, fl = ctc.ctc_align(F.log_softmax(logits, -1).to(dev), R.pad_targets(seqs), il, tl)
    assert float(scores[2]) <= -1e30 and float(scores[1]) <= -1e30 and float(scores[0]) > -1e3
    assert (fl[1, :3] >= 0).all() and (fl[1, 3:] == -1).all() and (fl[2] >= 0).all()


def test_from_logits_equals_loss_of_log_softmax(hip_device):
    from pika_amd import ctc
    for case in (RAGGED, CLASS_AXIS[4], STATE_AXIS[3]):
        il, tl = case.lens()
        x = case.logits.to(hip_device)
        a = ctc.ctc_loss_from_logits(x, case.targets(), il, tl, blank=case.blank, reduction="none")
        b = ctc.ctc_loss(F.log_softmax(x, -1), case.targets(), il, tl, blank=case.blank, reduction="none")
        # two fp32 log-softmax roundings of every one of the T_n entries a path sums
        assert torch.allclose(a, b, rtol=0, atol=case.T * 2 ** -22 * float(case.logits.abs().max() + np.log(case.C)))


def test_two_runs_are_bit_identical(hip_device):
    for case in (REPEATS[0], REPEATS[1]):
        for logits_form in (False, True):
            a, b = run_loss(case, hip_device, logits_form), run_loss(case, hip_device, logits_form)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


ALIGN_CASES = STATE_AXIS + TIME_AXIS + REPEATS + [RAGGED] + CLASS_AXIS


def align_reference(case):
    """Per utterance: (score, frame labels, bound, unique) from the float64 Viterbi of the fp32 log-probs."""
    lp = case.lp32().double().numpy()
    out = []
    for n, seq in enumerate(case.seqs):
        x = lp[:case.ils[n], n]
        score, labels, _, delta = R.viterbi(x, seq, case.blank)
        b = R.bound(delta, case.ils[n])
        out.append((score, labels, b, R.margin(x, seq, case.blank) > 2 * b))
    return out


def test_alignment_against_float64_viterbi(hip_device):
    from pika_amd import ctc
    total = unique = 0
    for case in ALIGN_CASES:
        il, tl = case.lens()
        ref = align_reference(case)
        for logits_form in (False, True):
            if logits_form:
                scores, fl = ctc.ctc_align_from_logits(case.logits.to(hip_device), case.targets(), il, tl, blank=case.blank)
            else:
                scores, fl = ctc.ctc_align(case.lp32().to(hip_device), case.targets(), il, tl, blank=case.blank)
            assert fl.dtype == torch.int32 and fl.shape == (case.B, case.T)
            scores, fl = scores.double().cpu().numpy(), fl.cpu().numpy()
            lp = case.lp32().double().numpy()
            for n, seq in enumerate(case.seqs):
                Tn = case.ils[n]
                score, labels, b, uniq = ref[n]
                # the from-logits plane is logit - lse in fp32: one more rounding per frame
                tol = b if not logits_form else 3 * b + Tn * 2 ** -22 * float(case.logits.abs().max() + np.log(case.C))
                got = fl[n, :Tn]
                assert (fl[n, Tn:] == -1).all()
                assert R.collapse(got, case.blank) == list(seq), (case.name, n)
                assert abs(scores[n] - score) <= tol + 1e-12, (case.name, n, scores[n], score, tol)
                assert abs(R.rescore(lp[:Tn, n], got) - scores[n]) <= tol + 1e-12
                if not logits_form:
                    total += 1
                    unique += bool(uniq)
                    if uniq:
                        assert got.tolist() == labels.tolist(), (case.name, n)
    print("alignment: %d of %d utterances unique by margin" % (unique, total))
    assert total - unique <= 0.1 * total


def test_alignment_ties_are_pinned(hip_device):
    from pika_amd import ctc
    lp = torch.full((4, 5, 3), float(np.log(1.0 / 3.0)), device=hip_device)
    seqs = [[1], [1, 2], [1, 1], [], [1, 2]]
    il = torch.tensor([4, 4, 4, 4, 2])
    scores, fl = ctc.ctc_align(lp, R.pad_targets(seqs), il, torch.tensor([len(s) for s in seqs]))
    assert fl.cpu().tolist() == [[1, 0, 0, 0], [1, 2, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0], [1, 2, -1, -1]]
    want = il.float() * float(np.log(1.0 / 3.0))
    assert torch.allclose(scores.cpu(), want, rtol=1e-6)


def test_align_between_forward_and_backward_changes_nothing(hip_device):
    from pika_amd import ctc
    case, dev = STATE_AXIS[3], hip_device
    il, tl = case.lens()
    grads = []
    for with_align in (False, True):
        x = case.lp32().to(dev).requires_grad_(True)
        costs = ctc.ctc_loss(x, case.targets(), il, tl, reduction="none")
        if with_align:      # on the very workspace the backward will read
            dil, dtl, ws = costs.grad_fn.saved_tensors[-3:]
            scores, fl = ctc.align_workspace(ws, dil, dtl, case.B, case.T, case.targets().shape[1])
            s2, fl2 = ctc.ctc_align(x.detach(), case.targets(), il, tl)
            assert torch.equal(scores, s2) and torch.equal(fl, fl2)
        costs.sum().backward()
        grads.append((costs.detach().clone(), x.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_graph_capture_forward_backward_align(hip_device):
    from pika_amd import ctc
    dev = hip_device
    T, B, U, C = 9, 3, 4, 8
    gen = torch.Generator().manual_seed(5)
    data = [(torch.randn(T, B, C, generator=gen), [9, 7, 8], [4, 2, 3]), (torch.randn(T, B, C, generator=gen), [6, 9, 9], [1, 4, 0]),
            (torch.randn(T, B, C, generator=gen), [9, 9, 5], [3, 3, 2])]
    tg = torch.tensor([[1, 2, 2, 3], [4, 5, 6, 7], [3, 3, 1, 2]], device=dev)

    def step(x, il, tl):
        costs = ctc.ctc_loss_from_logits(x, tg, il, tl, reduction="none")
        (g,) = torch.autograd.grad(costs.sum(), x)
        scores, fl = ctc.ctc_align_from_logits(x.detach(), tg, il, tl)
        return costs.detach(), g, scores, fl

    sx = data[0][0].to(dev).requires_grad_(True)
    sil, stl = torch.tensor(data[0][1], dtype=torch.int32, device=dev), torch.tensor(data[0][2], dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up off the default stream, then one linear capture
        step(sx, sil, stl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(sx, sil, stl)
    for x, il, tl in data[1:]:
        with torch.no_grad():
            sx.copy_(x.to(dev))
        sil.copy_(torch.tensor(il, dtype=torch.int32))
        stl.copy_(torch.tensor(tl, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = step(x.to(dev).requires_grad_(True), torch.tensor(il, dtype=torch.int32, device=dev),
                     torch.tensor(tl, dtype=torch.int32, device=dev))
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)
