"""CPU-side checks of the CTC surface: the float64 references of tests/ctc_common.py against brute force, the tie
rule, the Python signatures, and the C ABI's size formulas and argument refusals (no launch, no GPU)."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_common as R  # noqa: E402

# (T, C, transcript, blank): every T <= 5, C <= 3 family -- empty, single, repeats, skip rule, blank not at 0
BRUTE = [(1, 2, [], 0), (1, 3, [1], 0), (3, 2, [1], 0), (4, 3, [1, 2], 0), (5, 3, [1, 1], 0), (5, 3, [2, 1, 2], 0),
         (3, 3, [1, 1], 0), (5, 3, [0, 1], 2), (4, 3, [2, 0], 1), (5, 2, [1, 1, 1], 0), (2, 3, [1, 1], 0)]


@pytest.mark.parametrize("T,C,seq,blank", BRUTE)
def test_float64_reference_equals_brute_force(T, C, seq, blank):
    g = torch.Generator().manual_seed(100 * T + 10 * C + len(seq))
    logits = torch.randn(T, 1, C, generator=g)
    lp = F.log_softmax(logits.double(), -1)[:, 0].numpy()
    cost, best, arg = R.brute_force(lp, seq, blank)
    assert R.dp_cost(lp, seq, blank) == pytest.approx(cost, abs=1e-12) or (np.isinf(cost) and np.isinf(R.dp_cost(lp, seq, blank)))
    if np.isinf(cost):
        return                      # infeasible: nothing collapses to seq
    costs, _, _ = R.torch_reference(logits, [seq], [T], blank)
    assert float(costs[0]) == pytest.approx(cost, abs=1e-12)
    score, labels, _, _ = R.viterbi(lp, seq, blank)
    assert score == pytest.approx(best, abs=1e-12)
    assert labels.tolist() == arg.tolist()
    assert R.collapse(labels, blank) == list(seq)
    assert R.rescore(lp, labels) == pytest.approx(score, abs=1e-12)


def test_true_log_prob_gradient_is_minus_the_occupancy():
    # the derivation the GPU tests rest on: rows of the true d/d log_probs sum to -grad_cost on frames t < T_n
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(6, 2, 4, generator=g)
    gc = torch.tensor([0.5, 2.0])
    _, dlogits, dlp = R.torch_reference(logits, [[1, 2], [3]], [6, 4], 0, gc)
    assert torch.allclose(dlp[:, 0].sum(-1), torch.full((6,), -0.5, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(dlp[:4, 1].sum(-1), torch.full((4,), -2.0, dtype=torch.float64), atol=1e-12)
    assert (dlp[4:, 1] == 0).all() and (dlogits[4:, 1] == 0).all() and (dlp <= 1e-15).all()


def test_tie_rule_on_constant_inputs():
    lp = np.full((4, 3), np.log(1.0 / 3.0))
    # every path scores the same: end in the final blank, stay as long as the lattice allows
    assert R.viterbi(lp, [1], 0)[1].tolist() == [1, 0, 0, 0]
    assert R.viterbi(lp, [1, 2], 0)[1].tolist() == [1, 2, 0, 0]
    assert R.viterbi(lp, [1, 1], 0)[1].tolist() == [1, 0, 1, 0]
    assert R.viterbi(lp, [], 0)[1].tolist() == [0, 0, 0, 0]
    assert R.viterbi(lp[:2], [1, 2], 0)[1].tolist() == [1, 2]   # T = U: must end in the last label


def test_alignment_cases_meet_the_margin_cap_in_float64():
    # the GPU test compares paths exactly only where the float64 optimum is unique by margin > 2 * bound; at most one
    # utterance in ten of its seeded cases may fall under that margin -- a property of the reference alone
    import test_ctc_gpu as G
    flags = [uniq for case in G.ALIGN_CASES for (_, _, _, uniq) in G.align_reference(case)]
    assert len(flags) >= 20 and flags.count(False) <= 0.1 * len(flags), flags


def test_signatures_equal_torch():
    import pika_amd
    from pika_amd import ctc
    want = [(p.name, p.default) for p in inspect.signature(F.ctc_loss).parameters.values()]
    for fn in (ctc.ctc_loss, ctc.ctc_loss_from_logits, pika_amd.ctc_loss):
        assert [(p.name, p.default) for p in inspect.signature(fn).parameters.values()][1:] == want[1:]
    assert list(inspect.signature(ctc.ctc_loss).parameters)[0] == "log_probs"
    mod, ref = ctc.CTCLoss(), torch.nn.CTCLoss()
    assert (mod.blank, mod.reduction, mod.zero_infinity) == (ref.blank, ref.reduction, ref.zero_infinity)
    assert list(inspect.signature(mod.forward).parameters) == list(inspect.signature(ref.forward).parameters)
    assert [p.default for p in inspect.signature(ctc.CTCLoss.__init__).parameters.values()][1:] == [0, "mean", False]
    assert list(inspect.signature(ctc.ctc_align).parameters) == ["log_probs", "targets", "input_lengths",
                                                                "target_lengths", "blank"]
    for name in ("ctc_loss", "ctc_loss_from_logits", "CTCLoss", "ctc_align", "ctc_align_from_logits"):
        assert getattr(pika_amd, name) is getattr(ctc, name)


def test_cpu_tensors_are_refused():
    from pika_amd import ctc
    lp = torch.zeros(3, 1, 4)
    args = (lp, torch.ones(1, 1, dtype=torch.int64), torch.tensor([3]), torch.tensor([1]))
    for fn in (ctc.ctc_loss, ctc.ctc_loss_from_logits, ctc.ctc_align, ctc.ctc_align_from_logits, ctc.CTCLoss()):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(*args)


def test_size_formulas_follow_the_header():
    from pika_amd import _lib
    lib = _lib.lib()

    def ws(B, T, U):
        Wp = (2 * U + 1 + 63) // 64 * 64
        return 12 * B * T * Wp + 16 * B * T + 8 * B + 12 * B * Wp, B * T * Wp

    for dims in [(32, 240, 50), (1, 1, 0), (3, 9, 31), (3, 9, 32), (2, 420, 200), (1, 5, 511)]:
        assert (lib.pika_ctc_workspace_bytes(*dims), lib.pika_ctc_align_scratch_bytes(*dims)) == ws(*dims)
    for dims in [(0, 5, 1), (1, 0, 1), (1, 5, -1), (-1, 5, 1), (1, 5, 512)]:
        assert lib.pika_ctc_workspace_bytes(*dims) == 0 and lib.pika_ctc_align_scratch_bytes(*dims) == 0


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from pika_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2
    p = ctypes.c_void_p(0x1000)     # never dereferenced: EVERY call below is refused before any launch
    good = dict(B=2, T=5, U=3, C=4, blank=0)

    # q: the eight distinct pointers (log_probs/logits, targets, input_lengths, target_lengths, costs/scores, workspace,
    # grads/frame_labels/scratch, lse)
    CALLS = {
        "forward": lambda q, B, T, U, C, blank: lib.pika_ctc_loss_forward(
            q[0], q[1], p, q[2], q[3], B, T, U, C, blank, q[4], q[5], None),
        "backward": lambda q, B, T, U, C, blank: lib.pika_ctc_loss_backward(
            q[2], q[3], B, T, U, C, blank, p, q[5], q[6], None),
        "fused_forward": lambda q, B, T, U, C, blank: lib.pika_ctc_fused_forward(
            q[0], q[1], p, q[2], q[3], B, T, U, C, blank, q[4], q[7], q[5], None),
        "fused_backward": lambda q, B, T, U, C, blank: lib.pika_ctc_fused_backward(
            q[0], q[7], q[2], q[3], B, T, U, C, blank, p, q[5], q[6], None),
        "align": lambda q, B, T, U, C, blank: lib.pika_ctc_align(q[5], q[2], q[3], B, T, U, q[4], q[6], q[6], None),
    }
    full = [p] * 8
    for kw in (dict(B=0), dict(T=0), dict(B=-1), dict(T=-3), dict(U=-1), dict(C=0), dict(blank=-1), dict(blank=4)):
        for name, call in CALLS.items():
            if name == "align" and ("C" in kw or "blank" in kw):
                continue            # the alignment takes neither: not called, it would not be refused
            assert call(full, **dict(good, **kw)) == EINVAL, (kw, name)
    for name, call in CALLS.items():
        assert call(full, **dict(good, U=512)) == ETOOBIG, name
    # null pointers: q-index -> the calls that take that pointer (only those are called)
    needs = {0: ("forward", "fused_forward", "fused_backward"), 1: ("forward", "fused_forward"),
             2: tuple(CALLS), 3: tuple(CALLS), 4: ("forward", "fused_forward", "align"), 5: tuple(CALLS),
             6: ("backward", "fused_backward", "align"), 7: ("fused_forward", "fused_backward")}
    for i, names in needs.items():
        q = [None if j == i else p for j in range(8)]
        for name in names:
            assert CALLS[name](q, **good) == EINVAL, (i, name)
