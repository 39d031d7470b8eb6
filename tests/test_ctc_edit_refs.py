"""The host entry of the n-best edit distances (`pika_ctc_edit_distance_host`: the bit-vector recurrence of
csrc/ctc_edit_core.h, the one the kernel runs, in the kernel's block order) against dynamic programming, and the CPU
paths of `ctc_nbest_edit_distance`, `ctc_nbest_pairwise_distance` and `ctc_nbest_mbr_decode`.  No GPU.

References: `pika_amd.mbr.edit_distance` (plain Python) and `pika_edit_distances` (the library's two-row DP); every
distance is compared for exact equality.  The grid, the alphabets and the poisoned padding: tests/ctc_edit_common.py.
The MBR risks are float32 sums of at most N = 7 products P_j * d(i,j) of a float32 softmax: against the float64
restatement they are held to 16 * 2**-24 relative to the largest risk (exp and the division a few ulp each, N - 1
additions), the arg-min and the dead entries exactly -- the ties are built from duplicated entries, whose rows of the
distance matrix are identical, so their risks are the same float32 sum.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_edit_common as E  # noqa: E402


def one(a, r):
    a_t, a_l = E.pack([a], max(len(a), 1), 5)
    r_t, r_l = E.pack([r], max(len(r), 1), 5)
    return int(E.host(a_t[None], a_l[None], r_t[None], r_l[None])[0, 0, 0])


def test_hand_cases():
    assert one([1, 2, 3], [1, 2, 3]) == 0                       # equal
    assert one([1, 2, 3], [4, 5, 6, 7]) == 4                    # disjoint: the longer length
    assert one([4, 5, 6, 7], [1, 2, 3]) == 4
    assert one([], [1, 2, 3]) == 3 and one([1, 2, 3], []) == 3  # one side empty
    assert one([], []) == 0
    assert one([1, 3], [1, 2, 3]) == 1 and one([1, 2, 3], [1, 3]) == 1
    assert one([3, 2, 1, 4], [1, 2, 3]) == 3
    assert one([5, 5, 6, 6], [5, 6]) == 2
    assert one([2 ** 31 - 1, -2 ** 31, 0], [2 ** 31 - 1, 0]) == 1
    # kitten / sitting, and a reference that is one full block with the hypothesis equal to it but for both ends
    assert one([ord(c) for c in "kitten"], [ord(c) for c in "sitting"]) == 3
    block = list(range(100, 164))
    assert one(block, block) == 0 and one(block[1:], block) == 1 and one([7] + block[1:-1] + [8], block) == 2
    # widths 0: no token pointer at all
    for B, Na, Nr in ((2, 3, 2), (1, 1, 1)):
        a_l = np.array([[0, -1, 5][:Na]] * B, dtype=np.int32)
        r_l = np.array([[3, -2][:Nr]] * B, dtype=np.int32)
        r_t = np.arange(B * Nr * 4, dtype=np.int32).reshape(B, Nr, 4)
        out = E.host(np.zeros((B, Na, 0), np.int32), a_l, r_t, r_l)             # La = 0: the reference's length
        assert out.tolist() == [[[3, -1][:Nr], [-1, -1][:Nr], [3, -1][:Nr]][:Na]] * B
        out = E.host(r_t, r_l, np.zeros((B, Na, 0), np.int32), a_l)             # Lr = 0: the hypothesis's length
        assert out.tolist() == [[[3, -1, 3][:Na], [-1, -1, -1][:Na]][:Nr]] * B
    assert E.host(np.zeros((0, 3, 4)), np.zeros((0, 3)), np.zeros((0, 2, 4)), np.zeros((0, 2))).shape == (0, 3, 2)
    assert E.host(np.zeros((2, 0, 4)), np.zeros((2, 0)), np.ones((2, 2, 4)), np.ones((2, 2))).shape == (2, 0, 2)


@pytest.mark.parametrize("alphabet", E.ALPHABETS)
def test_length_grid_against_the_dp(alphabet):
    hyps, refs, poison = E.draw(alphabet, 11, E.HYP_LENGTHS, E.REF_LENGTHS)
    want = E.dp(hyps, refs)
    assert want.min() >= 0 and want[0].tolist() == list(E.REF_LENGTHS) and want[:, 0].tolist() == list(E.HYP_LENGTHS)
    # related sequences: away from the boundary the distance is neither 0 nor the longer length
    assert all(0 < want[i, j] < max(n, s) for i, n in enumerate(E.HYP_LENGTHS) for j, s in enumerate(E.REF_LENGTHS)
               if n >= 64 and s >= 63)
    a_t, a_l = E.pack(hyps, E.LA, poison)
    r_t, r_l = E.pack(refs, E.LR, poison)
    # one utterance, every reference against every hypothesis: (1,5,9)
    assert np.array_equal(E.host(a_t[None], a_l[None], r_t[None], r_l[None])[0], want)
    # one utterance per reference, Nr = 1, as `ctc_nbest_edit_distance` calls it: (9,5,1)
    got = E.host(np.broadcast_to(a_t, (len(refs),) + a_t.shape), np.broadcast_to(a_l, (len(refs),) + a_l.shape),
                 r_t[:, None], r_l[:, None])
    assert np.array_equal(got[:, :, 0].T, want)
    # the sides exchanged (the hypotheses as the pattern, at their own width): the distance is symmetric
    assert np.array_equal(E.host(r_t[None], r_l[None], a_t[None], a_l[None])[0], want.T)


def test_missing_entries_long_lengths_and_poisoned_padding():
    hyps, refs, poison = E.draw("two", 5, (70, 130, 9, 64), (129, 65, 40))
    # stored lengths beyond the row width count the row; the row is then full of real tokens
    a_rows = [hyps[0], (hyps[1], E.LA + 50), None, hyps[3], (hyps[2], 9)]
    r_rows = [(refs[0], 5000), None, refs[2], refs[1]]
    a_t, a_l = E.pack(a_rows, E.LA, poison)
    r_t, r_l = E.pack(r_rows, 129, poison)
    assert a_l.tolist() == [70, 180, -1, 64, 9] and r_l.tolist() == [5000, -1, 40, 65]
    want = E.dp([hyps[0], hyps[1], None, hyps[3], hyps[2]], [refs[0], None, refs[2], refs[1]])
    assert (want[2] == -1).all() and (want[:, 1] == -1).all() and (np.delete(np.delete(want, 2, 0), 1, 1) > 0).all()
    got = E.host(a_t[None], a_l[None], r_t[None], r_l[None])[0]
    assert np.array_equal(got, want)
    # other poison, same answer; the poison is a token of the alphabet, so reading one entry past a length would show
    for fill in (3, 7):
        a2, r2 = a_t.copy(), r_t.copy()
        for t, l in ((a2, a_l), (r2, r_l)):
            for k in range(len(l)):
                t[k, max(0, min(int(l[k]), t.shape[1])):] = fill
        assert np.array_equal(E.host(a2[None], a_l[None], r2[None], r_l[None])[0], want)
    # every negative length is "missing"
    a_l[0], r_l[2] = -2 ** 31, -7
    got = E.host(a_t[None], a_l[None], r_t[None], r_l[None])[0]
    assert (got[0] == -1).all() and (got[:, 2] == -1).all() and np.array_equal(got[1:, [0, 3]], want[1:, [0, 3]])


def hand_list():
    """The hand-checked list of tests/test_ctc_nbest_loss_surface.py."""
    tokens = torch.tensor([[[1, 2, 3, 9], [1, 3, 9, 9], [3, 2, 1, 4], [9, 9, 9, 9], [7, 7, 7, 7]],
                           [[5, 6, 9, 9], [9, 9, 9, 9], [6, 5, 9, 9], [5, 5, 6, 6], [1, 1, 1, 1]]])
    lengths = torch.tensor([[3, 2, 4, 0, -1], [2, 0, 2, 4, -1]])
    targets = torch.tensor([[1, 2, 3], [5, 6, 0]])
    return tokens, lengths, targets, torch.tensor([3, 2])


def test_cpu_path_equals_nbest_errors():
    from pika_amd import ctc
    tokens, lengths, targets, tl = hand_list()
    out = ctc.ctc_nbest_edit_distance(tokens, lengths, targets, tl)
    assert out.dtype == torch.float32 and out.device.type == "cpu"
    assert out.tolist() == [[0.0, 1.0, 3.0, 3.0, 0.0], [0.0, 2.0, 2.0, 2.0, 0.0]]
    assert torch.equal(out, ctc.ctc_nbest_errors(tokens, lengths, targets, tl))
    one_utt = ctc.ctc_nbest_edit_distance(tokens[1].to(torch.int32), lengths[1], targets[1, :2], torch.tensor(2))
    assert one_utt.tolist() == [0.0, 2.0, 2.0, 2.0, 0.0]
    # target lengths outside [0, S]: below 0 an empty transcript (not a missing one), beyond S the row
    for bad in ([-4, 9], [0, 3], [3, -1]):
        tl2 = torch.tensor(bad)
        got = ctc.ctc_nbest_edit_distance(tokens, lengths, targets, tl2)
        assert torch.equal(got, ctc.ctc_nbest_errors(tokens, lengths, targets, tl2)), bad
    assert ctc.ctc_nbest_edit_distance(tokens, lengths, targets, torch.tensor([-4, 9]))[0].tolist() == [3, 2, 4, 0, 0]
    # a seeded list: lengths beyond L, missing entries, int32 / int64 mixed, targets wider than the list
    g = torch.Generator().manual_seed(7)
    B, N, L, S = 3, 6, 70, 131
    tokens = torch.randint(1, 4, (B, N, L), generator=g)
    lengths = torch.randint(0, L + 9, (B, N), generator=g)
    lengths[0, 0], lengths[1, 1], lengths[2, 5], lengths[2, 2] = -1, L + 5, -3, 0
    targets = torch.randint(1, 4, (B, S), generator=g, dtype=torch.int32)
    tl = torch.tensor([131, 64, 200])
    got = ctc.ctc_nbest_edit_distance(tokens, lengths.to(torch.int32), targets, tl)
    assert torch.equal(got, ctc.ctc_nbest_errors(tokens, lengths, targets, tl)) and float(got.max()) > 60
    assert (lengths < 0).any() and (lengths > L).any() and ((got == 0) == (lengths < 0)).all()
    # empty shapes on either axis
    assert tuple(ctc.ctc_nbest_edit_distance(tokens[:, :, :0], lengths, targets, tl).shape) == (B, N)
    assert torch.equal(ctc.ctc_nbest_edit_distance(tokens, lengths, targets[:, :0], tl),
                       ctc.ctc_nbest_errors(tokens, lengths, targets[:, :0], tl))


def test_pairwise_is_symmetric_with_a_zero_diagonal():
    from pika_amd import ctc
    hyps, _, poison = E.draw("two", 21, (0, 1, 64, 65, 130, 65, 33), ())
    hyps[5] = list(hyps[3])                                         # a duplicate: distance 0 off the diagonal
    rows = hyps[:6] + [None] + hyps[6:]
    a_t, a_l = E.pack(rows, E.LA, poison)
    tokens, lengths = torch.from_numpy(a_t).long()[None].repeat(2, 1, 1), torch.from_numpy(a_l)[None].repeat(2, 1)
    lengths[1, 0] = -1
    d = ctc.ctc_nbest_pairwise_distance(tokens, lengths)
    assert tuple(d.shape) == (2, 8, 8) and d.dtype == torch.float32
    want = torch.from_numpy(E.dp(rows, rows)).clamp(min=0).float()
    assert torch.equal(d[0], want) and torch.equal(d[0], d[0].T) and torch.equal(d[1], d[1].T)
    assert (d.diagonal(dim1=1, dim2=2) == 0).all() and (d[0, 6] == 0).all() and (d[1, 0] == 0).all()
    assert d[0, 3, 5] == 0 and torch.equal(d[1, 1:, 1:], want[1:, 1:]) and d[0, 0].tolist() == a_l.clip(0).tolist()
    assert torch.equal(ctc.ctc_nbest_pairwise_distance(tokens[0].to(torch.int32), lengths[0]), d[0])


def test_mbr_decode_against_float64():
    from pika_amd import ctc
    hyps, _, poison = E.draw("two", 31, (12, 12, 13, 11, 12, 12, 9), ())
    hyps[1] = list(hyps[0])                         # entries 0 and 1 tie, whatever their scores
    hyps[5] = list(hyps[4])
    a_t, a_l = E.pack(hyps, 16, poison)
    B, N = 4, 7
    tokens, lengths = torch.from_numpy(a_t)[None].repeat(B, 1, 1), torch.from_numpy(a_l)[None].repeat(B, 1)
    g = torch.Generator().manual_seed(3)
    scores = 3.0 * torch.randn(B, N, generator=g)
    scores[0] = 0.0                                 # a flat posterior: the tied entries tie for the minimum or not at all
    lengths[1, 2], scores[1, 0], scores[1, 6] = -1, float("-inf"), float("nan")     # dead: missing, -inf, NaN
    lengths[2], scores[3] = -1, float("-inf")       # no live entry, by the lengths and by the scores
    d = E.dp(hyps, hyps).astype(np.float64)
    for scale in (1.0, 0.25):
        best, risks = ctc.ctc_nbest_mbr_decode(tokens, lengths, scores, scale=scale)
        assert best.dtype == torch.int64 and tuple(best.shape) == (B,) and risks.dtype == torch.float32
        s64, ln = scores.double().numpy(), lengths.numpy()
        for b in range(B):
            live = (ln[b] >= 0) & np.isfinite(s64[b])
            want = np.full(N, np.inf)
            if live.any():
                w = np.where(live, np.exp(np.where(live, scale * s64[b], 0.0) - (scale * s64[b][live]).max()), 0.0)
                want[live] = (d[live] * (w / w.sum())[None]).sum(-1)
            got = risks[b].double().numpy()
            assert np.array_equal(np.isinf(got), ~live) and (got[~live] > 0).all()
            if live.any():
                err, bound = np.abs(got[live] - want[live]).max(), 16 * 2.0 ** -24 * want[live].max()
                print("MBR b=%d scale=%.2f risk err %.3g (bound %.3g)" % (b, scale, err, bound))
                assert err <= bound
                # the lowest index among the entries whose float32 risk is the least
                assert int(best[b]) == int(np.flatnonzero(live & (got == got[live].min()))[0])
                near = np.flatnonzero(live & (want <= want[live].min() + 2 * bound))
                assert int(best[b]) in near
            else:
                assert int(best[b]) == -1
        assert risks[0, 0] == risks[0, 1] and risks[0, 4] == risks[0, 5] and int(best[0]) not in (1, 5)
        assert int(best[1]) not in (0, 2, 6)
    one_best, one_risks = ctc.ctc_nbest_mbr_decode(tokens[1], lengths[1], scores[1], scale=0.25)
    assert one_best.dim() == 0 and int(one_best) == int(best[1]) and torch.equal(one_risks, risks[1])
