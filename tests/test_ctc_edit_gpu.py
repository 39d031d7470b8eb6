"""The n-best edit-distance kernel on the MI355X (`pika_ctc_edit_distance`, csrc/ctc_edit.hip) against the library's host
entry -- which tests/test_ctc_edit_refs.py holds to dynamic programming on a machine without a GPU -- and the device paths
of `ctc_nbest_edit_distance`, `ctc_nbest_pairwise_distance` and `ctc_nbest_mbr_decode`.  Every distance is compared for
exact equality.  The grid, the alphabets and the poisoned padding: tests/ctc_edit_common.py.

The point of the feature is the last test: `ctc_beam_search`, `ctc_nbest_edit_distance` and `ctc_mwer_loss` forward and
backward captured in ONE `torch.cuda.graph`, replayed on a second draw, bit-identical to the eager sequence.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_edit_common as E  # noqa: E402

pytestmark = pytest.mark.gpu


def device(dev, a_tokens, a_lengths, r_tokens, r_lengths):
    """pika_ctc_edit_distance on numpy arrays -> (B,Na,Nr) int32 numpy; the output starts from a value no pair gives."""
    from pika_amd import _lib
    t = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev) for x in (a_tokens, a_lengths, r_tokens, r_lengths)]
    (B, Na, La), (_, Nr, Lr) = t[0].shape, t[2].shape
    out = torch.full((B, Na, Nr), -77, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().pika_ctc_edit_distance(t[0].data_ptr(), t[1].data_ptr(), Na, La, t[2].data_ptr(),
                                                     t[3].data_ptr(), Nr, Lr, B, out.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "pika_ctc_edit_distance")
    return out.cpu().numpy()


def grid_case(alphabet):
    """B = 2, Na = Nr = 8: every reference length of the grid against every hypothesis length, plus a missing entry and
    a stored length beyond the row on each side."""
    ref_lengths = (E.REF_LENGTHS[:8], (4096, 129, 65, 1, 0, 64, 127, 63))
    a, r = [], []
    for b in range(2):
        hyps, refs, poison = E.draw(alphabet, 40 + b, E.HYP_LENGTHS + (130, 33), ref_lengths[b])
        a_rows = hyps[:5] + [(hyps[5], E.LA + 9), None, hyps[6]]
        r_rows = list(refs)
        if b == 1:
            r_rows[0], r_rows[7] = (refs[0], 4100), None
        a.append(E.pack(a_rows, E.LA, poison))
        r.append(E.pack(r_rows, E.LR, poison))
    return (np.stack([x[0] for x in a]), np.stack([x[1] for x in a]), np.stack([x[0] for x in r]),
            np.stack([x[1] for x in r]))


@pytest.mark.parametrize("alphabet", E.ALPHABETS)
def test_length_grid_against_the_host_entry(hip_device, alphabet):
    case = grid_case(alphabet)
    want = E.host(*case)
    assert want.shape == (2, 8, 8) and (want[:, 6] == -1).all() and (want[1, :, 7] == -1).all()
    live = np.delete(want, 6, 1)
    assert (live[0] >= 0).all() and (live[1, :, :7] >= 0).all() and want.max() == 4096
    got = device(hip_device, *case)
    assert np.array_equal(got, want)
    # the sides exchanged: the hypotheses (130 wide) as the pattern
    assert np.array_equal(device(hip_device, case[2], case[3], case[0], case[1]), want.transpose(0, 2, 1))
    # two runs are identical
    assert np.array_equal(device(hip_device, *case), got)


def test_one_pair_at_the_limit(hip_device):
    hyps, refs, poison = E.draw("int32", 50, (70,), (4096,))
    a_t, a_l = E.pack(hyps, 70, poison)
    r_t, r_l = E.pack(refs, 4096, poison)
    case = (a_t[None], a_l[None], r_t[None], r_l[None])
    want = E.host(*case)
    assert want.shape == (1, 1, 1) and 4096 - 70 <= want[0, 0, 0] < 4096
    assert np.array_equal(device(hip_device, *case), want)
    # no pair, and empty rows: nothing is launched or nothing is read
    assert device(hip_device, a_t[None][:, :0], a_l[None][:, :0], r_t[None], r_l[None]).shape == (1, 0, 1)
    assert device(hip_device, a_t[None][:, :, :0], a_l[None], r_t[None], r_l[None]).tolist() == [[[4096]]]
    assert device(hip_device, a_t[None], a_l[None], r_t[None][:, :, :0], r_l[None]).tolist() == [[[70]]]


def search_output(dev):
    """The list of tests/test_ctc_nbest_loss_gpu.py::test_mwer_end_to_end: (T,B,C,beam) = (40,3,12,8), one utterance's
    list set to missing."""
    from pika_amd import ctc
    T, B, C, beam = 40, 3, 12, 8
    g = torch.Generator().manual_seed(40)
    lp = torch.log_softmax(2.0 * torch.randn(T, B, C, generator=g).double(), -1).float().to(dev)
    il = torch.tensor([40, 33, 40], dtype=torch.int32, device=dev)
    tokens, lengths, scores = ctc.ctc_beam_search(lp, il, beam=beam, nbest=beam)
    lengths = lengths.clone()
    lengths[2] = -1
    targets = torch.randint(1, C, (B, 9), generator=g)
    return lp, il, tokens, lengths, scores, targets, torch.tensor([9, 7, 8])


def test_search_output_equals_nbest_errors_int32_and_int64(hip_device):
    from pika_amd import ctc
    dev = hip_device
    _, _, tokens, lengths, scores, targets, tl = search_output(dev)
    want = ctc.ctc_nbest_errors(tokens, lengths, targets, tl)            # the host route, copies and all
    assert float(want[:2].max()) > 0 and (want[2] == 0).all() and int(lengths[:2].min()) >= 0
    assert tokens.dtype == torch.int32 and targets.dtype == torch.int64
    for tk, ln, tg, t in ((tokens, lengths, targets.to(dev), tl.to(dev)),                     # everything on the device
                          (tokens.long(), lengths.long(), targets.to(dev, torch.int32), tl.to(dev, torch.int32)),
                          (tokens, lengths.long(), targets, tl)):                             # the reference on the host
        got = ctc.ctc_nbest_edit_distance(tk, ln, tg, t)
        assert got.dtype == torch.float32 and got.device == tokens.device and torch.equal(got, want)
    one = ctc.ctc_nbest_edit_distance(tokens[1], lengths[1], targets[1].to(dev), tl[1].to(dev))
    assert torch.equal(one, want[1])
    # CPU tensors take the host entry: the same numbers
    assert torch.equal(ctc.ctc_nbest_edit_distance(tokens.cpu(), lengths.cpu(), targets, tl), want.cpu())

    # pairwise on the same list against the host entry
    tk, ln = tokens.cpu().numpy(), lengths.cpu().numpy()
    pair = torch.from_numpy(E.host(tk, ln, tk, ln)).clamp(min=0).float()
    got = ctc.ctc_nbest_pairwise_distance(tokens, lengths)
    assert got.device == tokens.device and torch.equal(got.cpu(), pair) and float(pair[:2].max()) > 0
    assert torch.equal(got, got.transpose(1, 2)) and (got.diagonal(dim1=1, dim2=2) == 0).all() and (got[2] == 0).all()
    assert torch.equal(ctc.ctc_nbest_pairwise_distance(tokens.long(), lengths.long()), got)
    assert torch.equal(ctc.ctc_nbest_pairwise_distance(tokens, lengths), got)             # two runs
    # MBR decoding: the device path is the CPU path
    best, risks = ctc.ctc_nbest_mbr_decode(tokens, lengths, scores, scale=0.5)
    cpu_best, cpu_risks = ctc.ctc_nbest_mbr_decode(tokens.cpu(), lengths.cpu(), scores.cpu(), scale=0.5)
    assert best.device == tokens.device and int(best[2]) == -1 and int(cpu_best[2]) == -1
    for b in range(2):
        assert int(best[b]) == int(risks[b].argmin()) and int(cpu_best[b]) == int(cpu_risks[b].argmin())
    assert torch.isinf(risks[2]).all() and torch.isfinite(risks[:2]).all()
    assert float((risks[:2].cpu() - cpu_risks[:2]).abs().max()) <= 16 * 2.0 ** -24 * float(cpu_risks[:2].max())


def capture(step, static):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up off the default stream, then one capture
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(*static)
    return graph, outs


def test_no_synchronisation_under_capture(hip_device):
    from pika_amd import ctc
    dev = hip_device
    case = [torch.from_numpy(x).to(dev) for x in grid_case("two")]
    want = torch.from_numpy(E.host(*grid_case("two")))

    def step(a_t, a_l, r_t, r_l):
        return (ctc.ctc_nbest_edit_distance(a_t, a_l, r_t[:, 3], r_l[:, 3]), ctc.ctc_nbest_pairwise_distance(a_t, a_l),
                ctc.ctc_nbest_mbr_decode(a_t, a_l, a_l.float())[1])
    graph, outs = capture(step, case)
    eager = step(*case)
    case[1].copy_(case[1].roll(1, 1))       # other lengths under the same graph: what was padding is now read
    graph.replay()
    torch.cuda.synchronize()
    again = step(*case)
    for o, e, a in zip(outs, eager, again):
        assert torch.equal(o, a) and not torch.equal(o, e)
    assert torch.equal(eager[0].cpu(), want[:, :, 3].clamp(min=0).float())


def test_search_errors_and_mwer_in_one_graph(hip_device):
    from pika_amd import ctc
    dev, T, B, C, beam = hip_device, 40, 3, 12, 8
    data = []
    for seed, ils in ((40, [40, 33, 40]), (41, [31, 40, 40])):
        g = torch.Generator().manual_seed(seed)
        lp = torch.log_softmax(2.0 * torch.randn(T, B, C, generator=g).double(), -1).float()
        data.append((lp, torch.tensor(ils, dtype=torch.int32), torch.randint(1, C, (B, 9), generator=g),
                     torch.tensor([[9, 7, 8], [6, 9, 9]][seed - 40])))

    def step(x, il, targets, tl):
        tokens, lengths, _ = ctc.ctc_beam_search(x.detach(), il, beam=beam, nbest=beam)
        lengths = lengths.clone()
        lengths[2] = -1                                     # an utterance whose list is entirely dead
        errors = ctc.ctc_nbest_edit_distance(tokens, lengths, targets, tl)
        risk = ctc.ctc_mwer_loss(x, il, tokens, lengths, errors, reduction="none")
        return tokens, lengths, errors, risk.detach(), torch.autograd.grad(risk.sum(), x)[0]
    static = [t.to(dev) for t in data[0]]
    static[0].requires_grad_(True)
    graph, outs = capture(step, static)
    first = [o.clone() for o in outs]
    with torch.no_grad():
        for dst, src in zip(static, data[1]):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager = [t.to(dev) for t in data[1]]
    eager[0].requires_grad_(True)
    want = step(*eager)
    for name, p, q in zip(("tokens", "lengths", "errors", "risk", "grad"), outs, want):
        assert torch.equal(p, q), name
    tokens, lengths, errors, risk, grad = outs
    assert torch.equal(errors, ctc.ctc_nbest_errors(tokens, lengths, eager[2], eager[3]))
    assert float(errors[:2].max()) > 0 and float(risk[:2].abs().max()) > 0 and float(risk[2]) == 0.0
    assert float(grad[:, :2].abs().max()) > 0 and (grad[:, 2] == 0).all() and torch.isfinite(grad).all()
    assert not torch.equal(first[2], errors) and not torch.equal(first[4], grad)      # the replay saw the second draw
