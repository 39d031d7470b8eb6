"""`modified_beam_search_skip` and the training chain on reduced frames, on the tiny LSTM and stateless models of
tests/test_msearch_gpu.py and tests/test_stateless_search_gpu.py.

Everything is bit for bit.  With a threshold above 1 nothing is dropped and the call is `modified_beam_search`.  With real
dropping the reference is `modified_beam_search` itself on a model whose encoder is a stub that returns the frames reduced
in numpy (tests/frame_skip_common.py) by the plan's frame_index, with x_len = kept_lengths; the plan in turn is checked
against the numpy definition on its own blank_lp.  The CTC head is a seeded linear layer; the threshold is the median
blank posterior it gives on the utterances' frames, so about half of them go."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frame_skip_common as FC  # noqa: E402

pytestmark = pytest.mark.gpu


def tiny(dec, dev):
    """-> (net, x on the device, x_len): the tiny model with the LSTM ('rnn') or the stateless prediction network."""
    if dec == "stateless":
        import test_stateless_search_gpu as TS
        return TS.tiny(dev)
    import test_msearch_gpu as TG
    net, (x, x_len) = TG.tiny(dec, dev)
    return net, x.to(dev), x_len


class StubEncoder(object):
    """The model with an encoder that returns `frames` whatever it is given."""

    def __init__(self, net, frames):
        self._net, self._frames = net, frames

    def __getattr__(self, name):
        return getattr(self._net, name)

    def encode(self, x, x_len):
        return self._frames

    def encoder(self, x):
        return self._frames


def head_and_threshold(net, x, x_len, dev):
    """A seeded CTC head on the encoder output and the median blank posterior over the utterances' frames."""
    with torch.no_grad():
        enc = net.encode(x, x_len) if net.pack_seq else net.encoder(x)
        torch.manual_seed(3)
        head = torch.nn.Linear(enc.shape[2], net.output_dim).to(dev)
        head.weight.mul_(4.0)
        post = torch.softmax(head(enc).double(), dim=2)[:, :, 0].cpu().numpy()
    valid = np.arange(enc.shape[1])[None, :] < np.asarray(x_len)[:, None]
    values = np.sort(post[valid])
    mid = len(values) // 2
    return head, float(0.5 * (values[mid] + values[mid - 1])), enc


def check_plan(plan, x_len, threshold):
    want = FC.plan(plan.blank_lp.cpu().numpy(), np.asarray(x_len), threshold)
    for g, w in zip(plan[:3], want[:3]):
        assert np.array_equal(g.cpu().numpy(), w)
    kept, total = int(want[0].sum()), int(np.asarray(x_len).sum())
    assert 0.25 * total <= kept <= 0.75 * total                     # frames really go, frames really stay
    return want


@pytest.mark.parametrize("dec", ["rnn", "stateless"])
def test_nothing_dropped_is_the_plain_search(hip_device, dec):
    from pika_amd import modified_beam_search, modified_beam_search_skip
    net, x, x_len = tiny(dec, hip_device)
    head, _, _ = head_and_threshold(net, x, x_len, hip_device)
    K = 4
    want = modified_beam_search(net, x, x_len, beam=K, nbest=K, sm_scale=0.85, precision="fp32")
    got = modified_beam_search_skip(net, x, x_len, head, threshold=1.5, beam=K, nbest=K, sm_scale=0.85, precision="fp32")
    assert len(got) == 5
    for g, w in zip(got[:3] + got[4:], want):
        assert torch.equal(g, w)
    plan = got[3]
    assert plan.kept_lengths.tolist() == [min(int(n), x.shape[1]) for n in x_len]


@pytest.mark.parametrize("dec", ["rnn", "stateless"])
def test_dropping_equals_the_search_on_the_reduced_frames(hip_device, dec):
    from pika_amd import CtcHotwords, modified_beam_search, modified_beam_search_lm, modified_beam_search_skip
    dev = hip_device
    net, x, x_len = tiny(dec, dev)
    head, thr, _ = head_and_threshold(net, x, x_len, dev)
    kw = dict(beam=4, nbest=4, sm_scale=0.85, precision="fp32")
    for use_graph in (True, False):
        plain = modified_beam_search(net, x, x_len, use_graph=use_graph, **kw)
        enc = plain[3]                                              # (the encoder's output in this call's precision)
        got = modified_beam_search_skip(net, x, x_len, head, threshold=thr, use_graph=use_graph, **kw)
        plan = got[3]
        want_plan = check_plan(plan, x_len, thr)
        assert torch.equal(got[4], enc)                             # the ORIGINAL encoder output comes back
        reduced = torch.from_numpy(FC.apply(enc.cpu().numpy(), want_plan[1])).to(dev)
        want = modified_beam_search(StubEncoder(net, reduced), x, plan.kept_lengths, use_graph=use_graph, **kw)
        for g, w in zip(got[:3], want[:3]):
            assert torch.equal(g, w)
        assert not torch.equal(plain[2], got[2])                    # (the dropped frames did change the search)
    hot = CtcHotwords([[3, 4], [5]], net.output_dim, 1.0, 0, dev)
    lm_kw = dict(lm_weight=0.7, length_bonus=0.25, candidates=8)
    got = modified_beam_search_skip(net, x, x_len, head, threshold=thr, lm=hot, **kw, **lm_kw)
    assert len(got) == 6
    want = modified_beam_search_lm(StubEncoder(net, reduced), x, got[4].kept_lengths, hot, **kw, **lm_kw)
    for g, w in zip(got[:4], want[:4]):
        assert torch.equal(g, w)
    assert not torch.equal(got[2], got[3])                          # (the LM's bonus is in the scores)


@pytest.mark.parametrize("dec", ["rnn", "stateless"])
def test_times_are_original_encoder_frames(hip_device, dec):
    from pika_amd import modified_beam_search_skip, modified_beam_search_timed
    dev = hip_device
    net, x, x_len = tiny(dec, dev)
    head, thr, _ = head_and_threshold(net, x, x_len, dev)
    kw = dict(beam=4, nbest=4, sm_scale=0.85, precision="fp32")
    tokens, lengths, scores, times, plan, enc = modified_beam_search_skip(net, x, x_len, head, threshold=thr,
                                                                          timed=True, **kw)
    want_plan = check_plan(plan, x_len, thr)
    reduced = torch.from_numpy(FC.apply(enc.cpu().numpy(), want_plan[1])).to(dev)
    t2, l2, s2, reduced_times, _ = modified_beam_search_timed(StubEncoder(net, reduced), x, plan.kept_lengths, **kw)
    assert torch.equal(tokens, t2) and torch.equal(lengths, l2) and torch.equal(scores, s2)
    times, reduced_times, lengths = times.cpu().numpy(), reduced_times.cpu().numpy(), lengths.cpu().numpy()
    labels = 0
    for b in range(tokens.shape[0]):
        for j in range(tokens.shape[1]):
            n = max(int(lengths[b, j]), 0)
            assert (times[b, j, n:] == -1).all()
            row = times[b, j, :n]
            assert np.array_equal(row, want_plan[1][b, reduced_times[b, j, :n]])
            assert (np.diff(row) > 0).all() and (row >= 0).all() and (row < int(x_len[b])).all()
            labels += n
    assert labels > 4
    assert (times != reduced_times).any()                           # (the map is not the identity here)


def test_training_chain_reaches_the_encoder_output(hip_device):
    """`frame_skip_apply` -> `rnnt_pruned_joint_loss_modified` on kept_lengths, min_frames = labels_lengths, at
    tests/test_joint_banded_gpu.py's end-to-end shape (B,T,U,H,V,S) = (3,20,6,64,16,3): the loss is finite (T' >= U), the
    gradient reaches enc and is zero exactly on the dropped rows."""
    import test_joint_banded_gpu as J
    from pika_amd import ctc_skip_plan, frame_skip_apply, rnnt_pruned_joint_loss_modified
    dev = hip_device
    S, H, V = (J.E2E[k] for k in "SHV")
    enc0, pred0, y, tl, ul = J._e2e_inputs(11)
    layers = J._layers(H, H, V, dev, 2, simple=True)
    torch.manual_seed(5)
    head = torch.nn.Linear(H, V).to(dev)
    enc, pred = enc0.to(dev).requires_grad_(True), pred0.to(dev).requires_grad_(True)
    tld, uld = tl.to(dev), ul.to(dev)
    with torch.no_grad():
        post = torch.softmax(4.0 * head(enc).double(), dim=2)[:, :, 0].cpu().numpy()
    valid = np.arange(enc.shape[1])[None, :] < tl.numpy()[:, None]
    thr = float(np.quantile(post[valid], 0.2))                      # most frames go: min_frames has work to do
    plan = ctc_skip_plan(4.0 * head(enc), tld, 0, thr, min_frames=uld, from_logits=True)
    want = FC.plan(plan.blank_lp.cpu().numpy(), tl.numpy(), thr, ul.numpy())
    for g, w in zip(plan[:3], want[:3]):
        assert np.array_equal(g.cpu().numpy(), w)
    natural = FC.plan(plan.blank_lp.cpu().numpy(), tl.numpy(), thr)[0]
    assert (want[0] >= ul.numpy()).all() and (natural < ul.numpy()).any() and (want[0] < tl.numpy()).all()
    enc2 = frame_skip_apply(enc, plan)
    simple, pruned, _ = rnnt_pruned_joint_loss_modified(enc2, pred, y.to(dev), plan.kept_lengths, uld, *layers,
                                                        s_range=S, reduction=None)
    assert bool(torch.isfinite(simple).all()) and bool(torch.isfinite(pruned).all())
    (simple.sum() + pruned.sum()).backward()
    grad = enc.grad.cpu().numpy()
    assert np.isfinite(grad).all()
    dropped = want[2] < 0
    assert (grad[dropped] == 0).all()
    assert (np.abs(grad[~dropped]).max(axis=1) > 0).all()           # every kept frame got a gradient
