"""The one-symbol-per-frame searches on a transducer with the STATELESS prediction network (`Net` with
decoder_type='stateless'): graph against eager, beam = 1 against a float64 greedy run of the definition, the LM, neural-LM
and timed drivers at zero weights against the plain one, and `ModifiedStreamDecoder` against the one-shot call.

The tiny model: encoder_type='rnn', rnn_size=32, 12 classes, input width 8, B = 3, ragged T of 9, 8, 7.  SEED and SCALE
are such that in the float64 greedy run ALONE every step's margin between the best and the second candidate exceeds
1.5e-3, the project's measured score noise (README), for every utterance (found on the CPU: python
tests/test_stateless_search_gpu.py; asserted on the reference below)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stateless_common as SC  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, SCALE = 4, 3.0
X_LEN = [9, 8, 7]
MARGIN = 1.5e-3


def tiny(device, seed=SEED, scale=SCALE):
    """-> (the model in float32 on `device`, x (3, 9, 8), x_len)."""
    from pika_amd.model import transducer
    torch.manual_seed(seed)
    net = transducer.Net(SC.tiny_opt(), 8, 12).eval()
    with torch.no_grad():
        net.fc2.weight.mul_(scale)                  # wider logits: decisions well apart
        net.decoder.embedding.weight.mul_(scale)
    x = torch.randn(3, max(X_LEN), 8)
    return net.to(device), x.to(device), torch.tensor(X_LEN)


def greedy_float64(seed=SEED, scale=SCALE):
    """The modified greedy search of the definition in float64 on the CPU, from the model's weights
    -> (tokens per utterance, the least margin between the best and the second candidate over all steps)."""
    net, x, x_len = tiny("cpu", seed, scale)
    net = net.double()
    with torch.no_grad():
        enc = net.encode(x.double(), x_len).numpy()
    p = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    E, w = p["decoder.embedding.weight"], p["decoder.conv.weight"]
    ctx = w.shape[2]
    out, least = [], np.inf
    for b, n in enumerate(X_LEN):
        hyp = []
        for t in range(n):
            c = np.array([SC.context_of(hyp, ctx)])
            pred = np.maximum(SC.forward(c, E, w)[0][0, -1], 0.0)
            both = np.concatenate((enc[b, t], pred))
            h = np.tanh(p["fc1.weight"] @ both + p["fc1.bias"]) * (1.0 / (1.0 + np.exp(-(p["fc_gate.weight"] @ both
                                                                                        + p["fc_gate.bias"]))))
            logits = p["fc2.weight"] @ h + p["fc2.bias"]
            order = np.argsort(-logits, kind="stable")
            least = min(least, float(logits[order[0]] - logits[order[1]]))        # (log_softmax shifts both alike)
            if order[0] != 0:
                hyp.append(int(order[0]))
        out.append(hyp)
    return out, least


@functools.lru_cache(maxsize=None)
def model(dev):
    return tiny(dev)


def same(a, b, n):
    return all(torch.equal(p, q) for p, q in zip(a[:n], b[:n]))


@pytest.mark.parametrize("beam", [1, 3, 4])
def test_graph_and_eager_give_the_same_bits(hip_device, beam):
    from pika_amd import modified_beam_search
    net, x, x_len = model(hip_device)
    runs = [modified_beam_search(net, x, x_len, beam=beam, nbest=beam, use_graph=g) for g in (True, False)]
    assert same(runs[0], runs[1], 3)
    assert int((runs[0][1][:, 0] > 0).sum()) >= 2               # labels were emitted: the context was followed


def test_beam_one_is_the_float64_greedy_search(hip_device):
    from pika_amd import modified_beam_search
    want, least = greedy_float64()
    assert least > MARGIN, least                                # on the reference alone; no utterance left out
    assert all(len(h) >= 2 for h in want)                       # the context is full, and shifted, in every utterance
    net, x, x_len = model(hip_device)
    for g in (True, False):
        tokens, lengths, _, _ = modified_beam_search(net, x, x_len, beam=1, use_graph=g, precision="fp32")
        got = [tokens[b, 0, :int(lengths[b, 0])].tolist() for b in range(3)]
        assert got == want, (g, got, want)


def test_the_other_drivers_at_zero_weights_are_the_plain_search(hip_device):
    from pika_amd import (CtcHotwords, LstmLm, modified_beam_search, modified_beam_search_lm, modified_beam_search_nnlm,
                          modified_beam_search_timed)
    dev, K = hip_device, 4
    net, x, x_len = model(dev)
    V = net.output_dim
    t0, l0, s0, _ = modified_beam_search(net, x, x_len, beam=K, nbest=K, precision="fp32")
    hot = CtcHotwords([[3, 4], [5]], V, 1.0, 0, dev)            # reaches every class from its root
    t1, l1, s1, a1, _ = modified_beam_search_lm(net, x, x_len, hot, beam=K, nbest=K, precision="fp32", lm_weight=0.0,
                                                length_bonus=0.0, candidates=K, use_final=False)
    assert torch.equal(t0, t1) and torch.equal(l0, l1) and torch.equal(s0, s1) and torch.equal(s1, a1)
    torch.manual_seed(11)
    nnlm = LstmLm(V, 8, 16).eval().to(dev)
    t2, l2, s2, a2, _ = modified_beam_search_nnlm(net, x, x_len, nnlm, beam=K, nbest=K, precision="fp32", nn_weight=0.0,
                                                  lm=None, length_bonus=0.0, candidates=K)
    assert torch.equal(t0, t2) and torch.equal(l0, l2) and torch.equal(s0, a2) and torch.equal(s2, a2)
    # with a weight the LM moves scores: the stateless model really runs beside it
    s3 = modified_beam_search_nnlm(net, x, x_len, nnlm, beam=K, nbest=K, precision="fp32", nn_weight=0.5)[2]
    assert not torch.equal(s3, s0)
    t4, l4, s4, times, _ = modified_beam_search_timed(net, x, x_len, beam=K, nbest=K, precision="fp32")
    assert torch.equal(t0, t4) and torch.equal(l0, l4) and torch.equal(s0, s4)
    times, l4 = times.cpu().numpy(), l4.cpu().numpy()
    for b in range(3):
        for j in range(K):
            if l4[b, j] >= 0:
                row = times[b, j, :l4[b, j]]
                assert (np.diff(row) > 0).all() and (row >= 0).all() and (row < X_LEN[b]).all(), (b, j)


def test_stream_decoder_on_the_stateless_model(hip_device):
    from pika_amd import ModifiedStreamDecoder, modified_beam_search
    dev, K = hip_device, 4
    net, x, x_len = model(dev)
    tokens, lengths, scores, enc = modified_beam_search(net, x, x_len, beam=K, nbest=K, use_graph=False, precision="fp32")
    tokens, lengths = tokens.cpu().numpy(), lengths.cpu().numpy()
    B, T = enc.shape[:2]
    xl = x_len.to(dev)
    ctx = net.decoder.context_size
    for chunk in (1, 3, T):
        dec = ModifiedStreamDecoder(net, B, 16, beam=K, precision="fp32")
        for start in range(0, T, chunk):
            piece = enc[:, start:start + chunk]
            dec.advance(piece, (xl - start).clamp(0, piece.shape[1]))
            dec.commit()                                                    # exact commits after every chunk
        assert not dec.stream.overflowed.any() and torch.equal(dec.stream.consumed.long(), xl)
        ctok, clen, ttok, tlen, tsc = dec.results(nbest=K)
        assert torch.equal(tsc, scores), chunk                              # no rebase: the one-shot scores, bit for bit
        ctok, clen, ttok, tlen = (t.cpu().numpy() for t in (ctok, clen, ttok, tlen))
        for b in range(B):
            for j in range(K):
                assert (tlen[b, j] >= 0) == (lengths[b, j] >= 0)
                if lengths[b, j] >= 0:
                    got = list(ctok[b, :clen[b]]) + list(ttok[b, j, :tlen[b, j]])
                    assert got == list(tokens[b, j, :lengths[b, j]]), (chunk, b, j)
        dec.reset(which=[True] + [False] * (B - 1))                         # the selected stream starts over
        tok = dec._context.tokens.cpu().numpy()
        assert (tok[0] == np.array(SC.context_of([], ctx))).all()
        assert dec.stream.consumed.tolist() == [0] + X_LEN[1:]
    # forced commits drop slots and re-order the rest: every live slot's context is still the end of its text
    dec = ModifiedStreamDecoder(net, B, 16, beam=K, precision="fp32")
    moved = 0
    for start in range(0, T, 3):
        piece = enc[:, start:start + 3]
        dec.advance(piece, (xl - start).clamp(0, piece.shape[1]))
        slot_map = dec.commit(max_tail=1)[2]
        moved += int((slot_map != torch.arange(K, device=dev)).sum())
        hyp, ln = (t.cpu().numpy() for t in dec.stream.hyps())
        live = (dec.stream.scores > -float("inf")).cpu().numpy()
        tok = dec._context.tokens.cpu().numpy()
        for b in range(B):
            for j in range(K):
                if live[b, j]:
                    text = dec._text[b] + list(hyp[b, j, :ln[b, j]])
                    assert list(tok[b, j]) == SC.context_of(text, ctx), (start, b, j)
        want = net.decoder(dec._context.tokens.view(B * K, ctx).long())[:, -1, :]
        assert torch.equal(dec._context.rows, want)
    assert moved > 0                                                        # the case is one: a commit re-ordered slots


if __name__ == "__main__":      # the seed and the scale, found on the CPU
    for seed in range(6):
        for scale in (1.0, 2.0, 3.0, 4.0):
            hyps, least = greedy_float64(seed, scale)
            print(seed, scale, "%.5f" % least, hyps)
