"""The stateless prediction network without a GPU: the module's torch path against the float64 numpy definition
(tests/stateless_common.py), its gradient, padding, parameter names, `StatelessContext` on a hand-written script, `Net`
with decoder_type='stateless', and the C entry points' refusals."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stateless_common as SC  # noqa: E402


def make_net(V, D, ctx, cpg, seed=0, dtype=torch.float64):
    from pika_amd import StatelessPredNet
    net = StatelessPredNet(V, D, ctx, groups=D // cpg)
    E, w = SC.weights(V, D, cpg, ctx, seed)
    with torch.no_grad():
        net.embedding.weight.copy_(torch.from_numpy(E))
        net.conv.weight.copy_(torch.from_numpy(w))
    return net.to(dtype), E, w


@pytest.mark.parametrize("ctx", [1, 2, 3])
@pytest.mark.parametrize("cpg", [1, 4, 8])          # D = 8: depthwise, icefall's four, a single group
def test_torch_path_equals_the_numpy_definition(ctx, cpg):
    V, D = 9, 8
    net, E, w = make_net(V, D, ctx, cpg, seed=ctx * 10 + cpg)
    y = SC.labels(3, 5, V, seed=ctx)
    z, _ = SC.forward(y, E, w)
    got = net(torch.from_numpy(y)).detach().numpy()
    assert got.shape == (3, 5, D) and got.dtype == np.float64
    assert np.abs(got - np.maximum(z, 0.0)).max() <= 1e-12
    # and the backward of the definition, with the mask of this very forward
    rng = np.random.RandomState(5)
    dout = rng.standard_normal(z.shape)
    (d_E, _, _), (d_w, _, _) = SC.backward(y, E, w, dout * (z > 0))
    net.zero_grad()
    net(torch.from_numpy(y)).backward(torch.from_numpy(dout))
    assert np.abs(net.embedding.weight.grad.numpy() - d_E).max() <= 1e-12
    assert np.abs(net.conv.weight.grad.numpy() - d_w).max() <= 1e-12


def test_gradcheck_in_float64():
    from pika_amd.model.stateless import stateless_reference
    V, D, ctx, cpg = 6, 8, 2, 4
    E, w = SC.weights(V, D, cpg, ctx, 3)
    E = torch.from_numpy(E).double().requires_grad_(True)
    w = torch.from_numpy(w).double().requires_grad_(True)
    y = torch.from_numpy(SC.labels(3, 4, V, seed=1))
    assert (y < 0).any()
    assert torch.autograd.gradcheck(lambda E_, w_: stateless_reference(y, E_, w_), (E, w), eps=1e-6, atol=1e-6)


def test_negative_tokens_give_zero_rows_and_get_no_gradient():
    V, D = 7, 8
    net, E, w = make_net(V, D, 2, 4)
    y = torch.tensor([[-1, -1, 3], [0, -1, -1]])
    out = net(y)
    assert (out[0, :2] == 0).all() and (out[1, 2] == 0).all()
    # position (0, 2) sees [-1, 3]: only the last tap; equal to a row of one label behind padding
    alone = net(torch.tensor([[-1, 3]]))[0, 1]
    assert torch.equal(out[0, 2], alone)
    out.sum().backward()
    g = net.embedding.weight.grad
    seen = sorted(set(t for t in y.reshape(-1).tolist() if t >= 0))
    for v in range(V):
        assert bool((g[v] != 0).any()) == (v in seen), v
    # padding must not alias row 0 (a clamp without the mask would): the gradient of row 0 comes from (1, 0) alone
    only = net(torch.tensor([[0, -1, -1]]))
    net.zero_grad()
    only.sum().backward()
    assert torch.allclose(g[0], net.embedding.weight.grad[0], rtol=0, atol=1e-12)


def test_state_dict_keys_and_defaults():
    from pika_amd import StatelessPredNet
    net = StatelessPredNet(11, 16)
    assert list(net.state_dict()) == ["embedding.weight", "conv.weight"]
    assert net.embedding.padding_idx is None and net.conv.bias is None
    assert net.conv.groups == 4 and tuple(net.conv.weight.shape) == (16, 4, 2)
    other = StatelessPredNet(11, 16)
    other.load_state_dict(net.state_dict())
    y = torch.tensor([[0, 4, 10]])
    assert torch.equal(net(y), other(y))
    with pytest.raises(ValueError):
        StatelessPredNet(11, 10, groups=4)
    with pytest.raises(ValueError):
        net(torch.zeros(3, dtype=torch.int64))


def test_context_follows_a_script_on_the_cpu():
    from pika_amd import StatelessContext
    V, D, ctx, K = 9, 8, 3, 3
    net, E, w = make_net(V, D, ctx, 4)
    c = StatelessContext(net, 2, K)
    assert c.tokens.dtype == torch.int32 and tuple(c.rows.shape) == (2 * K, D)
    hyps = [[[] for _ in range(K)] for _ in range(2)]
    script = [
        # (parent, token): repeated parents, blanks, a parent with a higher index than the slot
        ([[0, 0, 0], [0, 0, 0]], [[3, 0, 4], [0, 5, 5]]),
        ([[2, 2, 1], [1, 0, 1]], [[0, 6, 7], [8, 0, 0]]),
        ([[1, 0, 2], [2, 2, 2]], [[1, 1, 0], [0, 2, 3]]),
        ([[5, -1, 1], [0, 1, 2]], [[0, 0, 2], [0, 0, 0]]),       # parents out of range are clamped
    ]

    def check():
        want = [[SC.context_of(h, ctx) for h in row] for row in hyps]
        assert c.tokens.tolist() == want
        flat = np.array(want).reshape(2 * K, ctx)
        z, _ = SC.forward(flat, E, w)
        assert np.abs(c.rows.numpy() - np.maximum(z[:, -1], 0.0)).max() <= 1e-12

    check()
    for parent, token in script:
        c.follow(torch.tensor(parent), torch.tensor(token))
        hyps = [[hyps[b][min(max(parent[b][j], 0), K - 1)] + ([token[b][j]] if token[b][j] != 0 else [])
                 for j in range(K)] for b in range(2)]
        check()
    c.reset(which=[False, True])
    hyps[1] = [[] for _ in range(K)]
    check()
    c.reorder(torch.tensor([[2, 2, 0], [0, 1, 2]]))
    hyps[0] = [hyps[0][2], hyps[0][2], hyps[0][0]]
    check()
    c.reset()
    hyps = [[[] for _ in range(K)] for _ in range(2)]
    check()
    with pytest.raises(ValueError):
        c.follow(torch.zeros(2, K, dtype=torch.int32), torch.zeros(2, K, dtype=torch.int64))


def test_net_with_the_stateless_decoder():
    from pika_amd.model import transducer
    from pika_amd import StatelessPredNet
    torch.manual_seed(3)
    net = transducer.Net(SC.tiny_opt(), 8, 12)
    assert isinstance(net.decoder, StatelessPredNet) and net.embed is net.decoder.embedding
    assert net.decoder.vocab_size == 13 and net.decoder.dim == 32 and net.decoder.context_size == 2
    assert net.decoder.groups == 8
    assert "decoder.embedding.weight" in net.state_dict() and "decoder.conv.weight" in net.state_dict()
    y = torch.tensor([[0, 5, 12, 1], [0, 0, 3, 3]])
    assert torch.equal(net.predict(y), net.decoder(y))
    z, _ = SC.forward(y.numpy(), net.decoder.embedding.weight.detach().numpy(), net.decoder.conv.weight.detach().numpy())
    assert np.abs(net.predict(y).detach().numpy() - np.maximum(z, 0)).max() < 1e-5
    out = net(torch.randn(2, 6, 8), y[:, 1:], x_len=torch.tensor([6, 6]), softmax=True)     # the whole forward
    assert tuple(out.shape) == (2, 6, 4, 12)
    wide = transducer.Net(SC.tiny_opt(context_size=3, decoder_groups=2), 8, 12)
    assert tuple(wide.decoder.conv.weight.shape) == (32, 16, 3)
    # the other two types are what they were
    assert isinstance(transducer.Net(SC.tiny_opt("rnn"), 8, 12).decoder, torch.nn.LSTM)


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from pika_amd import _lib
    lib = _lib.lib()
    EINVAL, ETOOBIG = -1, -2

    def fwd(B=1, U=1, V=5, D=8, cpg=4, ctx=2, ld=None, ldy=None):
        return lib.pika_stateless_forward(None, U if ldy is None else ldy, None, None, B, U, V, D, cpg, ctx, None,
                                          D if ld is None else ld, None)

    def bwd(B=1, U=1, V=5, D=8, cpg=4, ctx=2):
        return lib.pika_stateless_backward(None, U, None, None, None, None, None, D, None, D, B, U, V, D, cpg, ctx, None,
                                           None, None, None)

    def step(B=1, K=1, ctx=2, blank=0, V=5, D=8, cpg=4, ld=None):
        return lib.pika_stateless_step(None, None, None, B, K, ctx, blank, None, None, V, D, cpg, None,
                                       D if ld is None else ld, None)

    for call in (fwd, bwd, step):
        assert call() == EINVAL                                   # null pointers, dimensions fine
        assert call(ctx=9) == ETOOBIG and call(ctx=0) == EINVAL
        assert call(cpg=17, D=34) == ETOOBIG and call(cpg=0) == EINVAL
        assert call(D=10, cpg=4) == ETOOBIG                       # D % cpg != 0
        assert call(D=8196) == ETOOBIG and call(D=0) == EINVAL
        assert call(B=65536) == ETOOBIG and call(B=0) == EINVAL
        assert call(V=0) == EINVAL
    assert fwd(U=0) == EINVAL and bwd(U=0) == EINVAL
    assert fwd(B=65535, U=1 << 20) == ETOOBIG
    assert step(K=65) == ETOOBIG and step(K=0) == EINVAL
    # with real (host) pointers everywhere, a short row stride or a blank outside the vocabulary is still refused
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.pika_stateless_forward(p, 1, p, p, 1, 1, 5, 8, 4, 2, p, 7, None) == EINVAL          # ld < D
    assert lib.pika_stateless_forward(p, 0, p, p, 1, 1, 5, 8, 4, 2, p, 8, None) == EINVAL          # ldy < U
    assert lib.pika_stateless_step(p, p, p, 1, 1, 2, 0, p, p, 5, 8, 4, p, 7, None) == EINVAL
    assert lib.pika_stateless_step(p, p, p, 1, 1, 2, 5, p, p, 5, 8, 4, p, 8, None) == EINVAL       # blank >= V
    assert lib.pika_stateless_backward(p, 1, p, p, p, p, p, 7, p, 8, 1, 1, 5, 8, 4, 2, p, p, p, None) == EINVAL
    ws = lib.pika_stateless_backward_workspace_bytes
    assert ws(0, 1, 8, 4, 2) == 0 and ws(1, 1, 8, 4, 9) == 0 and ws(1, 1, 10, 4, 2) == 0 and ws(65536, 1, 8, 4, 2) == 0
    # go (B U D floats, rounded to 16 bytes) + one chunk sum of d_w per 32 rows
    assert ws(32, 51, 512, 4, 2) == 32 * 51 * 512 * 4 + 51 * 512 * 4 * 2 * 4
    assert ws(1, 1, 4, 4, 2) == 16 + 4 * 4 * 2 * 4
    assert ws(3, 5, 20, 4, 2) == 3 * 5 * 20 * 4 + 20 * 4 * 2 * 4


def test_symbols_beside_an_unchanged_abi_version():
    from pika_amd import _lib
    lib = _lib.lib()
    for name in ("pika_stateless_forward", "pika_stateless_backward_workspace_bytes", "pika_stateless_backward",
                 "pika_stateless_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.pika_amd_abi_version() == _lib.ABI_VERSION       # new symbols only: no signature changed


def test_stream_decoder_takes_the_stateless_model_and_no_other_new_one():
    from pika_amd import ModifiedStreamDecoder
    from pika_amd.model import transducer
    torch.manual_seed(0)
    net = transducer.Net(SC.tiny_opt(), 8, 12).double()
    dec = ModifiedStreamDecoder(net, 2, 8, beam=2, precision="fp32")
    assert dec._context is not None and dec.H == 32
    enc = torch.randn(2, 3, 32, dtype=torch.float64)
    dec.advance(enc)
    dec.commit()
    assert dec.stream.consumed.tolist() == [3, 3]
