"""The persistent LSTM recurrence of training (include/pika_lstm.h, pika_amd/model/lstm.py) against torch's nn.LSTM in fp32
on the same device: outputs, input gradient and every parameter gradient, at the prediction network's own shape
(reference trainer/model/transducer.py:55-61,93-96: B x (U + 1) labels, H = 1024, two layers) and at ragged shapes."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _nets(E, H, layers, seed, dropout=0.0):
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(E, H, layers, batch_first=True, dropout=dropout).cuda()
    return ref


def _run(ref, x, dy, persistent, mode):
    from pika_amd import gemm as G
    from pika_amd.model import lstm, transducer
    old, lstm.PERSISTENT, oldp = lstm.PERSISTENT, persistent, G.PRECISION
    G.PRECISION = mode
    try:
        ref.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        took = lstm.applies(ref, xi)
        out = transducer._lstm_forward(ref, xi)
        out.backward(dy)
        torch.cuda.synchronize()
        return took, out.detach(), xi.grad.detach(), {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    finally:
        lstm.PERSISTENT, G.PRECISION = old, oldp


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("B,S,E,H,layers", [(32, 51, 100, 1024, 2), (5, 7, 36, 256, 1), (19, 3, 64, 512, 3), (48, 1, 100, 768, 2)])
def test_recurrence_matches_torch_lstm(B, S, E, H, layers):
    from pika_amd.model import lstm
    ref = _nets(E, H, layers, seed=B + S)
    ref.train()
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B, S, E, device="cuda", generator=g)
    dy = torch.randn(B, S, H, device="cuda", generator=g)
    took, out, dx, grads = _run(ref, x, dy, True, "bf16x3")
    assert took, "the persistent recurrence did not take the call"
    assert lstm.status() == 0
    with torch.no_grad():
        want, _ = ref(x)
    xi = x.clone().requires_grad_(True)
    ref.zero_grad(set_to_none=True)
    o2, _ = ref(xi)
    o2.backward(dy)
    assert _rel(out, want) < 2e-4, _rel(out, want)
    assert _rel(dx, xi.grad) < 1e-3, _rel(dx, xi.grad)
    for n, p in ref.named_parameters():
        assert _rel(grads[n], p.grad) < 1e-3, (n, _rel(grads[n], p.grad))


def test_fp32_mode_keeps_the_library_recurrence():
    from pika_amd.model import lstm
    ref = _nets(100, 1024, 2, seed=3)
    x = torch.randn(4, 5, 100, device="cuda")
    took, out, _, _ = _run(ref, x, torch.ones(4, 5, 1024, device="cuda"), True, "fp32")
    assert not took
    with torch.no_grad():
        assert torch.equal(out, ref(x)[0])
    assert not lstm.applies(ref, x.double())


def test_oversized_batch_falls_back():
    from pika_amd import gemm as G
    from pika_amd.model import lstm
    ref = _nets(100, 1024, 1, seed=4)
    old = G.PRECISION
    G.PRECISION = "mixed"
    try:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        rows = 16 * (cus // 64) + 1                    # one row block more than fits
        assert not lstm.applies(ref, torch.zeros(rows, 2, 100, device="cuda"))
        assert lstm.applies(ref, torch.zeros(rows - 1, 2, 100, device="cuda"))
    finally:
        G.PRECISION = old


def test_c_abi_refuses_bad_arguments():
    from pika_amd import _lib
    lib = _lib.lib()
    assert lib.pika_lstm_train_packed_bytes(1000) == -1 and lib.pika_lstm_train_packed_bytes(2048) == -1
    assert lib.pika_lstm_train_packed_bytes(1024) == 2 * 4 * 1024 * 1024 * 4
    assert lib.pika_lstm_train_fwd_work_bytes(0, 4, 256) == -1 and lib.pika_lstm_train_bwd_work_bytes(4, 0, 256) == -1
    assert lib.pika_lstm_train_bwd_work_bytes(51, 32, 1024) == 256 + 4 * 51 * 2 * 64 * 64 * 256
    assert lib.pika_lstm_train_fwd(None, None, None, None, None, None, 0, 4, 4, 256, None) == -1
    assert lib.pika_lstm_train_bwd(None, None, None, None, None, None, 0, 1, 4, 4, 256, None) == -1


def test_forward_hooks_of_the_module_see_the_call():
    from pika_amd import gemm as G
    from pika_amd.model import transducer
    ref = _nets(100, 1024, 2, seed=5)
    seen = {}
    h = ref.register_forward_hook(lambda m, i, o: seen.update(out=o[0].detach(), h_n=o[1][0], c_n=o[1][1], x=i[0]))
    old = G.PRECISION
    G.PRECISION = "bf16x3"
    try:
        x = torch.randn(3, 6, 100, device="cuda")
        out = transducer._lstm_forward(ref, x)
    finally:
        G.PRECISION = old
        h.remove()
    with torch.no_grad():
        want, (h_n, c_n) = ref(x)
    assert seen["x"] is x and torch.equal(seen["out"], out.detach())
    assert _rel(seen["out"], want) < 2e-4 and _rel(seen["h_n"], h_n) < 2e-4 and _rel(seen["c_n"], c_n) < 2e-4


def test_graphed_backward_gives_summed_parameters_their_own_gradient_buffers():
    """b_ih + b_hh enters the model as a sum: autograd.grad hands both parameters ONE tensor; the captured backward must
    not (the clip scales gradients in place)."""
    from pika_amd import train_graph
    a = torch.ones(4, device="cuda")
    g = [a, None, a, a.clone()]
    out = train_graph.distinct_buffers(g)
    ptrs = [t.data_ptr() for t in out if t is not None]
    assert out[1] is None and len(set(ptrs)) == 3 and all(torch.equal(t, a) for t in out if t is not None)


def test_backward_scratch_is_left_as_a_memset_leaves_it():
    """`armed`: a completed backward launch resets every exchange word it read, over changing shapes too."""
    from pika_amd.model import lstm
    for B, S, H in ((32, 51, 1024), (7, 9, 256), (20, 4, 512)):
        ref = _nets(100, H, 2, seed=S)
        x = torch.randn(B, S, 100, device="cuda")
        _run(ref, x, torch.randn(B, S, H, device="cuda"), True, "bf16x3")
        w = lstm._WORK[(0, True)]
        assert lstm.status() == 0
        assert bool((w[256:] == 255).all()), (B, S, H)


def test_no_grad_forward_and_growing_shapes_keep_earlier_scratch_alive():
    """Evaluation (no autograd) takes the same launch; a larger shape later gets a larger scratch while the outgrown one
    stays allocated (a captured training step may hold its address)."""
    from pika_amd import gemm as G
    from pika_amd.model import lstm, transducer
    ref = _nets(100, 512, 2, seed=9).eval()
    old = G.PRECISION
    G.PRECISION = "mixed"
    try:
        with torch.no_grad():
            x = torch.randn(4, 6, 100, device="cuda")
            assert lstm.applies(ref, x)
            got = transducer._lstm_forward(ref, x)
            assert _rel(got, ref(x)[0]) < 2e-4
            first = lstm._WORK[(0, True)]
            big = torch.randn(33, 40, 100, device="cuda")
            got = transducer._lstm_forward(ref, big)
            assert _rel(got, ref(big)[0]) < 2e-4
        now = lstm._WORK[(0, True)]
        if now is not first:
            assert any(w is first for w in lstm._RETIRED) and now.numel() >= first.numel() + first.numel() // 2
        assert lstm.status() == 0
    finally:
        G.PRECISION = old


# ---------------------------------------------------------------------------------------------------------------------------
# Against nn.LSTM in float64 on the CPU, every width with recurrent steps, several row blocks and several layers, in every
# arithmetic `lstm.applies` admits.  Bounds relative to the tensor's maximum: the two-term arithmetics ("bf16x3", and "mixed",
# where the network is an island of it) inside the bounds of the fp32 comparison above; "bf16" (one-term gx and
# weight-gradient products) inside those tests/test_gemm_gpu.py and tests/test_model_full.py use for that arithmetic.
# Measured on an MI355X, worst over the shapes (dropout and the non-dense upstream gradients included):
#   bf16x3, mixed: output 4.5e-6, dx 1.0e-5, parameter gradients 7.8e-6;  bf16: output 3.1e-3, dx 3.7e-3, parameters 5.4e-3.

SHAPES = [(32, 51, 100, 1024, 2), (5, 7, 36, 256, 1), (19, 3, 64, 512, 3), (48, 1, 100, 768, 2),
          (33, 20, 100, 768, 2), (17, 51, 100, 512, 2), (40, 9, 36, 256, 3)]
BOUNDS = {"bf16x3": (2e-4, 1e-3), "mixed": (2e-4, 1e-3), "bf16": (2.0 ** -7, 3e-2)}          # mode: (output, gradients)


def _run_loss(ref, x, loss_fn, mode):
    """_run with a scalar loss of the output instead of an upstream gradient."""
    from pika_amd import gemm as G
    from pika_amd.model import lstm, transducer
    old, lstm.PERSISTENT, oldp = lstm.PERSISTENT, True, G.PRECISION
    G.PRECISION = mode
    try:
        ref.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        assert lstm.applies(ref, xi), "the persistent recurrence did not take the call"
        out = transducer._lstm_forward(ref, xi)
        loss_fn(out).backward()
        torch.cuda.synchronize()
        assert lstm.status() == 0
        return out.detach(), xi.grad.detach(), {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    finally:
        lstm.PERSISTENT, G.PRECISION = old, oldp


def _float64(ref, x, loss_fn, masks=(), p=0.0):
    """nn.LSTM in float64 on the CPU with the parameters of `ref`.  With dropout masks: the stack of its layers as one-layer
    nn.LSTMs, mask / (1 - p) between them."""
    import copy
    xi = x.detach().cpu().double().requires_grad_(True)
    if not masks:
        net = copy.deepcopy(ref).cpu().double()
        net.dropout = 0.0
        out = net(xi)[0]
        loss_fn(out).backward()
        return out.detach(), xi.grad, {n: q.grad for n, q in net.named_parameters()}
    layers, out = [], xi
    for l in range(ref.num_layers):
        one = torch.nn.LSTM(ref.input_size if l == 0 else ref.hidden_size, ref.hidden_size, 1, batch_first=True).double()
        with torch.no_grad():
            for n in ("weight_ih_l", "weight_hh_l", "bias_ih_l", "bias_hh_l"):
                getattr(one, n + "0").copy_(getattr(ref, n + str(l)).detach().cpu().double())
        layers.append(one)
        out = one(out)[0]
        if l + 1 < ref.num_layers:
            out = out * masks[l].cpu().double() / (1.0 - p)
    loss_fn(out).backward()
    grads = {n + str(l): getattr(one, n + "0").grad for l, one in enumerate(layers)
             for n in ("weight_ih_l", "weight_hh_l", "bias_ih_l", "bias_hh_l")}
    return out.detach(), xi.grad, grads


_F64 = {}


def _float64_once(key, ref, x, loss_fn):
    """The float64 reference of a case is the same for every arithmetic: computed once."""
    if key not in _F64:
        _F64[key] = _float64(ref, x, loss_fn)
    return _F64[key]


def _rel64(a, b):
    return _rel(a.detach().cpu().double(), b)


def _check64(tag, mode, got, want):
    t_out, t_grad = BOUNDS[mode]
    (out, dx, grads), (out64, dx64, grads64) = got, want
    e_out, e_dx = _rel64(out, out64), _rel64(dx, dx64)
    e_par = {n: _rel64(grads[n], grads64[n]) for n in grads64}
    worst = max(e_par, key=e_par.get)
    print("LSTM64 %s %s: out %.2e  dx %.2e  parameters %.2e (%s)" % (tag, mode, e_out, e_dx, e_par[worst], worst))
    assert set(grads) == set(grads64)
    assert e_out < t_out, (tag, mode, e_out)
    assert e_dx < t_grad, (tag, mode, e_dx)
    for n, e in e_par.items():
        assert e < t_grad, (tag, mode, n, e)


@pytest.mark.parametrize("mode", ["bf16x3", "mixed", "bf16"])
@pytest.mark.parametrize("B,S,E,H,layers", SHAPES)
def test_recurrence_matches_float64_lstm(B, S, E, H, layers, mode):
    ref = _nets(E, H, layers, seed=B + S).train()
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B, S, E, device="cuda", generator=g)
    dy = torch.randn(B, S, H, device="cuda", generator=g)
    loss = lambda o: (o * dy.to(o)).sum()       # noqa: E731
    tag = "B%d-S%d-H%d-L%d" % (B, S, H, layers)
    _check64(tag, mode, _run_loss(ref, x, loss, mode), _float64_once(tag, ref, x, loss))


@pytest.mark.parametrize("mode", ["bf16x3", "mixed"])
@pytest.mark.parametrize("B,S,E,H,layers", [(33, 20, 100, 768, 2), (17, 51, 100, 512, 2), (40, 9, 36, 256, 3)])
def test_upstream_gradients_that_are_not_dense_tensors(B, S, E, H, layers, mode):
    """out.sum(): the upstream gradient is a stride-0 expand; the last step alone: zero everywhere else."""
    ref = _nets(E, H, layers, seed=B + S + 1).train()
    x = torch.randn(B, S, E, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    for name, loss in (("sum", lambda o: o.sum()), ("last", lambda o: o[:, -1].square().sum())):
        tag = "B%d-S%d-H%d-L%d %s" % (B, S, H, layers, name)
        _check64(tag, mode, _run_loss(ref, x, loss, mode), _float64_once(tag, ref, x, loss))


def _record_dropout(monkeypatch):
    masks, real = [], torch.nn.functional.dropout

    def recording(inp, p=0.5, training=True, inplace=False):
        y = real(inp, p, training, inplace)
        seen = (y.detach() != 0) | (inp.detach() == 0)
        # the mask autograd kept, where there is one: an input that is exactly 0 (the fast tanh gives one now and then)
        # does not show in the values whether it was dropped, and the backward knows
        kept = getattr(y.grad_fn, "_saved_result1", None)
        if kept is not None:
            kept = kept.bool()
            assert torch.equal(kept | (inp.detach() == 0), seen)
        masks.append(seen if kept is None else kept)
        return y
    monkeypatch.setattr(torch.nn.functional, "dropout", recording)
    return masks


@pytest.mark.parametrize("mode", ["bf16x3", "mixed"])
@pytest.mark.parametrize("B,S,E,H,layers", [(33, 20, 100, 768, 2), (17, 51, 100, 512, 3), (40, 9, 36, 256, 3)])
def test_dropout_between_the_layers(monkeypatch, B, S, E, H, layers, mode):
    """The masks the path drew, recorded, make the float64 reference: one-layer nn.LSTMs with mask / (1 - p) between them."""
    p = 0.3
    ref = _nets(E, H, layers, seed=B + S + 2, dropout=p).train()
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(B, S, E, device="cuda", generator=g)
    dy = torch.randn(B, S, H, device="cuda", generator=g)
    loss = lambda o: (o * dy.to(o)).sum()       # noqa: E731
    masks = _record_dropout(monkeypatch)
    got = _run_loss(ref, x, loss, mode)
    first = list(masks)
    assert len(first) == layers - 1 and all(m.shape == (B, S, H) for m in first)
    _check64("B%d-S%d-H%d-L%d dropout" % (B, S, H, layers), mode, got, _float64(ref, x, loss, first, p))
    n = B * S * H
    for m in first:
        kept = float(m.sum()) / n
        assert abs(kept - (1 - p)) <= 4 * (p * (1 - p) / n) ** 0.5, kept
    del masks[:]
    _run_loss(ref, x, loss, mode)
    assert len(masks) == layers - 1 and not any(torch.equal(a, b) for a, b in zip(first, masks)), "the same masks twice"


def test_eval_draws_no_dropout_mask(monkeypatch):
    B, S, E, H, layers = 20, 6, 36, 512, 3
    with_p, without = _nets(E, H, layers, seed=6, dropout=0.3).eval(), _nets(E, H, layers, seed=6).train()
    assert all(torch.equal(a, b) for a, b in zip(with_p.parameters(), without.parameters()))
    x = torch.randn(B, S, E, device="cuda")
    masks = _record_dropout(monkeypatch)
    got = _run_loss(with_p, x, lambda o: o.sum(), "bf16x3")
    want = _run_loss(without, x, lambda o: o.sum(), "bf16x3")
    assert not masks
    assert torch.equal(got[0], want[0])
    assert _rel(got[1], want[1]) < 1e-3          # (the input-gradient product is not the same bits from run to run)
