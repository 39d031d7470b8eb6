"""inf-norm clipping + Nesterov SGD of the training scripts
(train_transducer_bmuf_otfaug.py:105-110) as three multi-tensor HIP launches (pika_amd/optim.py) against the stock
torch calls on the same tensors: identical parameters, momentum buffers, gradients and returned norm over several
steps, for whole tensors and for views of one flat vector at odd offsets (how parameters live under BMUF)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_common as Y  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 240), (1024,), (7,), (3, 5, 11), (4096, 1024), (1,), (513,)]


def _views(flat, shapes, off, wrap=torch.nn.Parameter):
    out = []
    for s in shapes:
        k = int(np.prod(s))
        out.append(wrap(flat[off:off + k].view(s)))
        off += k
    return out


def _params(dev, flat_views):
    g = torch.Generator().manual_seed(12)
    if flat_views:
        n = sum(int(np.prod(s)) for s in SHAPES) + 3
        flat = torch.randn(n, generator=g).to(dev)
        return _views(flat, SHAPES, 3)            # start 12 bytes off 16-byte alignment
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in SHAPES]


def _np(t):
    return t.detach().cpu().numpy().reshape(-1).copy()


@pytest.mark.parametrize("flat_views", [False, True, "grads_too"])
@pytest.mark.parametrize("grad_scale", [0.01, 40.0])          # below / above the clip threshold of 3.0
def test_fused_clip_and_nesterov_sgd_equal_torch(hip_device, flat_views, grad_scale):
    """Against torch within the tolerances below and against the float32 yardstick exactly.  flat_views: BOTH sides are
    views of a flat vector of their own that starts 12 bytes off 16-byte alignment; "grads_too": the gradients of the
    kernels' side are views of another flat vector, 4 bytes off."""
    from pika_amd import optim as O
    ref = _params(hip_device, flat_views)
    if flat_views:
        flat = torch.empty(sum(p.numel() for p in ref) + 3, device=hip_device)
        ours = _views(flat, SHAPES, 3)
        with torch.no_grad():
            for a, b in zip(ref, ours):
                b.copy_(a)
        assert ours[0].data_ptr() % 16 == 12 and ref[0].data_ptr() % 16 == 12
        assert sum(p.data_ptr() % 16 != 0 for p in ours) >= 5        # (7,), (165,), (1,) move the offset on
    else:
        ours = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    o_ref = O._TorchSGD(ref, 0.003, momentum=0.9, nesterov=True)
    o_our = O.SGD(ours, 0.003, momentum=0.9, nesterov=True)
    yp, yb = [_np(p) for p in ours], [None] * len(ours)
    g = torch.Generator().manual_seed(3)

    def fresh_gradients():
        grads = [(torch.randn(a.shape, generator=g) * grad_scale).to(hip_device) for a in ref]
        if flat_views == "grads_too":
            gflat = torch.empty(sum(p.numel() for p in ref) + 1, device=hip_device)
            mine = _views(gflat, SHAPES, 1, wrap=lambda t: t)
            for a, b in zip(grads, mine):
                b.copy_(a)
            assert mine[0].data_ptr() % 16 == 4
        else:
            mine = [gr.clone() for gr in grads]
        for a, b, gr, m in zip(ref, ours, grads, mine):
            a.grad, b.grad = gr, m
        return [_np(gr) for gr in grads]

    for step in range(4):
        yg = fresh_gradients()
        n_ref = O._torch_clip(ref, 3.0, norm_type=float("inf"))
        n_our = O.clip_grad_norm_(ours, 3.0, norm_type=float("inf"))
        assert torch.equal(n_ref, n_our)
        y_norm, yg = Y.clip(yg, 3.0)
        assert Y.same_bits(_np(n_our)[0], y_norm)
        for i, (a, b) in enumerate(zip(ref, ours)):
            assert torch.allclose(a.grad, b.grad, rtol=2e-7, atol=0), step      # x * clamp(c, max=1) vs x * c
            assert Y.same(_np(b.grad), yg[i]), (step, i)
        o_ref.step()
        o_our.step()
        for i, (a, b) in enumerate(zip(ref, ours)):
            assert torch.allclose(a, b, rtol=0, atol=1e-7 * float(a.abs().max())), step
            mb = o_ref.state[a]["momentum_buffer"]
            assert torch.allclose(mb, o_our.state[b]["momentum_buffer"], rtol=0, atol=3e-7 * float(mb.abs().max()))
            yp[i], yb[i] = Y.nesterov(yp[i], yg[i], yb[i], 0.003, 0.9, step == 0)
            assert Y.same(_np(b), yp[i]) and Y.same(_np(o_our.state[b]["momentum_buffer"]), yb[i]), (step, i)
    # a rebuilt optimizer starts without momentum again (the scripts rebuild it after every BMUF sync, :121-123)
    o_our2 = O.SGD(ours, 0.003, momentum=0.9, nesterov=True)
    o_ref2 = O._TorchSGD(ref, 0.003, momentum=0.9, nesterov=True)
    yg = fresh_gradients()      # fresh gradients: torch's multi-tensor Nesterov step leaves g + momentum*buf in .grad
    o_our2.step()
    o_ref2.step()
    for i, (a, b) in enumerate(zip(ref, ours)):
        assert torch.allclose(a, b, rtol=0, atol=2e-7 * float(a.abs().max()))
        assert Y.same(_np(b), Y.nesterov(yp[i], yg[i], None, 0.003, 0.9, True)[0]), i
    if flat_views:
        assert ours[0].data_ptr() == flat.data_ptr() + 12        # still the views the test started with


SMALL = [(33, 7), (5,), (16385,)]


def _small(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev)) for s in SMALL]


def _grads(dev, g, scale=1.0):
    return [(torch.randn(*s, generator=g) * scale).to(dev) for s in SMALL]


@pytest.mark.parametrize("missing", [1, 0])
def test_first_step_is_per_parameter_after_a_step_with_a_missing_gradient(hip_device, missing):
    """(a) a step in which one parameter has no gradient (the stock step: buffers for the others only), (b) a step with
    all gradients.  "First" is per parameter, as in torch: in (b) the parameter that had no gradient starts its
    buffer (b = g) and the others continue theirs.  Deciding it from parameter 0 alone raised KeyError for missing = 1
    and silently dropped the momentum of parameters 1 and 2 for missing = 0."""
    from pika_amd import optim as O
    ours = _small(hip_device, 5)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    o_our = O.SGD(ours, 0.003, momentum=0.9, nesterov=True)
    o_ref = O._TorchSGD(ref, 0.003, momentum=0.9, nesterov=True)
    g = torch.Generator().manual_seed(6)
    for a, b, gr in zip(ref, ours, _grads(hip_device, g)):            # (a)
        a.grad, b.grad = gr.clone(), gr.clone()
    ref[missing].grad = ours[missing].grad = None
    o_ref.step()
    o_our.step()
    assert "momentum_buffer" not in o_our.state[ours[missing]]
    yp = [_np(p) for p in ours]                                       # (a) was torch's step: the yardstick starts here
    yb = [_np(o_our.state[p]["momentum_buffer"]) if i != missing else None for i, p in enumerate(ours)]
    grads = _grads(hip_device, g)                                     # (b)
    for a, b, gr in zip(ref, ours, grads):
        a.grad, b.grad = gr.clone(), gr.clone()
    o_ref.step()
    o_our.step()
    for i, (a, b) in enumerate(zip(ref, ours)):
        mb, ob = o_ref.state[a]["momentum_buffer"], o_our.state[b]["momentum_buffer"]
        assert torch.allclose(a, b, rtol=0, atol=1e-7 * float(a.abs().max())), i
        assert torch.allclose(mb, ob, rtol=0, atol=3e-7 * float(mb.abs().max())), i
        want_p, want_b = Y.nesterov(yp[i], _np(grads[i]), yb[i], 0.003, 0.9, i == missing)
        assert Y.same(_np(b), want_p) and Y.same(_np(ob), want_b), i
        assert ob.shape == b.shape


def test_state_dict_round_trip_continues_the_run_exactly(hip_device):
    from pika_amd import optim as O
    run = _small(hip_device, 7)
    o_run = O.SGD(run, 0.003, momentum=0.9, nesterov=True)
    g = torch.Generator().manual_seed(8)
    for _ in range(2):
        for p, gr in zip(run, _grads(hip_device, g)):
            p.grad = gr
        o_run.step()
    again = [torch.nn.Parameter(p.detach().clone()) for p in run]
    o_again = O.SGD(again, 0.5, momentum=0.1, nesterov=True)
    o_again.load_state_dict(copy.deepcopy(o_run.state_dict()))
    assert o_again.param_groups[0]["lr"] == 0.003 and o_again.param_groups[0]["momentum"] == 0.9
    for _ in range(2):
        for p, q, gr in zip(run, again, _grads(hip_device, g)):
            p.grad, q.grad = gr, gr.clone()
        o_run.step()
        o_again.step()
    for p, q in zip(run, again):
        assert torch.equal(p, q)
        assert torch.equal(o_run.state[p]["momentum_buffer"], o_again.state[q]["momentum_buffer"])


def test_pointer_table_ring_survives_a_host_that_runs_ahead(hip_device):
    """Two parameter sets of identical shapes share one `_Tables` entry, so every call uploads its pointer rows anew.
    20 alternating steps (more than RING = 8) on freshly allocated gradients, with nothing in the loop that makes the
    host wait for the device: a staging row rewritten before its copy ran would send a step to the other set's
    tensors."""
    from pika_amd import optim as O
    steps, scale = 20, 2.0
    sets = [_small(hip_device, 9), _small(hip_device, 10)]
    assert O._tables(sets[0]) is O._tables(sets[1]) and steps > O._Tables.RING
    opts = [O.SGD(s, 0.003, momentum=0.9, nesterov=True) for s in sets]
    yp = [[_np(p) for p in s] for s in sets]
    yb = [[None] * len(SMALL) for _ in sets]
    g = torch.Generator().manual_seed(11)
    host = [[[torch.randn(*s, generator=g) * scale for s in SMALL] for _ in sets] for _ in range(steps)]
    staged = [[[t.to(hip_device) for t in per_set] for per_set in per_step] for per_step in host]
    torch.cuda.synchronize()
    for step in range(steps):
        for k, s in enumerate(sets):
            for p, gr in zip(s, staged[step][k]):
                p.grad = gr.clone()                         # a fresh allocation, no host wait
            O.clip_grad_norm_(s, 3.0, norm_type=float("inf"))
            opts[k].step()
    torch.cuda.synchronize()
    for step in range(steps):
        for k in range(2):
            _, yg = Y.clip([t.numpy().reshape(-1) for t in host[step][k]], 3.0)
            for i in range(len(SMALL)):
                yp[k][i], yb[k][i] = Y.nesterov(yp[k][i], yg[i], yb[k][i], 0.003, 0.9, step == 0)
    for k, s in enumerate(sets):
        for i, p in enumerate(s):
            assert Y.same(_np(p), yp[k][i]) and Y.same(_np(opts[k].state[p]["momentum_buffer"]), yb[k][i]), (k, i)


def test_install_routes_the_script_calls_and_leaves_the_rest_to_torch(hip_device):
    from pika_amd import optim as O
    O.install()
    try:
        p = [torch.nn.Parameter(torch.randn(300, 7, device=hip_device))]
        p[0].grad = torch.randn(300, 7, device=hip_device) * 10
        ref = float(p[0].grad.abs().max())
        n = torch.nn.utils.clip_grad_norm_(p, 3.0, norm_type=float("inf"))
        assert abs(float(n) - ref) < 1e-6 and abs(float(p[0].grad.abs().max()) - 3.0) < 1e-4
        assert isinstance(torch.optim.SGD(p, 0.1, momentum=0.9, nesterov=True), O._TorchSGD)
        # other norm types / CPU tensors / plain SGD: stock implementations
        n2 = torch.nn.utils.clip_grad_norm_(p, 1.0)                      # 2-norm
        assert abs(float(p[0].grad.norm()) - 1.0) < 1e-4 and float(n2) > 1.0
        q = [torch.nn.Parameter(torch.randn(5))]
        q[0].grad = torch.ones(5)
        before = q[0].detach().clone()
        torch.optim.SGD(q, 0.5).step()
        assert torch.allclose(q[0], before - 0.5)
        nan = [torch.nn.Parameter(torch.zeros(4, device=hip_device))]
        nan[0].grad = torch.tensor([1.0, float("nan"), 2.0, 3.0], device=hip_device)
        assert torch.isnan(torch.nn.utils.clip_grad_norm_(nan, 3.0, norm_type=float("inf")))
    finally:
        O.uninstall()
