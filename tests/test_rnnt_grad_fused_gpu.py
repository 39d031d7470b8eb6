"""pika_rgrad_backward_fe over a tensor that holds an earlier gradient: ONE launch (rnnt_grad_rowmeta_update_kernel) computes
the row metadata, stores it and updates the tensor in place.

Yardstick: the two-call route on identical inputs -- pika_rnnt_loss_backward_fe(grads = NULL), which is
rnnt_rowmeta_kernel, then pika_rgrad_dense_grads_update, which is rnnt_grad_update_kernel -- on a clone of the same
previous gradient tensor, the same previous cols and a clone of the same forward workspace.  Both routes evaluate the same
function, so the comparison is bit for bit: the whole gradient tensor as int32 (-0.0f is not +0.0f), cols_out, and every
byte of the workspace.

A case is a chain of backward calls on one tensor: a streaming call (prev_cols = NULL), then fused updates whose previous
state is itself a product of the fused route.  One chain is also compared with the fp64 oracle at the tolerance of
tests/test_rnnt_grad_reuse_gpu.py for the same quantity (|err| <= 1e-4 |g| + 1e-5).
"""
import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import make_case

pytestmark = pytest.mark.gpu

PIKA_EINVAL = -1


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Step(object):
    """One call's inputs.  (B, T, U) as helpers.make_case takes them (U1 = U + 1); gc: None, or one factor per utterance."""

    def __init__(self, B, T, U, V, seed, ragged=True, blank=0, lam=0.0, gc=None, labels=None, label_is_blank=False):
        self.B, self.T, self.U1, self.V, self.blank, self.lam = B, T, U + 1, V, blank, lam
        self.lp, self.y, self.tl, self.ul = make_case(B, T, U, V, seed, ragged=ragged, blank=blank)
        if labels is not None:       # another step's labels and lengths: new entries land on old ones
            self.y, self.tl, self.ul = labels.y, labels.tl, labels.ul
        if label_is_blank:
            self.y[0, 0] = blank     # utterance 0 is full size: its first label column IS the blank column
        self.gc = None if gc is None else np.resize(np.asarray(gc, np.float32), B)
        self.rows = B * T * self.U1


def _forward(lib, dev, st):
    """The step's device arguments and its workspace after the forward."""
    lp, y, tl, ul, gc = (_dev(a, dev) for a in (st.lp, st.y if st.U1 > 1 else None, st.tl, st.ul, st.gc))
    ws = torch.empty(lib.pika_rnnt_workspace_bytes(st.B, st.T, st.U1), dtype=torch.uint8, device=dev)
    costs = torch.empty(st.B, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pika_rnnt_loss_forward(_ptr(lp), _ptr(y), _ptr(tl), _ptr(ul), st.B, st.T, st.U1, st.V, st.blank, _ptr(costs),
                                      _ptr(ws), stream) == 0
    return (y, tl, ul, gc), ws, stream


def _fused(lib, st, args, ws, grads, prev, cols_out, stream):
    y, tl, ul, gc = args
    return lib.pika_rgrad_backward_fe(_ptr(y), _ptr(tl), _ptr(ul), st.B, st.T, st.U1, st.V, st.blank, _ptr(gc), _ptr(ws),
                                      _ptr(grads), st.lam, _ptr(prev[0]), prev[1], prev[2], _ptr(cols_out), stream)


def _two_calls(lib, st, args, ws, grads, prev, cols_out, stream):
    y, tl, ul, gc = args
    assert lib.pika_rnnt_loss_backward_fe(_ptr(y), _ptr(tl), _ptr(ul), st.B, st.T, st.U1, st.V, st.blank, _ptr(gc), _ptr(ws),
                                          None, st.lam, stream) == 0
    return lib.pika_rgrad_dense_grads_update(_ptr(ws), st.B, st.T, st.U1, st.V, st.blank, _ptr(grads), _ptr(prev[0]),
                                             prev[1], prev[2], _ptr(cols_out), stream)


def _chain(dev, steps):
    """Run the steps on one tensor; every fused update is compared with the two-call route.  Returns the gradient of
    every step (numpy, the step's rows) and the whole tensor's words after it."""
    from pika_amd import _lib
    lib = _lib.lib()
    V = steps[0].V
    cap = max(st.rows for st in steps)
    grads = torch.zeros(cap * V, dtype=torch.float32, device=dev)
    cols = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    prev, outs = (None, 0, 0), []
    for i, st in enumerate(steps):
        assert st.V == V
        args, ws, stream = _forward(lib, dev, st)
        if i == 0:      # the streaming writer and the cols kernel: nothing known about the tensor
            assert _fused(lib, st, args, ws, grads, prev, cols, stream) == 0
        else:
            ws2, grads2, cols2 = ws.clone(), grads.clone(), cols.clone()
            assert _fused(lib, st, args, ws, grads, prev, cols, stream) == 0
            assert _two_calls(lib, st, args, ws2, grads2, (cols2, prev[1], prev[2]), cols2, stream) == 0
            torch.cuda.synchronize()
            g, g2 = grads.view(torch.int32), grads2.view(torch.int32)
            assert torch.equal(g, g2), "step %d: %d words differ" % (i, int((g != g2).sum()))
            assert torch.equal(cols[:st.rows], cols2[:st.rows]), "step %d: cols_out" % i
            assert torch.equal(ws, ws2), "step %d: workspace" % i
            assert not g[st.rows * V:].any(), "step %d: rows beyond the call's are not +0.0f" % i
        prev = (cols, st.rows, st.blank)
        outs.append((grads[:st.rows * V].view(st.B, st.T, st.U1, V).cpu().numpy(), grads.view(torch.int32).cpu().numpy()))
    return outs


def test_no_labels(hip_device):
    """U1 = 1: labels = NULL, every row has its blank entry alone."""
    _chain(hip_device, [_Step(2, 1, 0, 5, 11, ragged=False), _Step(2, 1, 0, 5, 12, ragged=False, gc=[0.5, -2.0]),
                        _Step(2, 1, 0, 5, 13, ragged=False, lam=0.5)])


@pytest.mark.parametrize("V", [5, 8])
def test_ragged_lengths_fastemit_and_grad_costs_against_the_oracle(hip_device, V):
    """B=3, T=5, U1=4, one odd V and one divisible by 4; ragged lengths with T_n = 1, U_n = 0 (helpers.make_case puts it
    second) and labels padded with V; FastEmit 0.5; grad_costs NULL and non-unit."""
    steps = [_Step(3, 5, 3, V, 21, ragged=False), _Step(3, 5, 3, V, 22, lam=0.5, gc=[0.25, 3.0, -1.5]),
             _Step(3, 5, 3, V, 23, lam=0.5)]
    outs = _chain(hip_device, steps)
    for st, (g, _) in zip(steps[1:], outs[1:]):
        _, g64 = O.rnnt_loss(st.lp, st.y, st.tl, st.ul, blank=st.blank)
        for n in range(st.B):
            if st.ul[n]:
                u = np.arange(st.ul[n])
                g64[n, :st.tl[n], u, st.y[n, u]] *= 1.0 + st.lam
        if st.gc is not None:
            g64 = g64 * st.gc.astype(np.float64)[:, None, None, None]
        err = np.abs(g - g64)
        assert not (err > 1e-4 * np.abs(g64) + 1e-5).any(), "max abs err %g" % float(err.max())


def test_lattice_width_128(hip_device):
    """U1 = 66: two waves of columns."""
    _chain(hip_device, [_Step(2, 7, 65, 12, 31, ragged=False), _Step(2, 7, 65, 12, 32, gc=[2.0, 0.5]),
                        _Step(2, 7, 65, 12, 33, lam=0.5)])


def test_fewer_rows_then_more_rows(hip_device):
    """prev_rows > rows: the tail rows are cleared and stay zero; then prev_rows < rows inside the larger tensor."""
    outs = _chain(hip_device, [_Step(3, 5, 3, 8, 41, ragged=False), _Step(2, 4, 2, 8, 42), _Step(3, 5, 3, 8, 43),
                               _Step(1, 1, 0, 8, 44, ragged=False), _Step(3, 5, 3, 8, 45, gc=[1.0, 2.0, 3.0])])
    assert outs[0][1][2 * 4 * 3 * 8:].any()      # the first call did leave entries where the second has no rows


def test_another_blank_a_label_equal_to_blank_and_the_same_labels_again(hip_device):
    first = _Step(2, 5, 3, 8, 52, blank=3, label_is_blank=True)
    _chain(hip_device, [_Step(2, 5, 3, 8, 51, ragged=False), first, _Step(2, 5, 3, 8, 53, blank=5, label_is_blank=True),
                        _Step(2, 5, 3, 8, 54, blank=5, labels=first, gc=[0.5, 2.0]),
                        _Step(2, 5, 3, 8, 55, blank=5, labels=first, lam=0.5)])


def test_products_that_underflow_to_signed_zero(hip_device):
    """grad_costs so small that -sc * exp(..) is -0.0f: stored like any value, and cleared like any value afterwards.
    (1e-38 is subnormal already; 1e-45 is the smallest subnormal, so every entry of the full-size utterance 0 whose
    occupation is below one half rounds to -0.0f, and to +0.0f under the negative factor.)"""
    outs = _chain(hip_device, [_Step(3, 5, 3, 8, 61, ragged=False), _Step(3, 5, 3, 8, 62, gc=[1e-45, 1e-38, -1e-45]),
                               _Step(3, 5, 3, 8, 63, gc=[1e-45, -1e-45, 1e-38]), _Step(3, 5, 3, 8, 64)])
    for _, words in outs[1:3]:
        assert (words.view(np.uint32) == 0x80000000).any()      # the case does reach -0.0f
    assert not (outs[3][1].view(np.uint32) == 0x80000000).any()


def test_rejections_are_the_parents(hip_device):
    """pika_rgrad_backward_fe answers PIKA_EINVAL for a negative prev_rows, a prev_blank out of range, a NULL cols_out and a
    negative fastemit_lambda, and launches nothing (the tensor stays as it was)."""
    from pika_amd import _lib
    lib = _lib.lib()
    st = _Step(2, 5, 3, 8, 71)
    args, ws, stream = _forward(lib, hip_device, st)
    grads = torch.zeros(st.rows * st.V, dtype=torch.float32, device=hip_device)
    cols = torch.full((st.rows,), -1, dtype=torch.int32, device=hip_device)
    assert _fused(lib, st, args, ws, grads, (cols, -1, 0), cols, stream) == PIKA_EINVAL
    assert _fused(lib, st, args, ws, grads, (cols, st.rows, st.V), cols, stream) == PIKA_EINVAL
    assert _fused(lib, st, args, ws, grads, (cols, st.rows, -1), cols, stream) == PIKA_EINVAL
    assert _fused(lib, st, args, ws, grads, (cols, st.rows, 0), None, stream) == PIKA_EINVAL
    assert _fused(lib, st, args, ws, grads, (None, 0, 0), None, stream) == PIKA_EINVAL
    st.lam = -0.5
    assert _fused(lib, st, args, ws, grads, (cols, st.rows, 0), cols, stream) == PIKA_EINVAL
    assert _fused(lib, st, args, ws, grads, (None, 0, 0), cols, stream) == PIKA_EINVAL
    torch.cuda.synchronize()
    assert not grads.view(torch.int32).any()
