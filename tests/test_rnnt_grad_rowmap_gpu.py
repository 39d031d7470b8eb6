"""The frame map of the fused backward (rnnt_grad_rowmeta_update_frames_kernel) and the strided grad_costs entry
(pika_rgrad_backward_fe_s): a workgroup of 512 threads owns F = 512 // U1 whole frames of one utterance, runs of frame
chunks go to one XCD, rows of a larger earlier gradient go to workgroups of their own, and U1 > 512 keeps the linear map.

Yardstick, as in tests/test_rnnt_grad_fused_gpu.py: the two-call route on identical inputs --
pika_rnnt_loss_backward_fe(grads = NULL), then pika_rgrad_dense_grads_update -- on a clone of the same previous tensor
(guard words included), the same previous cols and a clone of the same forward workspace, with the factors of a strided
grad_costs laid out one after the other.  Bit for bit: the whole buffer as int32 (-0.0f is not +0.0f; the guard words in
front of and behind the tensor with it), cols_out, every byte of the workspace.  One chain is also compared with the fp64
oracle at the fused test's tolerance (|err| <= 1e-4 |g| + 1e-5).

Shapes are the smallest at which a piece of the map can go wrong: U1 with and without unused threads in the workgroup
(7: 512 = 73 * 7 + 1), at and around the workgroup size, T at and around F and beyond two workgroups, one and three
utterances with ragged lengths (T_n = 1 and U_n = 0 among them).
"""
import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import make_case

pytestmark = pytest.mark.gpu

PIKA_EINVAL = -1
NT = 512          # the fused kernel's workgroup
GUARD = 8         # floats in front of and behind the tensor (32 bytes: the tensor keeps the allocation's alignment)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Step(object):
    """One call's inputs.  (B, T, U) as helpers.make_case takes them (U1 = U + 1).  gc: None, or factors (resized to B);
    gc_stride: how the strided entry sees them -- None: the unstrided entry, 0: the first factor for every utterance
    (gc None with a stride: NULL factors through the strided entry)."""

    def __init__(self, B, T, U, V, seed, ragged=True, blank=0, lam=0.0, gc=None, gc_stride=None, labels=None, of=None):
        self.B, self.T, self.U1, self.V, self.blank, self.lam = B, T, U + 1, V, blank, lam
        self.lp, self.y, self.tl, self.ul = make_case(B, T, U, V, seed, ragged=ragged, blank=blank)
        if labels is not None:       # another step's lengths under (a variation of) its labels
            self.y, self.tl, self.ul = labels, of.tl, of.ul
        self.gc = None if gc is None else np.resize(np.asarray(gc, np.float32), B)
        if gc_stride == 0 and gc is not None:
            self.gc[:] = self.gc[0]
        self.gc_stride = gc_stride
        self.rows = B * T * self.U1


def _forward(lib, dev, st):
    """The step's device arguments and its workspace after the forward.  Returns the factors twice: as the fused call
    reads them (pointer, stride) and one after the other."""
    lp, y, tl, ul, gc = (_dev(a, dev) for a in (st.lp, st.y if st.U1 > 1 else None, st.tl, st.ul, st.gc))
    gcs = gc
    if gc is not None and st.gc_stride == 0:
        gcs = gc[:1].clone()
    elif gc is not None and st.gc_stride not in (None, 1):
        gcs = torch.full((st.B * st.gc_stride,), float("nan"), dtype=torch.float32, device=dev)
        gcs[::st.gc_stride] = gc
    ws = torch.empty(lib.pika_rnnt_workspace_bytes(st.B, st.T, st.U1), dtype=torch.uint8, device=dev)
    costs = torch.empty(st.B, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pika_rnnt_loss_forward(_ptr(lp), _ptr(y), _ptr(tl), _ptr(ul), st.B, st.T, st.U1, st.V, st.blank, _ptr(costs),
                                      _ptr(ws), stream) == 0
    return (y, tl, ul, gc, gcs), ws, stream


def _fused(lib, st, args, ws, grads, prev, cols_out, stream):
    y, tl, ul, _, gcs = args
    if st.gc_stride is None:
        return lib.pika_rgrad_backward_fe(_ptr(y), _ptr(tl), _ptr(ul), st.B, st.T, st.U1, st.V, st.blank, _ptr(gcs), _ptr(ws),
                                          _ptr(grads), st.lam, _ptr(prev[0]), prev[1], prev[2], _ptr(cols_out), stream)
    return lib.pika_rgrad_backward_fe_s(_ptr(y), _ptr(tl), _ptr(ul), st.B, st.T, st.U1, st.V, st.blank, _ptr(gcs),
                                        st.gc_stride, _ptr(ws), _ptr(grads), st.lam, _ptr(prev[0]), prev[1], prev[2],
                                        _ptr(cols_out), stream)


def _two_calls(lib, st, args, ws, grads, prev, cols_out, stream):
    y, tl, ul, gc, _ = args
    assert lib.pika_rnnt_loss_backward_fe(_ptr(y), _ptr(tl), _ptr(ul), st.B, st.T, st.U1, st.V, st.blank, _ptr(gc), _ptr(ws),
                                          None, st.lam, stream) == 0
    return lib.pika_rgrad_dense_grads_update(_ptr(ws), st.B, st.T, st.U1, st.V, st.blank, _ptr(grads), _ptr(prev[0]),
                                             prev[1], prev[2], _ptr(cols_out), stream)


def _chain(dev, steps, shift=0):
    """Run the steps on one tensor of the largest step's rows, `shift` floats past a 32-byte boundary, between guard
    words; every fused update is compared with the two-call route.  Returns the gradient of every step (numpy, the
    step's rows) and the whole tensor's words after it."""
    from pika_amd import _lib
    lib = _lib.lib()
    V = steps[0].V
    n = max(st.rows for st in steps) * V
    buf = torch.full((GUARD + shift + n + GUARD,), 12345.0, dtype=torch.float32, device=dev)
    grads = buf[GUARD + shift:GUARD + shift + n]
    grads.zero_()
    assert grads.data_ptr() % 32 == 4 * shift
    cols = torch.full((n // V,), -7, dtype=torch.int32, device=dev)
    prev, outs = (None, 0, 0), []
    for i, st in enumerate(steps):
        assert st.V == V
        args, ws, stream = _forward(lib, dev, st)
        if i == 0:      # the streaming writer and the cols kernel: nothing known about the tensor
            assert _fused(lib, st, args, ws, grads, prev, cols, stream) == 0
        else:
            ws2, buf2, cols2 = ws.clone(), buf.clone(), cols.clone()
            grads2 = buf2[GUARD + shift:GUARD + shift + n]
            assert _fused(lib, st, args, ws, grads, prev, cols, stream) == 0
            assert _two_calls(lib, st, args, ws2, grads2, (cols2, prev[1], prev[2]), cols2, stream) == 0
            torch.cuda.synchronize()
            g, g2 = buf.view(torch.int32), buf2.view(torch.int32)
            assert torch.equal(g, g2), "step %d: %d words differ" % (i, int((g != g2).sum()))
            assert torch.equal(cols[:st.rows], cols2[:st.rows]), "step %d: cols_out" % i
            assert torch.equal(ws, ws2), "step %d: workspace" % i
            assert not grads.view(torch.int32)[st.rows * V:].any(), "step %d: rows beyond the call's are not +0.0f" % i
        assert bool((buf[:GUARD + shift] == 12345.0).all()) and bool((buf[GUARD + shift + n:] == 12345.0).all()), \
            "step %d: guard words" % i
        prev = (cols, st.rows, st.blank)
        outs.append((grads[:st.rows * V].view(st.B, st.T, st.U1, V).cpu().numpy(), grads.view(torch.int32).cpu().numpy()))
    return outs


def _frames(U1):
    """The frame counts around the workgroup's F = 512 // U1 frames; beyond 512 columns (the linear map) a few small ones."""
    if U1 > NT:
        return [1, 2, 3]
    F = NT // U1
    return sorted({T for T in (1, F - 1, F, F + 1, 2 * F + 3) if T >= 1})


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("U1", [1, 2, 7, 51, 64, 65, 256, 512, 513, 1024])
def test_frame_counts_around_the_workgroup(hip_device, U1, B):
    """Every (U1, T, B): a streaming call, then a fused update with contiguous factors and one with FastEmit and the
    expanded scalar, on ragged lengths (B = 3: T_n = 1 and U_n = 0 in utterance 1).  V = 8: the dword route and, where
    it is built, the sector route."""
    for k, T in enumerate(_frames(U1)):
        s = 1000 * U1 + 10 * k
        _chain(hip_device, [_Step(B, T, U1 - 1, 8, s, ragged=False), _Step(B, T, U1 - 1, 8, s + 1, gc=[0.5, -2.0, 3.0], gc_stride=1),
                            _Step(B, T, U1 - 1, 8, s + 2, lam=0.25, gc=[1.5], gc_stride=0)])


@pytest.mark.parametrize("V", [8, 16, 40, 5000, 4, 12, 5001])
@pytest.mark.parametrize("shift", [0, 1])
def test_vocabulary_sizes_and_a_base_4_bytes_past_the_sector(hip_device, V, shift):
    """V % 8 == 0 with an aligned base may take whole sectors; every other V, and a tensor base offset by 4 bytes, takes
    the dword stores.  U1 = 7 leaves a thread of the workgroup without a row; T = 2 F + 3 = 149 is three workgroups."""
    T = 149 if V < 100 else 5
    _chain(hip_device, [_Step(3, T, 6, V, 200 + V, ragged=False), _Step(3, T, 6, V, 201 + V, gc=[2.0, 0.5, 1.0], gc_stride=2),
                        _Step(3, T, 6, V, 202 + V, lam=0.25, gc_stride=2)], shift=shift)      # NULL factors, strided entry


def test_against_the_oracle(hip_device):
    """B=3, T=12, U1=51 (F = 10: two workgroups per utterance, the second partial), ragged, FastEmit 0.25, factors through
    a stride of 2 and the expanded scalar."""
    steps = [_Step(3, 12, 50, 16, 301, ragged=False), _Step(3, 12, 50, 16, 302, lam=0.25, gc=[0.25, 3.0, -1.5], gc_stride=2),
             _Step(3, 12, 50, 16, 303, lam=0.25, gc=[0.75], gc_stride=0)]
    outs = _chain(hip_device, steps)
    for st, (g, _) in zip(steps[1:], outs[1:]):
        _, g64 = O.rnnt_loss(st.lp, st.y, st.tl, st.ul, blank=st.blank)
        for n in range(st.B):
            if st.ul[n]:
                u = np.arange(st.ul[n])
                g64[n, :st.tl[n], u, st.y[n, u]] *= 1.0 + st.lam
        g64 = g64 * st.gc.astype(np.float64)[:, None, None, None]
        err = np.abs(g - g64)
        assert not (err > 1e-4 * np.abs(g64) + 1e-5).any(), "max abs err %g" % float(err.max())


def test_fewer_rows_the_same_rows_and_more_rows_in_one_storage(hip_device):
    """prev_rows larger than, equal to and smaller than rows, the storage kept at the largest.  (3, 30, 51) leaves 4590
    rows; (1, 3, 7) after it has one workgroup per utterance row of the grid, so the 4569 old rows beyond the call's
    take nine grid rows of their own; (2, 11, 51) after that has a tail inside one."""
    big = lambda s, **k: _Step(3, 30, 50, 8, s, **k)
    outs = _chain(hip_device, [big(401, ragged=False), _Step(1, 3, 6, 8, 402, ragged=False), big(403), big(404, lam=0.25),
                               _Step(2, 11, 50, 8, 405), _Step(2, 11, 50, 8, 406, gc=[1.0, 2.0], gc_stride=1),
                               _Step(3, 5, 3, 8, 407), big(408, gc=[3.0], gc_stride=0)])
    assert outs[0][1][21 * 8:].any()      # the first call did leave entries where the second has no rows


@pytest.mark.parametrize("V", [16, 40])
def test_blank_and_label_columns_in_and_out_of_one_sector(hip_device, V):
    """blank 0, 7, 8 and V - 1 in turn, so prev_blank != blank at every step but the repeated one.  Labels: random; the
    same again (new entries land on old ones); every label moved inside its 8-float sector (old label in the new
    label's sector) or by one sector (not in it); all in blank's sector, the first equal to blank."""
    B, T, U = 2, 75, 6
    first = _Step(B, T, U, V, 501, blank=7)
    near = first.y.copy()
    live = near < V
    near[live] = np.where(np.arange(near.size).reshape(near.shape)[live] % 2 == 0, near[live] ^ 1, (near[live] + 8) % V)
    at8 = first.y.copy()
    at8[at8 < V] = 8 + np.arange(int((at8 < V).sum())) % 8       # blank 8's sector, column 8 itself among them
    at8[0, 0] = 8
    last = first.y.copy()
    last[last < V] = V - 8 + np.arange(int((last < V).sum())) % 8
    _chain(hip_device, [_Step(B, T, U, V, 500, ragged=False), first, _Step(B, T, U, V, 502, blank=7, labels=first.y, of=first, lam=0.25),
                        _Step(B, T, U, V, 503, blank=8, labels=near, of=first), _Step(B, T, U, V, 504, blank=8, labels=at8, of=first),
                        _Step(B, T, U, V, 505, blank=V - 1, labels=last, of=first, gc=[0.5, 2.0], gc_stride=1),
                        _Step(B, T, U, V, 506, blank=0, labels=first.y, of=first)])


def test_products_that_underflow_to_signed_zero(hip_device):
    """grad_costs so small that -sc * exp(..) is -0.0f: stored like any value, and cleared like any value afterwards
    (tests/test_rnnt_grad_fused_gpu.py has the arithmetic); T = 75 is two workgroups of U1 = 7."""
    outs = _chain(hip_device, [_Step(3, 75, 6, 8, 601, ragged=False), _Step(3, 75, 6, 8, 602, gc=[1e-45, 1e-38, -1e-45], gc_stride=1),
                               _Step(3, 75, 6, 8, 603, gc=[1e-45], gc_stride=0), _Step(3, 75, 6, 8, 604, gc_stride=0)])
    for _, words in outs[1:3]:
        assert (words.view(np.uint32) == 0x80000000).any()      # the case does reach -0.0f
    assert not (outs[3][1].view(np.uint32) == 0x80000000).any()


def test_the_strided_entry_rejects_what_the_unstrided_one_rejects(hip_device):
    """The cases tests/test_rnnt_grad_fused_gpu.py pins, through both entries: the same codes, nothing launched; and a
    negative stride."""
    from pika_amd import _lib
    lib = _lib.lib()
    st = _Step(2, 5, 3, 8, 71)
    args, ws, stream = _forward(lib, hip_device, st)
    grads = torch.zeros(st.rows * st.V, dtype=torch.float32, device=hip_device)
    cols = torch.full((st.rows,), -1, dtype=torch.int32, device=hip_device)

    def both(prev, cols_out, lam=0.0):
        st.lam, codes = lam, []
        for st.gc_stride in (None, 1):
            codes.append(_fused(lib, st, args, ws, grads, prev, cols_out, stream))
        assert codes[0] == codes[1]
        return codes[1]

    assert both((cols, -1, 0), cols) == PIKA_EINVAL
    assert both((cols, st.rows, st.V), cols) == PIKA_EINVAL
    assert both((cols, st.rows, -1), cols) == PIKA_EINVAL
    assert both((cols, st.rows, 0), None) == PIKA_EINVAL
    assert both((None, 0, 0), None) == PIKA_EINVAL
    assert both((cols, st.rows, 0), cols, lam=-0.5) == PIKA_EINVAL
    assert both((None, 0, 0), cols, lam=-0.5) == PIKA_EINVAL
    st.lam, st.gc_stride = 0.0, -1
    assert _fused(lib, st, args, ws, grads, (cols, st.rows, 0), cols, stream) == PIKA_EINVAL
    assert _fused(lib, st, args, ws, grads, (None, 0, 0), cols, stream) == PIKA_EINVAL
    torch.cuda.synchronize()
    assert not grads.view(torch.int32).any()


def test_sum_backward_reads_the_expanded_factor_in_place(hip_device):
    """`costs.sum().backward()` hands the backward a stride-0 grad_costs: the reused gradient is word for word that of
    explicit unit factors, and of a strided slice of factors that of the contiguous copy."""
    from pika_amd import rnnt as R
    lp, y, tl, ul = make_case(3, 12, 50, 16, 801, ragged=True)
    y, tl, ul = (_dev(a, hip_device) for a in (y, tl, ul))
    w = torch.tensor([1.0, 9.0, 0.5, 9.0, -2.0, 9.0], device=hip_device)

    def grad(how):
        x = _dev(lp, hip_device).requires_grad_(True)
        costs = R.rnnt_loss(x, y, tl, ul)
        if how == "sum":
            costs.sum().backward()
        else:
            costs.backward(how)
        g = x.grad.view(torch.int32).clone()
        x.grad = None
        return g

    R.release_grad_buffer()
    try:
        before = dict(R.GRAD_REUSE_STATS)
        ones = grad(torch.ones(3, device=hip_device))                  # streams; then every call reuses
        assert torch.equal(grad("sum"), ones)
        assert torch.equal(grad(w[::2]), grad(w[::2].contiguous()))
        assert R.GRAD_REUSE_STATS["reused"] - before["reused"] == 3
    finally:
        R.release_grad_buffer()
