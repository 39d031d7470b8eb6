"""The dense-gradient writer of the RNN-T loss at the edges of its launch geometry.

The yardstick is the library's own generic route.  One forward and one `pika_rnnt_loss_backward_fe(grads=NULL)` fill
the workspace's row metadata; `pika_rnnt_loss_dense_grads` then writes the same tensor twice: into a 16-byte-aligned
buffer (the vectorised writers: `rnnt_grad_kernel<true,2>` with its workgroup-to-chunk map for V/4 >= 64,
`rnnt_grad_kernel<false,4>` below) and into a view 4 bytes further on, which takes `rnnt_grad_scalar_kernel`, one float
per thread and no geometry at all.  The two must agree bit for bit (compared as int32, so -0.0 and NaN cannot hide).
Both buffers start as NaN and the elements around them must still be NaN afterwards; a third write over a different
poison shows that every element was written.

Shapes: a workgroup of the vectorised writer covers 512 16-byte groups and its chunk map permutes aligned groups of
512 workgroups, so the cases put B*T*U1*V/4 one below, at and one above a multiple of 512, below one span, and past
one and two whole groups of 512 workgroups with a partial group behind them.
"""
import numpy as np
import pytest
import torch

from oracle import rnnt as O
from helpers import make_case
from test_rnnt_loss_gpu import grads_close

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
ALT_BITS = 0x55555555
GUARD = 8


def _L():
    from pika_amd import _lib
    return _lib.lib()


def _ok(rc, what):
    from pika_amd import _lib
    _lib.check(rc, what)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poisoned(n, bits, dev):
    return torch.full((n,), bits, dtype=torch.int32, device=dev)


def _three_writes(dev, n, write):
    """write(ptr) fills n floats at ptr.  Returns the aligned result as int32 (cpu) after the checks every case shares."""
    a = _poisoned(n + GUARD, NAN_BITS, dev)                 # aligned: [0, n) written, [n, n + GUARD) guard
    b = _poisoned(n + 2 * GUARD, NAN_BITS, dev)             # 4 bytes off: [1, 1 + n) written
    c = _poisoned(n + GUARD, ALT_BITS, dev)                 # aligned again, other poison
    assert a.data_ptr() % 16 == 0 and c.data_ptr() % 16 == 0 and (b.data_ptr() + 4) % 16 == 4
    write(a.data_ptr())
    write(b.data_ptr() + 4)
    write(c.data_ptr())
    torch.cuda.synchronize()
    a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    assert np.all(a[n:] == NAN_BITS), "aligned route wrote past the end"
    assert b[0] == NAN_BITS and np.all(b[1 + n:] == NAN_BITS), "generic route wrote outside its view"
    assert np.all(c[n:] == ALT_BITS), "aligned route wrote past the end"
    bad = np.flatnonzero(a[:n] != b[1:1 + n])
    assert bad.size == 0, "aligned and generic routes differ at %d elements, first %s" % (bad.size, bad[:8])
    assert np.array_equal(a[:n], c[:n]), "an element kept its poison (not every element is written)"
    return a[:n]


def _dense(dev, lp, y, tl, ul, blank):
    B, T, U1, V = lp.shape
    lib = _L()
    x, yd, tld, uld = (_d(v, dev) for v in (lp, y, tl, ul))
    ws = torch.empty(int(lib.pika_rnnt_workspace_bytes(B, T, U1)), dtype=torch.uint8, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    _ok(lib.pika_rnnt_loss_forward(x.data_ptr(), yd.data_ptr(), tld.data_ptr(), uld.data_ptr(), B, T, U1, V, blank,
                                   costs.data_ptr(), ws.data_ptr(), _s()), "forward")
    _ok(lib.pika_rnnt_loss_backward_fe(yd.data_ptr(), tld.data_ptr(), uld.data_ptr(), B, T, U1, V, blank, None,
                                       ws.data_ptr(), None, 0.0, _s()), "backward_fe (metadata only)")

    def write(ptr):
        _ok(lib.pika_rnnt_loss_dense_grads(ws.data_ptr(), B, T, U1, V, blank, ptr, _s()), "dense_grads")
    g = _three_writes(dev, B * T * U1 * V, write)
    return g.reshape(B, T, U1, V)


# B, T, U1, V: n4 = B*T*U1*V/4 against the 512-group workgroup span and the 512-workgroup map group
GEOMETRY = [
    pytest.param(1, 3, 2, 256, id="V4=64-below-one-span"),            # 384 groups
    pytest.param(1, 4, 2, 256, id="V4=64-one-span"),                  # 512
    pytest.param(1, 3, 2, 252, id="V4=63-lane-route"),                # below the scalar-metadata threshold
    pytest.param(2, 5, 3, 252, id="V4=63-lane-route-two-blocks"),
    pytest.param(2, 5, 3, 260, id="V4=65"),
    pytest.param(1, 4, 3, 512, id="V4=128-three-spans"),              # 1536 = 3 * 512
    pytest.param(1, 71, 9, 516, id="V4=129-span-minus-1"),            # 82431 = 161 * 512 - 1
    pytest.param(5, 7, 11, 516, id="V4=129-span-plus-1"),             # 49665 = 97 * 512 + 1
    pytest.param(3, 29, 25, 516, id="group-plus-36-spans-minus-1"),   # 280575 = 548 * 512 - 1: 548 workgroups
    pytest.param(5, 31, 19, 516, id="group-plus-230-spans-plus-1"),   # 379905 = 742 * 512 + 1: 743 workgroups
    pytest.param(4, 64, 16, 512, id="two-whole-groups"),              # 524288 = 1024 * 512
    pytest.param(2, 7, 51, 5000, id="benchmark-row-length"),          # 892500 groups, 1744 workgroups; 1250 % 64 != 0
]


@pytest.mark.parametrize("B,T,U1,V", GEOMETRY)
def test_aligned_route_equals_generic_route(hip_device, B, T, U1, V):
    lp, y, tl, ul = make_case(B, T, U1 - 1, V, seed=B * 1000 + T + V, ragged=False)
    g = _dense(hip_device, lp, y, tl, ul, 0)
    assert np.count_nonzero(g) > 0
    assert np.count_nonzero(g.reshape(-1, V), axis=1).max() <= 2     # a row holds the blank and the label entry


@pytest.mark.parametrize("V", [252, 256, 260, 516])
@pytest.mark.parametrize("blank", ["last", 5])
def test_blank_positions_labels_and_ragged_lengths(hip_device, V, blank):
    B, T, U = 4, 9, 6
    blank = V - 1 if blank == "last" else blank
    assert blank & 3 != 0
    lp, y, tl, ul = make_case(B, T, U, V, seed=V + blank, ragged=True, blank=blank)
    assert ul[0] == U and tl[0] == T
    tl[2], ul[2] = T - 2, U - 1
    y[2, :ul[2]] = (blank + 2 + np.arange(ul[2])) % V
    y[2, 0] = blank           # a label equal to blank: the label entry wins
    y[0, 1] = V + 3           # labels outside [0, V): no label entry
    y[0, 2] = -2
    y[2, ul[2]:] = V
    g = _dense(hip_device, lp, y, tl, ul, blank)
    for n in range(B):        # rows outside the sub-lattice are all zero
        assert not g[n, tl[n]:].any() and not g[n, :, ul[n] + 1:].any()
    others = np.delete(np.arange(V), blank)
    assert not g[0][:, 1:3][:, :, others].any()                       # cells whose label is out of range: blank only
    assert np.count_nonzero(g[2, :, 0], axis=-1).max() <= 1            # label == blank: one entry, in the blank column
    assert not g[2, :, 0][:, others].any()


def test_packed_call(hip_device):
    dev = hip_device
    B, T, U, V, blank = 5, 9, 6, 260, 3
    lp, y, tl, ul = make_case(B, T, U, V, seed=11, ragged=True, blank=blank)
    tl[2:], ul[2:] = (7, 5, 9), (3, 5, 4)
    for n in range(2, B):
        y[n] = V
        y[n, :ul[n]] = blank + 1 + 7 * (n + np.arange(ul[n]))       # in range, never the blank
    rows =tl.astype(np.int64) * (ul + 1)
    N = int(rows.sum())
    assert N % 2 == 1 and (N * V // 4) % 512 not in (0, 1, 511)
    roff = (np.cumsum(rows) - rows).astype(np.int32)
    loff = (np.cumsum(ul) - ul).astype(np.int32)
    xp = np.concatenate([lp[n, :tl[n], :ul[n] + 1].reshape(-1, V) for n in range(B)])
    yp = np.concatenate([y[n, :ul[n]] for n in range(B)]).astype(np.int32)
    lib = _L()
    x, yd, tld, uld, rd, ld = (_d(v, dev) for v in (xp, yp, tl, ul, roff, loff))
    Tm, U1m = int(tl.max()), int(ul.max()) + 1
    ws = torch.empty(int(lib.pika_rnnt_workspace_bytes(B, Tm, U1m)), dtype=torch.uint8, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    _ok(lib.pika_rnnt_packed_forward(x.data_ptr(), yd.data_ptr(), tld.data_ptr(), uld.data_ptr(), rd.data_ptr(),
                                     ld.data_ptr(), B, Tm, U1m, N, V, blank, costs.data_ptr(), ws.data_ptr(), _s()),
        "packed_forward")

    def write(ptr):
        _ok(lib.pika_rnnt_packed_backward(yd.data_ptr(), tld.data_ptr(), uld.data_ptr(), rd.data_ptr(), ld.data_ptr(),
                                          B, Tm, U1m, N, V, blank, None, ws.data_ptr(), ptr, 0.0, _s()),
            "packed_backward")
    g = _three_writes(dev, N * V, write).view(np.float32).reshape(N, V)
    # against the fp64 oracle of the padded batch, row by row
    c64, g64 = O.rnnt_loss(lp, y, tl, ul, blank=blank)
    ref = np.concatenate([g64[n, :tl[n], :ul[n] + 1].reshape(-1, V) for n in range(B)])
    grads_close(g, ref)


def test_end_to_end_against_fp64(hip_device):
    from pika_amd.rnnt import rnnt_loss
    dev = hip_device
    B, T, U, V = 3, 20, 5, 320
    lp, y, tl, ul = make_case(B, T, U, V, seed=5, ragged=True)
    c64, g64 = O.rnnt_loss(lp, y, tl, ul)
    x = _d(lp, dev).requires_grad_(True)
    costs = rnnt_loss(x, *[_d(a, dev) for a in (y, tl, ul)])
    costs.sum().backward()
    torch.cuda.synchronize()
    assert x.grad.data_ptr() % 16 == 0
    assert np.allclose(costs.detach().cpu().numpy(), c64, rtol=1e-5)
    grads_close(x.grad.cpu().numpy(), g64)
