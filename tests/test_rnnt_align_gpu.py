"""RNN-T forced alignment on the device against the float64 Viterbi of tests/align_common.py.

For utterance n, bound = (T_n + U_n) * 2^-23 * max|delta64|: the worst case of T_n + U_n rounded fp32 additions on
values no larger than the fp64 lattice's own (computed here from the fp64 sweep, never from the code under test).
Frames are compared exactly wherever the optimum is unique by margin (margin > 2 * bound); validity and the two
self-consistency checks hold for every utterance.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_common as A  # noqa: E402
from helpers import make_case  # noqa: E402

pytestmark = pytest.mark.gpu

NEG = -1.0e30
SMALL = [(4, 50, 10, 24), (3, 33, 7, 64), (4, 20, 4, 24), (3, 50, 10, 16)]   # (B, T, U, V), ragged
SEEDS = [0, 1, 2, 3]


def _dev(hip_device, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(hip_device) for a in arrays]


class Ref(object):
    """fp64 side of one utterance."""

    def __init__(self, lpb, lpe):
        self.lpb, self.lpe = lpb, lpe
        self.T, self.U = lpb.shape[0], lpe.shape[1]
        self.score, self.frames, delta = A.viterbi(lpb, lpe)
        self.bound = A.bound(delta, self.T, self.U)
        self.margin = A.margin(lpb, lpe, self.frames)
        self.unique = self.margin > 2 * self.bound


def _refs(lp, y, tl, ul, blank=0):
    return [Ref(*A.planes(lp, y, n, tl[n], ul[n], blank)) for n in range(lp.shape[0])]


def _check(refs, scores, frames, ul, costs=None, what=""):
    """Items 4-6 for a padded result (frames (B, U) numpy)."""
    for n, r in enumerate(refs):
        f = frames[n, :r.U]
        tag = "%s utterance %d (T=%d U=%d)" % (what, n, r.T, r.U)
        assert A.valid_frames(f, r.T), (tag, f)
        assert (frames[n, r.U:] == -1).all(), tag
        re = A.rescore(r.lpb, r.lpe, f)
        print("%s: score %.6f fp64 %.6f rescored %.6f bound %.3g margin %.3g unique %s" % (
            tag, scores[n], r.score, re, r.bound, r.margin, r.unique))
        assert abs(re - float(scores[n])) <= r.bound, tag
        assert abs(re - r.score) <= r.bound, tag
        if costs is not None:
            assert float(scores[n]) <= -float(costs[n]) + r.bound, tag
        if r.unique:
            assert f.tolist() == r.frames.tolist(), tag


def test_most_small_random_utterances_qualify_for_exact_frames():
    """Item 6's cap, from the fp64 sweep alone: at most 1 utterance in 10 may fail margin > 2 * bound."""
    n = q = 0
    for (B, T, U, V) in SMALL:
        for seed in SEEDS:
            lp, y, tl, ul = make_case(B, T, U, V, seed=seed, ragged=True)
            for r in _refs(lp, y, tl, ul):
                n += 1
                q += bool(r.unique)
    print("qualifying: %d of %d" % (q, n))
    assert 10 * (n - q) <= n


@pytest.mark.parametrize("dims", SMALL)
@pytest.mark.parametrize("seed", SEEDS)
def test_small_random(hip_device, dims, seed):
    from pika_amd.rnnt import rnnt_align, rnnt_loss
    B, T, U, V = dims
    lp, y, tl, ul = make_case(B, T, U, V, seed=seed, ragged=True)
    refs = _refs(lp, y, tl, ul)
    d = _dev(hip_device, lp, y, tl, ul)
    scores, frames = rnnt_align(*d)
    costs = rnnt_loss(*d)
    assert scores.dtype == torch.float32 and frames.dtype == torch.int32
    assert scores.shape == (B,) and frames.shape == (B, U) and not scores.requires_grad
    _check(refs, scores.cpu().numpy(), frames.cpu().numpy(), ul, costs.cpu().numpy(), "small %s seed %d" % (dims, seed))


def test_nonzero_blank(hip_device):
    from pika_amd.rnnt import rnnt_align
    lp, y, tl, ul = make_case(3, 30, 6, 24, seed=5, ragged=True, blank=7)
    refs = _refs(lp, y, tl, ul, blank=7)
    scores, frames = rnnt_align(*_dev(hip_device, lp, y, tl, ul), blank=7)
    _check(refs, scores.cpu().numpy(), frames.cpu().numpy(), ul, None, "blank 7")


def test_long_random_is_self_consistent(hip_device):
    """T = 1000, U = 50: random inputs do not qualify for exact frames; items 4-5 apply."""
    from pika_amd.rnnt import rnnt_align, rnnt_loss
    lp, y, tl, ul = make_case(2, 1000, 50, 64, seed=11, ragged=True)
    tl[1], ul[1] = 731, 37
    y[1, :37] = np.random.default_rng(3).integers(1, 64, 37)
    refs = _refs(lp, y, tl, ul)
    d = _dev(hip_device, lp, y, tl, ul)
    scores, frames = rnnt_align(*d)
    _check(refs, scores.cpu().numpy(), frames.cpu().numpy(), ul, rnnt_loss(*d).cpu().numpy(), "long")


# ---------------------------------------------------------------------------------------------
# planted paths
# ---------------------------------------------------------------------------------------------
def _plant(hip_device, T, U1, V, tl, ul, paths, seed, bonus=30.0):
    """Logits (B,T,U1,V) on the device: standard normal, plus `bonus` on the column of the planted path's outgoing edge
    in every cell the path visits.  Returns (logits, labels (B, U1-1) numpy)."""
    B = len(paths)
    g = torch.Generator(device=hip_device)
    g.manual_seed(seed)
    x = torch.randn((B, T, U1, V), generator=g, device=hip_device, dtype=torch.float32)
    rng = np.random.default_rng(seed)
    y = rng.integers(1, V, (B, U1 - 1)).astype(np.int32)
    for n, fr in enumerate(paths):
        Tn, Un = int(tl[n]), int(ul[n])
        fr = np.asarray(fr, dtype=np.int64)
        assert fr.shape == (Un,) and A.valid_frames(fr, Tn)
        on = A.path_cells(fr, Tn)                                   # (Tn, Un+1)
        t, u = np.nonzero(on)
        emits = np.zeros_like(on)
        emits[fr, np.arange(Un)] = True
        col = np.where(emits[t, u], y[n, np.minimum(u, max(Un - 1, 0))] if Un else 0, 0)
        x[n, torch.from_numpy(t).to(hip_device), torch.from_numpy(u).to(hip_device),
          torch.from_numpy(col.astype(np.int64)).to(hip_device)] += bonus
        y[n, Un:] = V
    return x, y


def _planes_from_device(lp, y, tl, ul):
    """fp64 planes of every utterance from the two gathered columns per cell of a device (B,T,U1,V) tensor."""
    B, T, U1, V = lp.shape
    lpb = lp[..., 0].double().cpu().numpy()
    idx = torch.from_numpy(np.minimum(y, V - 1).astype(np.int64)).to(lp.device)           # (B, U1-1)
    lpe = torch.gather(lp[:, :, :U1 - 1, :], 3, idx[:, None, :, None].expand(B, T, U1 - 1, 1))[..., 0].double().cpu().numpy()
    return [(np.ascontiguousarray(lpb[n, :tl[n], :ul[n] + 1]), np.ascontiguousarray(lpe[n, :tl[n], :ul[n]]))
            for n in range(B)]


def _random_path(rng, Tn, Un):
    return np.sort(rng.integers(0, Tn, Un))


def _planted_case(name):
    rng = np.random.default_rng(17)
    if name == "bench":          # the benchmark's lattice, ragged
        T, U1, V = 1000, 51, 5000
        tl, ul = [1000, 777], [50, 31]
        p1 = _random_path(rng, 777, 31)
        p1[5:9] = p1[5]                                   # several labels on one frame
        paths = [_random_path(rng, 1000, 50), np.sort(p1)]
    elif name == "two_waves":    # U1 in 65..128
        T, U1, V = 200, 100, 32
        tl, ul = [200, 1, 150, 200, 120], [99, 40, 0, 70, 99]
        paths = [_random_path(rng, 200, 99), np.zeros(40, np.int64), np.zeros(0, np.int64),
                 np.full(70, 199), _random_path(rng, 120, 99)]
    elif name == "six_waves":    # U1 > 256 (and more diagonals than the LDS buffer holds at this width)
        T, U1, V = 120, 300, 16
        tl, ul = [120, 90, 120], [299, 299, 130]
        paths = [_random_path(rng, 120, 299), _random_path(rng, 90, 299), np.zeros(130, np.int64)]
    elif name == "long":         # one wave, more diagonals than the kernel's LDS buffer holds: back-pointers in scratch
        T, U1, V = 1700, 21, 16
        tl, ul = [1700, 1650], [20, 20]
        paths = [_random_path(rng, 1700, 20), np.full(20, 1649)]
    else:                        # one wave: the corners
        T, U1, V = 60, 12, 24
        tl, ul = [60, 1, 60, 60, 41, 60], [11, 7, 0, 11, 11, 9]
        paths = [np.zeros(11, np.int64), np.zeros(7, np.int64), np.zeros(0, np.int64), np.full(11, 59),
                 _random_path(rng, 41, 11), np.array([3, 3, 3, 3, 20, 20, 59, 59, 59])]
    return T, U1, V, np.asarray(tl, np.int32), np.asarray(ul, np.int32), paths


@pytest.mark.parametrize("name", ["corners", "two_waves", "six_waves", "long", "bench"])
def test_planted_paths_are_recovered_exactly(hip_device, name):
    from pika_amd.rnnt import rnnt_align, rnnt_align_from_logits
    T, U1, V, tl, ul, paths = _planted_case(name)
    x, y = _plant(hip_device, T, U1, V, tl, ul, paths, seed=23)
    lp = torch.log_softmax(x, dim=-1)
    refs = [Ref(lpb, lpe) for lpb, lpe in _planes_from_device(lp, y, tl, ul)]
    for n, r in enumerate(refs):
        print("%s utterance %d: margin %.3f bound %.3g" % (name, n, r.margin, r.bound))
        assert r.unique, (name, n, r.margin, r.bound)
        assert r.frames.tolist() == np.asarray(paths[n]).tolist(), (name, n)
    yd, tld, uld = _dev(hip_device, y, tl, ul)
    scores, frames = rnnt_align(lp, yd, tld, uld)
    scores, frames = scores.cpu().numpy(), frames.cpu().numpy()
    _check(refs, scores, frames, ul, None, name)
    for n in range(len(paths)):
        assert frames[n, :ul[n]].tolist() == np.asarray(paths[n]).tolist(), (name, n)
    del lp
    # the fused source of the planes (V % 4 == 0): identical frames, scores within 2 * bound
    s2, f2 = rnnt_align_from_logits(x, yd, tld, uld)
    assert np.array_equal(f2.cpu().numpy(), frames)
    for n, r in enumerate(refs):
        assert abs(float(s2[n]) - float(scores[n])) <= 2 * r.bound, (name, n)


# ---------------------------------------------------------------------------------------------
# tie rule, sources of the planes, non-interference, capture, infeasible transcripts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,U1", [(20, 11), (9, 64), (25, 130), (7, 300)])
def test_ties_resolve_to_the_earliest_emission(hip_device, T, U1):
    from pika_amd.rnnt import rnnt_align
    B, V = 3, 8
    lp = torch.full((B, T, U1, V), float(np.log(1.0 / V)), device=hip_device)
    y = torch.randint(1, V, (B, U1 - 1), dtype=torch.int32, device=hip_device)
    tl = torch.tensor([T, max(T // 2, 1), 1], dtype=torch.int32, device=hip_device)
    ul = torch.tensor([U1 - 1, U1 // 2, U1 - 1], dtype=torch.int32, device=hip_device)
    scores, frames = rnnt_align(lp, y, tl, ul)
    frames = frames.cpu().numpy()
    for n in range(B):
        Un = int(ul[n])
        assert (frames[n, :Un] == 0).all() and (frames[n, Un:] == -1).all()
        assert float(scores[n]) == pytest.approx((int(tl[n]) + Un) * np.log(1.0 / V), rel=1e-5)


def _pack(lp, y, tl, ul):
    rows = [lp[n, :tl[n], :ul[n] + 1].reshape(-1, lp.shape[-1]) for n in range(lp.shape[0])]
    return np.concatenate(rows), np.concatenate([y[n, :ul[n]] for n in range(lp.shape[0])]).astype(np.int32)


@pytest.mark.parametrize("dims", [(4, 50, 10, 24), (3, 40, 80, 16)])
def test_padded_and_packed_agree_bit_for_bit(hip_device, dims):
    from pika_amd.rnnt import rnnt_align, rnnt_align_from_logits
    B, T, U, V = dims
    lp, y, tl, ul = make_case(B, T, U, V, seed=4, ragged=True)
    plp, py = _pack(lp, y, tl, ul)
    s1, f1 = rnnt_align(*_dev(hip_device, lp, y, tl, ul))
    s2, f2 = rnnt_align(*_dev(hip_device, plp, py, tl, ul), compact=True)
    assert f2.shape == (int(ul.sum()),) and f2.dtype == torch.int32
    assert torch.equal(s1, s2)
    f1, f2 = f1.cpu().numpy(), f2.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(ul)])
    for n in range(B):
        assert f1[n, :ul[n]].tolist() == f2[off[n]:off[n + 1]].tolist()
    # raw logits, padded vs packed
    rng = np.random.default_rng(8)
    x = rng.standard_normal(lp.shape).astype(np.float32) * 2
    px, _ = _pack(x, y, tl, ul)
    s3, f3 = rnnt_align_from_logits(*_dev(hip_device, x, y, tl, ul))
    s4, f4 = rnnt_align_from_logits(*_dev(hip_device, px, py, tl, ul), compact=True)
    assert torch.equal(s3, s4)
    f3, f4 = f3.cpu().numpy(), f4.cpu().numpy()
    for n in range(B):
        assert f3[n, :ul[n]].tolist() == f4[off[n]:off[n + 1]].tolist()


@pytest.mark.parametrize("dims", [(4, 50, 10, 24), (3, 33, 7, 64)])
def test_from_logits_agrees_with_log_softmax(hip_device, dims):
    from pika_amd.rnnt import rnnt_align, rnnt_align_from_logits
    B, T, U, V = dims
    _, y, tl, ul = make_case(B, T, U, V, seed=6, ragged=True)
    x = (np.random.default_rng(6).standard_normal((B, T, U + 1, V)) * 2).astype(np.float32)
    xd, yd, tld, uld = _dev(hip_device, x, y, tl, ul)
    lp = torch.log_softmax(xd, dim=-1)
    refs = _refs(lp.cpu().numpy(), y, tl, ul)
    s1, f1 = rnnt_align(lp, yd, tld, uld)
    s2, f2 = rnnt_align_from_logits(xd, yd, tld, uld)
    f1, f2 = f1.cpu().numpy(), f2.cpu().numpy()
    _check(refs, s1.cpu().numpy(), f1, ul, None, "log_softmax")
    for n, r in enumerate(refs):
        assert A.valid_frames(f2[n, :r.U], r.T) and (f2[n, r.U:] == -1).all()
        assert abs(float(s1[n]) - float(s2[n])) <= 2 * r.bound, n
        if r.unique:
            assert f2[n].tolist() == f1[n].tolist(), n


def test_lazy_log_probs_are_read_raw(hip_device):
    """A LazyLogProbs of the package's joint goes the fused way: same answer as from_logits, buffer still raw."""
    from pika_amd import rnnt
    _, y, tl, ul = make_case(3, 30, 6, 24, seed=9, ragged=True)
    x = (np.random.default_rng(9).standard_normal((3, 30, 7, 24)) * 2).astype(np.float32)
    xd, yd, tld, uld = _dev(hip_device, x, y, tl, ul)
    state = rnnt.LogitsState(1.0)
    lazy = rnnt.LazyLogProbs(state, xd.clone())
    s1, f1 = rnnt.rnnt_align(lazy, yd, tld, uld)
    s2, f2 = rnnt.rnnt_align_from_logits(xd, yd, tld, uld)
    assert state.raw and torch.equal(lazy.buf, xd)
    assert torch.equal(s1, s2) and torch.equal(f1, f2)


def _align_on(ws, tl, ul, loff, B, T, U1, n_frames, guard=64):
    """pika_rnnt_align on a workspace the loss has filled; the output sits between two guard bands."""
    from pika_amd import _lib
    L = _lib.lib()
    dev = ws.device
    scores = torch.full((B + 2 * guard,), 7.0, dtype=torch.float32, device=dev)
    frames = torch.full((n_frames + 2 * guard,), -77, dtype=torch.int32, device=dev)
    scratch = torch.empty(L.pika_rnnt_align_scratch_bytes(B, T, U1), dtype=torch.uint8, device=dev)
    rc = L.pika_rnnt_align(ws.data_ptr(), tl.data_ptr(), ul.data_ptr(), None if loff is None else loff.data_ptr(), B, T,
                           U1, scores[guard:].data_ptr(), frames[guard:].data_ptr(), scratch.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert (scores[:guard] == 7.0).all() and (scores[B + guard:] == 7.0).all()
    assert (frames[:guard] == -77).all() and (frames[n_frames + guard:] == -77).all()
    return scores[guard:B + guard].clone(), frames[guard:n_frames + guard].clone()


@pytest.mark.parametrize("lam", [0.0, 0.25])
@pytest.mark.parametrize("packed", [False, True])
def test_align_between_forward_and_backward_changes_no_gradient(hip_device, lam, packed):
    from pika_amd.rnnt import rnnt_align, rnnt_loss
    B, T, U, V = 4, 50, 10, 24
    lp, y, tl, ul = make_case(B, T, U, V, seed=2, ragged=True)
    if packed:
        lp, y = _pack(lp, y, tl, ul)
    lpd, yd, tld, uld = _dev(hip_device, lp, y, tl, ul)
    w = torch.linspace(0.5, 1.5, B, device=hip_device)

    def run(align):
        x = lpd.clone().requires_grad_(True)
        costs = rnnt_loss(x, yd, tld, uld, fastemit_lambda=lam, compact=packed)
        out = None
        if align:
            saved = costs.grad_fn.saved_tensors
            ws = saved[3]
            before = ws.clone()
            if packed:
                out = _align_on(ws, tld, uld, saved[5], B, int(tl.max()), int(ul.max()) + 1, int(ul.sum()))
            else:
                out = _align_on(ws, tld, uld, None, B, T, U + 1, B * U)
            assert torch.equal(ws, before)                     # the workspace is read, never written
        (costs * w).sum().backward()
        return x.grad.clone(), out

    g0, _ = run(False)
    g1, (scores, frames) = run(True)
    assert torch.equal(g0, g1)
    # the raw call gives what the Python function gives (and wrote nothing outside its outputs)
    s, f = rnnt_align(lpd, yd, tld, uld, compact=packed)
    assert torch.equal(s, scores) and torch.equal(f.reshape(-1), frames)


def test_padded_call_is_capturable_and_packed_call_refuses(hip_device):
    from pika_amd.rnnt import rnnt_align
    B, T, U, V = 4, 50, 10, 24
    lp, y, tl, ul = make_case(B, T, U, V, seed=0, ragged=True)
    stat = _dev(hip_device, lp, y, tl, ul)
    rnnt_align(*stat)                                          # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gs, gf = rnnt_align(*stat)
            with pytest.raises(RuntimeError, match="stream capture"):
                rnnt_align(stat[0].reshape(-1, V), stat[1].reshape(-1), stat[2], stat[3], compact=True)
    torch.cuda.current_stream().wait_stream(side)
    for seed in (1, 2):
        fresh = make_case(B, T, U, V, seed=seed, ragged=True)
        for dst, src in zip(stat, fresh):
            dst.copy_(torch.from_numpy(src))
        graph.replay()
        torch.cuda.synchronize()
        es, ef = rnnt_align(*stat)
        assert torch.equal(gs, es) and torch.equal(gf, ef)
        _check(_refs(*fresh), es.cpu().numpy(), ef.cpu().numpy(), fresh[3], None, "replay %d" % seed)


@pytest.mark.parametrize("U", [10, 90])
def test_infeasible_transcript_returns_a_valid_path(hip_device, U):
    from pika_amd.rnnt import rnnt_align
    B, T, V = 3, 40, 24
    lp, y, tl, ul = make_case(B, T, U, V, seed=1, ragged=True)
    tl[2], ul[2] = T - 3, U
    y[2] = np.random.default_rng(0).integers(1, V, U)
    y[0, U // 2] = V + 3                                       # a label outside [0, V): the loss takes it as log zero
    y[2, 0] = V
    y[2, U - 1] = 2 ** 30
    scores, frames = rnnt_align(*_dev(hip_device, lp, y, tl, ul))
    scores, frames = scores.cpu().numpy(), frames.cpu().numpy()
    for n in range(B):
        assert A.valid_frames(frames[n, :ul[n]], tl[n]) and (frames[n, ul[n]:] == -1).all()
    assert scores[0] <= NEG / 2 and scores[2] <= NEG / 2
    r = Ref(*A.planes(lp, y, 1, tl[1], ul[1]))                 # the feasible neighbour is untouched
    assert abs(float(scores[1]) - r.score) <= r.bound
