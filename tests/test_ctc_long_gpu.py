"""GPU checks of the long-form alignment (pika_amd.ctc.ctc_long_align*, csrc/ctc_long.hip) against the numpy fp32 reference
of its contract (tests/ctc_long_common.py), at the smallest shapes at which the tiling can go wrong: with W =
LONG_ALIGN_TILE owned states per tile and F = LONG_ALIGN_FRAMES frames per launch, S = 2U+1 in {W-1, W+1, 2W+1, 2W+3}
(S is odd, so W and 2W themselves cannot occur) and T in {U + repeats, F, F+1, 2F+1, a multiple of F, about 2.5 U}.
Paths, times and token scores must be equal bit for bit; scores within 2 ulp of the reference's fp64 figure."""
import functools

import numpy as np
import pytest
import torch

import ctc_common as R
import ctc_long_common as L

pytestmark = pytest.mark.gpu
W, F = 896, 64      # asserted against the package below


def _geometry():
    from pika_amd import ctc
    assert (ctc.LONG_ALIGN_TILE, ctc.LONG_ALIGN_FRAMES) == (W, F)


def _labels(rng, U, C):
    return rng.integers(1, C, size=U)


def _needed(seq):
    seq = list(seq)
    return len(seq) + sum(a == b for a, b in zip(seq, seq[1:]))


def _log_probs(rng, T, B, C):
    return torch.log_softmax(torch.from_numpy(rng.normal(size=(T, B, C)) * 3.0), -1).float().numpy()


class Case(object):
    def __init__(self, name, x, targets, ils, tls, blank=0):
        self.name, self.x, self.targets, self.ils, self.tls, self.blank = name, x, targets, ils, tls, blank
        self.T, self.B, self.C = x.shape

    @functools.lru_cache(maxsize=None)
    def ref(self):
        return L.batch_reference(self.x, self.targets, self.ils, self.tls, self.blank)


@functools.lru_cache(maxsize=None)
def exact_cases():
    """Random log-probs, garbage beyond every length: NaN rows beyond T_b, wild tokens beyond U_b."""
    rng = np.random.default_rng(2024)
    out = []
    # (name, C, [(T_b, U_b)]): the first recording sets T and U_max
    plans = [
        ("S=W-1,T=tight", 5, [(None, (W - 2) // 2)]),
        ("S=W+1,T=2.5U|F+1", 4, [(int(2.5 * (W // 2)), W // 2), (F + 1, 30)]),
        ("S=2W+1,T=35F", 3, [(35 * F, W)]),
        ("S=2W+3,T=2.5U|2F+1|F", 7, [(int(2.5 * (W + 1)) + 1, W + 1), (2 * F + 1, 50), (F, 0)]),
        ("S=2W+3,T=tight", 6, [(None, W + 1)]),
    ]
    for name, C, rows in plans:
        seqs = [_labels(rng, U, C) for _, U in rows]
        ils = [(_needed(s) if T is None else T) for (T, _), s in zip(rows, seqs)]
        T, U_max, B = ils[0], rows[0][1], len(rows)
        x = _log_probs(rng, T, B, C)
        targets = rng.integers(-9, 10 ** 6, size=(B, U_max))
        for b, s in enumerate(seqs):
            x[ils[b]:, b] = np.nan
            targets[b, :len(s)] = s
        out.append(Case(name, x, targets, ils, [len(s) for s in seqs]))
    return out


def _run(fn, case, dev, x=None, lengths_on_device=False, **kw):
    x = torch.from_numpy(case.x).to(dev) if x is None else x
    il, tl = torch.tensor(case.ils, dtype=torch.int32), torch.tensor(case.tls, dtype=torch.int64)
    if lengths_on_device:
        il, tl = il.to(dev), tl.to(dev)
    out = fn(x, torch.from_numpy(case.targets).to(dev), il, tl, blank=case.blank, **kw)
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.int32, torch.float32]
    assert out[0].shape == (case.B,) and all(o.shape == (case.B, case.targets.shape[1]) for o in out[1:])
    return [o.cpu().numpy() for o in out]


def _ulp_close(got, want64, ulps=2):
    want64 = np.asarray(want64, dtype=np.float64)
    fin = np.isfinite(want64)
    assert (got[~fin] == want64[~fin]).all()
    tol = ulps * np.spacing(np.abs(want64[fin]).astype(np.float32)).astype(np.float64)
    assert (np.abs(got[fin].astype(np.float64) - want64[fin]) <= tol).all(), (got, want64)


def _same(got, want):
    for g, w, what in zip(got[1:], want[1:], ("starts", "ends", "token_scores")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


@pytest.mark.parametrize("index", range(5))
def test_paths_times_and_token_scores_equal_the_fp32_reference(hip_device, index):
    from pika_amd import ctc
    _geometry()
    case = exact_cases()[index]
    results, scores, starts, ends, tscores = case.ref()
    assert all(r.path is not None for r in results), case.name      # every recording of these cases is feasible
    got = _run(ctc.ctc_long_align, case, hip_device)
    print("CTCLONG %s T=%d B=%d U_max=%d ties=%s" % (case.name, case.T, case.B, case.targets.shape[1],
                                                    [r.ties for r in results]))
    _same(got, (scores, starts, ends, tscores))                     # no exemptions
    _ulp_close(got[0], [r.score64 for r in results])
    if case.B == 1:     # the unbatched form
        one = ctc.ctc_long_align(torch.from_numpy(case.x[:, 0]).to(hip_device), torch.from_numpy(case.targets[0]), None, None)
        assert one[0].shape == () and one[1].shape == (case.targets.shape[1],)
        assert all(o.cpu().numpy().tobytes() == g.tobytes() for o, g in zip(one, got))


@functools.lru_cache(maxsize=None)
def tie_case():
    """Dyadic inputs, C = 3, few distinct values: a tied cell in every (tile, block), a tied REACHABLE cell in every one
    that holds reachable cells.  Asserted here, from the reference's own maps."""
    rng = np.random.default_rng(77)
    U = W + 20                  # S = 2W + 41: three tiles, the last a sliver
    seq = _labels(rng, U, 3)
    T = 36 * F - 5              # about 2.5 U; the last block is nearly full
    x = L.dyadic(rng, (T, 1, 3), kmax=640, step=64)
    ref = L.reference(x[:, 0], [int(c) for c in seq], 0, maps=True)
    assert ref.path is not None
    S = 2 * U + 1
    for t0 in range(0, T, F):
        for s0 in range(0, S, W):
            tied, live = ref.tied[max(t0, 1):t0 + F, s0:s0 + W], ref.live[max(t0, 1):t0 + F, s0:s0 + W]
            assert tied.any(), (t0, s0)
            assert not live.any() or (tied & live).any(), (t0, s0)
    assert min(ref.kinds) > 0           # each of the three preferences decides a cell ON the path
    return Case("ties", x, seq[None, :].copy(), [T], [U]), ref


def test_ties_in_every_tile_and_block(hip_device):
    from pika_amd import ctc
    _geometry()
    case, ref = tie_case()
    got = _run(ctc.ctc_long_align, case, hip_device)
    assert got[1][0].tolist() == ref.starts.tolist() and got[2][0].tolist() == ref.ends.tolist()
    assert got[3][0].tobytes() == ref.token_scores.tobytes()
    assert float(got[0][0]) == ref.score64      # dyadic: exact


@pytest.mark.parametrize("U", [(W - 2) // 2, W // 2])
def test_agreement_with_ctc_align_on_dyadic_inputs(hip_device, U):
    from pika_amd import ctc
    _geometry()
    assert U <= 511
    rng = np.random.default_rng(U)
    B, C = 2, 4
    T = int(1.6 * U)
    seqs = [_labels(rng, U, C), _labels(rng, U - 37, C)]
    ils = [T, T - 90]
    assert all(_needed(s) <= t for s, t in zip(seqs, ils))
    x = L.dyadic(rng, (T, B, C))
    targets = np.zeros((B, U), dtype=np.int64)
    for b, s in enumerate(seqs):
        targets[b, :len(s)] = s
    case = Case("dyadic", x, targets, ils, [len(s) for s in seqs])
    got = _run(ctc.ctc_long_align, case, hip_device)
    scores, labels = ctc.ctc_align(torch.from_numpy(x).to(hip_device), torch.from_numpy(targets), torch.tensor(ils),
                                   torch.tensor(case.tls))
    scores, labels = scores.cpu().numpy(), labels.cpu().numpy()
    for b, s in enumerate(seqs):
        implied = L.frame_labels(got[1][b], got[2][b], s, ils[b])
        assert implied.tolist() == labels[b, :ils[b]].tolist(), b
        assert got[0][b] == scores[b], (b, got[0][b], scores[b])


def test_logits_form(hip_device):
    from pika_amd import ctc
    _geometry()
    dev = hip_device
    # dyadic logits: the recurrence runs on logit - maxlogit, whatever lse is -- the paths of the two forms are the same
    case, ref = tie_case()
    a = _run(ctc.ctc_long_align, case, dev)
    b = _run(ctc.ctc_long_align_from_logits, case, dev)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    # random logits across a tile edge: against the float64 Viterbi of log_softmax, with the allowance
    # tests/test_ctc_gpu.py makes for ctc_align_from_logits; token scores against logit - lse summed in float64
    rng = np.random.default_rng(9)
    T, U, C = 1100, W // 2, 5
    seq = _labels(rng, U, C)
    logits = torch.from_numpy(rng.normal(size=(T, 1, C)) * 3.0).float()
    lp64 = torch.log_softmax(logits.double(), -1).numpy()[:, 0]
    score, labels, path, delta = R.viterbi(lp64, seq, 0)
    bound = R.bound(delta, T)
    tol = 3 * bound + T * 2 ** -22 * float(logits.abs().max() + np.log(C))
    got = ctc.ctc_long_align_from_logits(logits.to(dev), torch.from_numpy(seq)[None], [T], [U])
    got = [g.cpu().numpy() for g in got]
    assert abs(float(got[0][0]) - score) <= tol + 1e-12, (got[0][0], score, tol)
    implied = L.frame_labels(got[1][0], got[2][0], seq, T)
    assert R.collapse(implied, 0) == seq.tolist()
    assert abs(R.rescore(lp64, implied) - score) <= tol + 1e-12
    if R.margin(lp64, seq, 0) > 2 * tol:
        assert implied.tolist() == labels.tolist()
    for j in range(0, U, 17):
        want = lp64[got[1][0][j]:got[2][0][j] + 1, seq[j]].sum()
        n = got[2][0][j] - got[1][0][j] + 1
        assert abs(got[3][0][j] - want) <= n * 2 ** -22 * (abs(want) + float(logits.abs().max()) + np.log(C)) + 1e-6


def test_ragged_batches_ignore_what_lies_beyond_the_lengths(hip_device):
    from pika_amd import ctc
    _geometry()
    case = exact_cases()[3]     # T_b = (2.5 U, 2F+1, F), U_b = (W+1, 50, 0); NaN rows and wild tokens beyond them
    assert case.tls[2] == 0 and np.isnan(case.x[case.ils[1]:, 1]).all() and case.targets[1, case.tls[1]:].max() > case.C
    dirty = _run(ctc.ctc_long_align, case, hip_device, lengths_on_device=True)
    clean = Case("clean", np.nan_to_num(case.x, nan=0.0), case.targets.copy(), case.ils, case.tls)
    for b in range(case.B):
        clean.targets[b, case.tls[b]:] = 1
    got = _run(ctc.ctc_long_align, clean, hip_device)
    assert all(d.tobytes() == g.tobytes() for d, g in zip(dirty, got))
    _same(dirty, case.ref()[1:])
    # beyond a length: -1, -1, -inf
    for b in range(case.B):
        assert (dirty[1][b, case.tls[b]:] == -1).all() and (dirty[2][b, case.tls[b]:] == -1).all()
        assert np.isneginf(dirty[3][b, case.tls[b]:]).all()
    # lengths beyond the tensors are clamped: the full-length call
    full = Case("full", clean.x, clean.targets, [10 ** 6] * case.B, [10 ** 6] * case.B)
    a = _run(ctc.ctc_long_align, full, hip_device)
    b = ctc.ctc_long_align(torch.from_numpy(clean.x).to(hip_device), torch.from_numpy(clean.targets))
    assert all(p.tobytes() == q.cpu().numpy().tobytes() for p, q in zip(a, b))


def test_infeasible_rows_leave_their_neighbours_alone(hip_device):
    from pika_amd import ctc
    _geometry()
    rng = np.random.default_rng(31)
    T, U, C = 700, W // 2 + 12, 5       # two tiles
    base = _labels(rng, U, C)
    assert _needed(base) <= T

    def batch(rows):
        targets = np.stack([r[0] for r in rows])
        return Case("infeasible", x, targets, [r[1] for r in rows], [U] * 3)
    x = _log_probs(rng, T, 3, C)
    spoil = lambda j, v: np.concatenate([base[:j], [v], base[j + 1:]])      # noqa: E731
    batches = [batch([(base, T), (spoil(U - 3, C), T), (spoil(5, -1), T)]),
               batch([(spoil(W // 2 + 3, 0), T), (base, T), (base, U - 1)]),
               batch([(spoil(0, 2 ** 31 - 1), T), (spoil(U - 1, -2 ** 31), T), (base, T - 1)])]
    feasible = [[True, False, False], [False, True, False], [False, False, True]]
    for case, ok in zip(batches, feasible):
        got = _run(ctc.ctc_long_align, case, hip_device)
        results, scores, starts, ends, tscores = case.ref()
        assert [r.path is not None for r in results] == ok
        _same(got, (scores, starts, ends, tscores))
        _ulp_close(got[0], [r.score64 for r in results])
        for b in range(3):
            if not ok[b]:
                assert np.isneginf(got[0][b]) and (got[1][b] == -1).all() and (got[2][b] == -1).all()
                assert np.isneginf(got[3][b]).all()
        logits = _run(ctc.ctc_long_align_from_logits, case, hip_device)
        assert logits[1].tobytes() == got[1].tobytes() and np.isneginf(logits[0]).tolist() == [not o for o in ok]


def test_strides(hip_device):
    from pika_amd import ctc
    _geometry()
    case = exact_cases()[1]
    want = _run(ctc.ctc_long_align, case, hip_device)
    x = torch.from_numpy(case.x).to(hip_device)
    transposed = x.permute(1, 0, 2).contiguous().permute(1, 0, 2)           # (B,T,C) storage
    wide = torch.full((case.T, case.B + 1, case.C + 3), float("nan"), device=hip_device)
    wide[:, :case.B, :case.C] = x
    sliced = wide[:, :case.B, :case.C]
    assert not transposed.is_contiguous() and not sliced.is_contiguous() and sliced.stride(2) == 1
    for view in (transposed, sliced):
        for fn in (ctc.ctc_long_align, ctc.ctc_long_align_from_logits):
            got = _run(fn, case, hip_device, x=view)
            ref = want if fn is ctc.ctc_long_align else _run(fn, case, hip_device)
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, ref))


def test_determinism_and_graph_capture(hip_device):
    from pika_amd import ctc
    _geometry()
    dev = hip_device
    rng = np.random.default_rng(55)
    T, U, C, B = 2 * F + 1, W // 2 + 4, 5, 2         # three frame blocks, two tiles
    T = max(T, 700)
    data = []
    for i in range(3):
        seqs = [_labels(rng, U - 3 * i, C), _labels(rng, 40 + i, C)]
        targets = np.ones((B, U), dtype=np.int64)
        for b, s in enumerate(seqs):
            targets[b, :len(s)] = s
        data.append((_log_probs(rng, T, B, C), targets, [T - 7 * i, 2 * F + 1 - i], [len(s) for s in seqs]))

    def dev_args(d):
        return (torch.from_numpy(d[0]).to(dev), torch.from_numpy(d[1]).to(dev),
                torch.tensor(d[2], dtype=torch.int32, device=dev), torch.tensor(d[3], dtype=torch.int32, device=dev))
    static = dev_args(data[0])
    first = ctc.ctc_long_align(*static)
    again = ctc.ctc_long_align(*static)
    assert all(torch.equal(a, b) or (a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()) for a, b in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctc.ctc_long_align_from_logits(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ctc.ctc_long_align(*static) + ctc.ctc_long_align_from_logits(*static)
    for d in data[1:] + data[:1]:
        for s, n in zip(static, dev_args(d)):
            s.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        eager = ctc.ctc_long_align(*dev_args(d)) + ctc.ctc_long_align_from_logits(*dev_args(d))
        for o, e in zip(outs, eager):
            assert o.cpu().numpy().tobytes() == e.cpu().numpy().tobytes()
        _same([o.cpu().numpy() for o in outs[:4]], L.batch_reference(d[0], d[1], d[2], d[3])[1:])


def test_segment_scores_on_device_outputs(hip_device):
    from pika_amd import ctc
    _geometry()
    case = exact_cases()[1]
    x = torch.from_numpy(case.x).to(hip_device)
    _, starts, ends, ts = ctc.ctc_long_align(x, torch.from_numpy(case.targets), case.ils, case.tls)
    U = case.targets.shape[1]
    offsets = torch.tensor([[0, 100, 100, 300, U], [0, 7, 30, 31, 40]])
    on_device = ctc.ctc_segment_scores(starts, ends, ts, offsets.to(hip_device))
    on_host = ctc.ctc_segment_scores(starts.cpu(), ends.cpu(), ts.cpu(), offsets)
    assert all(d.is_cuda for d in on_device)
    for d, h in zip(on_device[:2], on_host[:2]):
        assert torch.equal(d.cpu(), h)
    assert torch.allclose(on_device[2].cpu(), on_host[2], rtol=1e-6, atol=0, equal_nan=True)
    for b in range(2):
        want = L.segment_loop(starts[b].cpu().numpy(), ends[b].cpu().numpy(), ts[b].cpu().numpy(), offsets[b].tolist())
        assert on_host[0][b].tolist() == want[0] and on_host[1][b].tolist() == want[1]
        assert np.allclose(on_host[2][b].numpy(), want[2], rtol=1e-6, equal_nan=True)
    assert on_host[0][0, 1] == -1 and torch.isnan(on_host[2][0, 1])      # the empty segment
    assert on_host[0][1, 3] == -1 and torch.isnan(on_host[2][1, 3])      # tokens beyond the second recording's length
