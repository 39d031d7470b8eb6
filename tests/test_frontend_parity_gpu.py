"""The audio front end (pika_amd/csrc/audio.hip through pika_amd/loader/frontend.py and the C ABI) against its fp64
oracle (oracle/fbank_ref.py) and plain numpy, across the configurations, waveforms and shapes the kernels take as
ARGUMENTS: every fbank geometry `FbankConfig` can derive (nfft 256 / 512 / 1024, other banks, no pre-emphasis), the
dither generator as a distribution, splice / subsample / pad bit for bit, perturbation at its edges and the "same"
convolution at the shapes around one workgroup and one chunk of taps.  Helpers, the waveform zoo and the fp32 restatement
of the oracle that sizes the fbank tolerance: tests/frontend_common.py (CPU only)."""
import numpy as np
import pytest
import torch

import frontend_common as C
from oracle import fbank_ref as F

pytestmark = pytest.mark.gpu
EINVAL = -1
CANARY = 0x5A5AA5A5          # as float32: 1.5388e+16, nothing a kernel here would write


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _offsets(counts, dev):
    return _dev(np.concatenate(([0], np.cumsum(counts))).astype(np.int64), dev)


def _canary(shape, dev):
    return torch.full(shape, CANARY, dtype=torch.int32, device=dev)


def _front_end(name, dev, dither=0.0, **kw):
    from pika_amd.loader.frontend import GpuFrontEnd
    kw.setdefault("lctx", 0)
    kw.setdefault("rctx", 0)
    kw.setdefault("stride", 1)
    return GpuFrontEnd(C.fbank_config(name, dither), dev, **kw)


def _fbank_abi(dev, cfg, waves, dither=0.0, seed=0):
    """pika_fbank through ctypes on float waveforms: (return code, feats (total_frames, bins) as numpy)."""
    from pika_amd import _lib
    frames = [cfg.num_frames(len(w)) for w in waves]
    total = int(sum(frames))
    wave = _dev(np.concatenate(waves).astype(np.float32), dev)
    w_off, f_off = _offsets([len(w) for w in waves], dev), _offsets(frames, dev)
    plan = [_dev(a, dev) for a in cfg.mel_plan()]
    feats = torch.empty((max(total, 1), cfg.num_mel_bins), dtype=torch.float32, device=dev)
    rc = _lib.lib().pika_fbank(wave.data_ptr(), w_off.data_ptr(), f_off.data_ptr(), len(waves), total, cfg.frame_len,
                               cfg.shift, cfg.nfft, cfg.preemphasis_coefficient, dither, seed, cfg.num_mel_bins,
                               *[p.data_ptr() for p in plan], feats.data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    return rc, feats[:total].cpu().numpy()


# ---------------- 1. pika_fbank x configurations x waveforms -------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_fbank_matches_oracle_in_every_configuration(hip_device, name):
    """One batch per configuration holding the whole zoo; each utterance against the fp64 oracle with
    tol = max(2e-3, 4 * |fp32 restatement of the oracle - oracle|).  The restatement decides the bound for two pairs only
    (short window: chirp, square wave), asserted on the CPU before anything is compared.  Prints the measured error per
    pair (copied into DESIGN.md)."""
    wide = C.check_restatement_condition()
    assert {w[:2] for w in wide} <= {("short_window", "chirp"), ("short_window", "square")}
    cfg = C.fbank_config(name)
    assert (cfg.frame_len, cfg.shift, cfg.nfft) == C.GEOMETRY[name]
    zoo, tables = C.waveforms(name), C.reference_tables(name)
    fe = _front_end(name, hip_device)
    data, lens = fe(list(zoo.values()), [1.0] * len(zoo), [0.0] * len(zoo), perturb=False)
    data = data.cpu().numpy()
    assert lens == [t[0].shape[0] for t in tables.values()] and lens[-1] == 0 and lens[-2] == lens[-3] == 1
    assert data.shape == (len(zoo), max(lens), cfg.num_mel_bins)
    failures = []
    for b, (wname, (ref, rest_err, tol)) in enumerate(tables.items()):
        got = data[b, :lens[b]]
        err = float(np.abs(got - ref).max()) if lens[b] else 0.0
        print("fbank %-18s %-14s frames %3d  gpu %.2e  restatement %.2e  tol %.2e"
              % (name, wname, lens[b], err, rest_err, tol))
        if not (np.isfinite(got).all() and err <= tol):
            failures.append((wname, err, tol))
        if lens[b]:      # padding repeats the last frame; an entry without a frame stays zero
            assert np.array_equal(data[b, lens[b]:], np.repeat(got[-1:], data.shape[1] - lens[b], 0))
        else:
            assert not data[b].any()
    assert not failures, failures
    # DC only: nothing is left after the mean is removed, every bin sits on the floor (oracle: exactly)
    floor = np.log(np.float64(np.finfo(np.float32).eps))
    assert np.all(tables["dc"][0] == floor) and np.abs(data[list(zoo).index("dc")] - floor).max() <= C.LOGMEL_ATOL


@pytest.mark.parametrize("name", list(C.CONFIGS))
def test_fbank_ill_conditioned_frame_in_mel_energies(hip_device, name):
    """DC 20000 + noise of sigma 1: the mean takes all but a few bits of each sample and the log of the nearly empty bins
    amplifies what is left (the fp32 restatement of the oracle is up to 4e-2 from fp64 in the log domain).  Asserted on
    the mel ENERGIES relative to the frame's largest: |E_gpu - E_ref| / max_bin E_ref <= 4 x the restatement's value."""
    kw = C.oracle_kwargs(name)
    pcm = C.ill_conditioned(name)
    ref = F.kaldi_fbank(pcm.astype(np.float64), **kw)
    rest = C.relative_energy_error(C.kaldi_fbank_f32(pcm, **kw), ref)
    assert 1e-7 < rest < 1e-3, rest             # the input is ill-conditioned, not hopeless
    fe = _front_end(name, hip_device)
    data, lens = fe([pcm], [1.0], [0.0], perturb=False)
    got = data[0].cpu().numpy()
    assert lens == [ref.shape[0]] and np.isfinite(got).all()
    err = C.relative_energy_error(got, ref)
    print("fbank %-18s ill-conditioned: relative mel-energy error gpu %.2e  restatement %.2e  (log domain: gpu %.2e)"
          % (name, err, rest, np.abs(got - ref).max()))
    assert err <= C.RESTATEMENT_MARGIN * rest, (err, rest)


def test_fbank_entry_refuses_sizes_it_has_no_kernel_for(hip_device):
    """Argument checks made before any launch; nothing here reaches a kernel with an out-of-range size."""
    from pika_amd import _lib
    lib, dev = _lib.lib(), hip_device
    cfg = C.fbank_config("recipe")
    plan = [_dev(a, dev) for a in cfg.mel_plan()]
    wave = torch.zeros(4096, dtype=torch.float32, device=dev)
    w_off, f_off = _offsets([4096], dev), _offsets([1], dev)
    out = _canary((8, 80), dev)

    def call(total=1, frame_len=400, shift=160, nfft=512, bins=80):
        return lib.pika_fbank(wave.data_ptr(), w_off.data_ptr(), f_off.data_ptr(), 1, total, frame_len, shift, nfft, 0.97,
                              0.0, 0, bins, *[p.data_ptr() for p in plan], out.data_ptr(), _stream(dev))
    assert call(nfft=500) == EINVAL             # not a power of two
    assert call(nfft=256) == EINVAL             # nfft < frame_len
    assert call(nfft=2048) == EINVAL            # beyond the LDS buffers
    assert call(frame_len=1, nfft=2) == EINVAL  # the window divides by frame_len - 1
    assert call(bins=0) == EINVAL
    assert call(total=0) == 0                   # an empty batch is not an error and launches nothing
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    assert call() == 0                          # the same call with sane sizes does write
    torch.cuda.synchronize()
    assert bool((out[0] != CANARY).all()) and bool((out[1:] == CANARY).all())


# ---------------- 2. dither ----------------------------------------------------------------------------------------
DITHER_SAMPLES = 1600000      # 100 s: 9998 frames per utterance


def _assert_dither_sample_matches(got, oracle, what):
    p = C.ks_min_p(got, oracle)
    print("dither %s: smallest per-bin KS p-value %.3g over %d + %d frames" % (what, p, len(got), len(oracle)))
    assert p > C.KS_P_MIN, (what, p)


def test_dither_is_the_oracles_distribution_and_independent(hip_device):
    """Silence in, dither 1: per mel bin the log-mel sample has the oracle's distribution (two-sample KS, p > 1e-6 per bin:
    family-wise false alarm below 1e-4), adjacent frames are uncorrelated and so are the two utterances of the batch
    (|r| < 5 / sqrt(n) per bin)."""
    kw = C.oracle_kwargs("recipe")
    silence = np.zeros(DITHER_SAMPLES, np.int16)
    fe = _front_end("recipe", hip_device, dither=1.0)
    data, lens = fe([silence, silence], [1.0, 1.0], [0.0, 0.0], perturb=False)
    n = lens[0]
    assert lens == [9998, 9998]
    oracle = C.oracle_dither_sample(2 * n, seed=11, **kw)
    other = C.oracle_dither_sample(2 * n, seed=12, **kw)
    assert C.ks_min_p(oracle, other) > C.KS_P_MIN          # the criterion passes the oracle against itself
    assert C.ks_min_p(oracle, other + np.log(1.21)) < C.KS_P_MIN   # and sees a variance off by 10 %
    got = data.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    _assert_dither_sample_matches(got.reshape(2 * n, -1), oracle, "front end, 2 x 100 s of silence")
    bound = 5.0 / np.sqrt(n - 1)
    for b in range(2):
        r = C.column_correlations(got[b, :-1], got[b, 1:])
        print("dither utterance %d: largest |r| between adjacent frames %.4f (bound %.4f)" % (b, np.abs(r).max(), bound))
        assert np.abs(r).max() < bound
    r = C.column_correlations(got[0], got[1])
    print("dither: largest |r| between the two utterances, frame by frame %.4f" % np.abs(r).max())
    assert np.abs(r).max() < 5.0 / np.sqrt(n)


def test_dither_seed_through_the_abi(hip_device):
    """Same seed -> the same bits; one low (batch) bit or one bit of the high (instance) field changed -> other noise of
    the same distribution."""
    kw = C.oracle_kwargs("recipe")
    cfg = C.fbank_config("recipe")
    waves = [np.zeros(DITHER_SAMPLES, np.float32)] * 2
    seed = (5 << 40) | (3 << 32) | 77
    rc, a = _fbank_abi(hip_device, cfg, waves, 1.0, seed)
    rc2, a2 = _fbank_abi(hip_device, cfg, waves, 1.0, seed)
    assert rc == 0 and rc2 == 0 and np.array_equal(a.view(np.uint32), a2.view(np.uint32))
    oracle = C.oracle_dither_sample(len(a), seed=13, **kw)
    for what, other in (("low bit", seed ^ 1), ("instance bit", seed ^ (1 << 32)), ("base-seed bit", seed ^ (1 << 40))):
        rc, b = _fbank_abi(hip_device, cfg, waves, 1.0, other)
        assert rc == 0 and (a != b).mean() > 0.999, what
        r = C.column_correlations(a.astype(np.float64), b.astype(np.float64))
        assert np.abs(r).max() < 5.0 / np.sqrt(len(a)), what
        _assert_dither_sample_matches(b.astype(np.float64), oracle, "seed with another " + what)


def test_dither_scale_on_silence(hip_device):
    """dither 0.5 on silence: every energy is a quarter of dither 1's, so the whole distribution moves by log 4 -- the
    scale factor, where nothing else is in the signal.  Same criteria as above against the oracle at dither 0.5."""
    kw = C.oracle_kwargs("recipe")
    cfg = C.fbank_config("recipe")
    rc, got = _fbank_abi(hip_device, cfg, [np.zeros(DITHER_SAMPLES, np.float32)], 0.5, 99)
    assert rc == 0
    got = got.astype(np.float64)
    oracle = C.oracle_dither_sample(len(got), seed=14, dither=0.5, **kw)
    full = C.oracle_dither_sample(len(got), seed=15, dither=1.0, **kw)
    assert C.ks_min_p(oracle, full) < C.KS_P_MIN           # the criterion tells dither 0.5 from dither 1
    _assert_dither_sample_matches(got, oracle, "0.5 on silence")
    tol = 5.0 * oracle.std(0, ddof=1) * np.sqrt(2.0 / len(got))    # two independent sample means
    assert np.all(np.abs(got.mean(0) - oracle.mean(0)) <= tol)
    assert np.all(np.abs(got.mean(0) - full.mean(0)) > tol)


def test_dither_scale_on_the_1khz_tone(hip_device):
    """dither 0.5 on the 1 kHz tone (amplitude 30000): mean log-mel per bin against the oracle with the same dither,
    within 5 sigma / sqrt(n) from the oracle's own per-bin variance over the n frames.  Measured on the MI355X: tolerance
    1.3e-6 .. 6.3e-4 per bin, |difference| 3.0e-7 .. 3.5e-4, largest ratio 0.94.  The tone's leakage is 20 dB and more above
    the dither in every bin, so this pins the mean under a loud signal; the scale factor itself is pinned by
    test_dither_scale_on_silence (the oracle at dither 0.5 and at dither 1 pass this one against each other)."""
    kw = C.oracle_kwargs("recipe")
    cfg = C.fbank_config("recipe")
    tone = C.waveforms("recipe")["tone_1k"]
    oracle = F.kaldi_fbank(tone.astype(np.float64), dither=0.5, rng=np.random.default_rng(16), **kw)
    rc, got = _fbank_abi(hip_device, cfg, [tone.astype(np.float32)], 0.5, 123)
    assert rc == 0 and got.shape == oracle.shape
    n = len(oracle)
    tol = 5.0 * oracle.std(0, ddof=1) / np.sqrt(n)
    diff = np.abs(got.astype(np.float64).mean(0) - oracle.mean(0))
    print("dither 0.5 on the tone: n %d, tolerance per bin %.2e .. %.2e, |mean difference| %.2e .. %.2e, "
          "largest ratio %.2f, bins over %d" % (n, tol.min(), tol.max(), diff.min(), diff.max(), (diff / tol).max(),
                                               int((diff > tol).sum())))
    assert np.all(diff <= tol), (diff / tol).max()


# ---------------- 3. pika_splice_pad, exactly --------------------------------------------------------------------------
def _splice_abi(dev, x, counts, dim, lctx, rctx, stride, t_max):
    from pika_amd import _lib
    feats = _dev(x, dev)
    f_off = _offsets(counts, dev)
    out = _canary((len(counts), t_max, dim * (lctx + 1 + rctx)), dev)
    rc = _lib.lib().pika_splice_pad(feats.data_ptr(), f_off.data_ptr(), len(counts), dim, lctx, rctx, stride, t_max,
                                    out.data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy().view(np.uint32)


def _assert_splice_exact(got, x, counts, lctx, rctx, stride, t_max, tag):
    off = np.concatenate(([0], np.cumsum(counts)))
    for b, n in enumerate(counts):
        if n == 0:
            assert np.all(got[b] == CANARY), (tag, b)         # untouched: the caller's fill stays
            continue
        want = C.splice_pad_expected(x[off[b]:off[b + 1]], lctx, rctx, stride, t_max)
        assert np.array_equal(got[b], want.view(np.uint32)), (tag, b, n)


CONTEXTS = [(0, 0, 1), (1, 1, 1), (2, 1, 3), (5, 5, 1), (0, 3, 4), (3, 0, 7)]


@pytest.mark.parametrize("dim", [1, 23, 80, 257])
def test_splice_pad_is_exact(hip_device, dim):
    """Bit equality with F.splice(x, l, r)[::stride] padded by its last row: utterances shorter than the context and than
    the stride, n % stride in {0, 1, stride - 1}, t_max at and beyond the longest; dim 257 x 3 columns takes three passes of
    the 256-thread loop."""
    rng = np.random.default_rng(dim)
    for lctx, rctx, stride in CONTEXTS:
        counts = [n for n in (1, 2, stride - 1, stride, stride + 1, 3 * stride, 50) if n > 0]
        x = rng.standard_normal((sum(counts), dim)).astype(np.float32)
        longest = max((n + stride - 1) // stride for n in counts)
        for t_max in (longest, longest + 5):
            got = _splice_abi(hip_device, x, counts, dim, lctx, rctx, stride, t_max)
            _assert_splice_exact(got, x, counts, lctx, rctx, stride, t_max, (dim, lctx, rctx, stride, t_max))


@pytest.mark.parametrize("counts", [[0, 5, 3], [5, 0, 3], [5, 0, 0, 3], [5, 3, 0], [0, 1, 0, 0, 9, 0]])
def test_splice_pad_leaves_entries_without_a_frame_alone(hip_device, counts):
    rng = np.random.default_rng(len(counts))
    for dim in (23, 257):
        for lctx, rctx, stride in CONTEXTS[1:]:
            x = rng.standard_normal((sum(counts), dim)).astype(np.float32)
            t_max = max((n + stride - 1) // stride for n in counts) + 2
            got = _splice_abi(hip_device, x, counts, dim, lctx, rctx, stride, t_max)
            _assert_splice_exact(got, x, counts, lctx, rctx, stride, t_max, (dim, lctx, rctx, stride))


@pytest.mark.parametrize("empty", [(0,), (2,), (1, 2), (4,), (0, 2, 3)])
def test_front_end_batches_with_entries_too_short_for_a_frame(hip_device, empty):
    """Utterances below one frame first, in the middle, twice in a row and last: length 0 and zero rows for them, and the
    fbank kernel's utterance search steps over them -- the others equal the oracle, spliced, exactly as when alone."""
    rng = np.random.default_rng(7)
    kw = C.oracle_kwargs("recipe")
    pcms = [C._i16(rng.standard_normal(n) * 2500) for n in (3000, 1234, 5000, 400, 2000)]
    for b in empty:
        pcms[b] = pcms[b][:int(rng.integers(0, 400))]
    lctx, rctx, stride = 2, 1, 3
    fe = _front_end("recipe", hip_device, lctx=lctx, rctx=rctx, stride=stride)
    data, lens = fe(pcms, [1.0] * 5, [0.0] * 5, perturb=False)
    data = data.cpu().numpy()
    for b, pcm in enumerate(pcms):
        if b in empty:
            assert lens[b] == 0 and not data[b].any()
            continue
        ref = F.kaldi_fbank(pcm.astype(np.float64), **kw)
        rest_err = np.abs(C.kaldi_fbank_f32(pcm, **kw) - ref).max()
        tol = max(C.LOGMEL_ATOL, C.RESTATEMENT_MARGIN * rest_err)
        assert tol == C.LOGMEL_ATOL
        want = F.splice(ref, lctx, rctx)[::stride]
        assert lens[b] == want.shape[0]
        assert np.abs(data[b, :lens[b]] - want).max() <= tol, b
        assert np.array_equal(data[b, lens[b]:], np.repeat(data[b, lens[b] - 1:lens[b]], data.shape[1] - lens[b], 0))


def test_front_end_batch_without_any_frame(hip_device):
    fe = _front_end("recipe", hip_device, lctx=1, rctx=1)
    pcms = [np.full(n, 1000, np.int16) for n in (399, 0, 17)]
    data, lens = fe(pcms, [1.0] * 3, [0.0] * 3, perturb=False)
    assert lens == [0, 0, 0] and tuple(data.shape) == (3, 1, 240) and not bool(data.any())


# ---------------- 4. pika_audio_perturb at its edges -------------------------------------------------------------------
def _perturb(dev, pcms, rates, dbs):
    fe = _front_end("recipe", dev)
    fe(pcms, rates, dbs)
    torch.cuda.synchronize()
    wave, off = fe.last_wave.cpu().numpy(), fe.last_offsets[1]
    return [wave[off[i]:off[i + 1]] for i in range(len(pcms))]


def _assert_perturbed(got, pcm, rate, db, tag):
    """Unchanged speed: the reference stays in float32 and takes a float32 mean where the kernel sums in fp64, so a sample
    may sit one LSB off, on fewer than 1e-3 of them (tests/test_frontend.py); any other rate is fp64 on both sides: exact."""
    want = F.perturb(pcm, rate, db).astype(np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    diff = np.abs(got - want)
    if rate == 1.0:
        assert diff.max(initial=0) <= 1 and (diff > 0).mean() < 1e-3, (tag, diff.max(), (diff > 0).mean())
    else:
        assert not diff.any(), (tag, diff.max(), (diff > 0).mean(), int(np.argmax(diff > 0)))


PERTURB_LENGTHS = [9, 10, 11, 400, 5000, 48000, 160001]


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_perturb_mixed_lengths_and_rates_in_one_batch(hip_device, shift):
    """Lengths 9 .. 160 001 in one batch (the grid is sized by the longest; the short ones ride on idle blocks), rates
    0.9 / 1.0 / 1.1 mixed; over the three parametrisations every length meets every rate."""
    rng = np.random.default_rng(40 + shift)
    pcms = [C._i16(rng.standard_normal(n) * 3000) for n in PERTURB_LENGTHS]
    rates = [(0.9, 1.0, 1.1)[(i + shift) % 3] for i in range(len(pcms))]
    dbs = [float(rng.uniform(-50, -20)) for _ in pcms]
    for i, got in enumerate(_perturb(hip_device, pcms, rates, dbs)):
        _assert_perturbed(got, pcms[i], rates[i], dbs[i], (len(pcms[i]), rates[i]))


def test_perturb_single_utterances_silence_and_square_wave(hip_device):
    rng = np.random.default_rng(50)
    t = np.arange(16000)
    square = np.where((t // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    for rate in (0.9, 1.0, 1.1):
        for n in (9, 5000):                                                 # B = 1
            pcm = C._i16(rng.standard_normal(n) * 3000)
            _assert_perturbed(_perturb(hip_device, [pcm], [rate], [-25.0])[0], pcm, rate, -25.0, ("B=1", n, rate))
        # digital silence: the gain is capped at 300 dB and zeros come out; beside it a full-scale square wave
        silence = np.zeros(4000, np.int16)
        got = _perturb(hip_device, [silence, square, silence[:9]], [rate] * 3, [-20.0, -20.0, 0.0])
        assert not got[0].any() and not got[2].any() and len(got[0]) == len(F.perturb(silence, rate, -20.0))
        _assert_perturbed(got[1], square, rate, -20.0, ("square", rate))
        assert (F.perturb(square, rate, -20.0) < 0).any()


@pytest.mark.parametrize("sigma,db", [(9000, -3.0), (3000, 5.0)])
def test_perturb_levels_that_clip(hip_device, sigma, db):
    """16 % / 57 % of the samples at the rails.  Rates 0.9 and 1.1 only: at unchanged speed the reference's own float32
    mean flips more than 1e-3 of the samples of a loud target against any fp64 sum, so that case proves nothing."""
    rng = np.random.default_rng(int(sigma))
    pcms = [C._i16(rng.standard_normal(n) * sigma) for n in (9, 400, 48000, 160001)]
    for rate in (0.9, 1.1):
        for pcm in pcms[2:]:     # on the CPU, before anything is compared: the expected output has what the case is about
            frac = C.assert_clipping_case_is_not_vacuous(*C.perturb_expected(pcm, rate, db))
            assert 0.1 < frac < 0.7
        for i, got in enumerate(_perturb(hip_device, pcms, [rate] * len(pcms), [db] * len(pcms))):
            _assert_perturbed(got, pcms[i], rate, db, (sigma, db, len(pcms[i]), rate))


def test_perturb_resamples_whenever_the_rate_is_not_one(hip_device):
    """int(n / rate) == n with rate != 1: the reference still interpolates on linspace(0, n, n), a stretch by one sample
    over the utterance.  The output length alone cannot tell that from unchanged speed; the host's flag does."""
    rng = np.random.default_rng(60)
    cases = [(5000, 0.9999), (8, 0.9), (9998, 0.9999), (5000, 1.0), (8, 1.0)]
    pcms = [C._i16(rng.standard_normal(n) * 3000) for n, _ in cases]
    rates = [r for _, r in cases]
    for (n, r), pcm in zip(cases[:3], pcms):
        assert int(n / r) == n and not np.array_equal(F.perturb(pcm, r, -25.0), F.perturb(pcm, 1.0, -25.0))
    for i, got in enumerate(_perturb(hip_device, pcms, rates, [-25.0] * len(pcms))):
        _assert_perturbed(got, pcms[i], rates[i], -25.0, cases[i])


# ---------------- 5. pika_audio_convolve_same ------------------------------------------------------------------------
CONV_SHAPES = [(1, 1), (5, 5), (255, 2), (256, 256), (257, 3), (1024, 1024), (1025, 1025), (3000, 2049), (70000, 1)]


@pytest.mark.parametrize("n,m", CONV_SHAPES)
def test_convolve_same_shapes(hip_device, n, m):
    """m == n, even and odd m (the centre (m - 1) / 2 differs), n below / at / above one workgroup, m at / above one and two
    chunks of 1024 taps.  fp64 direct sum rounded once to fp32: 2e-7 of the largest output."""
    from pika_amd import _lib
    rng = np.random.default_rng(n * 7 + m)
    x = rng.standard_normal(n).astype(np.float32)
    h = (rng.standard_normal(m) * np.exp(-np.arange(m) / 300.0)).astype(np.float32)
    want = np.convolve(x.astype(np.float64), h.astype(np.float64))[(m - 1) // 2:(m - 1) // 2 + n]
    dx, dh = _dev(x, hip_device), _dev(h, hip_device)
    out = _canary((n + 64,), hip_device)
    rc = _lib.lib().pika_audio_convolve_same(dx.data_ptr(), n, dh.data_ptr(), m, out.data_ptr(), _stream(hip_device))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out[n:] == CANARY).all())
    got = out[:n].cpu().numpy().view(np.float32).astype(np.float64)
    err = np.abs(got - want).max()
    assert err <= 2e-7 * np.abs(want).max(), (n, m, err, np.abs(want).max())


def test_convolve_same_refuses_what_it_cannot_do(hip_device):
    from pika_amd import _lib
    lib = _lib.lib()
    x = torch.zeros(64, dtype=torch.float32, device=hip_device)
    h = torch.zeros(128, dtype=torch.float32, device=hip_device)
    out = _canary((64,), hip_device)
    st = _stream(hip_device)
    assert lib.pika_audio_convolve_same(x.data_ptr(), 64, h.data_ptr(), 65, out.data_ptr(), st) == EINVAL    # m > n
    assert lib.pika_audio_convolve_same(x.data_ptr(), 64, h.data_ptr(), 3, x.data_ptr(), st) == EINVAL      # in place
    assert lib.pika_audio_convolve_same(x.data_ptr(), 0, h.data_ptr(), 1, out.data_ptr(), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
