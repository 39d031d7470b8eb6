"""Shared by tests/test_frontend_parity_gpu.py: the fbank configurations, the waveform zoo and an fp32 RESTATEMENT OF THE
ORACLE (oracle/fbank_ref.kaldi_fbank step by step with every array float32; written from the oracle, never from the
kernel).  The restatement measures how far an honest fp32 evaluation of the formula is from fp64 on a given input, which
is the only thing allowed to widen the project's 2e-3 bound on the log-mel values.  Everything here runs on the CPU."""
import functools
from collections import OrderedDict

import numpy as np
import scipy.fft

from oracle import fbank_ref as F

LOGMEL_ATOL = 2e-3        # the project's bound for kernel vs oracle (tests/test_frontend.py)
RESTATEMENT_MARGIN = 4.0  # radix-2 + sincospif / __logf / __cosf against pocketfft + libm: over the REFERENCE's fp32 error

# name -> FbankConfig keywords (window_type / dither added by fbank_config)
CONFIGS = OrderedDict([
    ("recipe", dict(sample_frequency=16000.0, num_mel_bins=80, low_freq=40.0, high_freq=-200.0)),
    ("kaldi_default_bank", dict(sample_frequency=16000.0, num_mel_bins=23, low_freq=20.0, high_freq=0.0)),
    ("8khz", dict(sample_frequency=8000.0, num_mel_bins=40, low_freq=40.0, high_freq=-200.0)),
    ("long_window", dict(sample_frequency=16000.0, num_mel_bins=64, low_freq=40.0, high_freq=-200.0, frame_length=50.0)),
    ("short_window", dict(sample_frequency=16000.0, num_mel_bins=80, low_freq=40.0, high_freq=-200.0,
                          frame_length=20.0, frame_shift=8.0)),
    ("no_preemphasis", dict(sample_frequency=16000.0, num_mel_bins=80, low_freq=40.0, high_freq=-200.0,
                            preemphasis_coefficient=0.0)),
])
# what the kernel is handed under each: (frame_len, shift, nfft)
GEOMETRY = {"recipe": (400, 160, 512), "kaldi_default_bank": (400, 160, 512), "8khz": (200, 80, 256),
            "long_window": (800, 160, 1024), "short_window": (320, 128, 512), "no_preemphasis": (400, 160, 512)}


def fbank_config(name, dither=0.0):
    from pika_amd.loader.frontend import FbankConfig
    return FbankConfig(dither=dither, window_type="hamming", **CONFIGS[name])


def oracle_kwargs(name):
    """The same options in oracle/fbank_ref.kaldi_fbank's spelling."""
    c = CONFIGS[name]
    return dict(sample_freq=c["sample_frequency"], num_bins=c["num_mel_bins"], low=c["low_freq"], high=c["high_freq"],
                preemph=c.get("preemphasis_coefficient", 0.97), frame_len_ms=c.get("frame_length", 25.0),
                frame_shift_ms=c.get("frame_shift", 10.0))


def _i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def waveforms(name):
    """The zoo for one configuration: name -> int16 samples, one second each unless the name says otherwise."""
    sr = int(CONFIGS[name]["sample_frequency"])
    flen, shift, _ = GEOMETRY[name]
    rng = np.random.default_rng(1234)
    n = sr
    t = np.arange(n)
    z = OrderedDict()
    z["noise"] = _i16(rng.standard_normal(n) * 2500)
    z["quiet"] = _i16(rng.standard_normal(n) * 2)                      # a few LSBs: around the energy floor
    z["silence"] = np.zeros(n, np.int16)
    z["dc"] = np.full(n, 20000, np.int16)                              # 800 * 20000 < 2^24: fp32 removes the mean exactly
    z["dc_noise"] = _i16(12000 + rng.standard_normal(n) * 300)
    z["square"] = np.where((t // 37) % 2 == 0, 32767, -32768).astype(np.int16)   # period 74, both rails
    z["tone_1k"] = _i16(30000 * np.sin(2 * np.pi * 1000.0 * t / sr))
    z["tone_60"] = _i16(30000 * np.sin(2 * np.pi * 60.0 * t / sr))
    imp = np.zeros(n, np.int16)
    imp[::997] = 32767
    z["impulses"] = imp
    # the 50 -> 3950 Hz chirp of tests/test_fbank_crosscheck.py, swept over one second
    z["chirp"] = _i16(12000 * np.sin(2 * np.pi * (50 + 3900 * np.linspace(0, 1, n)) * t / sr))
    z["sawtooth"] = ((t * 257) % 65536 - 32768).astype(np.int16)       # the whole int16 range
    z["one_frame"] = z["noise"][:flen].copy()
    z["one_frame_plus"] = z["noise"][100:100 + flen + shift - 1].copy()  # one sample short of a second frame
    z["no_frame"] = z["noise"][:flen - 1].copy()                       # length 0
    return z


def ill_conditioned(name):
    """DC 20000 + noise of sigma 1: the frame mean takes all but a few bits of every sample."""
    sr = int(CONFIGS[name]["sample_frequency"])
    rng = np.random.default_rng(4321)
    return _i16(20000 + rng.standard_normal(sr))


@functools.lru_cache(maxsize=None)
def _banks32(num_bins, sample_freq, nfft, low, high):
    return F.mel_banks(num_bins, sample_freq, nfft, low, high).astype(np.float32)


def kaldi_fbank_f32(wave, sample_freq=16000.0, num_bins=80, low=40.0, high=-200.0, preemph=0.97,
                    frame_len_ms=25.0, frame_shift_ms=10.0):
    """oracle/fbank_ref.kaldi_fbank (dither 0) with float32 arrays throughout and a complex64 transform."""
    f32 = np.float32
    wave = np.asarray(wave, f32)
    flen = int(sample_freq * 0.001 * frame_len_ms)
    shift = int(sample_freq * 0.001 * frame_shift_ms)
    nfft = 1
    while nfft < flen:
        nfft *= 2
    if len(wave) < flen:
        return np.zeros((0, num_bins), f32)
    n = 1 + (len(wave) - flen) // shift
    window = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(flen) / (flen - 1))).astype(f32)   # the oracle's, stored fp32
    banks = _banks32(num_bins, sample_freq, nfft, low, high)
    eps = np.finfo(f32).eps
    out = np.zeros((n, num_bins), f32)
    buf = np.zeros(nfft, f32)
    for f in range(n):
        w = wave[f * shift: f * shift + flen].copy()
        w -= w.mean(dtype=f32)
        w[1:] -= f32(preemph) * w[:-1]
        w[0] -= f32(preemph) * w[0]
        w *= window
        buf[:flen] = w
        spec = scipy.fft.rfft(buf)
        assert spec.dtype == np.complex64 and window.dtype == f32 and w.dtype == f32
        power = (spec.real ** 2 + spec.imag ** 2)[:nfft // 2]
        out[f] = np.log(np.maximum(banks @ power, eps))
    return out


def relative_energy_error(got_log, ref_log):
    """max over frames and bins of |E_got - E_ref| / (the frame's largest E_ref), E = exp(log-mel), in fp64."""
    eg, er = np.exp(np.asarray(got_log, np.float64)), np.exp(np.asarray(ref_log, np.float64))
    if er.size == 0:
        return 0.0
    return float((np.abs(eg - er) / er.max(axis=1, keepdims=True)).max())


@functools.lru_cache(maxsize=None)
def reference_tables(name):
    """For one configuration: waveform -> (oracle fp64 log-mel, restatement's max |error|, tolerance for the kernel)."""
    kw = oracle_kwargs(name)
    out = OrderedDict()
    for wname, pcm in waveforms(name).items():
        ref = F.kaldi_fbank(pcm.astype(np.float64), **kw)
        r32 = kaldi_fbank_f32(pcm, **kw)
        assert ref.shape == r32.shape
        err = float(np.abs(r32.astype(np.float64) - ref).max()) if ref.size else 0.0
        out[wname] = (ref, err, max(LOGMEL_ATOL, RESTATEMENT_MARGIN * err))
    return out


@functools.lru_cache(maxsize=None)
def check_restatement_condition():
    """A condition on the INPUTS, asserted before any kernel output is looked at: over all (configuration, waveform)
    pairs the second term of tol = max(2e-3, 4 * restatement error) decides for at most 2 pairs and never exceeds 4e-3,
    so it cannot be what hides a kernel error.  Returns the pairs where it decides."""
    wide = []
    for name in CONFIGS:
        for wname, (_, err, tol) in reference_tables(name).items():
            assert RESTATEMENT_MARGIN * err <= 4e-3, (name, wname, err)
            if tol > LOGMEL_ATOL:
                wide.append((name, wname, err))
    assert len(wide) <= 2, wide
    return tuple(wide)


# ---------------- dither --------------------------------------------------------------------------------------------
KS_P_MIN = 1e-6     # per bin; 80 bins -> family-wise false alarm < 1e-4


def oracle_dither_sample(n_frames, seed, dither=1.0, **kw):
    """Log-mel of silence + dither from the oracle: (n_frames, num_bins), frames independent (fresh noise per frame)."""
    flen = int(kw.get("sample_freq", 16000.0) * 0.001 * kw.get("frame_len_ms", 25.0))
    shift = int(kw.get("sample_freq", 16000.0) * 0.001 * kw.get("frame_shift_ms", 10.0))
    return F.kaldi_fbank(np.zeros(flen + shift * (n_frames - 1)), dither=dither, rng=np.random.default_rng(seed), **kw)


def ks_min_p(a, b):
    """Smallest two-sample Kolmogorov-Smirnov p-value over the mel bins of two (frames, bins) samples."""
    from scipy.stats import ks_2samp
    assert a.shape[1] == b.shape[1]
    return min(ks_2samp(a[:, m], b[:, m]).pvalue for m in range(a.shape[1]))


def column_correlations(x, y):
    """Pearson r per column of two (n, bins) arrays."""
    x = x - x.mean(0)
    y = y - y.mean(0)
    return (x * y).sum(0) / np.sqrt((x * x).sum(0) * (y * y).sum(0))


# ---------------- perturbation ----------------------------------------------------------------------------------------
def perturb_expected(pcm, rate, target_db):
    """(F.perturb's int16 output, the scaled float samples it was cut from)."""
    x = pcm.astype(np.float32) * np.float32(1.0 / 32768)
    scaled = F.normalize(F.change_speed(x, rate), target_db) * 32768.0
    want = F.perturb(pcm, rate, target_db)
    return want, np.asarray(scaled, np.float64)


def assert_clipping_case_is_not_vacuous(want, scaled):
    """Both rails and truncation toward zero of a negative value occur in the EXPECTED output."""
    assert (want == 32767).any() and (want == -32768).any()
    inside = (scaled < 0) & (scaled > -32768) & (scaled != np.trunc(scaled))
    assert inside.any() and np.array_equal(want[inside], np.trunc(scaled[inside]).astype(np.int16))
    assert (np.trunc(scaled[inside]) != np.floor(scaled[inside])).all()
    return float(((want == 32767) | (want == -32768)).mean())


# ---------------- splice / pad ----------------------------------------------------------------------------------------
def splice_pad_expected(x, lctx, rctx, stride, t_max):
    """F.splice(x, l, r)[::stride], padded to t_max rows by repeating its last row."""
    s = F.splice(x, lctx, rctx)[::stride]
    assert 0 < s.shape[0] <= t_max
    return np.concatenate([s, np.repeat(s[-1:], t_max - s.shape[0], 0)])
