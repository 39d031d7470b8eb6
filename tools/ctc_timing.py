"""What the CTC search timing tools share (tools/ctc_decode_time.py, ctc_lm_time.py, ctc_stream_time.py,
ctc_bias_time.py): the event bracket, the warm-up and the alternating measure loop, the parent commit's library for an
A/B inside one session, an FST as the C ABI takes it, and the seeded LMs.  A module, not a tool: nothing runs on import.
"""
import contextlib
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pika_amd  # noqa: F401,E402  (first: places the HIP runtime flag before torch initialises it)
from pika_amd import _lib  # noqa: E402
from pika_amd.decoder.ngram_fst import NgramFst  # noqa: E402


def once(fn):
    """Milliseconds of one call of fn between two events on the current stream."""
    if isinstance(fn, tuple):               # (what happens before the bracket, what is timed)
        fn[0]()
        fn = fn[1]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(variants, warmup, runs):
    """[(name, fn)] -> {name: [ms] * runs}: every variant warmed up, then the variants alternating inside one loop."""
    times = {name: [] for name, _ in variants}
    for _ in range(warmup):
        for _, fn in variants:
            once(fn)
    for _ in range(runs):
        for name, fn in variants:           # alternating
            times[name].append(once(fn))
    return times


def load_parent(path):
    """The parent commit's library with the signatures it shares with this tree."""
    handle = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return handle


@contextlib.contextmanager
def library(handle):
    """The Python surface on another library for the length of a call."""
    mine = _lib.lib()
    _lib._lib = handle
    try:
        yield
    finally:
        _lib._lib = mine


def fst_args(m, start=True):
    """A `CtcNgramLm` as the C ABI takes it, with or without its start state."""
    return (m.offsets.data_ptr(), m.ilabel.data_ptr(), m.weight.data_ptr(), m.nextstate.data_ptr(),
            m.final.data_ptr(), m.num_states, m.num_arcs) + ((m.start,) if start else ()) + (m.backoff_id,
                                                                                             m.label_offset)


def bigram_lm(C, blank, per_state, seed):
    """(fst, backoff_id): state 0 the unigram state, state 1 the start state, state 2 + i the bigram state of the i-th
    non-blank class."""
    rng = np.random.RandomState(seed)
    classes = np.array([c for c in range(C) if c != blank])
    n, backoff_id = len(classes), C + 1
    state_of = np.zeros(C, dtype=np.int64)
    state_of[classes] = 2 + np.arange(n)
    offsets, ilabel, nextstate = [0], [], []

    def push(labels, targets):
        ilabel.append(labels)
        nextstate.append(targets)
        offsets.append(offsets[-1] + len(labels))
    push(classes + 1, state_of[classes])
    for _ in range(n + 1):                                  # the start state, then the bigram states
        own = np.sort(rng.choice(classes, size=per_state, replace=False))
        push(np.concatenate([own + 1, [backoff_id]]), np.concatenate([state_of[own], [0]]))
    ilabel, nextstate = np.concatenate(ilabel), np.concatenate(nextstate)
    weight = rng.uniform(0.3, 5.0, size=len(ilabel)).astype(np.float32)
    final = np.full(n + 2, np.inf, dtype=np.float32)
    final[0] = 1.0
    return NgramFst(offsets, ilabel, weight, nextstate, final, start=1), backoff_id


def unigram_lm(C, blank, seed):
    rng = np.random.RandomState(seed)
    classes = np.array([c for c in range(C) if c != blank])
    weight = rng.uniform(0.3, 5.0, size=len(classes)).astype(np.float32)
    return NgramFst([0, len(classes)], classes + 1, weight, np.zeros(len(classes), np.int32),
                    np.array([1.0], np.float32), start=0), C + 1
