"""Host side of the CTC loss, its gradient and forced alignment (include/pika_ctc.h, csrc/ctc_loss.hip).

The surface is `torch.nn.functional.ctc_loss`'s -- the loss the reference's LAS trainer builds as `nn.CTCLoss()`
(trainer/train_las_bmuf_otfaug.py:58-81):

    ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=0, reduction='mean', zero_infinity=False)
    ctc_loss_from_logits(logits, ...same...)      log-softmax + loss + log-softmax backward, no log-prob tensor
    CTCLoss(blank=0, reduction='mean', zero_infinity=False)     nn.Module, forward(log_probs, targets, il, tl)
    ctc_align(log_probs, targets, input_lengths, target_lengths, blank=0) -> (scores (B,), frame_labels (B, T))
    ctc_align_from_logits(logits, ...)

and the decoders (include/pika_ctc_decode.h, csrc/ctc_decode.hip), which need no transcript:

    ctc_greedy_decode(log_probs, input_lengths, blank=0) -> (tokens (B,T), lengths (B,), scores (B,), frames (B,T))
    ctc_beam_search(log_probs, input_lengths, beam=16, nbest=1, blank=0)
        -> (tokens (B,nbest,T), lengths (B,nbest), scores (B,nbest))
    ctc_greedy_decode_from_logits(logits, ...), ctc_beam_search_from_logits(logits, ...)

and the search with an n-gram LM fused in (include/pika_ctc_lm.h, csrc/ctc_lm.hip):

    CtcNgramLm(fst, backoff_id, label_offset=1, device=None)
    ctc_beam_search_lm(log_probs, input_lengths, lm, beam=16, nbest=1, blank=0, lm_weight=0.5, length_bonus=0.0,
                       candidates=None, use_final=True)
        -> (tokens (B,nbest,T), lengths (B,nbest), scores (B,nbest), am_scores (B,nbest))
    ctc_beam_search_lm_from_logits(logits, ...same...)

with contextual biasing as a second automaton beside the LM -- wherever an `lm` is taken, a `CtcBiasedLm` is too:

    CtcHotwords(phrases, num_classes, boost=1.0, blank=0, device=None)      a phrase list compiled to the LM's FST layout
    CtcBiasedLm(lm, bias, bias_weight=1.0)                                  an LM and a second automaton beside it

and both searches with their state carried across calls, for audio that arrives in chunks:

    CtcBeamStream(batch, max_frames, beam=16, blank=0, lm=None, lm_weight=0.5, length_bonus=0.0, candidates=None,
                  device=None)
        .reset(which=None)  .advance(log_probs, lengths=None)  .advance_from_logits(logits, lengths=None)
        .results(nbest=1, use_final=True)  .commit(which=None, max_tail=None)  .frames  .consumed  .room  .overflowed

and, for the n-best list any of these searches returns, what `ctc_align` and `ctc_loss` give for one transcript:

    ctc_nbest_align(log_probs, input_lengths, tokens, lengths, blank=0, max_len=None)
        -> (full_scores (B,N), best_scores (B,N), starts (B,N,L), ends (B,N,L), token_scores (B,N,L))
    ctc_nbest_align_from_logits(logits, ...same...)

and the same full-sum scores with autograd to the un-replicated input, and MWER training over the list on top of them:

    ctc_nbest_loss(log_probs, input_lengths, tokens, lengths, blank=0, max_len=None) -> full_scores (B,N)
    ctc_mwer_loss(log_probs, input_lengths, tokens, lengths, errors, blank=0, max_len=None, reduction='mean')
    ctc_nbest_loss_from_logits(logits, ...), ctc_mwer_loss_from_logits(logits, ...)
    ctc_nbest_errors(tokens, lengths, targets, target_lengths) -> errors (B,N)      host code: edit distances

and the same edit distances on the device (csrc/ctc_edit.hip), which closes the chain search -> errors -> MWER loss into
one capturable sequence, with MBR decoding over the list on top of them:

    ctc_nbest_edit_distance(tokens, lengths, targets, target_lengths) -> errors (B,N)   = ctc_nbest_errors, no host sync
    ctc_nbest_pairwise_distance(tokens, lengths) -> distances (B,N,N)
    ctc_nbest_mbr_decode(tokens, lengths, scores, scale=1.0) -> (best (B,), risks (B,N))

and long-form alignment (csrc/ctc_long.hip): the Viterbi path with the state axis tiled, for transcripts beyond the 511
labels every call above is bound by and recordings too long for a plane -- an hour of audio against its whole transcript:

    ctc_long_align(log_probs, targets, input_lengths=None, target_lengths=None, blank=0)
        -> (scores (B,), starts (B,U), ends (B,U), token_scores (B,U))
    ctc_long_align_from_logits(logits, ...same...)
    ctc_segment_scores(starts, ends, token_scores, segment_offsets) -> (seg_start, seg_end, seg_confidence)   (B,G)

and the long-form loss (csrc/ctc_long_loss.hip): `ctc_loss` over the same tiling, alpha and beta, for transcripts beyond
511 labels -- `ctc_loss`, `ctc_loss_from_logits` and `CTCLoss` route to it by themselves when 2 * U_max + 1 > 1024:

    ctc_long_loss(log_probs, targets, input_lengths, target_lengths, blank=0, reduction='mean', zero_infinity=False)
    ctc_long_loss_from_logits(logits, ...same...)

Differences from torch, on purpose:

* THE GRADIENT IS THE TRUE DERIVATIVE.  torch's native CTC backward returns `exp(log_probs) - occ` for d/d log_probs,
  not the derivative `-occ` of the cost with respect to its input; the two agree only after a `log_softmax` backward
  (whose projection removes any multiple of exp(lp) whose rows sum to the same total).  `ctc_loss` here returns
  `-occ`, as `rnnt_loss` does for its lattice; `ctc_loss_from_logits` returns d/d logits = softmax - occ, which IS what
  torch gives through `log_softmax`.  A caller that feeds unnormalised scores straight into the loss (the reference's
  LAS script does) gets a different gradient from the two libraries.
* An infeasible utterance (T_n < U_n + adjacent repeats, or a label outside [0, C)) has cost +inf and an all-zero
  gradient; torch gives NaN gradients there unless zero_infinity=True.  zero_infinity only turns the cost into 0.
* Lengths are clamped on the device (input_lengths to [1, T], target_lengths to [0, U_max]); nothing is checked on
  the host, so nothing synchronises.

Host synchronisation: none with padded 2-D targets (U_max = targets.shape[1]) -- with targets and lengths already on
the device the forward, backward and alignment calls can be captured in one `torch.cuda.graph`.  1-D concatenated
targets take their offsets from a device cumsum; U_max is the largest target length, read on the host when the
lengths live there (no sync) and by ONE device-to-host copy per call when they live on the device (the trade
`rnnt_loss(compact=True)` makes; it raises under stream capture).
"""
import numpy as np
import torch

from . import _lib

MAX_STATES = 1024   # 2 * U_max + 1: one workgroup spans the state axis
MAX_BEAM = 64       # one lane per beam slot
MAX_CANDIDATES = 128
MAX_BACKOFF_HOPS = 8
# a stream's record behind the tables of its blob (include/pika_ctc_decode.h): i32 words n, frames, overflow, ...
STREAM_FRAMES_WORD = 1      # PIKA_CTC_STREAM_FRAMES_OFFSET / 4
STREAM_OVERFLOW_WORD = 2    # PIKA_CTC_STREAM_OVERFLOW_OFFSET / 4
STREAM_RETIRED_WORD = 3     # PIKA_CTC_STREAM_RETIRED_OFFSET / 4


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_input(x, what, who, blank):
    """The checks on the input that the loss and the decoders share (`who`: the caller): (x as (T,B,C), unbatched)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("pika_amd %s: %s must live on a HIP device (there is no CPU path)" % (who, what))
    if x.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (what, x.dtype))
    unbatched = x.dim() == 2
    if unbatched:
        x = x.unsqueeze(1)
    if x.dim() != 3:
        raise ValueError("%s must be (T,B,C) or (T,C), got %s" % (what, tuple(x.shape)))
    T, B, C = x.shape
    if T < 1 or B < 1 or C < 1:
        raise ValueError("%s has an empty dimension: %s" % (what, tuple(x.shape)))
    if not 0 <= blank < C:
        raise ValueError("blank=%d outside [0,%d)" % (blank, C))
    return x, unbatched


def _prepare(x, what, targets, input_lengths, target_lengths, blank, tiled=False):
    """Checks and device copies: (x as (T,B,C), any stride; targets i32; offsets i32 or None; il i32; tl i32; U_max;
    unbatched).  `tiled`: the caller has the tiled path for a state axis wider than one workgroup."""
    x, unbatched = _check_input(x, what, "ctc_loss", blank)
    B, dev = x.shape[1], x.device
    targets = torch.as_tensor(targets)
    il_host, tl_host = torch.as_tensor(input_lengths), torch.as_tensor(target_lengths)
    for name, t in (("targets", targets), ("input_lengths", il_host), ("target_lengths", tl_host)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    if unbatched:
        targets = targets.reshape(1, -1)
    il = il_host.reshape(-1).to(dev, torch.int32).contiguous()
    tl = tl_host.reshape(-1).to(dev, torch.int32).contiguous()
    if il.numel() != B or tl.numel() != B:
        raise ValueError("input_lengths / target_lengths must hold B = %d entries" % B)
    toff = None
    if targets.dim() == 2:
        if targets.shape[0] != B:
            raise ValueError("targets must be (B,S) = (%d,S), got %s" % (B, tuple(targets.shape)))
        U = int(targets.shape[1])
    elif targets.dim() == 1:
        if tl_host.is_cuda:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ctc_loss with 1-D targets and device target_lengths reads U_max on the host and "
                                   "cannot run under stream capture; capture padded (B,S) targets instead")
            U = int(tl_host.max())        # the one device-to-host copy of this form
        else:
            U = int(tl_host.max())
            if int(tl_host.clamp(min=0).sum()) > targets.numel():
                raise ValueError("1-D targets hold %d labels, target_lengths sum to %d"
                                 % (targets.numel(), int(tl_host.clamp(min=0).sum())))
        U = max(0, min(U, int(targets.numel())))
        wide = tl.to(torch.int64)
        toff = (torch.cumsum(wide, 0) - wide).to(torch.int32)
    else:
        raise ValueError("targets must be (B,S) or 1-D, got %s" % (tuple(targets.shape),))
    if 2 * U + 1 > MAX_STATES and not tiled:
        raise ValueError("2*U_max+1 = %d > %d not supported" % (2 * U + 1, MAX_STATES))
    targets = targets.to(dev, torch.int32).contiguous()
    return x, targets, toff, il, tl, U, unbatched


def _fill(x, targets, toff, il, tl, U, blank, logits):
    """Fill a workspace: (costs, ws, lse)."""
    lib = _lib.lib()
    T, B, C = x.shape
    with torch.cuda.device(x.device):
        costs = torch.empty(B, dtype=torch.float32, device=x.device)
        ws = torch.empty(lib.pika_ctc_workspace_bytes(B, T, U), dtype=torch.uint8, device=x.device)
        tg = _ptr(targets) if U > 0 else None
        if logits:
            lse = torch.empty(T * B, dtype=torch.float32, device=x.device)
            _lib.check(lib.pika_ctc_fused_forward(_ptr(x), tg, _ptr(toff), _ptr(il), _ptr(tl), B, T, U, C, blank,
                                                  _ptr(costs), _ptr(lse), _ptr(ws), _stream()), "pika_ctc_fused_forward")
        else:
            lse = None
            _lib.check(lib.pika_ctc_loss_forward(_ptr(x), tg, _ptr(toff), _ptr(il), _ptr(tl), B, T, U, C, blank,
                                                 _ptr(costs), _ptr(ws), _stream()), "pika_ctc_loss_forward")
    return costs, ws, lse


class _CTCFn(torch.autograd.Function):
    """Per-utterance costs (B,); backward writes the dense (T,B,C) gradient once, already scaled by grad_output."""

    @staticmethod
    def forward(ctx, x, targets, toff, il, tl, U, blank, logits):
        xc = x.detach().contiguous()
        costs, ws, lse = _fill(xc, targets, toff, il, tl, U, blank, logits)
        ctx.save_for_backward(*((xc, lse) if logits else ()), il, tl, ws)
        ctx.dims = tuple(xc.shape) + (U, blank, logits)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        T, B, C, U, blank, logits = ctx.dims
        lib = _lib.lib()
        gc = grad_costs.to(torch.float32).contiguous()
        if logits:
            x, lse, il, tl, ws = ctx.saved_tensors
        else:
            il, tl, ws = ctx.saved_tensors
        with torch.cuda.device(ws.device):
            grads = torch.empty((T, B, C), dtype=torch.float32, device=ws.device)
            if logits:
                _lib.check(lib.pika_ctc_fused_backward(_ptr(x), _ptr(lse), _ptr(il), _ptr(tl), B, T, U, C, blank,
                                                       _ptr(gc), _ptr(ws), _ptr(grads), _stream()),
                           "pika_ctc_fused_backward")
            else:
                _lib.check(lib.pika_ctc_loss_backward(_ptr(il), _ptr(tl), B, T, U, C, blank, _ptr(gc), _ptr(ws),
                                                      _ptr(grads), _stream()), "pika_ctc_loss_backward")
        return grads, None, None, None, None, None, None, None


def _loss(x, what, targets, input_lengths, target_lengths, blank, reduction, zero_infinity, logits, tiled=False):
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("%r is not a valid value for reduction" % (reduction,))
    blank = int(blank)
    x, tg, toff, il, tl, U, unbatched = _prepare(x, what, targets, input_lengths, target_lengths, blank, True)
    if tiled or 2 * U + 1 > MAX_STATES:     # a state axis beyond one workgroup: the tiled path (csrc/ctc_long_loss.hip)
        costs = _CTCLongFn.apply(x, _padded_targets(tg, toff, tl, U), il, tl, U, blank, logits, what)
    else:
        # (any stride: the kernels read the one contiguous copy the forward makes when it is needed)
        costs = _CTCFn.apply(x, tg, toff, il, tl, U, blank, logits)
    if zero_infinity:
        costs = torch.where(torch.isinf(costs), torch.zeros_like(costs), costs)
    # the reduction acts on the (B,) costs: its factors reach the kernel folded into grad_costs, so no pass over the
    # (T,B,C) gradient follows the one that writes it
    if reduction == "mean":
        return (costs / tl.clamp(min=1).to(costs.dtype)).mean()
    if reduction == "sum":
        return costs.sum()
    return costs.reshape(()) if unbatched else costs


def ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=0, reduction='mean', zero_infinity=False):
    """`torch.nn.functional.ctc_loss` on the MI355X: same arguments, defaults, shapes and reductions.

    log_probs (T,B,C) or (T,C) float32 on a HIP device, any stride (one contiguous copy when needed); targets (B,S)
    padded or 1-D concatenated; lengths (B,); targets and lengths int32 or int64, on the CPU or the device.
    'mean' divides each cost by clamp(target_length, 1) and averages over the batch.

    The gradient is the true derivative -occ with respect to log_probs -- torch's native kernel returns
    exp(log_probs) - occ, which equals it only after a log_softmax backward (module docstring).  Infeasible utterances
    cost +inf (0 with zero_infinity) and have an all-zero gradient.  Host synchronisation: module docstring.

    Any transcript length: up to 511 labels (2 * U_max + 1 <= 1024) one workgroup spans the state axis; beyond, the call
    is `ctc_long_loss`, which tiles it."""
    return _loss(log_probs, "log_probs", targets, input_lengths, target_lengths, blank, reduction, zero_infinity, False)


def ctc_loss_from_logits(logits, targets, input_lengths, target_lengths, blank=0, reduction='mean',
                         zero_infinity=False):
    """`ctc_loss(log_softmax(logits, -1), ...)` without materialising the log-probabilities: the row log-sum-exp is
    taken in the pass that gathers the state plane, and the backward writes d/d logits = grad * (softmax - occ)."""
    return _loss(logits, "logits", targets, input_lengths, target_lengths, blank, reduction, zero_infinity, True)


class CTCLoss(torch.nn.Module):
    """`torch.nn.CTCLoss` on the MI355X: `CTCLoss(blank=0, reduction='mean', zero_infinity=False)` and
    `forward(log_probs, targets, input_lengths, target_lengths)`; values and gradient as `ctc_loss`."""

    def __init__(self, blank=0, reduction='mean', zero_infinity=False):
        super().__init__()
        self.blank, self.reduction, self.zero_infinity = int(blank), reduction, bool(zero_infinity)

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        return ctc_loss(log_probs, targets, input_lengths, target_lengths, self.blank, self.reduction,
                        self.zero_infinity)


def align_workspace(ws, il, tl, B, T, U):
    """pika_ctc_align on a workspace a forward call filled: (scores (B,), frame_labels (B,T)).  The workspace is only
    read."""
    lib = _lib.lib()
    with torch.cuda.device(ws.device):
        scores = torch.empty(B, dtype=torch.float32, device=ws.device)
        labels = torch.empty((B, T), dtype=torch.int32, device=ws.device)
        scratch = torch.empty(lib.pika_ctc_align_scratch_bytes(B, T, U), dtype=torch.uint8, device=ws.device)
        _lib.check(lib.pika_ctc_align(_ptr(ws), _ptr(il), _ptr(tl), B, T, U, _ptr(scores), _ptr(labels), _ptr(scratch),
                                      _stream()), "pika_ctc_align")
    return scores, labels


def _align(x, what, targets, input_lengths, target_lengths, blank, logits):
    blank = int(blank)
    x, tg, toff, il, tl, U, _ = _prepare(x, what, targets, input_lengths, target_lengths, blank)
    xc = x.detach().contiguous()
    _, ws, _ = _fill(xc, tg, toff, il, tl, U, blank, logits)
    T, B, _ = xc.shape
    return align_workspace(ws, il, tl, B, T, U)


def ctc_align(log_probs, targets, input_lengths, target_lengths, blank=0):
    """Forced alignment: the single best (Viterbi) path of every transcript through its CTC lattice.

    Returns (scores, frame_labels), detached: scores (B,) f32, the log-probability of the best path (<= -cost);
    frame_labels (B,T) i32, the class that path emits at every frame, blank included, -1 for t >= T_n -- merging
    repeats and dropping blanks gives the transcript back.  Tie rule: the path ends in the final blank rather than the
    last label, and in the back-trace staying in a state is preferred to coming from s-1, and that to s-2.  An
    infeasible transcript scores <= -1e30 and still yields a path of valid states.  Inputs as `ctc_loss`; no autograd;
    same host-synchronisation behaviour.  At most 511 labels (ValueError beyond): `ctc_long_align` has no such limit."""
    return _align(log_probs, "log_probs", targets, input_lengths, target_lengths, blank, False)


def ctc_align_from_logits(logits, targets, input_lengths, target_lengths, blank=0):
    """`ctc_align` of log_softmax(logits, -1) without materialising the log-probabilities."""
    return _align(logits, "logits", targets, input_lengths, target_lengths, blank, True)


def _rows_input(x, what, input_lengths, blank):
    """The checks of the calls that read x row by row: (x as (T,B,C) with unit class stride, il i32, unbatched)."""
    x, unbatched = _check_input(x, what, "ctc decode", blank)
    x = x.detach()
    T, B, C = x.shape
    il = torch.as_tensor(input_lengths)
    if il.dtype not in (torch.int32, torch.int64):
        raise TypeError("input_lengths must be int32 or int64, got %s" % il.dtype)
    il = il.reshape(-1).to(x.device, torch.int32).contiguous()
    if il.numel() != B:
        raise ValueError("input_lengths must hold B = %d entries" % B)
    # the kernels take the two outer strides: only the class axis has to be dense (one copy when it is not)
    if C > 1 and x.stride(2) != 1:
        x = x.contiguous()
    return x, il, unbatched


def _decode_rows(x, what, input_lengths, blank, K, logits):
    """Checks + the row pass: (x as (T,B,C) with unit class stride, il i32, blank_lp, top_val, top_idx, lse or None,
    unbatched)."""
    x, il, unbatched = _rows_input(x, what, input_lengths, blank)
    T, B, C = x.shape
    lib = _lib.lib()
    with torch.cuda.device(x.device):
        blank_lp = torch.empty((T, B), dtype=torch.float32, device=x.device)
        top_val = torch.empty((T, B, K), dtype=torch.float32, device=x.device)
        top_idx = torch.empty((T, B, K), dtype=torch.int32, device=x.device)
        lse = torch.empty((T, B), dtype=torch.float32, device=x.device) if logits else None
        _lib.check(lib.pika_ctc_decode_rows(_ptr(x), x.stride(0), x.stride(1), _ptr(il), B, T, C, blank, K, int(logits),
                                            _ptr(blank_lp), _ptr(top_val), _ptr(top_idx), _ptr(lse), _stream()),
                   "pika_ctc_decode_rows")
    return x, il, blank_lp, top_val, top_idx, lse, unbatched


def _greedy(x, what, input_lengths, blank, logits):
    blank = int(blank)
    x, il, blank_lp, top_val, top_idx, _, unbatched = _decode_rows(x, what, input_lengths, blank, 1, logits)
    T, B, C = x.shape
    lib = _lib.lib()
    with torch.cuda.device(x.device):
        tokens = torch.empty((B, T), dtype=torch.int32, device=x.device)
        frames = torch.empty((B, T), dtype=torch.int32, device=x.device)
        lengths = torch.empty(B, dtype=torch.int32, device=x.device)
        scores = torch.empty(B, dtype=torch.float32, device=x.device)
        _lib.check(lib.pika_ctc_greedy(_ptr(blank_lp), _ptr(top_val), _ptr(top_idx), _ptr(il), B, T, C, blank,
                                       _ptr(tokens), _ptr(lengths), _ptr(scores), _ptr(frames), _stream()),
                   "pika_ctc_greedy")
    out = (tokens, lengths, scores, frames)
    return tuple(o[0] for o in out) if unbatched else out


def _nbest_outputs(beam, nbest):
    """Checks beam / nbest; returns the function that allocates (tokens, lengths, scores) for the (T,B,C) input x."""
    if not 1 <= nbest <= beam <= MAX_BEAM:
        raise ValueError("need 1 <= nbest <= beam <= %d, got beam=%d nbest=%d" % (MAX_BEAM, beam, nbest))

    def alloc(x):
        T, B, _ = x.shape
        return (torch.empty((B, nbest, T), dtype=torch.int32, device=x.device),
                torch.empty((B, nbest), dtype=torch.int32, device=x.device),
                torch.empty((B, nbest), dtype=torch.float32, device=x.device))
    return alloc


def _beam(x, what, input_lengths, beam, nbest, blank, logits):
    blank, beam, nbest = int(blank), int(beam), int(nbest)
    alloc = _nbest_outputs(beam, nbest)
    x, il, blank_lp, top_val, top_idx, lse, unbatched = _decode_rows(x, what, input_lengths, blank, 2 * beam, logits)
    T, B, C = x.shape
    lib = _lib.lib()
    nbytes = lib.pika_ctc_beam_scratch_bytes(B, T, beam)
    if nbytes == 0:
        raise ValueError("(B,T,beam) = (%d,%d,%d) not supported" % (B, T, beam))
    with torch.cuda.device(x.device):
        out = tokens, lengths, scores = alloc(x)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.pika_ctc_beam_search(_ptr(x), x.stride(0), x.stride(1), _ptr(lse), _ptr(blank_lp), _ptr(top_val),
                                            _ptr(top_idx), _ptr(il), B, T, C, blank, beam, nbest, _ptr(tokens),
                                            _ptr(lengths), _ptr(scores), _ptr(scratch), _stream()),
                   "pika_ctc_beam_search")
    return tuple(o[0] for o in out) if unbatched else out


def ctc_greedy_decode(log_probs, input_lengths, blank=0):
    """Best path: the per-frame arg-max (equal values: the lowest class), repeats merged, blanks dropped.

    log_probs (T,B,C) or (T,C) float32 on a HIP device, any stride; input_lengths (B,) int32 or int64, on the CPU or the
    device, clamped on the device to [1,T].  Returns (tokens (B,T) i32, lengths (B,) i32, scores (B,) f32,
    frames (B,T) i32): scores is the sum of the chosen values over t < T_n, frames[n,k] the first frame of the run
    that emits tokens[n,k]; both tokens and frames are -1 beyond lengths[n].  (T,C) input: no batch axis in the
    outputs.  No autograd, no host synchronisation; capturable in a `torch.cuda.graph` with the lengths on the device."""
    return _greedy(log_probs, "log_probs", input_lengths, blank, False)


def ctc_greedy_decode_from_logits(logits, input_lengths, blank=0):
    """`ctc_greedy_decode` of log_softmax(logits, -1): the row's log-sum-exp is taken in the pass that picks the
    arg-max, and the scores are sums of logit - lse."""
    return _greedy(logits, "logits", input_lengths, blank, True)


def ctc_beam_search(log_probs, input_lengths, beam=16, nbest=1, blank=0):
    """Prefix beam search over the full vocabulary, 1 <= nbest <= beam <= 64 (ValueError beyond).

    Every prefix l of the beam carries (p_b, p_nb), tot = p_b (+) p_nb.  At each frame blank adds lp[blank] + tot to
    p_b(l); c == last(l) adds lp[c] + p_nb to p_nb(l) and lp[c] + p_b to p_nb(l+c); any other class adds lp[c] + tot to
    p_nb(l+c); contributions to one label sequence are summed whichever parent they come from; the `beam` best by tot
    survive.  No class is pruned.  Ties: higher tot (the fp32 value the search carries), then prefixes already in the
    beam by their previous rank, then fresh ones by parent rank; fresh children of one parent keep the row pass's order
    -- higher value, then lower class -- and the child that repeats the parent's last label stands among children of
    equal tot by its class.  So "class ascending" holds wherever equal tot comes from equal values; two children of one
    parent whose different values round to the same fp32 tot keep the order of their values
    (include/pika_ctc_decode.h).

    Returns (tokens (B,nbest,T) i32, lengths (B,nbest) i32, scores (B,nbest) f32), best first; an entry that does not
    exist (fewer distinct prefixes than nbest) has length -1, score -inf and tokens -1.  Inputs, synchronisation and
    graph capture as `ctc_greedy_decode`."""
    return _beam(log_probs, "log_probs", input_lengths, beam, nbest, blank, False)


def ctc_beam_search_from_logits(logits, input_lengths, beam=16, nbest=1, blank=0):
    """`ctc_beam_search` of log_softmax(logits, -1) without materialising the log-probabilities."""
    return _beam(logits, "logits", input_lengths, beam, nbest, blank, True)


def _hip_device(device, default, who):
    """`device`, or `default` when it is None, as an indexed HIP device (`who`: the class that asks)."""
    if not torch.cuda.is_available():
        raise RuntimeError("pika_amd %s: needs a HIP device (there is no CPU path)" % who)
    dev = torch.device(default if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("pika_amd %s: device %s is not a HIP device (there is no CPU path)" % (who, dev))
    # always an indexed device: "cuda" and "cuda:0" must compare equal to a tensor's device
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


class CtcNgramLm(object):
    """An n-gram back-off LM for `ctc_beam_search_lm`: the arrays of an `NgramFst` (pika_amd/decoder/ngram_fst.py: it
    reads OpenFST binary and text files), checked on the host, uploaded once and kept.

    Class c of the acoustic model is FST label c + label_offset (default 1: label 0 is epsilon); back-off arcs carry
    `backoff_id`.  ValueError when: a `nextstate` or `start` is out of range; a state has more than one back-off arc; the
    back-off graph has a cycle or a chain of more than 8 hops; `backoff_id` collides with a class label (it lies in
    [label_offset, the largest other label of the table]; `ctc_beam_search_lm` checks it against C as well); the
    offsets do not describe the arc arrays.  The device code ends on any table all the same."""

    def __init__(self, fst, backoff_id, label_offset=1, device=None):
        offsets = np.ascontiguousarray(fst.offsets, dtype=np.int64)
        ilabel = np.ascontiguousarray(fst.ilabel, dtype=np.int32)
        weight = np.ascontiguousarray(fst.weight, dtype=np.float32)
        nextstate = np.ascontiguousarray(fst.nextstate, dtype=np.int32)
        final = np.ascontiguousarray(fst.final, dtype=np.float32)
        S, A = len(offsets) - 1, len(ilabel)
        backoff_id, label_offset, start = int(backoff_id), int(label_offset), int(fst.start)
        if S < 1 or len(final) != S or len(weight) != A or len(nextstate) != A or A >= 2 ** 31 or S >= 2 ** 31:
            raise ValueError("CtcNgramLm: inconsistent FST arrays (%d states, %d arcs)" % (S, A))
        if offsets[0] != 0 or offsets[-1] != A or np.any(np.diff(offsets) < 0):
            raise ValueError("CtcNgramLm: offsets do not describe the arc arrays")
        if not 0 <= start < S:
            raise ValueError("CtcNgramLm: start state %d outside [0,%d)" % (start, S))
        if A and (nextstate.min() < 0 or nextstate.max() >= S):
            raise ValueError("CtcNgramLm: a nextstate lies outside [0,%d)" % S)
        src = np.repeat(np.arange(S, dtype=np.int64), np.diff(offsets))
        is_bo = ilabel == backoff_id
        if np.any(np.bincount(src[is_bo], minlength=S) > 1):
            raise ValueError("CtcNgramLm: a state has more than one back-off arc")
        other = ilabel[~is_bo]
        if other.size and label_offset <= backoff_id <= int(other.max()):
            raise ValueError("CtcNgramLm: backoff_id %d collides with a class label (labels %d..%d)"
                             % (backoff_id, label_offset, int(other.max())))
        bo = np.full(S, -1, dtype=np.int64)       # the state a back-off arc leads to
        bo[src[is_bo]] = nextstate[is_bo]
        cur = np.arange(S, dtype=np.int64)
        for _ in range(MAX_BACKOFF_HOPS):
            cur = np.where(cur >= 0, bo[np.maximum(cur, 0)], -1)
        if np.any((cur >= 0) & (bo[np.maximum(cur, 0)] >= 0)):
            raise ValueError("CtcNgramLm: a back-off chain is longer than %d hops (or the back-off graph has a cycle)"
                             % MAX_BACKOFF_HOPS)
        self.device = _hip_device(device, "cuda", "CtcNgramLm")
        self.num_states, self.num_arcs, self.start = S, A, start
        self.backoff_id, self.label_offset = backoff_id, label_offset
        self.offsets, self.ilabel, self.weight, self.nextstate, self.final = (
            torch.from_numpy(v).to(self.device) for v in (offsets, ilabel, weight, nextstate, final))


class CtcHotwords(CtcNgramLm):
    """A phrase list for contextual biasing, compiled on the host into the back-off FST layout of `CtcNgramLm`: every
    token that extends a match of a phrase earns `boost`, and a match that is abandoned gives its credit back.

    `phrases` is a list of sequences of class ids in [0, num_classes), `blank` excluded.  For a label sequence l the
    automaton's score is BIAS(l) = boost * (tokens inside completed matches + depth of the match in progress); with
    `use_final` the match in progress at the end of the utterance is refunded too.  Beside an LM:
    `ctc_beam_search_lm(lp, il, CtcBiasedLm(LM, hotwords, bias_weight=w))` ranks by tot + lm_weight * LM + w * BIAS +
    length_bonus * |l|.

    Being a `CtcNgramLm`, it also works alone: `ctc_beam_search_lm(lp, il, lm=hotwords, lm_weight=1.0)` is biasing
    without an LM, and so is `CtcBeamStream(..., lm=hotwords, lm_weight=1.0)`.

    The compiled graph (`CtcHotwords.compile`, host only):
      states   the root (state 0, the start state) and one state per distinct non-empty proper prefix of a phrase; a
               complete phrase is no state -- the arc that completes it leads back to the root
      credit(s) = boost * depth(s); fail(s) = the state of the longest proper suffix of s's tokens that is a state,
               the root if there is none
      labels   class c is label c + 1; backoff_id = num_classes + 1
      s != root: for every token c that continues a phrase an arc of weight -boost to the child (to the root when c
               completes a phrase); one back-off arc of weight credit(s) - credit(fail(s)) to fail(s): the refund
      root     for every non-blank class c an arc: weight -boost to the child (to the root for a one-token phrase) when c
               starts a phrase, weight 0 to the root otherwise; no back-off arc -- it reaches every non-blank class
      final(s) = credit(s), 0 at the root
    ValueError when a phrase is empty, holds `blank` or a class outside [0, num_classes), or has another phrase as a
    proper prefix (the shorter one would complete and return to the root every time: the longer could never match);
    when `boost` is not a finite number > 0; and, by `CtcNgramLm`'s own check, when a fail chain is longer than 8 hops
    -- the device walks at most 8 back-off arcs per step (a phrase that starts with ten times the same token has such
    a chain).  Duplicate phrases are merged."""

    def __init__(self, phrases, num_classes, boost=1.0, blank=0, device=None):
        fst = self.compile(phrases, num_classes, boost, blank)
        self.num_classes, self.boost, self.blank = int(num_classes), float(boost), int(blank)
        CtcNgramLm.__init__(self, fst, int(num_classes) + 1, 1, device)

    @staticmethod
    def compile(phrases, num_classes, boost=1.0, blank=0):
        """The phrase list as an `NgramFst` (numpy, no device): labels class + 1, back-off label num_classes + 1."""
        from .decoder.ngram_fst import NgramFst
        C, blank, boost = int(num_classes), int(blank), float(np.float32(boost))    # the fp32 value the device reads
        if not (boost > 0.0 and np.isfinite(boost)):
            raise ValueError("CtcHotwords: boost must be a finite number > 0, got %r" % (boost,))
        if C < 1 or not 0 <= blank < C:
            raise ValueError("CtcHotwords: need num_classes >= 1 and blank in [0,%d), got blank=%d" % (C, blank))
        words = set()
        for ph in phrases:
            ph = tuple(int(c) for c in ph)
            if not ph:
                raise ValueError("CtcHotwords: an empty phrase")
            if any(c == blank or not 0 <= c < C for c in ph):
                raise ValueError("CtcHotwords: phrase %s holds blank or a class outside [0,%d)" % (list(ph), C))
            words.add(ph)
        for ph in words:
            for k in range(1, len(ph)):
                if ph[:k] in words:
                    raise ValueError("CtcHotwords: phrase %s is a proper prefix of phrase %s" % (list(ph[:k]), list(ph)))
        state = {(): 0}                                     # token string -> state
        for ph in sorted(words, key=lambda p: (len(p), p)):
            for k in range(1, len(ph)):
                state.setdefault(ph[:k], len(state))
        cont = {}                                           # state -> {token: next state}
        for ph in words:
            for k in range(len(ph)):
                cont.setdefault(state[ph[:k]], {})[ph[k]] = state[ph[:k + 1]] if k + 1 < len(ph) else 0
        arcs, finals = [], {}
        for c in range(C):
            if c != blank:
                nxt = cont.get(0, {}).get(c)
                arcs.append((0, c + 1, 0.0 if nxt is None else -boost, 0 if nxt is None else nxt))
        for tokens, s in state.items():
            finals[s] = boost * len(tokens)
            if s == 0:
                continue
            for c, nxt in cont[s].items():
                arcs.append((s, c + 1, -boost, nxt))
            fail = next(tokens[k:] for k in range(1, len(tokens) + 1) if tokens[k:] in state)
            arcs.append((s, C + 1, boost * (len(tokens) - len(fail)), state[fail]))
        return NgramFst.from_arcs(len(state), arcs, finals, start=0)


class CtcBiasedLm(object):
    """An LM with a second automaton beside it, for every place that takes an `lm`: `ctc_beam_search_lm`,
    `ctc_beam_search_lm_from_logits` and `CtcBeamStream`.  `lm` and `bias` are `CtcNgramLm`s on one device (TypeError /
    ValueError otherwise); `bias` is typically a `CtcHotwords` phrase list, but a second, domain LM works as well.  The
    search ranks by tot + lm_weight * LM(l) + bias_weight * BIAS(l) + length_bonus * |l| (`ctc_beam_search_lm`); the
    object holds references only, so one LM serves any number of per-request phrase lists."""

    def __init__(self, lm, bias, bias_weight=1.0):
        for name, v in (("lm", lm), ("bias", bias)):
            if not isinstance(v, CtcNgramLm):
                raise TypeError("%s must be a CtcNgramLm, got %s" % (name, type(v).__name__))
        if lm.device != bias.device:
            raise ValueError("the LM lives on %s, bias on %s" % (lm.device, bias.device))
        self.lm, self.bias, self.bias_weight, self.device = lm, bias, float(bias_weight), lm.device


def _fst_args(lm, start):
    """An FST as the C ABI takes it, with or without its start state."""
    return (_ptr(lm.offsets), _ptr(lm.ilabel), _ptr(lm.weight), _ptr(lm.nextstate), _ptr(lm.final), lm.num_states,
            lm.num_arcs) + ((lm.start,) if start else ()) + (lm.backoff_id, lm.label_offset)


class _Search(object):
    """Which search a call runs -- plain, with an LM, with an LM and a second automaton -- decided once, from what the
    caller gave as `lm` (None, a `CtcNgramLm`, a `CtcBiasedLm`).  The only place that knows the variants: a call site
    checks through `check_against` and makes one C call through `call`, with the argument groups below spliced in.

        prefix           of the entry points: pika_ctc_, pika_ctc_lm_ or pika_ctc_lm2_
        scratch_bytes    the name, behind the prefix, of the entry point that sizes the tables
        candidates       the row pass's K: 2 * beam for the plain search (exact), else as asked, None = min(2 * beam, 128)
        dims             what follows (B, T, beam) in the sizes, the reset and the results: () or (candidates,)
        fsts(start)      the automata as the C ABI takes them, without or with their start states
        starts()         (num_states, start) of every automaton: the reset's
        weights          after the automata in a search call: (), (candidates, lm_weight, length_bonus) or
                         (candidates, lm_weight, bias_weight, length_bonus)
        results_weights  the same in a results call: (), (lm_weight,) or (lm_weight, bias_weight)
        fused            there is an LM: the calls take `use_final` and return am_scores

    Built in two steps, `_Search(lm, lm_weight, length_bonus, need_lm).sized(beam, candidates)`: the one-shot call,
    which needs an LM, checks beam / nbest between the type of `lm` and `candidates`; a stream may have no LM."""

    def __init__(self, lm, lm_weight, length_bonus, need_lm):
        bias, bias_weight = None, 1.0
        if isinstance(lm, CtcBiasedLm):
            lm, bias, bias_weight = lm.lm, lm.bias, lm.bias_weight
        if not isinstance(lm, CtcNgramLm) and (need_lm or lm is not None):
            raise TypeError("lm must be a CtcNgramLm%s, got %s" % ("" if need_lm else " or None", type(lm).__name__))
        self.lm, self.bias, self.bias_weight = lm, bias, float(bias_weight)
        self.lm_weight, self.length_bonus = float(lm_weight), float(length_bonus)
        # the variants: the automata (each with its name and its backoff_id as the messages put them), and per number of
        # automata the entry points' prefix, the name of the one that sizes the tables, the weights of a results call
        n = 0 if lm is None else 1 if bias is None else 2
        self.automata = ((lm, "the LM", "the LM's backoff_id %d"), (bias, "bias", "the backoff_id %d of bias"))[:n]
        self.prefix, self.scratch_bytes = (("pika_ctc_", "beam_scratch_bytes"), ("pika_ctc_lm_", "scratch_bytes"),
                                           ("pika_ctc_lm2_", "scratch_bytes"))[n]
        self.results_weights = (self.lm_weight, self.bias_weight)[:n]
        self.fused = n > 0

    def sized(self, beam, candidates):
        if not self.fused:
            candidates = 2 * beam                       # the row pass's K of the plain search: exact
        else:
            candidates = min(2 * beam, MAX_CANDIDATES) if candidates is None else int(candidates)
            if not 1 <= candidates <= MAX_CANDIDATES:
                raise ValueError("need 1 <= candidates <= %d, got %d" % (MAX_CANDIDATES, candidates))
        self.candidates = candidates
        self.dims = (candidates,) if self.fused else ()
        self.weights = (self.dims + self.results_weights + (self.length_bonus,)) if self.fused else ()
        return self

    # (the automata's fields are read when a call is put together: behind the checks of the input, as they always were)
    def fsts(self, start):
        args = ()
        for a in self.automata:
            args += _fst_args(a[0], start)
        return args

    def starts(self):
        args = ()
        for a in self.automata:
            args += (a[0].num_states, a[0].start)
        return args

    def check_against(self, C, device, where):
        """Every automaton against the C classes of an input and the device of `where` (its name in the message)."""
        for m, name, its_backoff_id in self.automata:
            if 0 <= m.backoff_id - m.label_offset < C:
                raise ValueError((its_backoff_id + " is the label of class %d") % (m.backoff_id,
                                                                                  m.backoff_id - m.label_offset))
            if m.device != device:
                raise ValueError("%s lives on %s, %s on %s" % (name, m.device, where, device))

    def size(self, name, *dims):
        """A size in bytes by the variant's entry point `name`."""
        return getattr(_lib.lib(), self.prefix + name)(*(dims + self.dims))

    def call(self, name, *args):
        _lib.check(getattr(_lib.lib(), self.prefix + name)(*args), self.prefix + name)


def _beam_lm(x, what, input_lengths, lm, beam, nbest, blank, lm_weight, length_bonus, candidates, use_final, logits):
    blank, beam, nbest = int(blank), int(beam), int(nbest)
    v = _Search(lm, lm_weight, length_bonus, True)
    alloc = _nbest_outputs(beam, nbest)
    v.sized(beam, candidates)
    x, il, blank_lp, top_val, top_idx, lse, unbatched = _decode_rows(x, what, input_lengths, blank, v.candidates, logits)
    T, B, C = x.shape
    v.check_against(C, x.device, what)
    nbytes = v.size(v.scratch_bytes, B, T, beam)
    if nbytes == 0:
        raise ValueError("(B,T,beam,candidates) = (%d,%d,%d,%d) not supported" % (B, T, beam, v.candidates))
    with torch.cuda.device(x.device):
        tokens, lengths, scores = alloc(x)
        am_scores = torch.empty((B, nbest), dtype=torch.float32, device=x.device)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        v.call("beam_search", *((_ptr(x), x.stride(0), x.stride(1), _ptr(lse), _ptr(blank_lp), _ptr(top_val),
                                 _ptr(top_idx), _ptr(il), B, T, C, blank, beam, nbest) + v.fsts(True) + v.weights + (
                                     int(bool(use_final)), _ptr(tokens), _ptr(lengths), _ptr(scores), _ptr(am_scores),
                                     _ptr(scratch), _stream())))
    out = (tokens, lengths, scores, am_scores)
    return tuple(o[0] for o in out) if unbatched else out


def ctc_beam_search_lm(log_probs, input_lengths, lm, beam=16, nbest=1, blank=0, lm_weight=0.5, length_bonus=0.0,
                       candidates=None, use_final=True):
    """Prefix beam search with an n-gram LM fused into the ranking (shallow fusion), 1 <= nbest <= beam <= 64,
    1 <= candidates <= 128 (ValueError beyond); `candidates=None` means min(2 * beam, 128).

    A prefix l is ranked by F(l) = tot(l) + lm_weight * LM(l) + length_bonus * |l|.  tot and its (p_b, p_nb) recursion
    are `ctc_beam_search`'s: contributions to one label sequence are summed whichever parent they come from, and only
    the ranking uses F.  LM(l) is the sum of the LM's log-probabilities along l from its start state, each step the
    first match along the back-off chain of `lm` (a `CtcNgramLm`): the wanted arc if the state has it, otherwise the
    back-off arc's cost and its target state, at most 8 hops.  A class the LM cannot reach has probability zero: that
    child is excluded whatever `lm_weight` is, 0 included.

    THE CANDIDATES ARE A PRUNING.  A parent offers, per frame, the `candidates` best non-blank classes of the row (higher
    value, then lower class), its own last label, and every class whose child is already in the beam.  This is exact
    only when candidates >= C - 1: with an LM term a child's score is not monotone in the frame's log-prob, so the
    argument that makes `ctc_beam_search` exact with 2 * beam classes does not hold here.

    Ties: higher F (the fp32 value the search carries), then prefixes already in the beam by their previous rank, then
    fresh ones by parent rank, then class ascending.  With `use_final` every surviving prefix adds lm_weight times the
    log of the LM's final probability (through back-off if need be), prefixes with none drop out, and the beam is
    sorted again by that score (ties: the rank before).

    Returns (tokens (B,nbest,T) i32, lengths (B,nbest) i32, scores (B,nbest) f32, am_scores (B,nbest) f32), best first:
    `scores` is the fused score the ranking used (with the final term when asked), `am_scores` is tot alone.  A missing
    entry has length -1, scores -inf and tokens -1.  Inputs, strides, length clamping, no autograd, no host
    synchronisation and graph capture as `ctc_beam_search`.

    BIASING BESIDE THE LM.  `lm` may be a `CtcBiasedLm(lm, bias, bias_weight)`: `bias` is a second automaton -- a
    `CtcHotwords` phrase list, or any `CtcNgramLm` such as a domain LM -- walked from its own start state next to the LM:
    F(l) = tot + lm_weight * LM(l) + bias_weight * BIAS(l) + length_bonus * |l|.  A child that either automaton cannot
    reach does not exist (a `CtcHotwords` graph reaches every non-blank class); with `use_final` a prefix adds both
    final terms and drops out if either automaton has none.  Everything else -- candidates, ties, am_scores -- is as
    above.  ValueError for the second automaton's device or its backoff_id, as for the LM's."""
    return _beam_lm(log_probs, "log_probs", input_lengths, lm, beam, nbest, blank, lm_weight, length_bonus, candidates,
                    use_final, False)


def ctc_beam_search_lm_from_logits(logits, input_lengths, lm, beam=16, nbest=1, blank=0, lm_weight=0.5,
                                   length_bonus=0.0, candidates=None, use_final=True):
    """`ctc_beam_search_lm` of log_softmax(logits, -1) without materialising the log-probabilities."""
    return _beam_lm(logits, "logits", input_lengths, lm, beam, nbest, blank, lm_weight, length_bonus, candidates,
                    use_final, True)


class CtcBeamStream(object):
    """`ctc_beam_search` (lm=None) or `ctc_beam_search_lm` (lm a `CtcNgramLm`) for `batch` independent streams whose
    frames arrive in chunks.  The beam, the fp64 offsets, the frame count and the trie of every stream rest in one blob
    of device memory between calls (include/pika_ctc_decode.h, "Streaming"), and the frames go through the per-frame
    code of the one-shot kernels, so ANY chunking gives bit for bit what the one-shot call gives on the whole tensor.

    advance(log_probs, lengths=None)   log_probs (Tc,B,C) float32 on the device, any stride, B == batch; C is fixed by
        the first call.  lengths (B,) int32 / int64, host or device, clamped on the device to [0,Tc], None = Tc: stream b
        takes the frames t < lengths[b] of the chunk; with 0 it is left exactly as it was.
    advance_from_logits(logits, lengths=None)   the same on log_softmax(logits, -1), which never exists.
    results(nbest=1, use_final=True)   the n-best of the beams as they stand, in the shapes of the one-shot call with
        T = max_frames: (tokens (B,nbest,max_frames), lengths, scores), and am_scores with an LM.  It only reads the
        state: partial hypotheses can be taken after every chunk and decoding goes on; with an LM the final term and
        the re-sort of `use_final` happen on the side, so either setting can be asked at any time (ignored without LM).
    reset(which=None)   every stream back to the empty prefix, or those selected by `which` ((B,) bool / int tensor or
        sequence, host or device); the others' state, tables included, is not touched, so one stream of a serving
        batch can start a new utterance while its neighbours continue.
    commit(which=None, max_tail=None)   -> (tokens (B,max_frames) i32, lengths (B,) i32): the labels that became FINAL in
        this call, -1 beyond lengths[b]; the caller concatenates them over the calls.  The prefix that every entry of the
        beam shares can never change again; the commit emits it, re-roots the trie of prefixes there and rebuilds the
        table with the live nodes only, which gives capacity back (`room`).  Decoding goes on and gives the same bits as
        without the commit: results() then returns the uncommitted tails -- `lengths` relative to the commit, scores
        unchanged and absolute -- and committed + tail is the one-shot call's hypothesis.  `which` as in reset(): the
        other streams are not touched and get length 0.  max_tail=m >= 0 is the FORCED commit, for audio on which the
        beam does not converge: when the best entry (the first of the stored beam, before any `use_final` re-sort)
        would keep more than m uncommitted labels, everything but its last m labels is committed and the entries that
        do not start with that prefix are DROPPED.  This changes the search -- it is the usual finalisation by best
        path -- while max_tail=None never does.  No host synchronisation; capturable in a `torch.cuda.graph` (the
        scratch is allocated once, at the first call: make that call before the capture).
    frames       (B,) int32 device tensor: frames held per stream -- consumed, less what commits gave back (a view of the
                 state: it follows the stream)
    consumed     (B,) int32 device tensor: frames consumed per stream since its reset (== frames without a commit)
    room         (B,) int32 device tensor: frames a stream can still take, max_frames - frames
    overflowed   (B,) bool device tensor: frames were dropped because the stream was full

    lm may be a `CtcBiasedLm` -- an LM with a second automaton (hotwords) beside it, as in `ctc_beam_search_lm`: the
        stream then carries a second state per slot, reset() restarts the selected streams in both start states, and any
        chunking still gives the one-shot call's bits.  Hotwords without an LM: lm=CtcHotwords(...), lm_weight=1.0.

    A stream holds at most max_frames frames.  On the host the object sums the chunk widths Tc fed since the last FULL
    reset() and raises ValueError before launching anything once the sum would exceed max_frames; this bound is
    conservative (it ignores `lengths`) and needs no synchronisation.  A partial reset does not lower it: the streams
    that continue still hold their frames.  What the host cannot see -- replays of a captured graph -- the device
    handles: a stream takes frames up to max_frames, ignores the rest of the chunk and sets `overflowed`.  The host
    cannot see what a commit freed either: from the first commit() until the next full reset() the host-side sum is not
    enforced and the device rule stands alone -- watch `room` and `overflowed`.

    Argument checks as the one-shot functions (1 <= nbest <= beam <= 64, 1 <= candidates <= 128 with None meaning
    min(2 * beam, 128), the LM's device, its backoff_id against C).  No autograd; no host synchronisation in `advance`
    or `results`: both can be captured in a `torch.cuda.graph` when the lengths are on the device."""

    def __init__(self, batch, max_frames, beam=16, blank=0, lm=None, lm_weight=0.5, length_bonus=0.0, candidates=None,
                 device=None):
        batch, max_frames, beam, blank = int(batch), int(max_frames), int(beam), int(blank)
        if not 1 <= beam <= MAX_BEAM:
            raise ValueError("need 1 <= beam <= %d, got beam=%d" % (MAX_BEAM, beam))
        v = self._search = _Search(lm, lm_weight, length_bonus, False).sized(beam, candidates)
        if batch < 1 or max_frames < 1 or blank < 0:
            raise ValueError("need batch >= 1, max_frames >= 1 and blank >= 0, got %d, %d, %d" % (batch, max_frames, blank))
        self.device = _hip_device(device, "cuda" if v.lm is None else v.lm.device, "CtcBeamStream")
        v.check_against(0, self.device, "the stream")   # (no class yet: the devices alone)
        self.lm, self.bias, self.bias_weight = v.lm, v.bias, v.bias_weight
        self.lm_weight, self.length_bonus, self.candidates = v.lm_weight, v.length_bonus, v.candidates
        self.batch, self.max_frames, self.beam, self.blank = batch, max_frames, beam, blank
        nbytes = v.size("stream_state_bytes", batch, max_frames, beam)
        if nbytes == 0:
            raise ValueError("(batch,max_frames,beam) = (%d,%d,%d) not supported" % (batch, max_frames, beam))
        tables = v.size(v.scratch_bytes, batch, max_frames, beam)
        rec = (nbytes - tables) // batch                # the record's size is the library's: the blob is tables + records
        self.classes = None                             # C, fixed by the first advance
        self._fed = 0                                   # chunk widths since the last full reset
        self._committed = False                         # a commit since then: the host's bound is off
        self._commit_scratch = None
        with torch.cuda.device(self.device):
            self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._hdr = self._state[tables:].view(torch.int32).view(batch, rec // 4)
        self._dims = (batch, max_frames, beam) + v.dims         # behind the state in reset and results
        self._fsts, self._starts = v.fsts(False), v.starts()    # flattened once: the automata do not change
        self.reset()

    @property
    def frames(self):
        return self._hdr[:, STREAM_FRAMES_WORD]

    @property
    def overflowed(self):
        return self._hdr[:, STREAM_OVERFLOW_WORD] != 0

    @property
    def consumed(self):
        return self._hdr[:, STREAM_FRAMES_WORD] + self._hdr[:, STREAM_RETIRED_WORD]

    @property
    def room(self):
        return self.max_frames - self._hdr[:, STREAM_FRAMES_WORD]

    def _which(self, which):
        """A selection of streams as the C ABI takes it: None, or (B,) int32 on the device."""
        if which is not None:
            which = torch.as_tensor(which)
            if which.dtype not in (torch.bool, torch.int32, torch.int64):
                raise TypeError("which must be bool, int32 or int64, got %s" % which.dtype)
            which = which.reshape(-1).to(self.device, torch.int32).contiguous()
            if which.numel() != self.batch:
                raise ValueError("which must hold batch = %d entries" % self.batch)
        return which

    def reset(self, which=None):
        which = self._which(which)
        v = self._search
        with torch.cuda.device(self.device):
            v.call("stream_reset", *((_ptr(self._state),) + self._dims + self._starts + (_ptr(which), _stream())))
        if which is None:
            self._fed = 0
            self._committed = False

    def commit(self, which=None, max_tail=None):
        which = self._which(which)
        if max_tail is None:
            max_tail = -1
        else:
            max_tail = int(max_tail)
            if max_tail < 0:
                raise ValueError("max_tail must be None or >= 0, got %d" % max_tail)
        B, L, dev, v = self.batch, self.max_frames, self.device, self._search
        with torch.cuda.device(dev):
            if self._commit_scratch is None:
                nbytes = v.size("stream_commit_scratch_bytes", B, L, self.beam)
                self._commit_scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            tokens = torch.empty((B, L), dtype=torch.int32, device=dev)
            lengths = torch.empty(B, dtype=torch.int32, device=dev)
            v.call("stream_commit", *((_ptr(self._state),) + self._dims + (
                _ptr(which), max_tail, L, _ptr(tokens), _ptr(lengths), _ptr(self._commit_scratch), _stream())))
        self._committed = True
        return tokens, lengths

    def _advance(self, x, what, lengths, logits):
        x, _ = _check_input(x, what, "CtcBeamStream", self.blank)
        Tc, B, C = x.shape
        if B != self.batch:
            raise ValueError("%s holds %d streams, the object %d" % (what, B, self.batch))
        if self.classes is not None and C != self.classes:
            raise ValueError("%s has %d classes, the chunks before had %d" % (what, C, self.classes))
        if x.device != self.device:
            raise ValueError("the stream lives on %s, %s on %s" % (self.device, what, x.device))
        v = self._search
        v.check_against(C, self.device, "the stream")
        if not self._committed and self._fed + Tc > self.max_frames:
            raise ValueError("%d frames were fed since the last full reset: %d more exceed max_frames = %d"
                             % (self._fed, Tc, self.max_frames))
        if lengths is None:
            with torch.cuda.device(self.device):
                lengths = torch.full((B,), Tc, dtype=torch.int32, device=self.device)
        x, il, blank_lp, top_val, top_idx, lse, _ = _decode_rows(x, what, lengths, self.blank, self.candidates, logits)
        with torch.cuda.device(self.device):
            v.call("stream_advance", *((_ptr(x), x.stride(0), x.stride(1), _ptr(lse), _ptr(blank_lp), _ptr(top_val),
                                        _ptr(top_idx), _ptr(il), B, Tc, C, self.blank, self.beam) + self._fsts + v.weights + (
                                            _ptr(self._state), self.max_frames, _stream())))
        self.classes = C
        self._fed += Tc

    def advance(self, log_probs, lengths=None):
        self._advance(log_probs, "log_probs", lengths, False)

    def advance_from_logits(self, logits, lengths=None):
        self._advance(logits, "logits", lengths, True)

    def results(self, nbest=1, use_final=True):
        nbest = int(nbest)
        _nbest_outputs(self.beam, nbest)
        B, L, dev, v = self.batch, self.max_frames, self.device, self._search
        with torch.cuda.device(dev):
            out = (torch.empty((B, nbest, L), dtype=torch.int32, device=dev),
                   torch.empty((B, nbest), dtype=torch.int32, device=dev),
                   torch.empty((B, nbest), dtype=torch.float32, device=dev))
            if v.fused:
                out += (torch.empty((B, nbest), dtype=torch.float32, device=dev),)
            v.call("stream_results", *((_ptr(self._state),) + self._dims + self._fsts + v.results_weights + (
                (int(bool(use_final)),) if v.fused else ()) + (nbest, L) + tuple(_ptr(o) for o in out) + (_stream(),)))
        return out


def _nbest_input(x, what, input_lengths, tokens, lengths, blank, max_len, logits):
    """The checks and device copies the n-best calls share: (x as (T,B,C) with unit class stride, detached; il i32;
    lse (T,B) or None; tokens i32 (B,N,L); lengths i32 (B,N); max_len; unbatched)."""
    blank = int(blank)
    tokens, lengths = torch.as_tensor(tokens), torch.as_tensor(lengths)
    for name, t in (("tokens", tokens), ("lengths", lengths)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    if tokens.dim() not in (2, 3) or lengths.dim() != tokens.dim() - 1 or tokens.shape[:-1] != lengths.shape:
        raise ValueError("tokens must be (B,N,L) and lengths (B,N) -- (N,L) and (N,) for (T,C) input -- got %s and %s"
                         % (tuple(tokens.shape), tuple(lengths.shape)))
    N, L = int(tokens.shape[-2]), int(tokens.shape[-1])
    if N < 1 or L < 1:
        raise ValueError("tokens has an empty dimension: %s" % (tuple(tokens.shape),))
    max_len = min(L, (MAX_STATES - 1) // 2) if max_len is None else int(max_len)
    if max_len < 0 or 2 * max_len + 1 > MAX_STATES:
        raise ValueError("need 0 <= max_len and 2*max_len+1 <= %d, got max_len=%d" % (MAX_STATES, max_len))
    if logits:      # the row pass with K = 1 writes the (T,B) log-sum-exps
        x, il, _, _, _, lse, unbatched = _decode_rows(x, what, input_lengths, blank, 1, True)
    else:
        (x, il, unbatched), lse = _rows_input(x, what, input_lengths, blank), None
    T, B, C = x.shape
    if unbatched != (tokens.dim() == 2) or (not unbatched and tokens.shape[0] != B):
        raise ValueError("%s is %s: tokens must be %s, got %s" % (
            what, tuple(x.shape[::2]) if unbatched else tuple(x.shape), "(N,L)" if unbatched else "(%d,N,L)" % B,
            tuple(tokens.shape)))
    tokens = tokens.to(x.device, torch.int32).contiguous().reshape(B, N, L)
    lengths = lengths.to(x.device, torch.int32).contiguous().reshape(B, N)
    return x, il, lse, tokens, lengths, max_len, unbatched


def _nbest_align(x, what, input_lengths, tokens, lengths, blank, max_len, logits):
    blank = int(blank)
    x, il, lse, tokens, lengths, max_len, unbatched = _nbest_input(x, what, input_lengths, tokens, lengths, blank,
                                                                   max_len, logits)
    (T, B, C), (N, L) = x.shape, tokens.shape[1:]
    lib = _lib.lib()
    nbytes = lib.pika_ctc_nbest_align_scratch_bytes(B, N, T, max_len)
    if nbytes == 0:
        raise ValueError("(B,N,T,max_len) = (%d,%d,%d,%d) not supported" % (B, N, T, max_len))
    with torch.cuda.device(x.device):
        out = (torch.empty((B, N), dtype=torch.float32, device=x.device),
               torch.empty((B, N), dtype=torch.float32, device=x.device),
               torch.empty((B, N, L), dtype=torch.int32, device=x.device),
               torch.empty((B, N, L), dtype=torch.int32, device=x.device),
               torch.empty((B, N, L), dtype=torch.float32, device=x.device))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.pika_ctc_nbest_align(_ptr(x), x.stride(0), x.stride(1), _ptr(lse), _ptr(il), _ptr(tokens),
                                            _ptr(lengths), B, N, L, T, C, blank, max_len, *(
                                                tuple(_ptr(o) for o in out) + (_ptr(scratch), _stream()))),
                   "pika_ctc_nbest_align")
    return tuple(o[0] for o in out) if unbatched else out


def ctc_nbest_align(log_probs, input_lengths, tokens, lengths, blank=0, max_len=None):
    """Token times, token scores and full-sum scores for an n-best list: what `ctc_align` and `ctc_loss` give for one
    transcript per utterance, for the `nbest` hypotheses of every utterance, without replicating the input.

    log_probs (T,B,C) or (T,C) float32 on a HIP device, any outer strides (one copy only when the class stride is not
    1); input_lengths (B,) int32 or int64, on the CPU or the device, clamped on the device to [1,T].  tokens (B,N,L)
    and lengths (B,N), int32 or int64, on either side: exactly what `ctc_beam_search*`, `ctc_beam_search_lm*` and
    `CtcBeamStream.results` return.  L need not equal T; a length below 0 marks a missing entry; tokens at or beyond an
    entry's length are never read.  (T,C) input takes (N,L) / (N,) and returns outputs without the batch axis.
    `max_len` (a host int; default min(L, 511)) sizes the state axis: ValueError when 2 * max_len + 1 > 1024 or
    max_len < 0.  The limit is on max_len, not on L.

    Returns (full_scores (B,N) f32, best_scores (B,N) f32, starts (B,N,L) i32, ends (B,N,L) i32, token_scores (B,N,L)
    f32), per hypothesis of length U over its utterance's T_b frames:
      full_scores   log of the sum over ALL alignments: -ctc_loss(reduction='none') for that transcript, with the
                    loss's numerics.  The search's `scores` / `am_scores` sum only the paths the beam kept: a lower
                    bound that depends on `beam` and `candidates`; this does not.
      best_scores   the log-probability of the best (Viterbi) path, `ctc_align`'s value and tie rule: at the end the
                    final blank is preferred to the last label; in the back-trace stay, then s-1, then s-2.
      starts, ends  the first and last frame (inclusive) of the run in which that path emits token j
      token_scores  the sum over t = starts[j] .. ends[j] of log_probs[t, b, token j], in fp32 in increasing t;
                    exp(token_scores / (ends - starts + 1)) is the token's confidence, the geometric mean of its
                    frame posteriors.
    Beyond an entry's length starts / ends are -1 and token_scores -inf.  A missing entry has both scores -inf, times
    -1 and token scores -inf; so has an infeasible one (T_b < U + adjacent repeats, a token outside [0,C), a token
    equal to blank) -- not a fault.  An entry longer than max_len has both scores NaN (per-token outputs as a missing
    entry), which tells it from an infeasible one.  The empty hypothesis has full = best = the sum of the blank's
    log-probs.

    No autograd here -- `ctc_nbest_loss` returns the same `full_scores` with their gradient; no host synchronisation;
    capturable in a `torch.cuda.graph` with all lengths on the device; two runs give bit-identical outputs.

    Streams: `CtcBeamStream.results` tails are relative to the last commit, and a stream does not keep its
    log-probabilities.  A caller who keeps them aligns committed + tail against the whole input."""
    return _nbest_align(log_probs, "log_probs", input_lengths, tokens, lengths, blank, max_len, False)


def ctc_nbest_align_from_logits(logits, input_lengths, tokens, lengths, blank=0, max_len=None):
    """`ctc_nbest_align` of log_softmax(logits, -1) without materialising the log-probabilities: every value is
    logit - lse rounded once, the rows' log-sum-exps coming from the decoders' row pass."""
    return _nbest_align(logits, "logits", input_lengths, tokens, lengths, blank, max_len, True)


class _NbestLossFn(torch.autograd.Function):
    """full_scores (B,N) of an n-best list; backward writes the dense (T,B,C) gradient once, every hypothesis's
    occupancies already weighted by grad_output.  `x` carries the graph; `xd` is the same data as the kernels read it."""

    @staticmethod
    def forward(ctx, x, xd, lse, il, tokens, lengths, blank, max_len):
        lib = _lib.lib()
        (T, B, C), (N, L) = xd.shape, tokens.shape[1:]
        nbytes = lib.pika_ctc_nbest_loss_workspace_bytes(B, N, T, max_len)
        if nbytes == 0:
            raise ValueError("(B,N,T,max_len) = (%d,%d,%d,%d) not supported" % (B, N, T, max_len))
        with torch.cuda.device(xd.device):
            full = torch.empty((B, N), dtype=torch.float32, device=xd.device)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
            _lib.check(lib.pika_ctc_nbest_loss_forward(_ptr(xd), xd.stride(0), xd.stride(1), _ptr(lse), _ptr(il),
                                                       _ptr(tokens), _ptr(lengths), B, N, L, T, C, blank, max_len,
                                                       _ptr(full), _ptr(ws), _stream()), "pika_ctc_nbest_loss_forward")
        ctx.save_for_backward(*((xd, il, ws) + ((lse,) if lse is not None else ())))
        ctx.dims = (T, B, C, N, blank, max_len, tuple(x.shape))
        return full

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_scores):
        T, B, C, N, blank, max_len, shape = ctx.dims
        xd, il, ws = ctx.saved_tensors[:3]
        lse = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        lib = _lib.lib()
        gs = grad_scores.to(torch.float32).contiguous()
        with torch.cuda.device(ws.device):
            grads = torch.empty((T, B, C), dtype=torch.float32, device=ws.device)
            _lib.check(lib.pika_ctc_nbest_loss_backward(_ptr(xd), xd.stride(0), xd.stride(1), _ptr(lse), _ptr(il), B, N,
                                                        T, C, blank, max_len, _ptr(gs), _ptr(ws), _ptr(grads),
                                                        _stream()), "pika_ctc_nbest_loss_backward")
        return grads.reshape(shape), None, None, None, None, None, None, None


def _nbest_loss(x, what, input_lengths, tokens, lengths, blank, max_len, logits):
    blank = int(blank)
    xd, il, lse, tokens, lengths, max_len, unbatched = _nbest_input(x, what, input_lengths, tokens, lengths, blank,
                                                                    max_len, logits)
    full = _NbestLossFn.apply(x, xd, lse, il, tokens, lengths, blank, max_len)
    return full[0] if unbatched else full


def ctc_nbest_loss(log_probs, input_lengths, tokens, lengths, blank=0, max_len=None):
    """The full-sum scores of an n-best list, DIFFERENTIABLE: `ctc_nbest_align`'s `full_scores` (B,N) f32 -- per
    hypothesis -ctc_loss(reduction='none') of that transcript, with the loss's numerics -- carrying autograd to
    `log_probs`, without replicating the (T,B,C) input N times.  Whatever is built on the scores with torch (MWER as
    `ctc_mwer_loss`, sMBR-style risks, cross-entropy over the list) back-propagates through ONE dense (T,B,C) gradient.

    Arguments, checks, strides, the (T,C) form (tokens (N,L), lengths (N,), result (N,)) and `max_len` are
    `ctc_nbest_align`'s, and so is the classification of an entry: a missing one (length < 0) and an infeasible one
    (T_b < U + adjacent repeats, a token outside [0,C), a token equal to blank) score -inf, one longer than max_len NaN.
    Such an entry is dead: it adds nothing to the gradient, and the gradient that arrives for it is ignored -- NaN or
    +-inf there (a softmax over -inf scores produces them) never reaches the input's gradient.

    The gradient is the true derivative, as `ctc_loss`'s: for weights g = d L / d full_scores,
    grad[t,b,c] = sum_k g[b,k] * occ_k(t,c) for t < T_b and exactly 0 beyond; it is dense, contiguous and written once,
    the hypotheses summed in increasing k without atomics, so two runs are bit-identical.  No double backward.  The
    backward workspace, 8 * B * N * T * Wp bytes of planes (Wp = 2 * max_len + 1 rounded up to 64) plus small rows, is
    filled whether or not the input requires grad; pass `max_len` = the longest hypothesis to keep it small.

    No host synchronisation; forward and backward are capturable in a `torch.cuda.graph` with all lengths on the
    device."""
    return _nbest_loss(log_probs, "log_probs", input_lengths, tokens, lengths, blank, max_len, False)


def ctc_nbest_loss_from_logits(logits, input_lengths, tokens, lengths, blank=0, max_len=None):
    """`ctc_nbest_loss` of log_softmax(logits, -1) without materialising the log-probabilities: every value is
    logit - lse rounded once, the rows' log-sum-exps coming from the decoders' row pass, and the backward writes
    d/d logits: grad[t,b,c] = sum_k g[b,k] * occ_k(t,c) - (sum of g over the live entries of b) * softmax_t(c)."""
    return _nbest_loss(logits, "logits", input_lengths, tokens, lengths, blank, max_len, True)


def _mwer(full, errors, reduction):
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("%r is not a valid value for reduction" % (reduction,))
    errors = torch.as_tensor(errors)
    if not errors.is_floating_point():
        raise TypeError("errors must be a float tensor, got %s" % errors.dtype)
    if tuple(errors.shape) != tuple(full.shape):
        raise ValueError("errors must be %s as the n-best list, got %s" % (tuple(full.shape), tuple(errors.shape)))
    live = torch.isfinite(full)                               # a dead entry scores -inf or NaN
    err = torch.where(live, errors.to(full.device, full.dtype), torch.zeros_like(full))
    score = torch.where(live, full, torch.full_like(full, float("-inf")))
    top = score.detach().max(-1, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))     # no live entry: exp(-inf - 0) = 0
    w = torch.where(live, (score - top).exp(), torch.zeros_like(full))
    total = w.sum(-1, keepdim=True)
    p = w / torch.where(total > 0, total, torch.ones_like(total))
    count = live.sum(-1, keepdim=True).clamp(min=1).to(full.dtype)
    risk = (p * (err - err.sum(-1, keepdim=True) / count)).sum(-1)
    if reduction == "mean":
        return risk.mean()
    if reduction == "sum":
        return risk.sum()
    return risk


def ctc_mwer_loss(log_probs, input_lengths, tokens, lengths, errors, blank=0, max_len=None, reduction='mean'):
    """Minimum word error rate (MWER / minimum Bayes risk) training over an n-best list, the CTC counterpart of
    `pika_amd.mbr`: plain torch on top of `ctc_nbest_loss`, one dense gradient whatever N is.

    `errors` (B,N) -- (N,) for (T,C) input -- is a float tensor of per-hypothesis error counts supplied by the caller
    (`ctc_nbest_errors` gives token edit distances), on the CPU or the device.  Over the LIVE entries of every utterance
    (finite full-sum score): P = softmax(full_scores), risk_b = sum_k P_k * (errors_k - mean_live(errors)).  Dead entries
    (missing, infeasible, longer than max_len: `ctc_nbest_loss`) get weight 0 and their `errors` are ignored; an
    utterance with no live entry has risk 0 and a zero gradient.  reduction: 'none' -> (B,), 'sum', 'mean' (the average
    over the batch).  The other arguments, synchronisation and graph capture are `ctc_nbest_loss`'s."""
    full = ctc_nbest_loss(log_probs, input_lengths, tokens, lengths, blank, max_len)
    return _mwer(full, errors, reduction)


def ctc_mwer_loss_from_logits(logits, input_lengths, tokens, lengths, errors, blank=0, max_len=None, reduction='mean'):
    """`ctc_mwer_loss` of log_softmax(logits, -1) without materialising the log-probabilities."""
    full = ctc_nbest_loss_from_logits(logits, input_lengths, tokens, lengths, blank, max_len)
    return _mwer(full, errors, reduction)


def ctc_nbest_errors(tokens, lengths, targets, target_lengths):
    """Token edit (Levenshtein) distances of an n-best list to the reference transcripts, the `errors` of
    `ctc_mwer_loss`: (B,N) float32 on the device of `tokens` (the CPU for a sequence).

    tokens (B,N,L) and lengths (B,N) as a search returns them; targets (B,S) padded and target_lengths (B,), int32 or
    int64, on either side.  (N,L) / (N,) with 1-D targets and a scalar length for one utterance: (N,).  An entry with
    length < 0 (missing) gets 0; a length beyond L counts L tokens.  HOST CODE (`pika_amd.mbr.edit_distances`): inputs
    on the device are copied to the host, which SYNCHRONISES -- call it outside a captured graph."""
    from .mbr import edit_distances
    tokens, lengths = torch.as_tensor(tokens), torch.as_tensor(lengths)
    targets, target_lengths = torch.as_tensor(targets), torch.as_tensor(target_lengths)
    for name, t in (("tokens", tokens), ("lengths", lengths), ("targets", targets), ("target_lengths", target_lengths)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    unbatched = tokens.dim() == 2
    if unbatched:
        tokens, lengths = tokens.unsqueeze(0), lengths.unsqueeze(0)
        targets, target_lengths = targets.reshape(1, -1), target_lengths.reshape(1)
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]):
        raise ValueError("tokens must be (B,N,L) and lengths (B,N) -- (N,L) and (N,) for one utterance -- got %s and %s"
                         % (tuple(tokens.shape), tuple(lengths.shape)))
    B, N, L = tokens.shape
    if targets.dim() != 2 or targets.shape[0] != B or tuple(target_lengths.shape) != (B,):
        raise ValueError("targets must be (B,S) = (%d,S) and target_lengths (%d,), got %s and %s"
                         % (B, B, tuple(targets.shape), tuple(target_lengths.shape)))
    tok, ln = tokens.cpu().tolist(), lengths.cpu().tolist()
    tg, tl = targets.cpu().tolist(), target_lengths.cpu().tolist()
    where = [(b, k) for b in range(B) for k in range(N) if ln[b][k] >= 0]
    dist = edit_distances([(tok[b][k][:min(ln[b][k], L)], tg[b][:max(0, min(tl[b], len(tg[b])))]) for b, k in where])
    out = torch.zeros((B, N), dtype=torch.float32)
    for (b, k), d in zip(where, dist):
        out[b, k] = float(d)
    out = out.to(tokens.device)
    return out[0] if unbatched else out


MAX_EDIT_REF = 4096     # PIKA_EDIT_MAX_REF: 64 blocks of 64 reference positions, one block's state per lane


def _edit_list(tokens, lengths, who):
    """The checks on an n-best list the edit-distance calls share: (tokens (B,N,L), lengths (B,N), unbatched)."""
    tokens, lengths = torch.as_tensor(tokens), torch.as_tensor(lengths)
    for name, t in (("tokens", tokens), ("lengths", lengths)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    unbatched = tokens.dim() == 2
    if unbatched:
        tokens, lengths = tokens.unsqueeze(0), lengths.unsqueeze(0)
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]):
        raise ValueError("%s: tokens must be (B,N,L) and lengths (B,N) -- (N,L) and (N,) for one utterance -- got %s and %s"
                         % (who, tuple(tokens.shape[1:] if unbatched else tokens.shape),
                            tuple(lengths.shape[1:] if unbatched else lengths.shape)))
    return tokens, lengths, unbatched


def _edit_distance(a_tokens, a_lengths, r_tokens, r_lengths):
    """(B,Na,La), (B,Na), (B,Nr,Lr), (B,Nr) on one device -> (B,Na,Nr) int32, -1 where either entry is missing: the
    kernel for device tensors (no synchronisation), the host entry for CPU tensors."""
    dev = a_tokens.device
    a_tokens, a_lengths, r_tokens, r_lengths = (t.to(dev, torch.int32).contiguous()
                                                for t in (a_tokens, a_lengths, r_tokens, r_lengths))
    (B, Na, La), (Nr, Lr) = a_tokens.shape, r_tokens.shape[1:]
    out = torch.empty((B, Na, Nr), dtype=torch.int32, device=dev)
    lib = _lib.lib()
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            _lib.check(lib.pika_ctc_edit_distance(_ptr(a_tokens), _ptr(a_lengths), Na, La, _ptr(r_tokens),
                                                  _ptr(r_lengths), Nr, Lr, B, _ptr(out), _stream()),
                       "pika_ctc_edit_distance")
    else:
        _lib.check(lib.pika_ctc_edit_distance_host(_ptr(a_tokens), _ptr(a_lengths), Na, La, _ptr(r_tokens),
                                                   _ptr(r_lengths), Nr, Lr, B, _ptr(out)),
                   "pika_ctc_edit_distance_host")
    return out


def ctc_nbest_edit_distance(tokens, lengths, targets, target_lengths):
    """`ctc_nbest_errors` WITHOUT the host: the token edit (Levenshtein) distances of an n-best list to the reference
    transcripts, (B,N) float32 on the device of `tokens`, `torch.equal` to `ctc_nbest_errors` on the same inputs.

    Arguments, shapes, dtypes, the (N,L) / (N,) form with 1-D targets and a scalar length, and the exceptions are
    `ctc_nbest_errors`'s.  A missing entry (length < 0) gets 0; a length beyond L counts L tokens; the target length is
    clamped to [0, S] (a negative one is an empty transcript).  ValueError for S > 4096.  Tokens are compared as int32.

    With all four tensors on the device of `tokens` there is no host synchronisation and the call can be captured in a
    `torch.cuda.graph` -- search, this, and `ctc_mwer_loss` forward and backward make ONE graph.  A tensor that lives
    elsewhere is copied to that device first.  CPU `tokens` take the library's host entry (the same recurrence, one
    thread).  One wave per (hypothesis, reference) pair, Myers' bit-vector recurrence (include/pika_ctc.h,
    `pika_ctc_edit_distance`); integers throughout: two runs are identical.  No autograd."""
    tokens, lengths, unbatched = _edit_list(tokens, lengths, "ctc_nbest_edit_distance")
    targets, target_lengths = torch.as_tensor(targets), torch.as_tensor(target_lengths)
    for name, t in (("targets", targets), ("target_lengths", target_lengths)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    if unbatched:
        targets, target_lengths = targets.reshape(1, -1), target_lengths.reshape(1)
    B = tokens.shape[0]
    if targets.dim() != 2 or targets.shape[0] != B or tuple(target_lengths.shape) != (B,):
        raise ValueError("targets must be (B,S) = (%d,S) and target_lengths (%d,), got %s and %s"
                         % (B, B, tuple(targets.shape), tuple(target_lengths.shape)))
    S = int(targets.shape[1])
    if S > MAX_EDIT_REF:
        raise ValueError("targets are %d wide: at most %d reference tokens" % (S, MAX_EDIT_REF))
    dev = tokens.device
    tl = target_lengths.to(dev).clamp(min=0, max=S)         # with torch: below 0 is empty here, not "missing"
    out = _edit_distance(tokens, lengths.to(dev), targets.to(dev).unsqueeze(1), tl.unsqueeze(1))
    out = out[:, :, 0].clamp(min=0).to(torch.float32)       # -1, a missing entry: 0
    return out[0] if unbatched else out


def ctc_nbest_pairwise_distance(tokens, lengths):
    """The token edit distances between the entries of an n-best list: (B,N,N) float32 -- (N,N) for (N,L) / (N,) -- on
    the device of `tokens`, d[b,i,j] = distance(entry i, entry j) of utterance b.  Exactly symmetric, zero on the
    diagonal, and 0 wherever either entry is missing (length < 0); a length beyond L counts L tokens.  ValueError for
    L > 4096.  tokens / lengths as a search returns them, int32 or int64.  Device tensors: the kernel of
    `ctc_nbest_edit_distance` with the list on both sides, no host synchronisation, capturable; CPU: the host entry."""
    tokens, lengths, unbatched = _edit_list(tokens, lengths, "ctc_nbest_pairwise_distance")
    if tokens.shape[2] > MAX_EDIT_REF:
        raise ValueError("tokens are %d wide: at most %d tokens per entry" % (tokens.shape[2], MAX_EDIT_REF))
    lengths = lengths.to(tokens.device)
    out = _edit_distance(tokens, lengths, tokens, lengths).clamp(min=0).to(torch.float32)
    return out[0] if unbatched else out


def ctc_nbest_mbr_decode(tokens, lengths, scores, scale=1.0):
    """Minimum-Bayes-risk decoding over an n-best list: the entry with the least expected token edit distance to the
    list under the list's own posterior.  Returns (best (B,) int64, risks (B,N) float32) -- a 0-d index and (N,) for
    (N,L) / (N,) / (N,) -- on the device of `tokens`.

    `scores` (B,N) float: a search's `scores` or `ctc_nbest_align`'s `full_scores`.  An entry is LIVE when its length is
    at least 0 and its score is finite.  P = softmax(scale * scores) over the live entries; risks[b,i] = sum_j P_j *
    d(i,j) for live i (d: `ctc_nbest_pairwise_distance`) and +inf for a dead one; best[b] = the arg-min, the lowest index
    on ties, -1 for an utterance with no live entry.  Plain torch on the pairwise distances: no host synchronisation, no
    autograd; ValueError for L > 4096."""
    tokens, lengths, unbatched = _edit_list(tokens, lengths, "ctc_nbest_mbr_decode")
    scores = torch.as_tensor(scores)
    if not scores.is_floating_point():
        raise TypeError("scores must be a float tensor, got %s" % scores.dtype)
    if unbatched:
        scores = scores.unsqueeze(0)
    if tuple(scores.shape) != tuple(lengths.shape):
        raise ValueError("scores must be %s as the n-best list, got %s" % (
            tuple(lengths.shape[1:] if unbatched else lengths.shape), tuple(scores.shape[1:] if unbatched else scores.shape)))
    dev = tokens.device
    dist = ctc_nbest_pairwise_distance(tokens, lengths)                                     # (B,N,N)
    scores = scores.detach().to(dev, torch.float32)
    live = (lengths.to(dev) >= 0) & torch.isfinite(scores)
    score = torch.where(live, float(scale) * scores, torch.full_like(scores, float("-inf")))
    top = score.max(-1, keepdim=True).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))     # no live entry: exp(-inf - 0) = 0
    w = torch.where(live, (score - top).exp(), torch.zeros_like(score))
    total = w.sum(-1, keepdim=True)
    p = w / torch.where(total > 0, total, torch.ones_like(total))
    risks = torch.where(live, (p.unsqueeze(-2) * dist).sum(-1), torch.full_like(score, float("inf")))
    index = torch.arange(risks.shape[-1], device=dev).expand_as(risks)
    lowest = risks.min(-1, keepdim=True).values
    best = torch.where(live & (risks == lowest), index, torch.full_like(index, risks.shape[-1])).min(-1).values
    best = torch.where(live.any(-1), best, torch.full_like(best, -1))
    return (best[0], risks[0]) if unbatched else (best, risks)


LONG_ALIGN_TILE = 896       # states a workgroup of the tiled recurrence owns (csrc/ctc_long.hip: LW)
LONG_ALIGN_FRAMES = 64      # frames per recurrence launch (LF); a tile recomputes the 2 * LONG_ALIGN_FRAMES states below it


def _long_align(x, what, targets, input_lengths, target_lengths, blank, logits):
    blank = int(blank)
    x, unbatched = _check_input(x, what, "ctc_long_align", blank)
    T, B, C = x.shape
    dev = x.device
    targets = torch.as_tensor(targets)
    if targets.dtype not in (torch.int32, torch.int64):
        raise TypeError("targets must be int32 or int64, got %s" % targets.dtype)
    if targets.dim() != (1 if unbatched else 2) or (not unbatched and targets.shape[0] != B):
        raise ValueError("%s is %s: targets must be %s, got %s" % (
            what, tuple(x.shape[::2]) if unbatched else tuple(x.shape), "(U,)" if unbatched else "(%d,U)" % B,
            tuple(targets.shape)))
    U = int(targets.shape[-1])
    targets = targets.to(dev, torch.int32).contiguous().reshape(B, U)
    lengths = []
    for name, t, full in (("input_lengths", input_lengths, T), ("target_lengths", target_lengths, U)):
        if t is None:
            lengths.append(torch.full((B,), full, dtype=torch.int32, device=dev))
            continue
        t = torch.as_tensor(t)
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
        t = t.reshape(-1).to(dev, torch.int32).contiguous()
        if t.numel() != B:
            raise ValueError("%s must hold B = %d entries" % (name, B))
        lengths.append(t)
    il, tl = lengths
    if logits:      # the decoders' row pass with K = 1 writes the (T,B) log-sum-exps
        x, il, _, _, _, lse, _ = _decode_rows(x, what, il, blank, 1, True)
    else:
        (x, il, _), lse = _rows_input(x, what, il, blank), None
    lib = _lib.lib()
    nbytes = lib.pika_ctc_long_align_scratch_bytes(B, T, U)
    if nbytes == 0:
        raise ValueError("(B,T,U_max) = (%d,%d,%d) not supported" % (B, T, U))
    with torch.cuda.device(dev):
        out = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty((B, U), dtype=torch.int32, device=dev),
               torch.empty((B, U), dtype=torch.int32, device=dev), torch.empty((B, U), dtype=torch.float32, device=dev))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        # the output pointers are never written through when U = 0; an empty tensor's may be null
        ptrs = tuple(_ptr(o) or _ptr(scratch) for o in out)
        _lib.check(lib.pika_ctc_long_align(_ptr(x), x.stride(0), x.stride(1), _ptr(lse), _ptr(il),
                                           _ptr(targets) if U else None, _ptr(tl), B, T, C, blank, U, *(
                                               ptrs + (_ptr(scratch), _stream()))), "pika_ctc_long_align")
    return tuple(o[0] for o in out) if unbatched else out


def ctc_long_align(log_probs, targets, input_lengths=None, target_lengths=None, blank=0):
    """Long-form forced alignment: the best (Viterbi) path of one transcript per recording, with no limit of 511 labels
    and no plane in memory -- an hour of audio against its whole transcript, which is what cuts audiobooks, meetings and
    broadcast into utterances, and what gives a long stream's committed text its time stamps.

    log_probs (T,B,C) or (T,C) float32 on a HIP device, any outer strides (one copy only when the class stride is not
    1).  targets (B,U) -- (U,) for (T,C) input -- int32 or int64, padded; entries at or beyond a length are never read.
    input_lengths / target_lengths (B,) int32 or int64 on either side, None meaning full (T, U); clamped on the device
    to [1,T] and [0,U].

    Returns (scores (B,) f32, starts (B,U) i32, ends (B,U) i32, token_scores (B,U) f32), detached -- without the batch
    axis for (T,C) input:
      scores        the log-probability of the best path
      starts, ends  the first and last frame (inclusive) of the run in which the path emits token j
      token_scores  the sum over that run of log_probs[t, b, token j], in fp32 in increasing t
    Beyond a length starts / ends are -1 and token_scores -inf.  An infeasible transcript (a token outside [0,C), a token
    equal to blank, T_b < U_b + adjacent repeats) has score -inf, times -1 and token scores -inf: not a fault.

    The path is `ctc_align`'s wherever both run (the same fp32 max-plus and tie rule: at the end the final blank over the
    last label; in the back-trace stay, then s-1, then s-2), and the per-token outputs are `ctc_nbest_align`'s.  Inside,
    every frame's values are taken relative to the frame's maximum, which moves all paths alike and keeps a good path's
    running score near 0 over 1e5 frames; the state axis is cut into tiles of LONG_ALIGN_TILE states and time into
    blocks of LONG_ALIGN_FRAMES frames, one launch per block.  Back-pointers take two bits per cell: T * (2U+1) / 4
    bytes of scratch per recording.

    A wildcard ("star") token needs no kernel support: append a class column holding whatever score garbage should get
    and put that class into `targets` wherever unknown speech may sit.

    No autograd; no host synchronisation; capturable in a `torch.cuda.graph` with the lengths on the device; two runs
    give bit-identical outputs.  `ctc_segment_scores` turns the result into utterance cuts."""
    return _long_align(log_probs, "log_probs", targets, input_lengths, target_lengths, blank, False)


def ctc_long_align_from_logits(logits, targets, input_lengths=None, target_lengths=None, blank=0):
    """`ctc_long_align` of log_softmax(logits, -1) without materialising the log-probabilities: every value is
    logit - lse rounded once, the rows' log-sum-exps coming from the decoders' row pass.  The recurrence itself runs on
    logit minus the row's largest logit, which does not depend on lse."""
    return _long_align(logits, "logits", targets, input_lengths, target_lengths, blank, True)


def ctc_segment_scores(starts, ends, token_scores, segment_offsets):
    """An alignment cut into segments (utterances): (seg_start (B,G) int, seg_end (B,G) int, seg_confidence (B,G) f32).

    starts, ends, token_scores (B,U) -- or (U,) -- as `ctc_long_align` / `ctc_nbest_align` return them, on either
    device.  segment_offsets (G+1,) shared by the batch, or (B,G+1): token indices, segment g covering tokens
    [o_g, o_{g+1}).  seg_start is the start of the segment's first token, seg_end the end of its last token, and
    seg_confidence = exp(sum token_scores / sum (ends - starts + 1)), the geometric mean of the frame posteriors of the
    segment's tokens.  An empty segment, and any segment that holds a token without a run (an infeasible row, tokens
    beyond a length), gives -1, -1 and NaN.  Plain torch (cumsum and gather): no host synchronisation, no autograd."""
    starts, ends, ts = torch.as_tensor(starts), torch.as_tensor(ends), torch.as_tensor(token_scores).detach()
    if starts.dim() not in (1, 2) or starts.shape != ends.shape or starts.shape != ts.shape:
        raise ValueError("starts, ends and token_scores must share one shape (B,U) or (U,), got %s, %s, %s"
                         % (tuple(starts.shape), tuple(ends.shape), tuple(ts.shape)))
    unbatched = starts.dim() == 1
    if unbatched:
        starts, ends, ts = starts.unsqueeze(0), ends.unsqueeze(0), ts.unsqueeze(0)
    B, U = starts.shape
    dev = starts.device
    off = torch.as_tensor(segment_offsets).to(dev)
    if off.dtype not in (torch.int32, torch.int64):
        raise TypeError("segment_offsets must be int32 or int64, got %s" % off.dtype)
    if off.dim() == 1:
        off = off.unsqueeze(0).expand(B, -1)
    if off.dim() != 2 or off.shape[0] != B or off.shape[1] < 1:
        raise ValueError("segment_offsets must be (G+1,) or (%d,G+1), got %s" % (B, tuple(off.shape)))
    off = off.long().clamp(0, U)
    o0, o1 = off[:, :-1], off[:, 1:]
    has = (starts >= 0) & (ends >= starts)
    zero = torch.zeros((B, 1), dtype=torch.float64, device=dev)

    def between(v):     # sum of v over tokens [o0, o1), by a running sum with a leading zero
        run = torch.cat([zero, v.to(torch.float64).cumsum(1)], 1)
        return run.gather(1, o1) - run.gather(1, o0)
    score = between(torch.where(has, ts.to(dev), torch.zeros_like(ts)))
    frames = between(torch.where(has, ends - starts + 1, torch.zeros_like(starts)))
    good = (o1 > o0) & (between(has) == (o1 - o0))
    pad = torch.full((B, 1), -1, dtype=starts.dtype, device=dev)    # a column to gather from when U = 0
    seg_start = torch.cat([starts, pad], 1).gather(1, o0)
    seg_end = torch.cat([ends, pad], 1).gather(1, (o1 - 1).clamp(min=0))
    seg_start = torch.where(good, seg_start, torch.full_like(seg_start, -1))
    seg_end = torch.where(good, seg_end, torch.full_like(seg_end, -1))
    conf = torch.where(good, (score / frames.clamp(min=1)).exp(), torch.full_like(score, float("nan"))).float()
    out = (seg_start, seg_end, conf)
    return tuple(o[0] for o in out) if unbatched else out


LONG_LOSS_TILE = 896        # states a workgroup of the tiled recurrences owns (csrc/ctc_long_loss.hip: QW)
LONG_LOSS_FRAMES = 64       # frames per recurrence launch (QF); a tile recomputes 2 * LONG_LOSS_FRAMES states beside its own


def _padded_targets(targets, toff, tl, U):
    """Targets as the tiled kernels take them, (B,U) padded: the 1-D form is spread out by torch, without a host
    synchronisation (U is already known on the host)."""
    if toff is None:
        return targets
    B, n = tl.numel(), targets.numel()
    if U == 0 or n == 0:
        return targets.new_zeros((B, U))
    pos = torch.arange(U, device=targets.device)[None, :]
    idx = (toff.to(torch.int64)[:, None] + pos).clamp(0, n - 1)
    return torch.where(pos < tl[:, None], targets[idx], torch.zeros_like(idx, dtype=targets.dtype)).contiguous()


class _CTCLongFn(torch.autograd.Function):
    """`_CTCFn` on the tiled kernels: per-utterance costs (B,), any number of labels; the backward writes the dense
    (T,B,C) gradient once, already scaled by grad_output.  Reads x through its two outer strides."""

    @staticmethod
    def forward(ctx, x, targets, il, tl, U, blank, logits, what):
        xd = x.detach()
        if logits:      # the decoders' row pass with K = 1 writes the (T,B) log-sum-exps
            xd, il, _, _, _, lse, _ = _decode_rows(xd, what, il, blank, 1, True)
        else:
            (xd, il, _), lse = _rows_input(xd, what, il, blank), None
        T, B, C = xd.shape
        lib = _lib.lib()
        nbytes = lib.pika_ctc_long_loss_workspace_bytes(B, T, U)
        if nbytes == 0:
            raise ValueError("(B,T,U_max) = (%d,%d,%d) not supported" % (B, T, U))
        with torch.cuda.device(xd.device):
            costs = torch.empty(B, dtype=torch.float32, device=xd.device)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
            _lib.check(lib.pika_ctc_long_loss_forward(_ptr(xd), xd.stride(0), xd.stride(1), _ptr(lse), _ptr(il),
                                                      _ptr(targets) if U else None, _ptr(tl), B, T, C, blank, U,
                                                      _ptr(costs), _ptr(ws), _stream()), "pika_ctc_long_loss_forward")
        ctx.save_for_backward(xd, il, tl, ws, *((lse,) if logits else ()))
        ctx.dims = (T, B, C, U, blank)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        T, B, C, U, blank = ctx.dims
        xd, il, tl, ws = ctx.saved_tensors[:4]
        lse = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        lib = _lib.lib()
        gc = grad_costs.to(torch.float32).contiguous()
        with torch.cuda.device(ws.device):
            grads = torch.empty((T, B, C), dtype=torch.float32, device=ws.device)
            _lib.check(lib.pika_ctc_long_loss_backward(_ptr(xd), xd.stride(0), xd.stride(1), _ptr(lse), _ptr(il), _ptr(tl),
                                                       B, T, C, blank, U, _ptr(gc), _ptr(ws), _ptr(grads), _stream()),
                       "pika_ctc_long_loss_backward")
        return grads, None, None, None, None, None, None, None


def ctc_long_loss(log_probs, targets, input_lengths, target_lengths, blank=0, reduction='mean', zero_infinity=False):
    """`ctc_loss` with the state axis tiled: the same arguments, shapes, reductions and gradient convention, and no limit
    of 511 labels -- a character-level model on 20-30 s segments, or training on what `ctc_long_align` can align.
    `ctc_loss` itself routes here when 2 * U_max + 1 > 1024; calling it directly runs the tiled kernels at any length.

    log_probs (T,B,C) or (T,C) float32 on a HIP device, read through its outer strides (one copy only when the class
    stride is not 1); targets (B,S) padded or 1-D concatenated (spread out to (B,U_max) by torch); lengths (B,), int32
    or int64, on the CPU or the device, clamped on the device to [1,T] and [0,U_max].  The gradient is the true
    derivative -occ with respect to log_probs; an infeasible utterance (T_b < U_b + adjacent repeats, a label outside
    [0,C)) costs +inf (0 with zero_infinity) and has an all-zero gradient.  The reduction's factors reach the kernel
    folded into grad_costs.

    Inside (csrc/ctc_long_loss.hip): the state axis is cut into tiles of LONG_LOSS_TILE states and time into blocks of
    LONG_LOSS_FRAMES frames; one launch per block advances alpha on block k and beta on block n-1-k, a tile recomputing
    the 2 * LONG_LOSS_FRAMES states beside its own, so tiles meet through stream order only.  Values are fp32 relative
    to each frame's row maximum and, once per block, to the column's maximum; both go into fp64 offsets.  Against
    `ctc_loss`, which renormalises every 8 frames, the fp32 state values are up to LONG_LOSS_FRAMES / 8 times larger.

    MEMORY: both planes are stored for the backward, about 8 * B * T * (2 * U_max + 1) bytes (rounded up to whole
    tiles) -- 0.7 GB for (T,B,U) = (3000,8,1500); an hour against its whole transcript does not fit.  No host
    synchronisation with padded targets and lengths on the device: forward and backward can be captured in one
    `torch.cuda.graph`; two runs give bit-identical results.  No double backward."""
    return _loss(log_probs, "log_probs", targets, input_lengths, target_lengths, blank, reduction, zero_infinity, False,
                 True)


def ctc_long_loss_from_logits(logits, targets, input_lengths, target_lengths, blank=0, reduction='mean',
                              zero_infinity=False):
    """`ctc_long_loss` of log_softmax(logits, -1) without materialising the log-probabilities: the rows' log-sum-exps
    come from the decoders' row pass and the backward writes d/d logits = grad * (softmax - occ), as
    `ctc_loss_from_logits` does."""
    return _loss(logits, "logits", targets, input_lengths, target_lengths, blank, reduction, zero_infinity, True, True)
