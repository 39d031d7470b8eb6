"""CTC-guided frame skipping for the transducer (include/pika_frame_skip.h, csrc/frame_skip.hip; DESIGN.md section 3,
"CTC-guided frame skipping"): a CTC head on the encoder output marks the frames whose blank posterior is at or above a
threshold, and those frames are removed before the joint network sees them (Wang et al., arXiv:2210.16481; Yang et al.,
arXiv:2305.11558; icefall's `frame_reducer.py`).  The search takes one step per frame and every pruned / modified loss is
linear in T, so the gain is the share of the frames dropped, paid for by one row pass and one compaction.

`ctc_skip_plan` decides, `frame_skip_apply` moves the rows (with autograd), `frame_skip_times` maps frame numbers counted
on the reduced axis back, `modified_beam_search_skip` is `modified_beam_search` (`_lm`, `_timed`) on the reduced frames.
Shapes never depend on the data: outputs keep the full (B,T,...) extent, `kept_lengths` says how much of it counts, and
the caller slices after whatever host read it makes anyway.  No entry reads a length on the host.

Training on the reduced frames needs no loss of its own:

    plan = ctc_skip_plan(ctc_logits, frames_lengths, threshold=0.95, min_frames=labels_lengths, from_logits=True)
    enc2 = frame_skip_apply(enc, plan)
    loss = rnnt_pruned_joint_loss_modified(enc2, ..., frames_lengths=plan.kept_lengths, ...)

`min_frames=labels_lengths` keeps T' >= U, which the modified topology needs; the gradient reaches `enc` through
`frame_skip_apply` (zero on the dropped rows) and does not flow through the plan.
"""
import collections
import math

import torch

from . import _lib

MAX_T = 8192            # PIKA_FSKIP_MAX_T
_NATIVE_X = (torch.float32, torch.float16, torch.bfloat16)

FrameSkipPlan = collections.namedtuple("FrameSkipPlan", ("kept_lengths", "frame_index", "position", "blank_lp"))
FrameSkipPlan.__doc__ = """What `ctc_skip_plan` returns, per utterance b with L = clamp(lengths[b], 0, T):
kept_lengths (B,) int32; frame_index (B,T) int32, the original frame of output row j and -1 for j >= kept;
position (B,T) int32, the output row of original frame t and -1 if it was dropped or t >= L; blank_lp (B,T) float32
(float64 for float64 scores), 0 beyond L."""


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _log_threshold(threshold):
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold must not be NaN")
    if threshold <= 0.0:
        return -float("inf")
    # float32(log(threshold)): what the kernels compare against
    return float(torch.tensor(math.log(threshold) if threshold != float("inf") else float("inf"),
                              dtype=torch.float64).float())


def _lengths(t, name, B, T, device):
    t = torch.as_tensor(t)
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    if t.numel() != B:
        raise ValueError("%s must hold B = %d entries" % (name, B))
    return t.reshape(-1).clamp(0, T).to(device, torch.int32).contiguous()


def _native_dims(B, T):
    return T <= MAX_T and B * T <= 0x7fffffff


def _torch_plan(blank_lp, L, min_frames, log_thr):
    """The plan's definition in plain torch on blank_lp (B,T) (any float dtype), L (B,) clamped, min_frames (B,) or None.
    Device operations only: nothing is read on the host."""
    B, T = blank_lp.shape
    dev = blank_lp.device
    L = L.long()
    t = torch.arange(T, device=dev).unsqueeze(0)
    valid = t < L.unsqueeze(1)
    lp = torch.where(valid, blank_lp, torch.zeros_like(blank_lp))
    drop = valid & (lp >= log_thr)                      # a NaN compares false: kept
    natural = (valid & ~drop).sum(1)
    m = torch.ones_like(L) if min_frames is None else min_frames.long()
    m = torch.where(L > 0, torch.minimum(m.clamp(min=1), L), torch.zeros_like(L))
    r = (m - natural).clamp(min=0)
    # the total order (dropped first, blank_lp ascending, t ascending) by two stable sorts
    o1 = torch.sort(torch.where(drop, lp + 0.0, torch.zeros_like(lp)), dim=1, stable=True).indices
    o2 = torch.sort((~drop).gather(1, o1).to(torch.uint8), dim=1, stable=True).indices
    order = o1.gather(1, o2)
    rank = torch.empty_like(order).scatter_(1, order, t.expand(B, T).contiguous())
    kept = (valid & ~drop) | (drop & (rank < r.unsqueeze(1)))
    pos = torch.cumsum(kept.long(), 1) - 1
    position = torch.where(kept, pos, torch.full_like(pos, -1))
    frame_index = torch.full((B, T + 1), -1, dtype=torch.long, device=dev)
    frame_index.scatter_(1, torch.where(kept, pos, torch.full_like(pos, T)), t.expand(B, T).contiguous())
    return FrameSkipPlan(kept.sum(1).to(torch.int32), frame_index[:, :T].to(torch.int32).contiguous(),
                         position.to(torch.int32), lp)


def ctc_skip_plan(scores, lengths, blank=0, threshold=0.95, min_frames=None, from_logits=False, time_major=False):
    """Which frames a CTC head lets the transducer skip.  -> `FrameSkipPlan`.

    scores   (B,T,C), or (T,B,C) with time_major=True as the `ctc_*` functions take it: log-probs, or raw logits with
             from_logits=True (the log-probs are then never materialised).  Any batch and time strides; the class axis
             must be dense (one copy when it is not).
    lengths  (B,) int32 or int64, on the CPU or the device; clamped to [0,T] on the device.
    threshold  a probability: frame t < L is DROPPED iff blank_lp[b,t] >= float32(log(threshold)); a NaN frame is kept.
             threshold > 1 drops nothing.
    min_frames  optional (B,) int: m = clamp(min_frames[b], 1, L) (m = 1 without it, 0 if L = 0).  If fewer than m frames
             are kept, dropped frames are put back in the order (blank_lp ascending, t ascending) until m are kept: a
             silent utterance does not vanish, and min_frames=labels_lengths keeps T' >= U for the modified topology.

    On a HIP device with float32 scores, T <= 8192 and B * T < 2^31 the row pass and the plan are HIP kernels: no host
    synchronisation, no atomics, capturable in a `torch.cuda.graph`, a function of the input alone.  Beyond those limits,
    on the CPU and in float64 the same definition runs in plain torch (half-precision scores in float32)."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 3:
        raise ValueError("scores must be a (B,T,C) tensor (or (T,B,C) with time_major=True)")
    if not scores.is_floating_point():
        raise TypeError("scores must be floating point, got %s" % scores.dtype)
    scores = scores.detach()
    if time_major:
        scores = scores.transpose(0, 1)
    B, T, C = scores.shape
    blank = int(blank)
    if B < 1 or T < 1 or C < 1:
        raise ValueError("scores has an empty dimension: %s" % (tuple(scores.shape),))
    if not 0 <= blank < C:
        raise ValueError("blank=%d outside [0,%d)" % (blank, C))
    log_thr = _log_threshold(threshold)
    dev = scores.device
    L = _lengths(lengths, "lengths", B, T, dev)
    mf = None if min_frames is None else _lengths(min_frames, "min_frames", B, T, dev)
    if scores.is_cuda and scores.dtype == torch.float32 and _native_dims(B, T):
        if C > 1 and scores.stride(2) != 1:
            scores = scores.contiguous()
        lib = _lib.lib()
        with torch.cuda.device(dev):
            blank_lp = torch.empty((B, T), dtype=torch.float32, device=dev)
            kept = torch.empty(B, dtype=torch.int32, device=dev)
            frame_index = torch.empty((B, T), dtype=torch.int32, device=dev)
            position = torch.empty((B, T), dtype=torch.int32, device=dev)
            _lib.check(lib.pika_fskip_rows(_ptr(scores), scores.stride(0), scores.stride(1), _ptr(L), B, T, C, blank,
                                           1 if from_logits else 0, _ptr(blank_lp), _stream()), "pika_fskip_rows")
            _lib.check(lib.pika_fskip_plan(_ptr(blank_lp), _ptr(L), _ptr(mf), B, T, log_thr, _ptr(kept),
                                           _ptr(frame_index), _ptr(position), _stream()), "pika_fskip_plan")
        return FrameSkipPlan(kept, frame_index, position, blank_lp)
    if scores.dtype not in (torch.float32, torch.float64):
        scores = scores.float()
    blank_lp = torch.log_softmax(scores, dim=2)[:, :, blank] if from_logits else scores[:, :, blank]
    return _torch_plan(blank_lp, L, mf, log_thr)


def _gather_rows(x, index):
    """out[b,j,:] = x[b, index[b,j], :] where index >= 0, zeros elsewhere: the apply and, with `position`, its backward."""
    B, T, D = x.shape
    if x.is_cuda and x.dtype in _NATIVE_X and _native_dims(B, T) and D >= 1 and D * x.element_size() <= 0x7fffffff:
        if D > 1 and x.stride(2) != 1:
            x = x.contiguous()
        es = x.element_size()
        with torch.cuda.device(x.device):
            out = torch.empty((B, T, D), dtype=x.dtype, device=x.device)
            _lib.check(_lib.lib().pika_fskip_apply(_ptr(x), x.stride(0) * es, x.stride(1) * es, _ptr(index), B, T,
                                                   D * es, es, _ptr(out), _stream()), "pika_fskip_apply")
        return out
    ok = (index >= 0).unsqueeze(2)
    rows = x.gather(1, index.clamp(min=0).long().unsqueeze(2).expand(B, T, D))
    return torch.where(ok, rows, torch.zeros_like(rows))


class _ApplyFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, frame_index, position):
        ctx.save_for_backward(position)
        return _gather_rows(x, frame_index)

    @staticmethod
    def backward(ctx, dout):
        position, = ctx.saved_tensors
        return _gather_rows(dout, position), None, None


def frame_skip_apply(x, plan):
    """out[b,j,:] = x[b, plan.frame_index[b,j], :] for j < kept_lengths[b], zeros after.  x (B,T,D) -> out (B,T,D): the
    shape is fixed, the caller slices it after whatever host read it already makes.  One plan may be applied to several
    tensors.  Autograd to x: dx[b,t,:] = dout[b, plan.position[b,t], :] where the frame was kept, zeros elsewhere -- every
    row written exactly once in one launch, no atomics, two runs bit-identical.

    On a HIP device float32, float16 and bfloat16 rows are moved by a HIP kernel, bit for bit (16-byte accesses where the
    row's bytes, the strides and both bases allow, element-sized accesses otherwise: the same bytes), without host
    synchronisation and capturable in a `torch.cuda.graph`.  Other dtypes, the CPU and shapes beyond T <= 8192,
    B * T < 2^31 run the same definition in plain torch."""
    if not isinstance(plan, FrameSkipPlan):
        raise TypeError("plan must be a FrameSkipPlan, got %s" % type(plan).__name__)
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("x must be a (B,T,D) tensor")
    B, T = plan.frame_index.shape
    if tuple(x.shape[:2]) != (B, T) or x.shape[2] < 1:
        raise ValueError("x must be (B,T,D) = (%d,%d,D >= 1) as the plan, got %s" % (B, T, tuple(x.shape)))
    if x.device != plan.frame_index.device:
        raise ValueError("x lives on %s, the plan on %s" % (x.device, plan.frame_index.device))
    return _ApplyFn.apply(x, plan.frame_index, plan.position)


def frame_skip_times(times, plan):
    """Frame numbers counted on the reduced axis -> original encoder frames: times (B, ...) integers, each a row j of
    utterance b's reduced frames (as the time stamps of a search on `frame_skip_apply`'s output are) -> same shape and
    dtype, plan.frame_index[b, j]; a -1 (and anything outside [0,T)) stays -1."""
    if not isinstance(plan, FrameSkipPlan):
        raise TypeError("plan must be a FrameSkipPlan, got %s" % type(plan).__name__)
    B, T = plan.frame_index.shape
    if not isinstance(times, torch.Tensor) or times.dim() < 1 or times.shape[0] != B \
            or times.dtype not in (torch.int32, torch.int64):
        raise ValueError("times must be an int32 or int64 tensor (B = %d, ...)" % B)
    flat = times.reshape(B, -1).long()
    ok = (flat >= 0) & (flat < T)
    out = plan.frame_index.long().gather(1, flat.clamp(0, T - 1))
    return torch.where(ok, out, torch.full_like(out, -1)).to(times.dtype).reshape(times.shape)


@torch.no_grad()
def modified_beam_search_skip(model, x, x_len, ctc_head, threshold=0.95, lm=None, timed=False, beam=4, nbest=1,
                              sm_scale=1.0, blank_penalty=0.0, use_graph=True, blank=0, precision="fp16x2",
                              lm_weight=0.5, length_bonus=0.0, candidates=None, use_final=True):
    """`modified_beam_search` (`lm` given: `modified_beam_search_lm`; timed=True: `modified_beam_search_timed`) on the
    frames a CTC head does not skip.  The encoder runs once; `ctc_head(enc_out)` gives (B,T,C) logits; `ctc_skip_plan`
    (from_logits, `threshold`, the same `blank`) and `frame_skip_apply` reduce the frames;
    the search then runs on them in min(max(kept_lengths), T) steps -- reading that number is still the call's single
    host read.  The remaining keywords are the search's.
    -> the search's tuple, then the plan, then the ORIGINAL enc_out: (tokens, lengths, scores[, am_scores][, times], plan,
    enc_out).  With timed=True the times are original encoder frames (`frame_skip_times` applied).  With a threshold above
    1 nothing is dropped and tokens, lengths and scores are `modified_beam_search`'s bit for bit."""
    from .decoder import modified_search as M
    if lm is None and (candidates is not None or lm_weight != 0.5 or length_bonus != 0.0 or use_final is not True):
        raise ValueError("lm_weight, length_bonus, candidates and use_final belong to the search with an LM")
    plans, rec = [], []

    def reduce(enc_out, lengths):
        logits = ctc_head(enc_out)
        plans.append(ctc_skip_plan(logits.float(), lengths, int(blank), threshold, from_logits=True))
        return frame_skip_apply(enc_out, plans[0]), plans[0].kept_lengths

    def make_state(B, T, dev, dtype):
        if lm is None:
            return M.ModifiedBeamState(B, T, int(beam), int(blank), dev, dtype)
        return M.ModifiedLmBeamState(B, T, lm, int(beam), int(blank), lm_weight, length_bonus, candidates, dev)

    def hook(state):
        rec.append(M.ModifiedBeamTimes(state))
        return rec[0].step

    def results(state):
        out = tuple(state.results(nbest=nbest) if lm is None else state.results(nbest=nbest, use_final=use_final))
        if timed:
            out += (frame_skip_times(rec[0].results(out[0], out[1]), plans[0]),)
        return out + (plans[0],)
    return M._drive(model, x, x_len, beam, sm_scale, blank_penalty, use_graph, blank, precision, make_state, results,
                    hook=hook if timed else None, reduce=reduce)
