"""pika_amd -- MI355X-native (gfx950) RNN-Transducer hot path behind PIKA's Python API.

Product code only: hand-written HIP kernels + the C ABI (``csrc/``, ``include/*.h``) and the
host-side mirror of the reference's operator interface (``warp_rnnt.RNNTLoss`` ...).  The
drop-in import surface (``warp_rnnt``, ``trainer.*``, ``decoder.*``, ``loader.*``, ``utils.*``)
lives under ``pika_amd/dropin`` and is put on ``sys.path`` by ``pika_amd.launch``.

Nothing in this package imports ``oracle/`` and there is no CPU fallback: ops raise if the
HIP library is missing or if they are handed non-GPU tensors.
"""
__version__ = "0.1.0"

import os as _os
import sys as _sys


def _hip_graph_workaround():
    """ROCm 7.0 HIP runtime, MI355X: with the runtime's "graph packet capture" fast path (AQL packets pre-built at
    hipGraphInstantiate; DEBUG_CLR_GRAPH_PACKET_CAPTURE, on by default) two graph execs replayed ALTERNATELY with ordinary
    launches in between -- the forward / backward graphs of pika_amd.train_graph around the eager loss, clip and SGD
    launches -- go wrong from about the tenth replay: a replay's kernels run on stale state (the training loss of a
    replayed loop leaves the eager loop's, bit-identical for nine steps, at the tenth; any host synchronisation placed
    between the launches moves the step at which it happens; with the fast path off the two loops agree step for step,
    tools/graph_dropout_diff.py).  The flag is read once, when the HIP runtime initialises, so it is set here, at import
    -- before torch makes its first HIP call in the normal order of imports (`pika_amd.launch`, bench.py and tests/conftest.py
    import this package first; a script that has already called torch.cuda.is_available() gets the eager step).  Decode (one exec replayed back to back) is
    not affected either way and costs the same with the flag off (171 vs 173 ms per batch at configs[4])."""
    if "DEBUG_CLR_GRAPH_PACKET_CAPTURE" in _os.environ:
        return _os.environ["DEBUG_CLR_GRAPH_PACKET_CAPTURE"] == "0"
    # Has the HIP runtime already read its flags?  torch.cuda.is_initialized() only knows about torch's own lazy init --
    # torch.cuda.is_available() / device_count() call hipGetDeviceCount without setting it -- so the question is put to the
    # process itself: the runtime opens /dev/kfd when it starts.  Unknown (no /proc) counts as "already started" when torch
    # is imported: the training step then stays eager, which is slower, never wrong.
    started = None
    try:
        started = False
        for fd in _os.listdir("/proc/self/fd"):
            try:
                if _os.readlink("/proc/self/fd/" + fd) == "/dev/kfd":
                    started = True
                    break
            except OSError:
                pass
    except OSError:
        started = None
    late = started if started is not None else ("torch" in _sys.modules)
    _os.environ["DEBUG_CLR_GRAPH_PACKET_CAPTURE"] = "0"
    return not late


# False: the HIP runtime was initialised before this package could turn the fast path off (or the user turned it on):
# pika_amd.train_graph then keeps the training step an eager launch sequence
HIP_GRAPHS_SAFE_TO_ALTERNATE = _hip_graph_workaround()


# The CTC surface (pika_amd/ctc.py), resolved on first use: importing it here would import torch before the flag above
# is placed.
_CTC_EXPORTS = ("ctc_loss", "ctc_loss_from_logits", "CTCLoss", "ctc_align", "ctc_align_from_logits",
                "ctc_greedy_decode", "ctc_greedy_decode_from_logits", "ctc_beam_search", "ctc_beam_search_from_logits",
                "CtcNgramLm", "ctc_beam_search_lm", "ctc_beam_search_lm_from_logits", "CtcBeamStream",
                "CtcHotwords", "CtcBiasedLm", "ctc_nbest_align", "ctc_nbest_align_from_logits",
                "ctc_nbest_loss", "ctc_nbest_loss_from_logits", "ctc_mwer_loss", "ctc_mwer_loss_from_logits",
                "ctc_nbest_errors", "ctc_nbest_edit_distance", "ctc_nbest_pairwise_distance", "ctc_nbest_mbr_decode",
                "ctc_long_align", "ctc_long_align_from_logits", "ctc_segment_scores",
                "ctc_long_loss", "ctc_long_loss_from_logits")


# The pruned RNN-T surface (pika_amd/rnnt.py), resolved the same way.
_RNNT_EXPORTS = ("rnnt_loss_pruned", "rnnt_loss_pruned_from_logits", "rnnt_loss_from_planes", "rnnt_prune_ranges",
                 "rnnt_simple_planes", "rnnt_prune_lm", "rnnt_pruned_joint_loss",
                 "rnnt_smoothed_planes", "rnnt_loss_smoothed", "rnnt_pruned_joint_loss_smoothed",
                 "rnnt_loss_from_planes_modified", "rnnt_prune_ranges_modified", "rnnt_loss_pruned_modified",
                 "rnnt_loss_pruned_modified_from_logits", "rnnt_loss_modified", "rnnt_loss_modified_from_logits",
                 "rnnt_pruned_joint_loss_modified",
                 "rnnt_align_pruned", "rnnt_align_pruned_from_logits", "rnnt_align_from_planes", "rnnt_align_modified",
                 "rnnt_align_modified_from_logits", "rnnt_align_pruned_modified",
                 "rnnt_align_pruned_modified_from_logits", "rnnt_align_from_planes_modified")

# The joint network on the band (pika_amd/model/ops.py).
_OPS_EXPORTS = ("joint_pruned",)

# The one-symbol-per-frame beam search (pika_amd/decoder/modified_search.py).
_MSEARCH_EXPORTS = ("ModifiedBeamState", "modified_beam_search", "ModifiedLmBeamState", "modified_beam_search_lm",
                    "ModifiedBeamStream", "ModifiedStreamDecoder", "ModifiedBeamTimes", "modified_beam_search_timed",
                    "ModifiedNnLmBeamState", "modified_beam_search_nnlm")

# The neural LM the search above fuses (pika_amd/model/lm.py).
_LM_EXPORTS = ("LstmLm",)

# The stateless prediction network and its search context (pika_amd/model/stateless.py).
_STATELESS_EXPORTS = ("StatelessPredNet", "StatelessContext")

# CTC-guided frame skipping (pika_amd/frame_skip.py).
_FSKIP_EXPORTS = ("FrameSkipPlan", "ctc_skip_plan", "frame_skip_apply", "frame_skip_times", "modified_beam_search_skip")


def __getattr__(name):
    if name in _CTC_EXPORTS:
        from . import ctc
        return getattr(ctc, name)
    if name in _RNNT_EXPORTS:
        from . import rnnt
        return getattr(rnnt, name)
    if name in _OPS_EXPORTS:
        from .model import ops
        return getattr(ops, name)
    if name in _MSEARCH_EXPORTS:
        from .decoder import modified_search
        return getattr(modified_search, name)
    if name in _LM_EXPORTS:
        from .model import lm
        return getattr(lm, name)
    if name in _STATELESS_EXPORTS:
        from .model import stateless
        return getattr(stateless, name)
    if name in _FSKIP_EXPORTS:
        from . import frame_skip
        return getattr(frame_skip, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def __dir__():
    return sorted(list(globals()) + list(_CTC_EXPORTS) + list(_RNNT_EXPORTS) + list(_OPS_EXPORTS)
                  + list(_MSEARCH_EXPORTS) + list(_LM_EXPORTS) + list(_STATELESS_EXPORTS) + list(_FSKIP_EXPORTS))
