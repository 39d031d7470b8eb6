"""Host side of the RNN-T loss: mirrors the `warp_rnnt` surface PIKA imports.

Reference call site (trainer/train_transducer_bmuf_otfaug.py:58,97-99):

    transducer_loss = RNNTLoss(blank=0, reduction='sum').apply
    loss = transducer_loss(outputs, target_batch.int(), len_batch, ali_lens)
    loss = loss.sum()

so `RNNTLoss(...)` must be constructible with keyword arguments and expose `.apply(log_probs,
labels, frames_lengths, labels_lengths)` returning per-utterance costs (B,) that the caller
sums (and in the MBR script pre-multiplies by a float, train_transducer_mbr_bmuf_otfaug.py:157).

MI355X-first split: forward runs only gather + alpha/beta (~0.1 ms) and keeps the lattice in a
34 MB workspace; the dense (B,T,U1,V) gradient is written ONCE, in backward, already scaled
by autograd's grad_output -- warp_rnnt instead materialises it in forward and multiplies it
again in backward (3 extra passes over 32 GB at the benchmark shape).  When log_probs came out of
this package's own joint network, the gradient goes back as a LazyDenseGrad: the joint's backward
reads the loss workspace and the dense tensor is written only if anything else touches it.

Two options of warp_rnnt's keyword surface (README "RNN-T loss"):
  fastemit_lambda  FastEmit (Yu et al. 2021, arXiv:2010.11148): the costs are unchanged, the gradient of every
                   label-emission entry (n, t, u, y_{u+1}), u < U_n, is multiplied by 1 + lambda.  The factor lives in
                   the row metadata of the loss workspace, so every backward route (dense, lazy, fused) carries it.
  compact=True     the packed layout: log_probs (N, V) with N = sum_n T_n (U_n + 1), rows utterance-major then t then u,
                   labels (sum_n U_n,) concatenated; gradient (N, V).  No padding is read or written.  It costs ONE
                   device-to-host copy of the two length vectors (T_max, U1_max and N size the launch), so it cannot run
                   under stream capture; the padded layout never synchronises.
"""
import math
import os
import threading

import torch

from . import _lib


# bench.py hook: when set to {"fwd": [], "bwd": []}, every C-ABI call is bracketed by HIP events
# recorded on the launch stream (torch's current stream) so kernel time is measured live.
KERNEL_EVENTS = None

# widest vocabulary the fused lattice kernels take (include/pika_rnnt.h: one wave covers a row in 64 x 4 x 32 columns; the
# benchmarked V = 5000 runs the 20-register instantiation, the recipes' 6268 the 32-register one)
MAX_FUSED_V = 8192


class _timed(object):
    def __init__(self, key):
        self.key = key

    def __enter__(self):         # (key None: a call nobody times -- alignment)
        self.on = KERNEL_EVENTS is not None and self.key is not None
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.on:
            self.e1.record()
            KERNEL_EVENTS[self.key].append((self.e0, self.e1))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_tensors(x, what, labels, frames_lengths, labels_lengths, no_cpu=""):
    # same argument checks, same exception types as the reference binding's Python wrapper
    if not x.is_cuda:
        raise RuntimeError("pika_amd RNNTLoss: %s must live on a HIP device%s" % (what, no_cpu))
    if x.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (what, x.dtype))
    for name, t in (("labels", labels), ("frames_lengths", frames_lengths), ("labels_lengths", labels_lengths)):
        if t.dtype != torch.int32:
            raise TypeError("%s must be int32, got %s" % (name, t.dtype))
        if t.device != x.device:
            raise RuntimeError("%s is on %s but %s is on %s" % (name, t.device, what, x.device))


def _check_inputs(log_probs, labels, frames_lengths, labels_lengths, blank):
    _check_tensors(log_probs, "log_probs", labels, frames_lengths, labels_lengths,
                   " (there is no CPU path; the CPU checker lives in oracle/ for tests only)")
    if log_probs.dim() != 4:
        raise ValueError("log_probs must be (B,T,U+1,V), got %s" % (tuple(log_probs.shape),))
    B, T, U1, V = log_probs.shape
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] != U1 - 1:
        raise ValueError("labels must be (B,U)=(%d,%d), got %s" % (B, U1 - 1, tuple(labels.shape)))
    if frames_lengths.shape != (B,) or labels_lengths.shape != (B,):
        raise ValueError("frames_lengths / labels_lengths must be (B,)")
    if not 0 <= blank < V:
        raise ValueError("blank=%d outside [0,%d)" % (blank, V))
    if U1 > 1024:
        raise ValueError("U+1=%d > 1024 not supported" % U1)


class CompactGrad(object):
    """What the backward leaves on the dense gradient tensor it returns (`grads._pika_compact`): the
    workspace whose row metadata hold the (at most two) non-zeros of every V-row.  A consumer that
    produced log_probs itself (pika_amd.model.hipops.JointOutFn) may use it instead of reading the
    7.8 GB dense tensor back -- only if the tensor it received IS this tensor, unmodified (`matches`)."""

    __slots__ = ("ws", "dims", "ptr", "version")

    def __init__(self, ws, dims, grads=None):
        # (grads None: the workspace alone, for a LazyDenseGrad -- there is no dense tensor to match)
        self.ws, self.dims = ws, dims
        self.ptr, self.version = (grads.data_ptr(), grads._version) if grads is not None else (0, 0)

    def matches(self, g):
        return g.data_ptr() == self.ptr and g._version == self.version and tuple(g.shape) == tuple(self.dims[:4])


def _lazy_enabled():
    import os
    return os.environ.get("PIKA_RNNT_LAZY_GRAD", "1") != "0"


class _LazyTensor(torch.Tensor):
    """A wrapper tensor whose values exist once somebody asks: every use other than the one its producer registered for
    goes through `dense()` of the subclass first."""

    def __reduce_ex__(self, proto):     # pickling / torch.save: the real values
        return self.dense().__reduce_ex__(proto)

    def __deepcopy__(self, memo):
        return self.dense().clone()

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_map
        un = lambda t: t.dense() if isinstance(t, _LazyTensor) else t   # noqa: E731
        return func(*tree_map(un, args), **tree_map(un, kwargs or {}))


class LazyDenseGrad(_LazyTensor):
    """The loss' (B,T,U1,V) gradient as a tensor that is only written when somebody looks at it.

    The backward of the loss always leaves the at most two non-zeros of every V-row in its workspace.  A
    producer that computed log_probs itself and registered for it (`log_probs._pika_lazy_grad_ok = True`, set
    by pika_amd.model.ops.joint on the output of JointOutFn) gets this object instead of 7.8 GB of mostly zeros;
    JointOutFn.backward recognises it and builds d(logits) from the workspace (`compact`).  ANY other use -- an
    aten op on it, autograd accumulating a second gradient into log_probs, a hook, `.grad` of a leaf -- goes
    through __torch_dispatch__, which first writes the dense tensor (`pika_rnnt_loss_dense_grads`, the very
    streaming pass the eager path runs) and then runs the op on it: values are identical in every case."""

    @staticmethod
    def __new__(cls, compact, labels, frames_lengths, labels_lengths, width=None):
        # width: the vocabulary the CALLER sees when the kernels run on a wider one (an output layer padded to a multiple of
        # four units inside the joint, pika_amd.model.ops.joint): the tensor this object stands for has `width` columns
        B, T, U1, V, _ = compact.dims
        r = torch.Tensor._make_wrapper_subclass(cls, (B, T, U1, V if width is None else int(width)), dtype=torch.float32,
                                                device=compact.ws.device, requires_grad=False)
        r.compact = compact
        r._keep = (labels, frames_lengths, labels_lengths)   # the metadata kernel has run; kept for symmetry of lifetimes
        r._dense = None
        r.lse = None
        return r

    def dense(self):
        if self._dense is None:
            B, T, U1, V, blank = self.compact.dims
            ws = self.compact.ws
            with torch.cuda.device(ws.device):
                g = torch.empty((B, T, U1, V), dtype=torch.float32, device=ws.device)
                with _timed("bwd"):
                    _lib.check(_lib.lib().pika_rnnt_loss_dense_grads(_ptr(ws), B, T, U1, V, blank, _ptr(g), _stream()),
                               "pika_rnnt_loss_dense_grads")
            self._dense = g if V == self.shape[-1] else g[..., :self.shape[-1]].contiguous()
        return self._dense

    def __repr__(self):
        return "LazyDenseGrad(shape=%s, written=%s)" % (tuple(self.shape), self._dense is not None)


class LogitsState(object):
    """Shared by a LazyLogProbs and the joint node that made it: does the (B,T,U1,V) buffer still hold raw logits?
    (Small on purpose: autograd nodes outlive their backward for as long as anything holds the graph, so nothing that
    hangs off them may keep the 7.8 GB buffer alive -- the buffer itself lives in autograd's saved tensors and in the
    LazyLogProbs the caller holds.)"""

    __slots__ = ("scale", "raw", "partials", "gathered", "recompute", "dense_lp")

    def __init__(self, scale):
        self.scale, self.raw = float(scale), True
        self.partials = None      # (2, rows, n_part) per-row partial (max, sum exp) pairs from the GEMM epilogue
        # 16-bit logits (pika_gemm_bf16_nt_lse_f16): the buffer is an fp16 matrix; `gathered` = (values (rows, 2) f32,
        # labels (B, U) i32, blank column) holds what the loss reads in fp32; `recompute()` runs the product again with an
        # fp32 output and returns log_softmax of it -- what ANY reader other than this package's loss gets (`dense_lp`)
        self.gathered = None
        self.recompute = None
        self.dense_lp = None

    def to_log_probs(self, buf):
        """The log-probabilities: in place in an fp32 buffer (buf <- log_softmax(scale * buf), once), or -- 16-bit logits --
        a separate fp32 tensor made by running the product again."""
        if self.recompute is not None:
            if self.dense_lp is None:
                self.dense_lp = self.recompute()
                self.raw = False
                self.partials = None
            return self.dense_lp
        if self.raw:
            B, T, U1, V = buf.shape
            with torch.cuda.device(buf.device):
                _lib.check(_lib.lib().pika_log_softmax_rows(buf.data_ptr(), B * T * U1, V, V, self.scale, _stream()),
                           "pika_log_softmax_rows")
            self.raw = False
            self.partials = None
        return buf


class LazyLogProbs(_LazyTensor):
    """log_softmax(logits) over the lattice as a tensor whose log-softmax pass only runs if somebody needs the
    values.  pika_amd.model.hipops.JointOutFn returns it; this module's loss takes the row log-sum-exp and the two
    log-probs per lattice cell it needs in ONE read of the raw logits (pika_rnnt_fused_forward), and the joint's
    backward subtracts that log-sum-exp on the fly for as long as the buffer is raw.  ANY other use -- an aten op,
    printing, `.float()`, a different loss -- goes through __torch_dispatch__, which first normalises the buffer in
    place (the same kernel the eager path runs in the forward) and then runs the op on the real log-probabilities."""

    @staticmethod
    def __new__(cls, state, buf, width=None):
        # (buf: the fp32 logits, or the fp16 matrix of a 16-bit joint; the tensor this object stands for is fp32 either way.
        #  width: the caller's vocabulary when the joint padded its output layer to a multiple of four units -- the extra
        #  columns hold logits of -6e4, probability zero: the tensor this object stands for has `width` columns)
        shape = tuple(buf.shape) if width is None else tuple(buf.shape[:-1]) + (int(width),)
        r = torch.Tensor._make_wrapper_subclass(cls, shape, dtype=torch.float32, device=buf.device, requires_grad=False)
        r.state, r.buf = state, buf
        return r

    def dense(self):
        full = self.state.to_log_probs(self.buf)
        return full if full.shape[-1] == self.shape[-1] else full[..., :self.shape[-1]]

    def __repr__(self):
        return "LazyLogProbs(shape=%s, normalised=%s)" % (tuple(self.shape), not self.state.raw)


def _check_lambda(fastemit_lambda):
    lam = float(fastemit_lambda)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("fastemit_lambda must be finite and >= 0, got %r" % (fastemit_lambda,))
    return lam


def _fused_v_ok(V):
    return V % 4 == 0 and V <= MAX_FUSED_V


def _raw_readable(lp):
    """May this LazyLogProbs be read as the raw logits of its buffer (log-sum-exp + gather in one read)?  Not once it is
    normalised, not when it is scaled, not outside the fused kernels' vocabularies; 16-bit logits only with the partial
    statistics their merge kernel starts from."""
    st = lp.state
    return bool(st.raw and st.scale == 1.0 and _fused_v_ok(lp.buf.shape[-1])
                and (st.gathered is None or st.partials is not None))


def _fill_padded(x, labels, frames_lengths, labels_lengths, blank, logits=False, lazy=True, loss=False):
    """Fill a loss workspace from a checked padded input with contiguous labels and lengths: (costs, ws, lse, V, width).

    x: log-probs (B,T,U1,V); raw logits (`logits`, the *_from_logits forms); or a LazyLogProbs of this package's joint,
    read as the raw logits of its buffer where `lazy` allows and it can be (`_raw_readable`: the plain, the partial
    statistics or the gathered call) and normalised HERE otherwise -- `.contiguous()` on the wrapper subclass
    short-circuits and would hand back the wrapper.  lse: the log-sum-exp of every row of RAW logits, None when
    log-probs were read.  V: the columns the kernels saw -- the buffer's, when a joint padded its output layer; `width`
    is then the caller's V, else None.
    loss: the caller is the loss, not a reader of the planes: it uses the partial statistics up (one use: 250 MB at the
    benchmark shape), writes into the buffers a replayed forward names (pika_amd/train_graph.py: the ones its captured
    backward reads) and its call counts as KERNEL_EVENTS["fwd"]."""
    lib = _lib.lib()
    B, T, U1, V = x.shape
    width = part = gath = bufs = None
    if not isinstance(x, LazyLogProbs):
        x = x.detach().contiguous()
    elif lazy and _raw_readable(x):
        state, logits = x.state, True
        part, gath = state.partials, state.gathered
        if loss:
            state.partials, bufs = None, getattr(x, "_pika_loss_buffers", None)
        x = x.buf
        if x.shape[-1] != V:
            width, V = V, x.shape[-1]
    else:
        x = x.dense().detach().contiguous()
    with torch.cuda.device(x.device):
        costs = torch.empty(B, dtype=torch.float32, device=x.device)
        ws, lse = bufs or (None, None)
        n_ws = lib.pika_rnnt_workspace_bytes(B, T, U1)
        if ws is None or ws.numel() != n_ws or lse.numel() != B * T * U1 or ws.device != x.device:
            ws = torch.empty(n_ws, dtype=torch.uint8, device=x.device)
            lse = torch.empty(B * T * U1, dtype=torch.float32, device=x.device) if logits else None
        head = (_ptr(labels), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1, V, blank, _ptr(costs))
        with _timed("fwd" if loss else None):
            if gath is not None:
                _lib.check(lib.pika_rnnt_fused_forward_gathered(
                    _ptr(x), x.stride(-2), _ptr(gath[0]), _ptr(gath[1]), int(gath[2]), part[0].data_ptr(),
                    part[1].data_ptr(), part.shape[2], *head, _ptr(lse), _ptr(ws), _stream()),
                    "pika_rnnt_fused_forward_gathered")
            elif part is not None:
                _lib.check(lib.pika_rnnt_fused_forward_partials(
                    _ptr(x), part[0].data_ptr(), part[1].data_ptr(), part.shape[2], *head, _ptr(lse), _ptr(ws), _stream()),
                    "pika_rnnt_fused_forward_partials")
            elif logits:
                _lib.check(lib.pika_rnnt_fused_forward(_ptr(x), *head, _ptr(lse), _ptr(ws), _stream()),
                           "pika_rnnt_fused_forward")
            else:
                _lib.check(lib.pika_rnnt_loss_forward(_ptr(x), *head, _ptr(ws), _stream()), "pika_rnnt_loss_forward")
    return costs, ws, lse, V, width


# ---------------------------------------------------------------------------------------------------------------------
# The dense gradient, written over the one returned before (DESIGN.md "RNN-T loss: the reused dense gradient").
# Every V-row of it has at most two non-zeros.  The backward keeps the STORAGE of the tensor it returned (an alias that
# shares storage and version counter, not the tensor: autograd still adopts the returned tensor as `.grad` without a
# copy) and the label column of every row.  When the next backward finds that storage owned by nobody else and unwritten
# since, the tensor is zero except where this module put something, so the kernel clears those words and stores the new
# ones (pika_rgrad_backward_fe) instead of streaming B*T*U1*V floats.  One record per device.
# ---------------------------------------------------------------------------------------------------------------------
GRAD_REUSE_STATS = {"reused": 0, "full": 0}
_retained = {}                    # device index -> _Retained
_retained_lock = threading.Lock()
_private_owners = []              # what _storage_Use_Count answers for a tensor nobody else holds: measured once


class _Retained(object):
    __slots__ = ("alias", "version", "cap_rows", "rows", "V", "blank", "cols", "stream")


def _grad_reuse_enabled():
    return os.environ.get("PIKA_RNNT_GRAD_REUSE", "1") != "0"


def _owners(t):
    return torch._C._storage_Use_Count(t.untyped_storage()._cdata)


def release_grad_buffer(device=None):
    """Free what the dense backward retains between calls (every device's, or one's): the storage of the last gradient
    it returned -- if nothing else holds it -- and the row columns beside it."""
    with _retained_lock:
        if device is None:
            _retained.clear()
        else:
            index = torch.device(device).index
            _retained.pop(torch.cuda.current_device() if index is None else index, None)


def _reusable(rec, rows, V, stream):
    if rec is None or rec.V != V or rows > rec.cap_rows or rec.stream != stream or rec.alias._version != rec.version:
        return False
    if not _private_owners:
        _private_owners.append(_owners(torch.empty(1, dtype=torch.float32, device=rec.alias.device)))
    return _owners(rec.alias) == _private_owners[0]


def _dense_backward(lib, ws, dims, labels, frames_lengths, labels_lengths, grad_costs, lam):
    """The dense (B,T,U1,V) gradient of the padded loss: into the retained storage where that is safe, else into a new
    tensor, which is retained in its place.  (Called with the workspace's device current.)  The reuse path's kernel reads a
    1-D fp32 grad_costs through its own stride -- 0 for the expanded scalar of `costs.sum().backward()` -- so only other
    dtypes and layouts, and the plain path, pay for a contiguous copy."""
    B, T, U1, V, blank = dims
    rows, stream = B * T * U1, _stream()
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing or not _grad_reuse_enabled():      # the plain path; a capture leaves the retention as it is
        if not capturing:
            release_grad_buffer(ws.device)
        GRAD_REUSE_STATS["full"] += 1
        gc = grad_costs.to(torch.float32).contiguous()
        grads = torch.empty((B, T, U1, V), dtype=torch.float32, device=ws.device)
        with _timed("bwd"):
            _lib.check(lib.pika_rnnt_loss_backward_fe(
                _ptr(labels), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1, V, blank,
                _ptr(gc), _ptr(ws), _ptr(grads), lam, stream), "pika_rnnt_loss_backward_fe")
        return grads
    if grad_costs.dtype == torch.float32 and grad_costs.dim() == 1:
        gc, gc_stride = grad_costs, grad_costs.stride(0)
    else:
        gc, gc_stride = grad_costs.to(torch.float32).contiguous(), 1
    with _retained_lock:
        rec = _retained.get(ws.device.index)
        if _reusable(rec, rows, V, stream):
            grads = rec.alias.view(-1)[:rows * V].view(B, T, U1, V)
            prev = (_ptr(rec.cols), rec.rows, rec.blank)
            GRAD_REUSE_STATS["reused"] += 1
        else:
            del rec
            _retained.pop(ws.device.index, None)      # first: two gradient-sized buffers never coexist
            grads = torch.empty((B, T, U1, V), dtype=torch.float32, device=ws.device)
            rec = _Retained()
            rec.alias, rec.cap_rows, rec.V = grads.detach(), rows, V
            rec.cols = torch.empty(rows, dtype=torch.int32, device=ws.device)
            prev = (None, 0, 0)
            GRAD_REUSE_STATS["full"] += 1
        with _timed("bwd"):
            _lib.check(lib.pika_rgrad_backward_fe_s(
                _ptr(labels), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1, V, blank,
                _ptr(gc), gc_stride, _ptr(ws), _ptr(grads), lam, prev[0], prev[1], prev[2], _ptr(rec.cols), stream),
                "pika_rgrad_backward_fe_s")
        rec.version, rec.rows, rec.blank, rec.stream = rec.alias._version, rows, blank, stream
        _retained[ws.device.index] = rec
    return grads


class _RNNTLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, labels, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0):
        wide = getattr(log_probs, "_pika_labels", None)
        if wide is not None and labels.dim() == 2 and log_probs.dim() == 4 and labels.shape[1] < log_probs.shape[2] - 1 \
                and wide.shape == (labels.shape[0], log_probs.shape[2] - 1):
            # a replayed forward (pika_amd/train_graph.py) padded the label axis to its bucket: its own copy of the labels
            # over that axis (same values in the caller's columns; nothing beyond labels_lengths is ever read)
            labels = wide
        _check_inputs(log_probs, labels, frames_lengths, labels_lengths, blank)
        ctx.lazy = bool(getattr(log_probs, "_pika_lazy_grad_ok", False)) and _lazy_enabled()
        labels, frames_lengths, labels_lengths = (t.contiguous() for t in (labels, frames_lengths, labels_lengths))
        B, T, U1, _ = log_probs.shape
        # raw logits of this package's joint, when the joint takes the lazy gradient: log-sum-exp + gather in one read, no
        # log-prob tensor.  lse only means something to the joint's backward while its buffer is still raw, which that
        # backward checks itself
        costs, ws, lse, V, ctx.width = _fill_padded(log_probs, labels, frames_lengths, labels_lengths, blank,
                                                    lazy=ctx.lazy, loss=True)
        ctx.save_for_backward(labels, frames_lengths, labels_lengths, ws, lse)
        ctx.dims = (B, T, U1, V, blank)
        ctx.fastemit_lambda = fastemit_lambda
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        labels, frames_lengths, labels_lengths, ws, lse = ctx.saved_tensors
        B, T, U1, V, blank = ctx.dims
        lam = ctx.fastemit_lambda
        lib = _lib.lib()
        if ctx.lazy:
            gc = grad_costs.to(torch.float32).contiguous()
            with torch.cuda.device(ws.device):
                _lib.check(lib.pika_rnnt_loss_backward_fe(
                    _ptr(labels), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1, V, blank,
                    _ptr(gc), _ptr(ws), None, lam, _stream()), "pika_rnnt_loss_backward_fe")
            lazy = LazyDenseGrad(CompactGrad(ws, (B, T, U1, V, blank)), labels, frames_lengths, labels_lengths, width=ctx.width)
            lazy.lse = lse
            return lazy, None, None, None, None, None
        with torch.cuda.device(ws.device):
            grads = _dense_backward(lib, ws, ctx.dims, labels, frames_lengths, labels_lengths, grad_costs, lam)
        grads._pika_compact = CompactGrad(ws, (B, T, U1, V, blank), grads)
        return grads, None, None, None, None, None


class _FusedLogitsLossFn(torch.autograd.Function):
    """RNN-T costs straight from the joint's RAW logits (SURVEY 8d M1', include/pika_rnnt.h): the log-softmax
    is folded into the two passes the loss makes anyway (log-sum-exp + gather; gradient), so the (B,T,U1,V)
    log-prob tensor and its dense gradient never exist: 3 tensor passes instead of 6."""

    @staticmethod
    def forward(ctx, logits, labels, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0):
        _check_inputs(logits, labels, frames_lengths, labels_lengths, blank)
        x = logits.contiguous()
        labels, frames_lengths, labels_lengths = (t.contiguous() for t in (labels, frames_lengths, labels_lengths))
        B, T, U1, V = x.shape
        costs, ws, lse, _, _ = _fill_padded(x, labels, frames_lengths, labels_lengths, blank, logits=True, loss=True)
        ctx.save_for_backward(x, labels, frames_lengths, labels_lengths, ws, lse)
        ctx.dims = (B, T, U1, V, blank)
        ctx.fastemit_lambda = fastemit_lambda
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        x, labels, frames_lengths, labels_lengths, ws, lse = ctx.saved_tensors
        B, T, U1, V, blank = ctx.dims
        gc = grad_costs.to(torch.float32).contiguous()
        with torch.cuda.device(x.device):
            grads = torch.empty_like(x)
            with _timed("bwd"):
                _lib.check(_lib.lib().pika_rnnt_fused_backward_fe(
                    _ptr(x), _ptr(lse), _ptr(labels), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1, V,
                    blank, _ptr(gc), _ptr(ws), _ptr(grads), 0, V, ctx.fastemit_lambda, _stream()),
                    "pika_rnnt_fused_backward_fe")
        return grads, None, None, None, None, None


class _Packed(object):
    """Host description of a packed batch: B, T_max, U1_max, N and the device row / label offsets."""

    __slots__ = ("B", "T", "U1", "N", "roff", "loff")


def _check_packed(x, labels, frames_lengths, labels_lengths, blank, what):
    """Validate a packed call before any launch; ONE device-to-host copy of the two length vectors."""
    _check_tensors(x, what, labels, frames_lengths, labels_lengths)
    if x.dim() != 2:
        raise ValueError("compact=True: %s must be (N, V), got %s" % (what, tuple(x.shape)))
    if labels.dim() != 1:
        raise ValueError("compact=True: labels must be (sum U_n,), got %s" % (tuple(labels.shape),))
    if frames_lengths.dim() != 1 or labels_lengths.shape != frames_lengths.shape or frames_lengths.numel() == 0:
        raise ValueError("compact=True: frames_lengths / labels_lengths must be (B,) with B >= 1")
    N, V = x.shape
    if not 0 <= blank < V:
        raise ValueError("blank=%d outside [0,%d)" % (blank, V))
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("rnnt_loss(compact=True) reads the length vectors on the host (T_max, U1_max, N) and cannot "
                           "run under stream capture; capture the padded layout instead")
    lens = torch.stack([frames_lengths, labels_lengths]).to("cpu", torch.int64)   # the packed call's one host sync
    tl, ul = lens[0], lens[1]
    if bool((tl < 1).any()):
        raise ValueError("compact=True: every frames_lengths entry must be >= 1, got %s" % (tl.tolist(),))
    if bool((ul < 0).any()):
        raise ValueError("compact=True: every labels_lengths entry must be >= 0, got %s" % (ul.tolist(),))
    if int(ul.max()) + 1 > 1024:
        raise ValueError("compact=True: U_n + 1 = %d > 1024 not supported" % (int(ul.max()) + 1))
    rows = tl * (ul + 1)
    if int(rows.sum()) != N:
        raise ValueError("compact=True: %s has %d rows, sum_n T_n (U_n + 1) = %d" % (what, N, int(rows.sum())))
    if int(ul.sum()) != labels.numel():
        raise ValueError("compact=True: labels has %d entries, sum_n U_n = %d" % (labels.numel(), int(ul.sum())))
    if N > 0x7fffffff:
        raise ValueError("compact=True: N = %d rows > 2^31 - 1" % N)
    p = _Packed()
    p.B, p.T, p.U1, p.N = int(tl.numel()), int(tl.max()), int(ul.max()) + 1, int(N)
    # offsets on the device, from the device copies of the lengths (exclusive prefix sums)
    r = frames_lengths.to(torch.int64) * (labels_lengths.to(torch.int64) + 1)
    u = labels_lengths.to(torch.int64)
    p.roff = (torch.cumsum(r, 0) - r).to(torch.int32)
    p.loff = (torch.cumsum(u, 0) - u).to(torch.int32)
    return p


def _fill_packed(x, labels, frames_lengths, labels_lengths, blank, caller=None, loss=False):
    """`_fill_padded` for the packed layout: checks the call and fills a workspace from log-probs (N, V) or -- `caller`,
    the name of a *_from_logits form -- raw logits.  Returns (p, (x, labels, frames_lengths, labels_lengths), costs, ws,
    lse): the batch's description and the contiguous tensors the kernels read.  loss: the call counts as
    KERNEL_EVENTS["fwd"]."""
    p = _check_packed(x, labels, frames_lengths, labels_lengths, blank, "logits" if caller else "log_probs")
    lib = _lib.lib()
    x = x.detach().contiguous()
    labels, frames_lengths, labels_lengths = (t.contiguous() for t in (labels, frames_lengths, labels_lengths))
    V = x.shape[1]
    if caller and not _fused_v_ok(V):
        raise ValueError("%s: V = %d must be a multiple of 4 and <= %d" % (caller, V, MAX_FUSED_V))
    with torch.cuda.device(x.device):
        costs = torch.empty(p.B, dtype=torch.float32, device=x.device)
        lse = torch.empty(p.N, dtype=torch.float32, device=x.device) if caller else None
        ws = torch.empty(lib.pika_rnnt_workspace_bytes(p.B, p.T, p.U1), dtype=torch.uint8, device=x.device)
        head = (_ptr(x), _ptr(labels), _ptr(frames_lengths), _ptr(labels_lengths), _ptr(p.roff), _ptr(p.loff),
                p.B, p.T, p.U1, p.N, V, blank, _ptr(costs))
        with _timed("fwd" if loss else None):
            if caller:
                _lib.check(lib.pika_rnnt_packed_fused_forward(*head, _ptr(lse), _ptr(ws), _stream()),
                           "pika_rnnt_packed_fused_forward")
            else:
                _lib.check(lib.pika_rnnt_packed_forward(*head, _ptr(ws), _stream()), "pika_rnnt_packed_forward")
    return p, (x, labels, frames_lengths, labels_lengths), costs, ws, lse


class _PackedLossFn(torch.autograd.Function):
    """RNN-T costs of a packed batch (N, V) of log-probs or -- `caller`, the *_from_logits form's name -- of raw logits
    (_FusedLogitsLossFn on the packed layout); gradient (N, V)."""

    @staticmethod
    def forward(ctx, x, labels, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0, caller=None):
        p, (x, labels, frames_lengths, labels_lengths), costs, ws, lse = _fill_packed(
            x, labels, frames_lengths, labels_lengths, blank, caller=caller, loss=True)
        # (log-probs are not kept: their gradient comes from the workspace alone; lse is None for them)
        ctx.save_for_backward(labels, frames_lengths, labels_lengths, ws, p.roff, p.loff, x if caller else None, lse)
        ctx.dims = (p.B, p.T, p.U1, p.N, x.shape[1], blank)
        ctx.fastemit_lambda = fastemit_lambda
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        labels, frames_lengths, labels_lengths, ws, roff, loff, x, lse = ctx.saved_tensors
        B, T, U1, N, V, blank = ctx.dims
        gc = grad_costs.to(torch.float32).contiguous()
        head = (_ptr(labels), _ptr(frames_lengths), _ptr(labels_lengths), _ptr(roff), _ptr(loff), B, T, U1, N, V, blank,
                _ptr(gc), _ptr(ws))
        with torch.cuda.device(ws.device):
            grads = torch.empty((N, V), dtype=torch.float32, device=ws.device)
            with _timed("bwd"):
                if x is None:
                    _lib.check(_lib.lib().pika_rnnt_packed_backward(*head, _ptr(grads), ctx.fastemit_lambda, _stream()),
                               "pika_rnnt_packed_backward")
                else:
                    _lib.check(_lib.lib().pika_rnnt_packed_fused_backward(
                        _ptr(x), _ptr(lse), *head, _ptr(grads), 0, V, ctx.fastemit_lambda, _stream()),
                        "pika_rnnt_packed_fused_backward")
        return grads, None, None, None, None, None, None


def rnnt_loss_from_logits(logits, labels, frames_lengths, labels_lengths, blank=0, fastemit_lambda=0.0,
                          compact=False):
    """Per-utterance costs of log_softmax(logits) under the RNN-T loss, differentiable w.r.t. the logits,
    without materialising the log-probabilities (V % 4 == 0, V <= 8192).

    fastemit_lambda: FastEmit (module docstring); d(logits) = g~ - softmax * sum(g~) with the scaled gradient g~.
    compact=True: packed raw logits (N, V) and labels (sum U_n,) as in `rnnt_loss`, one host sync."""
    lam = _check_lambda(fastemit_lambda)
    if compact:
        return _PackedLossFn.apply(logits, labels, frames_lengths, labels_lengths, blank, lam, "rnnt_loss_from_logits")
    return _FusedLogitsLossFn.apply(logits, labels, frames_lengths, labels_lengths, blank, lam)


def rnnt_loss(log_probs, labels, frames_lengths, labels_lengths, average_frames=False,
              reduction=None, blank=0, gather=False, fastemit_lambda=0.0, compact=False):
    """Functional form, with warp_rnnt.rnnt_loss's keywords.

    gather: accepted for compatibility; it changes no value -- the kernels only ever read the blank and label
      columns of a cell (warp_rnnt's `gather=True` saving is what they always do).
    fastemit_lambda: FastEmit regularisation, finite and >= 0 (Yu et al. 2021).  Costs unchanged; in the gradient every
      label-emission entry (n, t, u, y_{u+1}), u < U_n, is multiplied by 1 + fastemit_lambda.  0 is exactly the plain loss.
    compact: the packed layout.  log_probs (N, V) with N = sum_n T_n (U_n + 1), row off_n + t (U_n + 1) + u holding cell
      (n, t, u) (off_n the exclusive prefix sum of T_n (U_n + 1)); labels (sum_n U_n,) int32 concatenated; lengths (B,)
      int32 with T_n >= 1, U_n >= 0, U_n + 1 <= 1024, and the two sums equal to N and labels.numel() (ValueError before
      any launch otherwise: nothing is clamped).  Costs (B,), gradient (N, V).  Costs ONE device-to-host copy of the
      lengths, so it raises under stream capture; the padded layout keeps its no-sync behaviour."""
    lam = _check_lambda(fastemit_lambda)
    fn = _PackedLossFn if compact else _RNNTLossFn
    costs = fn.apply(log_probs, labels, frames_lengths, labels_lengths, blank, lam)
    return _reduce(costs, frames_lengths, average_frames, reduction)


def _reduce(costs, frames_lengths, average_frames, reduction):
    if average_frames:
        costs = costs / frames_lengths.to(costs)
    if reduction == "sum":
        return costs.sum()
    if reduction == "mean":
        return costs.mean()
    if reduction in (None, "none"):
        return costs
    raise ValueError("Unknown reduction: %r" % (reduction,))


def _align_call(lib, ws, frames_lengths, labels_lengths, loff, B, T, U1, n_frames, device, modified=False):
    """pika_rnnt_align (modified: pika_mrnnt_align, which has no packed form) on a workspace a forward call of that
    topology has just filled: (scores (B,), emit_frames)."""
    entry = "pika_mrnnt_align" if modified else "pika_rnnt_align"
    scores = torch.empty(B, dtype=torch.float32, device=device)
    frames = torch.empty(n_frames, dtype=torch.int32, device=device)
    scratch = torch.empty(getattr(lib, entry + "_scratch_bytes")(B, T, U1), dtype=torch.uint8, device=device)
    _lib.check(getattr(lib, entry)(_ptr(ws), _ptr(frames_lengths), _ptr(labels_lengths), *(() if modified else (_ptr(loff),)),
                                   B, T, U1, _ptr(scores), _ptr(frames) if n_frames else None, _ptr(scratch), _stream()),
               entry)
    return scores, frames


def _align(x, labels, frames_lengths, labels_lengths, blank, compact, caller=None):
    """Both alignment forms: fill a workspace the way the loss does (caller: the *_from_logits form's name), walk it."""
    lib = _lib.lib()
    if compact:
        p, (x, labels, frames_lengths, labels_lengths), _, ws, _ = _fill_packed(x, labels, frames_lengths, labels_lengths,
                                                                               blank, caller)
        with torch.cuda.device(x.device):
            return _align_call(lib, ws, frames_lengths, labels_lengths, p.loff, p.B, p.T, p.U1, labels.numel(), x.device)
    _check_inputs(x, labels, frames_lengths, labels_lengths, blank)
    labels, frames_lengths, labels_lengths = (t.contiguous() for t in (labels, frames_lengths, labels_lengths))
    B, T, U1, V = x.shape
    if caller and not _fused_v_ok(V):
        raise ValueError("%s: V = %d must be a multiple of 4 and <= %d" % (caller, V, MAX_FUSED_V))
    # (a LazyLogProbs: the planes come from the raw buffer as it is; the partial statistics, which the loss uses once,
    # stay for it)
    _, ws, _, _, _ = _fill_padded(x, labels, frames_lengths, labels_lengths, blank, logits=caller is not None)
    with torch.cuda.device(ws.device):
        scores, frames = _align_call(lib, ws, frames_lengths, labels_lengths, None, B, T, U1, B * (U1 - 1), ws.device)
    return scores, frames.view(B, U1 - 1)


def rnnt_align(log_probs, labels, frames_lengths, labels_lengths, blank=0, compact=False):
    """Forced alignment of every transcript against its lattice: the single best (Viterbi) path.

    Returns (scores, emit_frames), both detached: scores (B,) f32, the log-probability of the best alignment
    (scores[n] <= -cost_n); emit_frames i32 (B, U) -- entry [n][u], u < U_n, is the encoder frame at which that path
    emits label u (non-decreasing in u, in [0, T_n - 1]), entries u >= U_n are -1 -- or, compact=True, (sum U_n,) in
    the order of the packed labels.  Ties go to the earliest emission.  Inputs, checks and length clamping are those
    of `rnnt_loss` (a LazyLogProbs of this package's joint is read the way the loss reads it); no autograd.  The
    padded form never synchronises the host and can be captured in a graph; compact=True pays the packed layout's
    one length copy and raises under stream capture."""
    return _align(log_probs, labels, frames_lengths, labels_lengths, blank, compact)


def rnnt_align_from_logits(logits, labels, frames_lengths, labels_lengths, blank=0, compact=False):
    """`rnnt_align` of log_softmax(logits) without materialising the log-probabilities (V % 4 == 0, V <= 8192):
    the planes come from the one read of the raw logits `rnnt_loss_from_logits` makes."""
    return _align(logits, labels, frames_lengths, labels_lengths, blank, compact, "rnnt_align_from_logits")


# ---------------------------------------------------------------------------------------------------------------------
# Pruned RNN-T (k2 / icefall rnnt_loss_pruned; Kuang et al. 2022, arXiv:2206.13236): the loss on a banded lattice.
#   planes  = rnnt_simple_planes(am, lm, labels)                      the am + lm joiner's two planes (torch)
#   simple, bo, lo = rnnt_loss_from_planes(*planes, T_n, U_n, return_occupancy=True)
#   ranges  = rnnt_prune_ranges(bo, lo, T_n, U_n, S)                  (B, T) int32
#   logits  = joiner(am[:, :, None], rnnt_prune_lm(lm, ranges, S))    (B, T, S, V)
#   pruned  = rnnt_loss_pruned_from_logits(logits, labels, ranges, T_n, U_n)
# Nothing here reads a length on the host: every call can be captured in a torch.cuda.graph.
# ---------------------------------------------------------------------------------------------------------------------
def _check_pruned(x, what, labels, ranges, frames_lengths, labels_lengths, blank):
    _check_tensors(x, what, labels, frames_lengths, labels_lengths, " (there is no CPU path)")
    if ranges.dtype != torch.int32:
        raise TypeError("ranges must be int32, got %s" % (ranges.dtype,))
    if ranges.device != x.device:
        raise RuntimeError("ranges is on %s but %s is on %s" % (ranges.device, what, x.device))
    if x.dim() != 4:
        raise ValueError("%s must be (B,T,S,V), got %s" % (what, tuple(x.shape)))
    B, T, S, V = x.shape
    if labels.dim() != 2 or labels.shape[0] != B:
        raise ValueError("labels must be (B,U) with B=%d, got %s" % (B, tuple(labels.shape)))
    U1 = labels.shape[1] + 1
    if tuple(ranges.shape) != (B, T):
        raise ValueError("ranges must be (B,T)=(%d,%d), got %s" % (B, T, tuple(ranges.shape)))
    if frames_lengths.shape != (B,) or labels_lengths.shape != (B,):
        raise ValueError("frames_lengths / labels_lengths must be (B,)")
    if not 0 <= blank < V:
        raise ValueError("blank=%d outside [0,%d)" % (blank, V))
    if U1 > 1024:
        raise ValueError("U+1=%d > 1024 not supported" % U1)
    if not 1 <= S <= U1:
        raise ValueError("the band width S=%d must be in [1, U+1=%d]" % (S, U1))
    if B * T * S > 0x7fffffff:
        raise ValueError("B*T*S = %d rows > 2^31 - 1" % (B * T * S))
    return B, T, U1, S, V


def _check_full(x, what, labels, frames_lengths, labels_lengths, blank):
    """`_check_pruned` for a call without ranges, on the full lattice (B,T,U+1,V): the band is every column, S = U + 1."""
    _check_tensors(x, what, labels, frames_lengths, labels_lengths, " (there is no CPU path)")
    if x.dim() != 4:
        raise ValueError("%s must be (B,T,U+1,V), got %s" % (what, tuple(x.shape)))
    B, T, U1, V = x.shape
    if labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] != U1 - 1:
        raise ValueError("labels must be (B,U)=(%d,%d), got %s" % (B, U1 - 1, tuple(labels.shape)))
    if frames_lengths.shape != (B,) or labels_lengths.shape != (B,):
        raise ValueError("frames_lengths / labels_lengths must be (B,)")
    if not 0 <= blank < V:
        raise ValueError("blank=%d outside [0,%d)" % (blank, V))
    if U1 > 1024:
        raise ValueError("U+1=%d > 1024 not supported" % U1)
    if B * T * U1 > 0x7fffffff:
        raise ValueError("B*T*(U+1) = %d rows > 2^31 - 1" % (B * T * U1))
    return B, T, U1, U1, V


# (modified, logits) -> the forward and the backward entry of the (B,T,S,V) / (B,T,U1,V) calls and their workspace size
_BANDED_ENTRIES = {
    (False, False): ("pika_prnnt_forward", "pika_prnnt_backward", "pika_rnnt_workspace_bytes"),
    (False, True): ("pika_prnnt_fused_forward", "pika_prnnt_fused_backward", "pika_rnnt_workspace_bytes"),
    (True, False): ("pika_prnnt_mod_forward", "pika_prnnt_mod_backward", "pika_prnnt_mod_workspace_bytes"),
    (True, True): ("pika_prnnt_mod_fused_forward", "pika_prnnt_mod_fused_backward", "pika_prnnt_mod_workspace_bytes"),
}


class _BandedLossFn(torch.autograd.Function):
    """RNN-T costs from log-probs or raw logits (`logits`: no log-prob tensor, d(logits) out), in the regular or the
    `modified` topology, on the band (B,T,S,V) of `ranges` or -- ranges None, the modified topology only -- on the full
    lattice (B,T,U1,V); the gradient is dense and has the input's shape."""

    @staticmethod
    def forward(ctx, x, labels, ranges, frames_lengths, labels_lengths, blank, fastemit_lambda, logits, caller, modified):
        what = "logits" if logits else "log_probs"
        if ranges is None:
            B, T, U1, S, V = _check_full(x, what, labels, frames_lengths, labels_lengths, blank)
        else:
            B, T, U1, S, V = _check_pruned(x, what, labels, ranges, frames_lengths, labels_lengths, blank)
            ranges = ranges.contiguous()
        if logits and not _fused_v_ok(V):
            raise ValueError("%s: V = %d must be a multiple of 4 and <= %d" % (caller, V, MAX_FUSED_V))
        lib = _lib.lib()
        fwd, ctx.bwd, ws_bytes = _BANDED_ENTRIES[modified, logits]
        x = x.detach().contiguous()
        labels, frames_lengths, labels_lengths = (t.contiguous() for t in (labels, frames_lengths, labels_lengths))
        with torch.cuda.device(x.device):
            costs = torch.empty(B, dtype=torch.float32, device=x.device)
            lse = torch.empty(B * T * S, dtype=torch.float32, device=x.device) if logits else None
            ws = torch.empty(getattr(lib, ws_bytes)(B, T, U1), dtype=torch.uint8, device=x.device)
            with _timed("fwd"):
                _lib.check(getattr(lib, fwd)(_ptr(x), _ptr(frames_lengths), _ptr(labels_lengths), _ptr(labels), _ptr(ranges),
                                             B, T, U1, S, V, blank, _ptr(costs), *((_ptr(lse),) if logits else ()), _ptr(ws),
                                             _stream()), fwd)
        # (ranges None on the full lattice; log-probs are not kept: their gradient comes from the workspace alone)
        ctx.save_for_backward(labels, ranges, frames_lengths, labels_lengths, ws, x if logits else None, lse)
        ctx.dims = (B, T, U1, S, V, blank)
        ctx.fastemit_lambda = fastemit_lambda
        ctx.shape = tuple(x.shape)
        return costs

    @staticmethod
    def backward(ctx, grad_costs):
        labels, ranges, frames_lengths, labels_lengths, ws, x, lse = ctx.saved_tensors
        B, T, U1, S, V, blank = ctx.dims
        gc = grad_costs.to(torch.float32).contiguous()
        with torch.cuda.device(ws.device):
            grads = torch.empty(ctx.shape, dtype=torch.float32, device=ws.device)
            with _timed("bwd"):
                _lib.check(getattr(_lib.lib(), ctx.bwd)(
                    *((_ptr(x), _ptr(lse)) if x is not None else ()), _ptr(frames_lengths), _ptr(labels_lengths),
                    _ptr(labels), _ptr(ranges), B, T, U1, S, V, blank, _ptr(gc), _ptr(ws), _ptr(grads),
                    *((0, V) if x is not None else ()), ctx.fastemit_lambda, _stream()), ctx.bwd)
        return (grads,) + (None,) * 9


def _banded_loss(x, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank, fastemit_lambda,
                 logits, caller, modified):
    lam = _check_lambda(fastemit_lambda)
    if modified:
        blank = int(blank)
    costs = _BandedLossFn.apply(x, labels, ranges, frames_lengths, labels_lengths, blank, lam, logits, caller, modified)
    return _reduce(costs, frames_lengths, average_frames, reduction)


def rnnt_loss_pruned(log_probs, labels, ranges, frames_lengths, labels_lengths, average_frames=False, reduction=None,
                     blank=0, fastemit_lambda=0.0):
    """RNN-T costs on a pruned (banded) lattice, differentiable w.r.t. log_probs.

    log_probs (B, T, S, V) f32: row j of frame t is the distribution of lattice cell (t, ranges[b, t] + j); labels
    (B, U) int32; ranges (B, T) int32, every entry clamped on the device to [0, max(0, U_n + 1 - S)].  Only cells inside
    the band carry probability: the cost is that of `rnnt_loss` on a (B, T, U+1, V) tensor holding the band's rows at
    their cells and -1e30 elsewhere.  The gradient is dense (B, T, S, V); rows past T_n or U_n are zero.  With S = U + 1
    and all-zero ranges this is `rnnt_loss`, bit for bit.  Keywords as in `rnnt_loss`; no host synchronisation."""
    return _banded_loss(log_probs, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank,
                        fastemit_lambda, False, "rnnt_loss_pruned", False)


def rnnt_loss_pruned_from_logits(logits, labels, ranges, frames_lengths, labels_lengths, average_frames=False,
                                 reduction=None, blank=0, fastemit_lambda=0.0):
    """`rnnt_loss_pruned` of log_softmax(logits) for raw logits (B, T, S, V), V % 4 == 0 and V <= 8192, differentiable
    w.r.t. the logits: the log-probabilities and their dense gradient never exist."""
    return _banded_loss(logits, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank,
                        fastemit_lambda, True, "rnnt_loss_pruned_from_logits", False)


def _check_planes(a, b, frames_lengths, labels_lengths, names):
    for name, t in zip(names, (a, b)):
        if not t.is_cuda:
            raise RuntimeError("pika_amd RNNTLoss: %s must live on a HIP device (there is no CPU path)" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("%s and %s must both be (B,T,U+1), got %s and %s" % (names + (tuple(a.shape), tuple(b.shape))))
    B, T, U1 = a.shape
    for name, t in (("frames_lengths", frames_lengths), ("labels_lengths", labels_lengths)):
        if t.dtype != torch.int32:
            raise TypeError("%s must be int32, got %s" % (name, t.dtype))
        if t.device != a.device or b.device != a.device:
            raise RuntimeError("%s is on %s but %s is on %s" % (name, t.device, names[0], a.device))
        if t.shape != (B,):
            raise ValueError("frames_lengths / labels_lengths must be (B,)")
    if U1 > 1024:
        raise ValueError("U+1=%d > 1024 not supported" % U1)
    return B, T, U1


class _PlanesLossFn(torch.autograd.Function):
    """RNN-T costs of a lattice given by its blank and label planes, in the regular or the `modified` topology; also
    returns the two occupancy planes (detached)."""

    @staticmethod
    def forward(ctx, blank_lp, label_lp, frames_lengths, labels_lengths, modified=False):
        B, T, U1 = _check_planes(blank_lp, label_lp, frames_lengths, labels_lengths, ("blank_lp", "label_lp"))
        lib = _lib.lib()
        fn, ws_bytes = (("pika_prnnt_mod_planes_forward", "pika_prnnt_mod_workspace_bytes") if modified else
                        ("pika_prnnt_planes_forward", "pika_rnnt_workspace_bytes"))
        pb, pl = blank_lp.detach().contiguous(), label_lp.detach().contiguous()
        frames_lengths, labels_lengths = frames_lengths.contiguous(), labels_lengths.contiguous()
        with torch.cuda.device(pb.device):
            costs = torch.empty(B, dtype=torch.float32, device=pb.device)
            occ_b, occ_l = torch.empty_like(pb), torch.empty_like(pb)
            ws = torch.empty(getattr(lib, ws_bytes)(B, T, U1), dtype=torch.uint8, device=pb.device)
            with _timed(None):
                _lib.check(getattr(lib, fn)(_ptr(pb), _ptr(pl), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1,
                                            _ptr(costs), _ptr(occ_b), _ptr(occ_l), _ptr(ws), _stream()), fn)
        ctx.save_for_backward(occ_b, occ_l)
        ctx.mark_non_differentiable(occ_b, occ_l)
        return costs, occ_b, occ_l

    @staticmethod
    def backward(ctx, grad_costs, _gb, _gl):
        occ_b, occ_l = ctx.saved_tensors
        g = -grad_costs.to(torch.float32).view(-1, 1, 1)
        return occ_b * g, occ_l * g, None, None, None


def rnnt_loss_from_planes(blank_lp, label_lp, frames_lengths, labels_lengths, reduction=None, return_occupancy=False):
    """RNN-T costs of a lattice given directly by its two planes, differentiable w.r.t. both.

    blank_lp, label_lp (B, T, U+1) f32: the log-probability of the blank edge and of the label edge out of every cell
    (label_lp[.., u] is not read for u >= U_n); they need not be normalised.  This is the "simple" loss of pruned RNN-T
    on the planes of `rnnt_simple_planes`.  return_occupancy=True: (costs, blank_occ, label_occ), the two detached
    (B, T, U+1) planes of per-edge occupation probabilities -d cost / d lp, what `rnnt_prune_ranges` takes."""
    costs, occ_b, occ_l = _PlanesLossFn.apply(blank_lp, label_lp, frames_lengths, labels_lengths)
    costs = _reduce(costs, frames_lengths, False, reduction)
    return (costs, occ_b, occ_l) if return_occupancy else costs


def rnnt_prune_ranges(blank_occ, label_occ, frames_lengths, labels_lengths, s_range):
    """The band of `s_range` label positions every frame keeps: (B, T) int32 band starts.

    With occ = blank_occ + label_occ (B, T, U+1), S = s_range and s_max = max(0, U_n + 1 - S): raw(t) is the start of the
    window of S columns with the largest occupancy sum (ties to the smallest start; raw(T_n - 1) = s_max), m its suffix
    minimum, f(0) = 0, f(t) = min(m(t), f(t-1) + S - 1), and s_t = max(f(t), s_max - (T_n - 1 - t)(S - 1)); s_max for
    t >= T_n.  The band connects (0, 0) with (T_n - 1, U_n) -- s_0 = 0, s_{T_n-1} = s_max, steps in [0, S-1] -- whenever
    (T_n - 1)(S - 1) >= s_max; otherwise none of that width does and s_0 > 0."""
    return _prune_ranges("pika_prnnt_prune_ranges", blank_occ, label_occ, frames_lengths, labels_lengths, s_range)


def _prune_ranges(entry, blank_occ, label_occ, frames_lengths, labels_lengths, s_range):
    # the band search of either topology: `entry` is pika_prnnt_prune_ranges or pika_prnnt_mod_prune_ranges
    S = int(s_range)
    B, T, U1 = _check_planes(blank_occ, label_occ, frames_lengths, labels_lengths, ("blank_occ", "label_occ"))
    if not 1 <= S <= U1:
        raise ValueError("s_range=%d must be in [1, U+1=%d]" % (S, U1))
    ob, ol = blank_occ.detach().contiguous(), label_occ.detach().contiguous()
    frames_lengths, labels_lengths = frames_lengths.contiguous(), labels_lengths.contiguous()
    with torch.cuda.device(ob.device):
        ranges = torch.empty((B, T), dtype=torch.int32, device=ob.device)
        _lib.check(getattr(_lib.lib(), entry)(_ptr(ob), _ptr(ol), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1, S,
                                              _ptr(ranges), _stream()), entry)
    return ranges


def rnnt_simple_planes(am, lm, labels, blank=0):
    """The two planes of the joiner that is am + lm (plain torch, differentiable): (blank_lp, label_lp), (B, T, U+1).

    am (B, T, V) encoder logits, lm (B, U+1, V) prediction logits, labels (B, U).  Cell (t, u) has the distribution
    log_softmax(am[b, t] + lm[b, u]); its normaliser over V is a max-shifted exp-matmul, so no (B, T, U+1, V) tensor
    exists.  label_lp[.., u] = that distribution at labels[b, u] (padding labels are clamped into [0, V): the loss never
    reads u >= U_n); its last column u = U is -1e30."""
    if am.dim() != 3 or lm.dim() != 3 or am.shape[0] != lm.shape[0] or am.shape[2] != lm.shape[2]:
        raise ValueError("am must be (B,T,V) and lm (B,U+1,V), got %s and %s" % (tuple(am.shape), tuple(lm.shape)))
    B, U1, V = lm.shape
    if labels.dim() != 2 or labels.shape != (B, U1 - 1):
        raise ValueError("labels must be (B,U)=(%d,%d), got %s" % (B, U1 - 1, tuple(labels.shape)))
    if not 0 <= blank < V:
        raise ValueError("blank=%d outside [0,%d)" % (blank, V))
    am, lm = am.float(), lm.float()
    am_max, lm_max = am.amax(2, keepdim=True), lm.amax(2, keepdim=True)                    # (B,T,1), (B,U1,1)
    prod = torch.matmul((am - am_max).exp(), (lm - lm_max).exp().transpose(1, 2))          # (B,T,U1)
    norm = prod.clamp_min(torch.finfo(torch.float32).tiny).log() + am_max + lm_max.transpose(1, 2)
    blank_lp = am[:, :, blank].unsqueeze(2) + lm[:, :, blank].unsqueeze(1) - norm
    y = labels.long().clamp(0, V - 1)                                                      # (B,U)
    am_y = torch.gather(am, 2, y.unsqueeze(1).expand(B, am.shape[1], U1 - 1))              # (B,T,U)
    lm_y = torch.gather(lm[:, :U1 - 1], 2, y.unsqueeze(2)).squeeze(2)                      # (B,U)
    label_lp = am_y + lm_y.unsqueeze(1) - norm[:, :, :U1 - 1]
    label_lp = torch.cat([label_lp, label_lp.new_full((B, am.shape[1], 1), -1.0e30)], 2)
    return blank_lp, label_lp


def rnnt_prune_lm(lm, ranges, s_range):
    """The prediction-network rows of every frame's band: lm (B, U+1, D), ranges (B, T) -> (B, T, S, D), entry
    [b, t, j] = lm[b, s_t + j] with s_t clamped to [0, max(0, U + 1 - S)] and the row index to U (plain torch)."""
    S = int(s_range)
    B, U1, D = lm.shape
    if tuple(ranges.shape[:1]) != (B,) or ranges.dim() != 2:
        raise ValueError("ranges must be (B,T) with B=%d, got %s" % (B, tuple(ranges.shape)))
    if not 1 <= S <= U1:
        raise ValueError("s_range=%d must be in [1, U+1=%d]" % (S, U1))
    T = ranges.shape[1]
    idx = ranges.long().clamp(0, max(0, U1 - S)).unsqueeze(2) + torch.arange(S, device=ranges.device)   # (B,T,S)
    idx = idx.clamp_max(U1 - 1)
    return torch.gather(lm.unsqueeze(1).expand(B, T, U1, D), 2, idx.unsqueeze(3).expand(B, T, S, D))


def rnnt_pruned_joint_loss(enc, pred, labels, frames_lengths, labels_lengths, fc1, fc_gate, fc2, simple_am, simple_lm,
                           s_range=5, blank=0, fastemit_lambda=0.0, reduction="sum"):
    """The two losses of pruned RNN-T training in one call: (simple_loss, pruned_loss, ranges).

    enc (B, T, H) encoder output, pred (B, U+1, H) prediction-network output, labels (B, U) int32, lengths (B,) int32;
    fc1 / fc_gate (nn.Linear(2H, J)) and fc2 (nn.Linear(J, V)) are the gated joint network of `pika_amd.model.ops.joint`,
    simple_am / simple_lm (nn.Linear(H, V)) the two projections of the simple joiner am + lm.  The chain is the one above:
    `rnnt_simple_planes` of the two projections -> `rnnt_loss_from_planes(return_occupancy=True)` (the simple loss, trained
    through the planes) -> `rnnt_prune_ranges` (the band, s_range rows per frame, no gradient) -> `joint_pruned` (the
    gated joint on the band's rows only, (B, T, S, V)) -> `rnnt_loss_pruned_from_logits`.  A vocabulary that call does
    not take (V % 4 != 0 or V > 8192) goes through `joint_pruned(log_softmax=True)` and `rnnt_loss_pruned`.  The caller
    mixes the two losses (icefall: simple_scale * simple + pruned).  fastemit_lambda acts on the pruned loss; reduction
    ('sum', 'mean', None) on both.  No length is read on the host: forward plus backward capture into one torch.cuda.graph."""
    return _pruned_joint_chain(rnnt_simple_planes, enc, pred, labels, frames_lengths, labels_lengths, fc1, fc_gate, fc2,
                               simple_am, simple_lm, s_range, blank, fastemit_lambda, reduction)


def _pruned_joint_chain(planes, enc, pred, labels, frames_lengths, labels_lengths, fc1, fc_gate, fc2, simple_am, simple_lm,
                        s_range, blank, fastemit_lambda, reduction):
    # the chain of `rnnt_pruned_joint_loss`; planes(am, lm, labels, blank=) gives the simple joiner's two planes
    from .model.ops import joint_pruned, linear
    S = int(s_range)
    lam = _check_lambda(fastemit_lambda)
    am = linear(enc, simple_am.weight, simple_am.bias)
    lm = linear(pred, simple_lm.weight, simple_lm.bias)
    blank_lp, label_lp = planes(am, lm, labels, blank=blank)
    simple, occ_b, occ_l = rnnt_loss_from_planes(blank_lp, label_lp, frames_lengths, labels_lengths, reduction=reduction,
                                                 return_occupancy=True)
    ranges = rnnt_prune_ranges(occ_b, occ_l, frames_lengths, labels_lengths, S)
    if _fused_v_ok(fc2.weight.shape[0]):
        logits = joint_pruned(enc, pred, ranges, S, fc1, fc_gate, fc2, log_softmax=False)
        pruned = rnnt_loss_pruned_from_logits(logits, labels, ranges, frames_lengths, labels_lengths, reduction=reduction,
                                              blank=blank, fastemit_lambda=lam)
    else:
        log_probs = joint_pruned(enc, pred, ranges, S, fc1, fc_gate, fc2, log_softmax=True)
        pruned = rnnt_loss_pruned(log_probs, labels, ranges, frames_lengths, labels_lengths, reduction=reduction,
                                  blank=blank, fastemit_lambda=lam)
    return simple, pruned, ranges


_TINY = torch.finfo(torch.float32).tiny


def _check_scales(lm_only_scale, am_only_scale):
    try:
        ll, la = float(lm_only_scale), float(am_only_scale)
    except (TypeError, ValueError):
        raise ValueError("lm_only_scale / am_only_scale must be Python floats")
    if not (ll >= 0.0 and la >= 0.0 and ll + la < 1.0):
        raise ValueError("lm_only_scale=%r, am_only_scale=%r must be >= 0 and sum to < 1" % (lm_only_scale, am_only_scale))
    return ll, la


def _check_simple(am, lm, labels, blank):
    if am.dim() != 3 or lm.dim() != 3 or am.shape[0] != lm.shape[0] or am.shape[2] != lm.shape[2]:
        raise ValueError("am must be (B,T,V) and lm (B,U+1,V), got %s and %s" % (tuple(am.shape), tuple(lm.shape)))
    B, U1, V = lm.shape
    if labels.dim() != 2 or labels.shape != (B, U1 - 1):
        raise ValueError("labels must be (B,U)=(%d,%d), got %s" % (B, U1 - 1, tuple(labels.shape)))
    if labels.is_floating_point():
        raise ValueError("labels must be an integer tensor, got %s" % labels.dtype)
    if B < 1 or am.shape[1] < 1 or U1 < 1 or V < 1:
        raise ValueError("am (B,T,V) and lm (B,U+1,V) must not be empty, got %s and %s" % (tuple(am.shape), tuple(lm.shape)))
    if not 0 <= blank < V:
        raise ValueError("blank=%d outside [0,%d)" % (blank, V))
    if U1 > 1024:
        raise ValueError("U+1=%d > 1024 not supported" % U1)
    if lm.device != am.device or labels.device != am.device:
        raise RuntimeError("am is on %s, lm on %s, labels on %s" % (am.device, lm.device, labels.device))
    return B, am.shape[1], U1, V


def _labels_ext(labels, blank, V):
    # (B, U+1): the clamped labels, then `blank` for the last lattice column
    y = labels.long().clamp(0, V - 1)
    return torch.cat([y, y.new_full((y.shape[0], 1), blank)], 1)


def _smoothed_planes_torch(am, lm, labels, blank, ll, la):
    """The definition (DESIGN.md section 3 "Smoothed simple planes") in plain torch: max-shifted, differentiable, no
    (B, T, U+1, V) tensor.  The kernels' fp64 reference, and the path of CPU and float64 tensors."""
    B, T, V = am.shape
    U1 = lm.shape[1]
    c = 1.0 - ll - la
    am_max, lm_max = am.amax(2, keepdim=True), lm.amax(2, keepdim=True)                    # (B,T,1), (B,U1,1)
    e_am = (am - am_max).exp()
    norm = torch.matmul(e_am, (lm - lm_max).exp().transpose(1, 2)).clamp_min(_TINY).log() + am_max + lm_max.transpose(1, 2)
    yy = _labels_ext(labels, blank, V)                                                     # (B,U1)
    am_b = am[:, :, blank].unsqueeze(2)                                                    # (B,T,1)
    am_y = torch.gather(am, 2, yy.unsqueeze(1).expand(B, T, U1))                           # (B,T,U1)
    lm_b = lm[:, :, blank].unsqueeze(1)                                                    # (B,1,U1)
    lm_y = torch.gather(lm, 2, yy.unsqueeze(2)).squeeze(2).unsqueeze(1)                    # (B,1,U1)
    blank_lp, label_lp = c * (am_b + lm_b - norm), c * (am_y + lm_y - norm)
    if ll != 0.0:
        zl = torch.logsumexp(lm, 2).unsqueeze(1)                                           # (B,1,U1)
        blank_lp, label_lp = blank_lp + ll * (lm_b - zl), label_lp + ll * (lm_y - zl)
    if la != 0.0:
        q = torch.softmax(lm, 2).reshape(B * U1, V).mean(0) + _TINY                        # the batch unigram
        log_q = q.log()
        za = torch.matmul(e_am, q).unsqueeze(2).clamp_min(_TINY).log() + am_max            # (B,T,1)
        blank_lp = blank_lp + la * (am_b + log_q[blank] - za)
        label_lp = label_lp + la * (am_y + log_q[yy].unsqueeze(1) - za)
    label_lp = torch.cat([label_lp[:, :, :U1 - 1], label_lp.new_full((B, T, 1), -1.0e30)], 2)
    return blank_lp, label_lp


class _SmoothedPlanesFn(torch.autograd.Function):
    """The smoothed planes on the kernels of csrc/rnnt_simple.hip; what is (B, U+1, V)- or (V,)-sized is torch."""

    @staticmethod
    def forward(ctx, am, lm, labels, blank, ll, la):
        B, T, V = am.shape
        U1 = lm.shape[1]
        lib = _lib.lib()
        am_c, lm_c = am.detach().contiguous(), lm.detach().contiguous()
        lab = labels.to(torch.int32).contiguous()
        yy = _labels_ext(lab, blank, V)
        with torch.cuda.device(am_c.device):
            sh = lm_c - lm_c.amax(2, keepdim=True)
            elm = sh.exp()
            zl = elm.sum(2).log()                                                          # Zl - lmax, (B,U1)
            lm_b, lm_y = sh[:, :, blank], torch.gather(sh, 2, yy.unsqueeze(2)).squeeze(2)
            if la != 0.0:
                q = (elm * (-zl).exp().unsqueeze(2)).reshape(B * U1, V).mean(0) + _TINY
                log_q = q.log()
                side = torch.stack([lm_b, lm_y, zl, log_q[blank].expand(B, U1), log_q[yy]], 2).contiguous()
                e_all = torch.cat([elm, q.expand(B, 1, V)], 1)
            else:
                q = None
                side = torch.stack([lm_b, lm_y, zl, torch.zeros_like(zl), torch.zeros_like(zl)], 2).contiguous()
                e_all = elm
            NC = e_all.shape[1]
            amax = torch.empty((B, T), dtype=torch.float32, device=am_c.device)
            gathered = torch.empty((B, T, U1), dtype=torch.float32, device=am_c.device)
            sums = torch.empty((B, T, NC), dtype=torch.float32, device=am_c.device)
            blank_lp, label_lp = torch.empty_like(gathered), torch.empty_like(gathered)
            with _timed("fwd"):
                _lib.check(lib.pika_prnnt_smoothed_fwd(_ptr(am_c), _ptr(e_all), _ptr(side), _ptr(lab) if U1 > 1 else None, B, T,
                                                       U1, V, blank, ll, la, _ptr(amax), _ptr(gathered), _ptr(sums),
                                                       _ptr(blank_lp), _ptr(label_lp), _stream()),
                           "pika_prnnt_smoothed_fwd")
        ctx.save_for_backward(am_c, e_all, amax, sums, lab, yy, zl, q)
        ctx.args = (blank, ll, la)
        return blank_lp, label_lp

    @staticmethod
    def backward(ctx, g_blank, g_label):
        am_c, e_all, amax, sums, lab, yy, zl, q = ctx.saved_tensors
        blank, ll, la = ctx.args
        B, T, V = am_c.shape
        NC = e_all.shape[1]
        U1 = yy.shape[1]
        c = 1.0 - ll - la
        lib = _lib.lib()
        with torch.cuda.device(am_c.device):
            zeros = torch.zeros((B, T, U1), dtype=torch.float32, device=am_c.device)
            gb = zeros if g_blank is None else g_blank.to(torch.float32)
            gl = zeros if g_label is None else torch.cat([g_label.to(torch.float32)[:, :, :U1 - 1], zeros[:, :, :1]], 2)
            g = gb + gl
            s = sums.clamp_min(_TINY)
            w = torch.empty_like(sums)
            w[:, :, :U1] = c * g / s[:, :, :U1]
            if la != 0.0:
                w[:, :, U1] = la * g.sum(2) / s[:, :, U1]
            sg = (c + la) * gl
            sg[:, :, U1 - 1] = (c + la) * gb.sum(2)
            d_am = torch.empty_like(am_c)
            m = torch.empty_like(e_all)
            with _timed("bwd"):
                _lib.check(lib.pika_prnnt_smoothed_bwd(_ptr(am_c), _ptr(amax), _ptr(e_all), _ptr(w), _ptr(sg),
                                                       _ptr(lab) if U1 > 1 else None, B, T, U1, V, blank, ll, la,
                                                       _ptr(d_am), _ptr(m), _stream()), "pika_prnnt_smoothed_bwd")
            # the (B, U+1, V)-sized tail: scatter terms one row at a time (no index collides), softmax and unigram terms
            gbs, gls = gb.sum(1), gl.sum(1)                                                # (B,U1)
            ar = torch.arange(V, device=am_c.device)
            sc = gbs.unsqueeze(2) * (ar == blank) + gls.unsqueeze(2) * (ar == yy.unsqueeze(2))
            elm = e_all[:, :U1]
            d_lm = (c + ll) * sc - elm * m[:, :U1]
            if ll != 0.0 or la != 0.0:
                sm = elm * (-zl).exp().unsqueeze(2)
            if ll != 0.0:
                d_lm -= ll * (gbs + gls).unsqueeze(2) * sm
            if la != 0.0:
                dq = la * sc.sum((0, 1)) / q - m[:, U1].sum(0)
                d_lm += sm * (dq - (sm * dq).sum(2, keepdim=True)) / float(B * U1)
        return d_am, d_lm, None, None, None, None


def rnnt_smoothed_planes(am, lm, labels, blank=0, lm_only_scale=0.0, am_only_scale=0.0):
    """The two planes of k2's smoothed simple joiner (get_rnnt_logprobs_smoothed, regular topology): (blank_lp, label_lp),
    (B, T, U+1), differentiable w.r.t. am and lm.

    am (B, T, V), lm (B, U+1, V), labels (B, U) int (padding labels are clamped into [0, V)).  With c = 1 - lm_only_scale
    - am_only_scale, Z = logsumexp_v(am + lm), Zl = logsumexp_v lm, q the mean of softmax(lm) over all B (U+1) rows plus
    finfo(float32).tiny (the batch unigram; gradients flow through it) and Za = log sum_v exp(am) q, a class k scores
        c (am_k + lm_k - Z) + lm_only_scale (lm_k - Zl) + am_only_scale (am_k + log q_k - Za);
    blank_lp takes k = blank, label_lp[.., u] k = labels[b, u], label_lp[.., U] = -1e30.  Scales (0, 0) give
    `rnnt_simple_planes`' definition; the recipes train with (0.25, 0).  The scales are Python floats, >= 0, summing to
    < 1 (ValueError otherwise).  float32 tensors on a HIP device run the kernels of csrc/rnnt_simple.hip; CPU tensors and
    float64 tensors run the same definition in plain torch."""
    ll, la = _check_scales(lm_only_scale, am_only_scale)
    blank = int(blank)
    _check_simple(am, lm, labels, blank)
    if am.is_cuda and am.dtype == torch.float32 and lm.dtype == torch.float32:
        return _SmoothedPlanesFn.apply(am, lm, labels, blank, ll, la)
    if am.dtype != torch.float64 or lm.dtype != torch.float64:
        am, lm = am.float(), lm.float()
    return _smoothed_planes_torch(am, lm, labels, blank, ll, la)


def rnnt_loss_smoothed(am, lm, labels, frames_lengths, labels_lengths, blank=0, lm_only_scale=0.0, am_only_scale=0.0,
                       reduction=None, return_occupancy=False):
    """k2's rnnt_loss_smoothed: `rnnt_smoothed_planes` followed by `rnnt_loss_from_planes` (whose arguments and returns
    these are); differentiable w.r.t. am and lm."""
    blank_lp, label_lp = rnnt_smoothed_planes(am, lm, labels, blank=blank, lm_only_scale=lm_only_scale,
                                              am_only_scale=am_only_scale)
    return rnnt_loss_from_planes(blank_lp, label_lp, frames_lengths, labels_lengths, reduction=reduction,
                                 return_occupancy=return_occupancy)


def rnnt_pruned_joint_loss_smoothed(enc, pred, labels, frames_lengths, labels_lengths, fc1, fc_gate, fc2, simple_am,
                                    simple_lm, s_range=5, blank=0, fastemit_lambda=0.0, reduction="sum",
                                    lm_only_scale=0.0, am_only_scale=0.0):
    """`rnnt_pruned_joint_loss` with the planes of `rnnt_smoothed_planes`: the same chain, the same triple (simple_loss,
    pruned_loss, ranges), the simple loss smoothed as the pruned-transducer recipes train it (lm_only_scale = 0.25).
    Forward plus backward capture into one torch.cuda.graph."""
    ll, la = _check_scales(lm_only_scale, am_only_scale)

    def planes(am, lm, labels, blank):
        return rnnt_smoothed_planes(am, lm, labels, blank=blank, lm_only_scale=ll, am_only_scale=la)
    return _pruned_joint_chain(planes, enc, pred, labels, frames_lengths, labels_lengths, fc1, fc_gate, fc2, simple_am,
                               simple_lm, s_range, blank, fastemit_lambda, reduction)


# ---------------------------------------------------------------------------------------------------------------------
# Modified topology (k2's rnnt_loss / rnnt_loss_pruned with modified=True; include/pika_rnnt.h "Modified topology"): every
# frame emits exactly one symbol, the label edge runs (t, u) -> (t+1, u+1).  The same surface as the regular functions
# above, name for name with a `_modified` in it, over the same classes and the pika_prnnt_mod_* entries; feasible iff
# U_n <= T_n, an utterance without a path costs +inf and has a zero gradient.  Nothing reads a length on the host.
# ---------------------------------------------------------------------------------------------------------------------
def _modified_loss(x, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank, fastemit_lambda,
                   logits, caller):
    return _banded_loss(x, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank,
                        fastemit_lambda, logits, caller, True)


def rnnt_loss_modified(log_probs, labels, frames_lengths, labels_lengths, average_frames=False, reduction=None, blank=0,
                       fastemit_lambda=0.0):
    """`rnnt_loss` in the modified topology (k2's rnnt_loss(modified=True)): every frame emits exactly one symbol, so a
    label edge runs (t, u) -> (t+1, u+1), row T_n is terminal (a label may be emitted on the last frame) and an utterance
    is feasible iff U_n <= T_n; an infeasible one costs +inf, has a zero gradient and leaves the others alone.

    log_probs (B, T, U+1, V) f32, padded layout only; the other arguments as in `rnnt_loss`.  The gradient is dense,
    rows past T_n or U_n are zero.  No host synchronisation."""
    return _modified_loss(log_probs, labels, None, frames_lengths, labels_lengths, average_frames, reduction, blank,
                          fastemit_lambda, False, "rnnt_loss_modified")


def rnnt_loss_modified_from_logits(logits, labels, frames_lengths, labels_lengths, average_frames=False, reduction=None,
                                   blank=0, fastemit_lambda=0.0):
    """`rnnt_loss_modified` of log_softmax(logits) for raw logits (B, T, U+1, V), V % 4 == 0 and V <= 8192, differentiable
    w.r.t. the logits: the log-probabilities and their dense gradient never exist."""
    return _modified_loss(logits, labels, None, frames_lengths, labels_lengths, average_frames, reduction, blank,
                          fastemit_lambda, True, "rnnt_loss_modified_from_logits")


def rnnt_loss_pruned_modified(log_probs, labels, ranges, frames_lengths, labels_lengths, average_frames=False,
                              reduction=None, blank=0, fastemit_lambda=0.0):
    """`rnnt_loss_pruned` in the modified topology (k2's rnnt_loss_pruned(modified=True)): the cost of
    `rnnt_loss_modified` on a (B, T, U+1, V) tensor holding the band's rows at their cells and -1e30 elsewhere.

    Arguments as in `rnnt_loss_pruned`.  A band from `rnnt_prune_ranges_modified` holds a path whenever U_n <= T_n; one
    from `rnnt_prune_ranges` may move S - 1 columns per frame, which no path here can follow.  A band without a path costs
    +inf and has a zero gradient.  With S = U + 1 and all-zero ranges this is `rnnt_loss_modified`, bit for bit."""
    return _modified_loss(log_probs, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank,
                          fastemit_lambda, False, "rnnt_loss_pruned_modified")


def rnnt_loss_pruned_modified_from_logits(logits, labels, ranges, frames_lengths, labels_lengths, average_frames=False,
                                          reduction=None, blank=0, fastemit_lambda=0.0):
    """`rnnt_loss_pruned_modified` of log_softmax(logits) for raw logits (B, T, S, V), V % 4 == 0 and V <= 8192."""
    return _modified_loss(logits, labels, ranges, frames_lengths, labels_lengths, average_frames, reduction, blank,
                          fastemit_lambda, True, "rnnt_loss_pruned_modified_from_logits")


def rnnt_loss_from_planes_modified(blank_lp, label_lp, frames_lengths, labels_lengths, reduction=None,
                                   return_occupancy=False):
    """`rnnt_loss_from_planes` in the modified topology: blank_lp[b, t, u] is the edge (t, u) -> (t+1, u), label_lp[b, t, u]
    the edge (t, u) -> (t+1, u+1), ll = alpha(T_n, U_n).  The planes of `rnnt_simple_planes` / `rnnt_smoothed_planes` are
    topology-independent and are what this takes.  An utterance with U_n > T_n costs +inf; its gradient and occupancies
    are zero."""
    costs, occ_b, occ_l = _PlanesLossFn.apply(blank_lp, label_lp, frames_lengths, labels_lengths, True)
    costs = _reduce(costs, frames_lengths, False, reduction)
    return (costs, occ_b, occ_l) if return_occupancy else costs


def rnnt_prune_ranges_modified(blank_occ, label_occ, frames_lengths, labels_lengths, s_range):
    """`rnnt_prune_ranges` with step bound 1, the band search of the modified topology: (B, T) int32 band starts.

    raw and m as in `rnnt_prune_ranges`; f(0) = 0, f(t) = min(m(t), f(t-1) + 1), s_t = max(f(t), s_max - (T_n - 1 - t));
    s_max for t >= T_n.  s_0 = 0, 0 <= s_{t+1} - s_t <= 1 and s_{T_n-1} = s_max whenever T_n - 1 >= s_max (otherwise
    s_0 > 0); such a band holds the path u_t = min(t, s_t + S - 1) whenever U_n <= T_n."""
    return _prune_ranges("pika_prnnt_mod_prune_ranges", blank_occ, label_occ, frames_lengths, labels_lengths, s_range)


def rnnt_pruned_joint_loss_modified(enc, pred, labels, frames_lengths, labels_lengths, fc1, fc_gate, fc2, simple_am,
                                    simple_lm, s_range=5, lm_only_scale=0.0, am_only_scale=0.0, blank=0,
                                    fastemit_lambda=0.0, reduction="sum"):
    """`rnnt_pruned_joint_loss_smoothed` in the modified topology: `rnnt_smoothed_planes` ->
    `rnnt_loss_from_planes_modified` -> `rnnt_prune_ranges_modified` -> `joint_pruned` ->
    `rnnt_loss_pruned_modified_from_logits` (`rnnt_loss_pruned_modified` for a vocabulary that call does not take).
    Returns (simple_loss, pruned_loss, ranges).  Forward plus backward capture into one torch.cuda.graph."""
    from .model.ops import joint_pruned, linear
    ll, la = _check_scales(lm_only_scale, am_only_scale)
    S = int(s_range)
    lam = _check_lambda(fastemit_lambda)
    am = linear(enc, simple_am.weight, simple_am.bias)
    lm = linear(pred, simple_lm.weight, simple_lm.bias)
    blank_lp, label_lp = rnnt_smoothed_planes(am, lm, labels, blank=blank, lm_only_scale=ll, am_only_scale=la)
    simple, occ_b, occ_l = rnnt_loss_from_planes_modified(blank_lp, label_lp, frames_lengths, labels_lengths,
                                                          reduction=reduction, return_occupancy=True)
    ranges = rnnt_prune_ranges_modified(occ_b, occ_l, frames_lengths, labels_lengths, S)
    fused = _fused_v_ok(fc2.weight.shape[0])
    x = joint_pruned(enc, pred, ranges, S, fc1, fc_gate, fc2, log_softmax=not fused)
    loss = rnnt_loss_pruned_modified_from_logits if fused else rnnt_loss_pruned_modified
    pruned = loss(x, labels, ranges, frames_lengths, labels_lengths, reduction=reduction, blank=blank, fastemit_lambda=lam)
    return simple, pruned, ranges


# ---------------------------------------------------------------------------------------------------------------------
# Forced alignment on the pruned and the modified-topology lattices (include/pika_rnnt.h, pika_rnnt_align and
# pika_mrnnt_align): `rnnt_align` for every lattice a loss above is computed on.  Each call runs the forward entry of the
# loss it mirrors into a fresh workspace and the align entry of that topology on it; inputs and checks are the mirrored
# loss's, float32 only.  All return (scores (B,) f32, emit_frames (B, U) i32), detached; entries u >= U_n are -1.  Nothing
# reads a length on the host: every call can be captured in a torch.cuda.graph.
#   regular topology   emit_frames non-decreasing in u, in [0, T_n - 1]; a band without a path keeps pika_rnnt_align's
#                      behaviour for an infeasible transcript: a valid monotone path with a score <= -1e30.
#   modified topology  emit_frames strictly increasing in u (one symbol per frame), score = delta(T_n, U_n); an utterance
#                      whose loss is +inf (U_n > T_n, a band without a path, a label outside [0, V)) gets score -inf and
#                      frames -1, and leaves the others alone.
# Ties go to the earliest emission in both.
# ---------------------------------------------------------------------------------------------------------------------
def _align_banded(x, labels, ranges, frames_lengths, labels_lengths, blank, logits, caller, modified):
    """The (B,T,S,V) / (B,T,U1,V) forms: `_BandedLossFn.forward`'s checks and forward call, then the align entry."""
    what = "logits" if logits else "log_probs"
    if ranges is None:
        B, T, U1, S, V = _check_full(x, what, labels, frames_lengths, labels_lengths, blank)
    else:
        B, T, U1, S, V = _check_pruned(x, what, labels, ranges, frames_lengths, labels_lengths, blank)
        ranges = ranges.contiguous()
    if logits and not _fused_v_ok(V):
        raise ValueError("%s: V = %d must be a multiple of 4 and <= %d" % (caller, V, MAX_FUSED_V))
    lib = _lib.lib()
    fwd, _, ws_bytes = _BANDED_ENTRIES[modified, logits]
    x = x.detach().contiguous()
    labels, frames_lengths, labels_lengths = (t.contiguous() for t in (labels, frames_lengths, labels_lengths))
    with torch.cuda.device(x.device):
        costs = torch.empty(B, dtype=torch.float32, device=x.device)
        lse = torch.empty(B * T * S, dtype=torch.float32, device=x.device) if logits else None
        ws = torch.empty(getattr(lib, ws_bytes)(B, T, U1), dtype=torch.uint8, device=x.device)
        _lib.check(getattr(lib, fwd)(_ptr(x), _ptr(frames_lengths), _ptr(labels_lengths), _ptr(labels), _ptr(ranges),
                                     B, T, U1, S, V, int(blank), _ptr(costs), *((_ptr(lse),) if logits else ()), _ptr(ws),
                                     _stream()), fwd)
        scores, frames = _align_call(lib, ws, frames_lengths, labels_lengths, None, B, T, U1, B * (U1 - 1), x.device,
                                     modified)
    return scores, frames.view(B, U1 - 1)


def _align_planes(blank_lp, label_lp, frames_lengths, labels_lengths, modified):
    """The two-plane forms: `_PlanesLossFn.forward`'s checks and forward call, then the align entry."""
    B, T, U1 = _check_planes(blank_lp, label_lp, frames_lengths, labels_lengths, ("blank_lp", "label_lp"))
    lib = _lib.lib()
    fn, ws_bytes = (("pika_prnnt_mod_planes_forward", "pika_prnnt_mod_workspace_bytes") if modified else
                    ("pika_prnnt_planes_forward", "pika_rnnt_workspace_bytes"))
    pb, pl = blank_lp.detach().contiguous(), label_lp.detach().contiguous()
    frames_lengths, labels_lengths = frames_lengths.contiguous(), labels_lengths.contiguous()
    with torch.cuda.device(pb.device):
        costs = torch.empty(B, dtype=torch.float32, device=pb.device)
        occ_b, occ_l = torch.empty_like(pb), torch.empty_like(pb)
        ws = torch.empty(getattr(lib, ws_bytes)(B, T, U1), dtype=torch.uint8, device=pb.device)
        _lib.check(getattr(lib, fn)(_ptr(pb), _ptr(pl), _ptr(frames_lengths), _ptr(labels_lengths), B, T, U1,
                                    _ptr(costs), _ptr(occ_b), _ptr(occ_l), _ptr(ws), _stream()), fn)
        scores, frames = _align_call(lib, ws, frames_lengths, labels_lengths, None, B, T, U1, B * (U1 - 1), pb.device,
                                     modified)
    return scores, frames.view(B, U1 - 1)


def rnnt_align_pruned(log_probs, labels, ranges, frames_lengths, labels_lengths, blank=0):
    """`rnnt_align` on the pruned (banded) lattice of `rnnt_loss_pruned`: the best path through the band's cells.

    log_probs (B, T, S, V) f32, labels (B, U), ranges (B, T) int32 as in `rnnt_loss_pruned`.  Returns (scores (B,) f32,
    emit_frames (B, U) i32), detached: the path is that of `rnnt_align` on a (B, T, U+1, V) tensor holding the band's
    rows at their cells and -1e30 elsewhere, and with S = U + 1 and all-zero ranges it is `rnnt_align`, bit for bit.
    emit_frames is non-decreasing in u, in [0, T_n - 1], -1 from U_n on; ties go to the earliest emission.  A band that
    holds no path still yields a valid monotone path (through dead cells); its score is <= -1e30.  No host
    synchronisation."""
    return _align_banded(log_probs, labels, ranges, frames_lengths, labels_lengths, blank, False, "rnnt_align_pruned", False)


def rnnt_align_pruned_from_logits(logits, labels, ranges, frames_lengths, labels_lengths, blank=0):
    """`rnnt_align_pruned` of log_softmax(logits) for raw logits (B, T, S, V), V % 4 == 0 and V <= 8192: the planes come
    from the one read of the logits `rnnt_loss_pruned_from_logits` makes."""
    return _align_banded(logits, labels, ranges, frames_lengths, labels_lengths, blank, True,
                         "rnnt_align_pruned_from_logits", False)


def rnnt_align_from_planes(blank_lp, label_lp, frames_lengths, labels_lengths):
    """`rnnt_align` of a lattice given by its two (B, T, U+1) planes, those `rnnt_loss_from_planes` takes (the "simple"
    lattice of pruned RNN-T).  Returns (scores, emit_frames (B, U)) as `rnnt_align` does."""
    return _align_planes(blank_lp, label_lp, frames_lengths, labels_lengths, False)


def rnnt_align_modified(log_probs, labels, frames_lengths, labels_lengths, blank=0):
    """Forced alignment in the modified topology, the best path of `rnnt_loss_modified`'s lattice.

    log_probs (B, T, U+1, V) f32, padded layout.  Returns (scores (B,) f32, emit_frames (B, U) i32), detached:
    delta(0, 0) = 0, delta(t+1, u) = max(delta(t, u) + lpb(t, u), delta(t, u-1) + lpe(t, u-1)), scores[n] =
    delta(T_n, U_n) <= -cost_n; emit_frames[n][u], u < U_n, is the frame at which the path emits label u -- strictly
    increasing in u (a frame emits one symbol), in [0, T_n - 1] -- and -1 from U_n on.  Ties go to the earliest emission.
    An utterance whose loss is +inf (U_n > T_n, a label outside [0, V)) gets score -inf and frames -1 and leaves the
    others alone.  No host synchronisation."""
    return _align_banded(log_probs, labels, None, frames_lengths, labels_lengths, blank, False, "rnnt_align_modified", True)


def rnnt_align_modified_from_logits(logits, labels, frames_lengths, labels_lengths, blank=0):
    """`rnnt_align_modified` of log_softmax(logits) for raw logits (B, T, U+1, V), V % 4 == 0 and V <= 8192."""
    return _align_banded(logits, labels, None, frames_lengths, labels_lengths, blank, True,
                         "rnnt_align_modified_from_logits", True)


def rnnt_align_pruned_modified(log_probs, labels, ranges, frames_lengths, labels_lengths, blank=0):
    """`rnnt_align_modified` on the band (B, T, S, V) of `rnnt_loss_pruned_modified`: the best path through the band's
    cells.  A band that holds no path (one of `rnnt_prune_ranges` may jump S - 1 columns) gives score -inf and frames
    -1.  With S = U + 1 and all-zero ranges this is `rnnt_align_modified`, bit for bit."""
    return _align_banded(log_probs, labels, ranges, frames_lengths, labels_lengths, blank, False,
                         "rnnt_align_pruned_modified", True)


def rnnt_align_pruned_modified_from_logits(logits, labels, ranges, frames_lengths, labels_lengths, blank=0):
    """`rnnt_align_pruned_modified` of log_softmax(logits) for raw logits (B, T, S, V), V % 4 == 0 and V <= 8192."""
    return _align_banded(logits, labels, ranges, frames_lengths, labels_lengths, blank, True,
                         "rnnt_align_pruned_modified_from_logits", True)


def rnnt_align_from_planes_modified(blank_lp, label_lp, frames_lengths, labels_lengths):
    """`rnnt_align_from_planes` in the modified topology, on the planes `rnnt_loss_from_planes_modified` takes; an
    utterance with U_n > T_n gets score -inf and frames -1."""
    return _align_planes(blank_lp, label_lp, frames_lengths, labels_lengths, True)


class RNNTLoss(object):
    """`RNNTLoss(blank=0, reduction='sum').apply(...)` exactly as the reference scripts use it.

    As with the binding the reference imports, `reduction` does not change what `.apply` returns:
    per-utterance costs (B,), which the caller reduces itself (train_transducer_bmuf_otfaug.py:99
    `loss = loss.sum()`).  `fastemit_lambda` (finite, >= 0) scales the label-emission entries of the
    gradient by 1 + lambda, as in `rnnt_loss`.
    """

    def __init__(self, blank=0, reduction="sum", fastemit_lambda=0.0, **unused):
        self.blank = int(blank)
        self.reduction = reduction
        self.fastemit_lambda = _check_lambda(fastemit_lambda)

    def apply(self, log_probs, labels, frames_lengths, labels_lengths):
        return _RNNTLossFn.apply(log_probs, labels, frames_lengths, labels_lengths, self.blank, self.fastemit_lambda)

    __call__ = apply


def export_lattice(ctx_ws, frames_lengths, labels_lengths, B, T, U1):
    """Diagnostic: dense (B,T,U1) alpha/beta from a workspace tensor (tests only)."""
    lib = _lib.lib()
    a = torch.empty((B, T, U1), dtype=torch.float32, device=ctx_ws.device)
    b = torch.empty_like(a)
    _lib.check(lib.pika_rnnt_export_lattice(_ptr(ctx_ws), _ptr(frames_lengths), _ptr(labels_lengths),
                                            B, T, U1, _ptr(a), _ptr(b), _stream()),
               "pika_rnnt_export_lattice")
    return a, b
