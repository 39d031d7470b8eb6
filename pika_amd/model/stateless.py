"""The stateless prediction network of the pruned / modified-topology transducer recipes (icefall's `Decoder`): an
embedding, a grouped causal `Conv1d` over the last `context_size` labels and a ReLU.  A hypothesis' output is a function
of its last `context_size` tokens and of nothing else.

`StatelessPredNet` is the module, with icefall's parameter names (`embedding.weight`, `conv.weight`); on a HIP device in
float32 its forward and backward are the kernels of include/pika_stateless.h (csrc/stateless.hip): no atomics, the same
bits on every run.  `StatelessContext` is what a one-symbol-per-frame search keeps per slot instead of a network state:
the slot's last tokens, and the network's rows for them, followed through `advance`'s (parent, token) by one kernel.
The definition is in the header and in DESIGN.md section 3, "Stateless prediction network"."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib

MAX_CTX, MAX_CPG, MAX_DIM, MAX_BEAM, MAX_BATCH, MAX_ROWS = 8, 16, 8192, 64, 65535, 1 << 30


def _ptr(t):
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _within_limits(D, cpg, ctx):
    return 1 <= ctx <= MAX_CTX and 1 <= cpg <= MAX_CPG and 1 <= D <= MAX_DIM and D % cpg == 0


def stateless_reference(y, E, w):
    """The definition in plain torch, any device and float dtype: y (B, U) int64 -> (B, U, D)."""
    D, cpg, ctx = w.shape
    keep = (y >= 0).unsqueeze(-1)
    e = F.embedding(y.clamp(0, E.shape[0] - 1), E) * keep.to(E.dtype)
    z = F.conv1d(F.pad(e.transpose(1, 2), (ctx - 1, 0)), w, groups=D // cpg)
    return F.relu(z).transpose(1, 2)


class _StatelessFn(torch.autograd.Function):
    """forward / backward through pika_stateless_forward / _backward: y (B, U) int64, E (V, D), w (D, cpg, ctx) float32 on
    one HIP device."""

    @staticmethod
    def forward(ctx_, y, E, w):
        B, U = y.shape
        (V, D), (_, cpg, ctx) = E.shape, w.shape
        y, E, w = y.contiguous(), E.contiguous(), w.contiguous()
        with torch.cuda.device(E.device):
            out = torch.empty((B, U, D), dtype=torch.float32, device=E.device)
            _lib.check(_lib.lib().pika_stateless_forward(_ptr(y), U, _ptr(E), _ptr(w), B, U, V, D, cpg, ctx, _ptr(out), D,
                                                         _stream()), "pika_stateless_forward")
        ctx_.save_for_backward(y, E, w, out)
        return out

    @staticmethod
    def backward(ctx_, dout):
        y, E, w, out = ctx_.saved_tensors
        B, U = y.shape
        (V, D), (_, cpg, ctx) = E.shape, w.shape
        dout = dout.contiguous()
        lib = _lib.lib()
        with torch.cuda.device(E.device):
            # equal tokens in position order: the order in which d_E sums a token's positions
            sorted_tok, order = torch.sort(y.reshape(-1), stable=True)
            d_E = torch.empty_like(E)
            d_w = torch.empty_like(w)
            work = torch.empty(lib.pika_stateless_backward_workspace_bytes(B, U, D, cpg, ctx), dtype=torch.uint8,
                               device=E.device)
            _lib.check(lib.pika_stateless_backward(_ptr(y), U, _ptr(sorted_tok), _ptr(order), _ptr(E), _ptr(w), _ptr(out), D,
                                                   _ptr(dout), D, B, U, V, D, cpg, ctx, _ptr(d_E), _ptr(d_w), _ptr(work),
                                                   _stream()), "pika_stateless_backward")
        return None, d_E, d_w


class StatelessPredNet(nn.Module):
    """Embedding + grouped causal Conv1d over the last `context_size` labels + ReLU.

    vocab_size, dim   the embedding's shape; context_size (icefall: 2); groups of the convolution (None: dim // 4, icefall's
    choice: four channels per group); blank: the SOS token, an ordinary row of the embedding.
    Submodules `embedding` (nn.Embedding, no padding_idx) and `conv` (nn.Conv1d, bias=False): the state_dict keys are
    `embedding.weight` and `conv.weight`, so an icefall `Decoder` checkpoint loads.

    forward(y (B, U) int64, rows that already start with SOS; a negative token is padding: a zero vector that gets no
    gradient) -> (B, U, dim).  float32 parameters on a HIP device within the kernels' limits (context_size <= 8, channels per
    group <= 16, dim <= 8192, B <= 65535) run the HIP kernels, forward and backward; CPU tensors, float64 and anything
    beyond the limits run the same definition in plain torch."""

    def __init__(self, vocab_size, dim, context_size=2, groups=None, blank=0):
        super().__init__()
        vocab_size, dim, context_size, blank = int(vocab_size), int(dim), int(context_size), int(blank)
        groups = dim // 4 if groups is None else int(groups)
        if vocab_size < 1 or dim < 1 or context_size < 1:
            raise ValueError("need vocab_size, dim, context_size >= 1, got %d, %d, %d" % (vocab_size, dim, context_size))
        if groups < 1 or dim % groups != 0:
            raise ValueError("groups must divide dim, got dim=%d, groups=%s" % (dim, groups))
        if not 0 <= blank < vocab_size:
            raise ValueError("need 0 <= blank < vocab_size, got blank=%d" % blank)
        self.vocab_size, self.dim, self.context_size, self.groups, self.blank = vocab_size, dim, context_size, groups, blank
        self.embedding = nn.Embedding(vocab_size, dim)
        self.conv = nn.Conv1d(dim, dim, kernel_size=context_size, groups=groups, bias=False)

    def native(self, rows=1, length=1):
        """Do the HIP kernels serve a (rows, length) label batch with the parameters as they are?"""
        E, w = self.embedding.weight, self.conv.weight
        return (E.is_cuda and w.device == E.device and E.dtype == torch.float32 and w.dtype == torch.float32
                and _within_limits(self.dim, self.dim // self.groups, self.context_size)
                and 1 <= rows <= MAX_BATCH and length >= 1 and rows * length <= MAX_ROWS)

    def forward(self, y):
        if y.dim() != 2 or y.dtype != torch.int64:
            raise ValueError("y must be (B, U) int64, got %s %s" % (tuple(y.shape), y.dtype))
        E, w = self.embedding.weight, self.conv.weight
        if y.is_cuda and y.device == E.device and self.native(y.shape[0], y.shape[1]):
            return _StatelessFn.apply(y, E, w)
        return stateless_reference(y, E, w)


class StatelessContext(object):
    """What a one-symbol-per-frame search keeps per slot for a `StatelessPredNet`: `batch` utterances of `beam` slots.

    tokens   the live record, (batch, beam, context_size) int32: a slot's last tokens, -1 where the hypothesis is shorter;
             [-1, ..., -1, blank] after a reset.
    rows     (batch * beam, dim): the network's output for every slot's context -- the prediction half of the joint.
    reset(which=None)   every utterance, or those selected by `which` ((batch,) bool / int), back to the empty hypothesis.
    follow(parent, token)   with what `advance` returned, both (batch, beam) int64: slot j takes the OLD context of slot
             clamp(parent[b, j], 0, beam - 1); where token != blank it is shifted left by one and the token appended; `rows`
             is recomputed.  `parent` may repeat a slot.
    reorder(slot_map)   follow(slot_map, all blank): after a stream's commit.
             Empty slots carry whatever context they inherit; their rows are never used.
    blank    None: the network's.

    Where the network runs its kernels this is ONE launch of pika_stateless_step per call, no host synchronisation,
    capturable in a `torch.cuda.graph`, and `rows` equals the network's forward on the contexts bit for bit (one device
    function serves both).  Elsewhere the same semantics run in plain torch."""

    def __init__(self, net, batch, beam, blank=None):
        if not isinstance(net, StatelessPredNet):
            raise TypeError("net must be a StatelessPredNet, got %s" % type(net).__name__)
        batch, beam = int(batch), int(beam)
        if batch < 1 or beam < 1:
            raise ValueError("need batch >= 1 and beam >= 1, got %d, %d" % (batch, beam))
        self.net, self.batch, self.beam = net, batch, beam
        self.blank = net.blank if blank is None else int(blank)
        if not 0 <= self.blank < net.vocab_size:
            raise ValueError("need 0 <= blank < vocab_size, got blank=%d" % self.blank)
        E = net.embedding.weight
        self.device, self.ctx = E.device, net.context_size
        self.native = net.native() and batch <= MAX_BATCH and beam <= MAX_BEAM
        self.tokens = torch.empty((batch, beam, self.ctx), dtype=torch.int32, device=self.device)
        self.rows = torch.empty((batch * beam, net.dim), dtype=E.dtype, device=self.device)
        self._identity = torch.arange(beam, dtype=torch.int64, device=self.device).repeat(batch, 1)
        self._blanks = torch.full((batch, beam), self.blank, dtype=torch.int64, device=self.device)
        self._fresh = torch.full((self.ctx,), -1, dtype=torch.int32, device=self.device)
        self._fresh[-1] = self.blank
        self.reset()

    @torch.no_grad()
    def reset(self, which=None):
        if which is None:
            self.tokens.copy_(self._fresh.expand_as(self.tokens))
        else:
            which = torch.as_tensor(which)
            if which.dtype not in (torch.bool, torch.int32, torch.int64) or which.numel() != self.batch:
                raise ValueError("which must be (batch,) = (%d,) bool, int32 or int64" % self.batch)
            sel = which.reshape(-1).to(self.device).ne(0).view(-1, 1, 1)
            self.tokens.copy_(torch.where(sel, self._fresh.expand_as(self.tokens), self.tokens))
        self.follow(self._identity, self._blanks)

    def reorder(self, slot_map):
        """Slot j takes the context of slot slot_map[b, j]: what a stream's commit asks for."""
        self.follow(slot_map, self._blanks)

    @torch.no_grad()
    def follow(self, parent, token):
        B, K, ctx = self.batch, self.beam, self.ctx
        for t, name in ((parent, "parent"), (token, "token")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != (B, K):
                raise ValueError("%s must be a (%d, %d) int64 tensor" % (name, B, K))
            if t.device != self.device:
                raise ValueError("the context lives on %s, %s on %s" % (self.device, name, t.device))
        net = self.net
        E, w = net.embedding.weight, net.conv.weight
        if self.native:
            parent, token = parent.contiguous(), token.contiguous()
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().pika_stateless_step(
                    _ptr(self.tokens), _ptr(parent), _ptr(token), B, K, ctx, self.blank, _ptr(E), _ptr(w), net.vocab_size,
                    net.dim, net.dim // net.groups, _ptr(self.rows), net.dim, _stream()), "pika_stateless_step")
            return
        old = self.tokens.gather(1, parent.clamp(0, K - 1).unsqueeze(-1).expand(B, K, ctx))
        grown = torch.cat((old[..., 1:], token.clamp(-1, 2 ** 31 - 1).to(torch.int32).unsqueeze(-1)), dim=-1)
        self.tokens.copy_(torch.where(token.ne(self.blank).unsqueeze(-1), grown, old))
        self.rows.copy_(stateless_reference(self.tokens.view(B * K, ctx).long(), E, w)[:, -1, :])
