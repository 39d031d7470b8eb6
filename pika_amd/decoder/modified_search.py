"""One-symbol-per-frame ("modified") transducer beam search: the search that belongs to the modified topology of
`rnnt_loss_modified` / `rnnt_pruned_joint_loss_modified`, in which every frame emits exactly one symbol -- blank or a
label (k2's `modified=True`, icefall's `modified_beam_search`).  Every hypothesis consumes one frame per step, so an
utterance of T_n frames takes T_n steps, a batch max(T_n), known before the first launch: the loop reads nothing back.

`ModifiedBeamState` is the search state and its frame step (include/pika_msearch.h, csrc/msearch.hip);
`modified_beam_search` drives a transducer model through it.  The definition of a step is in the header and in DESIGN.md
section 3, "Modified beam search"; `_torch_step` below spells it in plain torch.

`ModifiedLmBeamState` / `modified_beam_search_lm` are the same with an n-gram LM, a hotword list or both fused into the
ranking (include/pika_msearch_lm.h; DESIGN.md section 3, "Modified beam search with an LM"): the `lm` is what the CTC
searches take -- a `CtcNgramLm`, a `CtcHotwords` alone, or a `CtcBiasedLm` pair.

`ModifiedNnLmBeamState` / `modified_beam_search_nnlm` fuse a NEURAL LM -- a dense row of LM logits per hypothesis and
frame (include/pika_msearch_nn.h; DESIGN.md section 3, "Modified beam search with a neural LM"), such as
`pika_amd.model.lm.LstmLm` -- alone or beside those automata; a low-order n-gram on a negative weight beside it is LODR.

`ModifiedBeamStream` wraps either state into a stream that outlives `max_frames` (include/pika_msearch_stream.h;
DESIGN.md section 3, "Streaming modified beam search"): `commit` emits the labels every hypothesis shares and gives the
capacity back.  `ModifiedStreamDecoder` drives a model with the LSTM prediction network through it chunk by chunk.

`ModifiedBeamTimes` keeps the token time stamps of any of the three next to it (include/pika_msearch_times.h; DESIGN.md
section 3, "Time stamps of the modified beam search"); `modified_beam_search_timed` and
`ModifiedStreamDecoder.track_times` are its drivers.
"""
import torch

from .. import _lib

MAX_BEAM = 64
ROOT = 0x7ffffffe


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _torch_step(scores, logits, blank, sm_scale, blank_penalty):
    """The step's definition on one utterance, in the dtype of `logits`: scores (K,), logits (K,V) ->
    [(merged score, representative's slot k, its v, [(k, v) of the members in rank order])] in the new beam's order."""
    K, V = logits.shape
    x = sm_scale * logits
    x[:, blank] = x[:, blank] - blank_penalty
    m = x.max(dim=1, keepdim=True).values
    dead = ~(m > -float("inf"))
    m = torch.where(dead, torch.zeros_like(m), m)
    lp = (x - m) - torch.log(torch.exp(x - m).sum(dim=1, keepdim=True))
    lp = torch.where(dead.expand_as(lp), torch.full_like(lp, -float("inf")), lp)
    cand = scores.to(logits.dtype).unsqueeze(1) + lp
    cand = torch.where((scores > -float("inf")).unsqueeze(1).expand_as(cand), cand, torch.full_like(cand, -float("inf")))
    # the total order: larger value, then lower k, then lower v -- a stable descending sort of the (k, v)-major array
    val, idx = torch.sort(cand.reshape(-1), descending=True, stable=True)
    sel = [(val[r], int(idx[r]) // V, int(idx[r]) % V) for r in range(min(K, K * V)) if val[r] > -float("inf")]
    return sel


class _BeamState(object):
    """What the search states share: the views of the state, and the checks and the allocation of a call's tensors."""

    @property
    def frames(self):
        return self._frames

    @property
    def scores(self):
        return self._scores

    @property
    def overflowed(self):
        return self._over != 0

    def _which(self, which):
        if which is not None:
            which = torch.as_tensor(which)
            if which.dtype not in (torch.bool, torch.int32, torch.int64):
                raise TypeError("which must be bool, int32 or int64, got %s" % which.dtype)
            which = which.reshape(-1).to(self.device, torch.int32).contiguous()
            if which.numel() != self.batch:
                raise ValueError("which must hold batch = %d entries" % self.batch)
        return which

    def _check_logits(self, logits, num_frames):
        if not isinstance(logits, torch.Tensor):
            raise TypeError("logits must be a tensor")
        if self.native and not logits.is_cuda:
            raise RuntimeError("pika_amd %s: logits must live on a HIP device (the state does)" % type(self).__name__)
        if logits.dtype != self.dtype:
            raise TypeError("logits must be %s, got %s" % (self.dtype, logits.dtype))
        if logits.device != self.device:
            raise ValueError("the state lives on %s, logits on %s" % (self.device, logits.device))
        if logits.dim() != 2 or logits.shape[0] != self.batch * self.beam:
            raise ValueError("logits must be (batch * beam, V) = (%d, V), got %s" % (self.batch * self.beam,
                                                                                 tuple(logits.shape)))
        V = logits.shape[1]
        if V < 2 or not 0 <= self.blank < V:
            raise ValueError("need V >= 2 and 0 <= blank < V, got V=%d, blank=%d" % (V, self.blank))
        if logits.stride(1) != 1 or logits.stride(0) < V:
            raise ValueError("logits rows must be contiguous (class stride 1, row stride >= V), got strides %s"
                             % (tuple(logits.stride()),))
        num_frames = torch.as_tensor(num_frames)
        if num_frames.dtype not in (torch.int32, torch.int64) or num_frames.numel() != self.batch:
            raise ValueError("num_frames must be (batch,) int32 or int64")
        return logits, num_frames.reshape(-1).to(self.device, torch.int64).contiguous()

    @staticmethod
    def _finite(sm_scale, blank_penalty):
        sm_scale, blank_penalty = float(sm_scale), float(blank_penalty)
        if sm_scale != sm_scale or sm_scale in (float("inf"), -float("inf")) or blank_penalty != blank_penalty \
                or blank_penalty in (float("inf"), -float("inf")):
            raise ValueError("sm_scale and blank_penalty must be finite")
        return sm_scale, blank_penalty

    def _nbest(self, nbest):
        nbest = int(nbest)
        if not 1 <= nbest <= self.beam:
            raise ValueError("need 1 <= nbest <= beam = %d, got nbest=%d" % (self.beam, nbest))
        return nbest

    def _read(self, n, max_len):
        L = self.max_frames if max_len is None else int(max_len)
        if L < 1:
            raise ValueError("max_len must be >= 1, got %d" % L)
        B, K = self.batch, self.beam
        if self.native:
            with torch.cuda.device(self.device):
                tokens = torch.empty((B, n, L), dtype=torch.int64, device=self.device)
                lengths = torch.empty((B, n), dtype=torch.int64, device=self.device)
            return tokens, lengths, L
        tokens = torch.full((B, n, L), -1, dtype=torch.int64)
        lengths = torch.full((B, n), -1, dtype=torch.int64)
        for b in range(B):
            nodes = self._tries[b][1]
            for j in range(n):
                if self._scores[b, j] > -float("inf"):
                    seq, node = [], self._node[b][j]
                    while node != 0:
                        node, tok = nodes[node]
                        seq.append(tok)
                    seq.reverse()
                    lengths[b, j] = len(seq)
                    tokens[b, j, :min(len(seq), L)] = torch.tensor(seq[:L], dtype=torch.int64)
        return tokens.to(self.device), lengths.to(self.device), L


class ModifiedBeamState(_BeamState):
    """The state of a one-symbol-per-frame beam search over `batch` utterances of at most `max_frames` frames with
    `beam` slots each, and its frame step.

    advance(logits, num_frames, sm_scale=1.0, blank_penalty=0.0) -> (parent, token), both (batch, beam) int64
        logits (batch * beam, V): row b * beam + k is the joint network's output for slot k of utterance b at frame
        frames[b]; any row stride >= V (the class stride must be 1).  num_frames (batch,) int64: utterance b is ACTIVE
        while frames[b] < min(num_frames[b], max_frames).  For an active utterance the beam's candidates
        score[k] + log_softmax(sm_scale * logits[k] - blank_penalty [blank])[v] are cut to the `beam` best, candidates
        that spell the same token sequence are merged (log-sum-exp), and slot j of the new beam came from slot
        parent[b, j] by token[b, j] (blank: the sequence did not grow).  An inactive utterance keeps its state and
        gets parent[b, j] = j, token = blank, so a caller that re-orders its prediction-network state by `parent` and
        steps it where token != blank leaves it alone.  Empty slots (fewer than `beam` candidates exist) have score
        -inf, parent 0, token blank.
    results(nbest=1, max_len=None) -> (tokens (batch, nbest, L) int64, -1 beyond the length; lengths (batch, nbest)
        int64, -1 for a missing entry; scores (batch, nbest), -inf for a missing entry), the beam's order (best
        first).  L = max_len or max_frames; a longer entry reports its true length and its first L tokens.
    hyps(max_len=None) -> (tokens (batch, beam, L), lengths (batch, beam)): the same for the current slots.
    reset(which=None)   every utterance, or those selected by `which` ((batch,) bool / int), back to the empty sequence.
    frames, scores, overflowed   live views of the state: (batch,) int32, (batch, beam) float, (batch,) bool
        (overflowed: num_frames[b] > max_frames and the state is full; the further frames are ignored).

    On a HIP device the state is one blob of device memory and every call is a HIP kernel launch with no host
    synchronisation, capturable in a `torch.cuda.graph`; logits must then be float32 on that device -- anything else
    raises.  On the CPU, or with dtype=torch.float64, the same definition runs in plain torch (per-utterance Python
    loops: a spelling of the definition, not a fast path)."""

    def __init__(self, batch, max_frames, beam=4, blank=0, device=None, dtype=None):
        batch, max_frames, beam, blank = int(batch), int(max_frames), int(beam), int(blank)
        if not 1 <= beam <= MAX_BEAM:
            raise ValueError("need 1 <= beam <= %d, got beam=%d" % (MAX_BEAM, beam))
        if batch < 1 or max_frames < 1 or blank < 0:
            raise ValueError("need batch >= 1, max_frames >= 1 and blank >= 0, got %d, %d, %d" % (batch, max_frames, blank))
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("dtype must be float32 or float64, got %s" % dtype)
        self.batch, self.max_frames, self.beam, self.blank = batch, max_frames, beam, blank
        self.device, self.dtype = dev, dtype
        self.native = dev.type == "cuda" and dtype == torch.float32
        if self.native:
            lib = _lib.lib()
            nbytes = lib.pika_msearch_state_bytes(batch, beam, max_frames)
            if nbytes == 0:
                raise ValueError("(batch,max_frames,beam) = (%d,%d,%d) not supported" % (batch, max_frames, beam))
            with torch.cuda.device(dev):
                self._state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            BK = batch * beam       # the layout of include/pika_msearch.h
            self._scores = self._state[:4 * BK].view(torch.float32).view(batch, beam)
            self._frames = self._state[12 * BK:12 * BK + 4 * batch].view(torch.int32)
            self._over = self._state[12 * BK + 4 * batch:12 * BK + 8 * batch].view(torch.int32)
        else:
            self._scores = torch.empty((batch, beam), dtype=dtype, device=dev)
            self._frames = torch.empty(batch, dtype=torch.int32, device=dev)
            self._over = torch.empty(batch, dtype=torch.int32, device=dev)
            self._node = [[0] * beam for _ in range(batch)]       # per slot: the node of its token sequence, 0 = root
            self._tries = [None] * batch                          # per utterance: ({(parent, token): node}, [(parent, token)])
        self.reset()

    def reset(self, which=None):
        which = self._which(which)
        if self.native:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().pika_msearch_reset(_ptr(self._state), self.batch, self.beam, self.max_frames,
                                                         _ptr(which), _stream()), "pika_msearch_reset")
            return
        sel = range(self.batch) if which is None else [b for b, w in enumerate(which.tolist()) if w]
        for b in sel:
            self._scores[b] = -float("inf")
            self._scores[b, 0] = 0.0
            self._frames[b] = 0
            self._over[b] = 0
            self._node[b] = [0] * self.beam
            self._tries[b] = ({}, [(-1, -1)])

    def advance(self, logits, num_frames, sm_scale=1.0, blank_penalty=0.0):
        sm_scale, blank_penalty = self._finite(sm_scale, blank_penalty)
        logits, num_frames = self._check_logits(logits, num_frames)
        B, K, V = self.batch, self.beam, logits.shape[1]
        if self.native:
            with torch.cuda.device(self.device):
                parent = torch.empty((B, K), dtype=torch.int64, device=self.device)
                token = torch.empty((B, K), dtype=torch.int64, device=self.device)
                _lib.check(_lib.lib().pika_msearch_advance(
                    _ptr(self._state), _ptr(logits), logits.stride(0), _ptr(num_frames), B, K, self.max_frames, V,
                    self.blank, sm_scale, blank_penalty, _ptr(parent), _ptr(token), _stream()), "pika_msearch_advance")
            return parent, token
        parent = torch.arange(K, dtype=torch.int64).repeat(B, 1)
        token = torch.full((B, K), self.blank, dtype=torch.int64)
        nf = num_frames.tolist()
        for b in range(B):
            frames = int(self._frames[b])
            if frames < min(max(nf[b], 0), self.max_frames):
                self._advance_one(b, logits[b * K:(b + 1) * K].clone(), sm_scale, blank_penalty, parent[b], token[b])
                frames += 1
                self._frames[b] = frames
            if frames >= self.max_frames and nf[b] > self.max_frames:
                self._over[b] = 1
        return parent.to(self.device), token.to(self.device)

    def _advance_one(self, b, logits, sm_scale, blank_penalty, parent, token):
        K, blank, ninf = self.beam, self.blank, -float("inf")
        index, nodes = self._tries[b]
        scores = self._scores[b].clone()
        groups, by_key = [], {}
        for c, k, v in _torch_step(scores, logits, blank, sm_scale, blank_penalty):
            pn = self._node[b][k]
            if v == blank:
                key = pn
            else:
                key = index.get((pn, v))
                if key is None:
                    key = index[(pn, v)] = len(nodes)
                    nodes.append((pn, v))
            if key not in by_key:
                by_key[key] = len(groups)
                groups.append([key, k, v, [c]])
            else:
                groups[by_key[key]][3].append(c)
        merged = []
        for rank, (key, k, v, cs) in enumerate(groups):
            s = torch.zeros((), dtype=logits.dtype)
            for c in cs:                                    # in rank order, from the group's largest value
                s = s + torch.exp(c - cs[0])
            merged.append((cs[0] + torch.log(s), rank, key, k, v))
        merged.sort(key=lambda g: (-float(g[0]), g[1]))     # (exact: a float64 holds every float32)
        new_nodes = [0] * K
        for j in range(K):
            if j < len(merged):
                sc, _, key, k, v = merged[j]
                self._scores[b, j] = sc
                new_nodes[j], parent[j], token[j] = key, k, v
            else:
                self._scores[b, j] = ninf
                parent[j], token[j] = 0, blank
        self._node[b] = new_nodes

    def results(self, nbest=1, max_len=None):
        nbest = self._nbest(nbest)
        tokens, lengths, L = self._read(nbest, max_len)
        if self.native:
            with torch.cuda.device(self.device):
                scores = torch.empty((self.batch, nbest), dtype=torch.float32, device=self.device)
                _lib.check(_lib.lib().pika_msearch_results(
                    _ptr(self._state), self.batch, self.beam, self.max_frames, nbest, L, _ptr(tokens), _ptr(lengths),
                    _ptr(scores), _stream()), "pika_msearch_results")
            return tokens, lengths, scores
        return tokens, lengths, self._scores[:, :nbest].clone()

    def hyps(self, max_len=None):
        tokens, lengths, L = self._read(self.beam, max_len)
        if self.native:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().pika_msearch_hyps(
                    _ptr(self._state), self.batch, self.beam, self.max_frames, L, _ptr(tokens), _ptr(lengths),
                    _stream()), "pika_msearch_hyps")
        return tokens, lengths


class ModifiedLmBeamState(_BeamState):
    """`ModifiedBeamState` with an n-gram LM, a hotword list or both fused into the ranking (include/pika_msearch_lm.h).

    lm   a `CtcNgramLm` -- which includes a `CtcHotwords` phrase list alone (use lm_weight=1.0) -- or a `CtcBiasedLm`
         pair; anything else is a TypeError.  The object is what the CTC searches take: one upload serves both.
    A slot carries am, the log-sum of the paths kept, and bonus = lm_weight * LM(l) + bias_weight * BIAS(l) +
    length_bonus * |l| of its token sequence l; the beam is ranked by the fused score F = am + bonus.  Per step the
    `candidates` best of F[k] + log_softmax(...)[v] are taken first (None: min(2 * beam, 64); beam <= candidates <= 64:
    `candidates=beam` is icefall's rule, more lets the LM rescue what the acoustic cut would drop), each label walks
    the automata -- a token an automaton does not reach is dropped whatever the weights -- equal sequences merge their
    am, and the `beam` best by fused score stay.  With zero weights, candidates=beam and automata that reach every
    class it is `ModifiedBeamState` bit for bit.

    advance(logits, num_frames, sm_scale=1.0, blank_penalty=0.0) -> (parent, token)   as `ModifiedBeamState.advance`
    results(nbest=1, max_len=None, use_final=True) -> (tokens, lengths, scores, am_scores): use_final adds lm_weight *
        final(state) + bias_weight * final2(state2), drops the entries without a final state and sorts again (a
        `CtcHotwords` refunds the match in progress there); the state is only read.
    hyps(max_len=None), reset(which=None)   as `ModifiedBeamState`'s
    frames, scores (F), am_scores, overflowed   live views of the state.

    HIP float32 only: there is no CPU path (RuntimeError), as for `CtcNgramLm`.  Every call is a kernel launch with no
    host synchronisation, capturable in a `torch.cuda.graph`."""

    def __init__(self, batch, max_frames, lm, beam=4, blank=0, lm_weight=0.5, length_bonus=0.0, candidates=None,
                 device=None):
        self._setup(batch, max_frames, lm, beam, blank, lm_weight, length_bonus, candidates, device, True, ())
        self.reset()

    def _setup(self, batch, max_frames, lm, beam, blank, lm_weight, length_bonus, candidates, device, need_lm, more):
        """The checks and the blob; need_lm: `lm` may not be None; more: further (name, weight) pairs to be finite."""
        from ..ctc import _Search, _hip_device
        batch, max_frames, beam, blank = int(batch), int(max_frames), int(beam), int(blank)
        if not 1 <= beam <= MAX_BEAM:
            raise ValueError("need 1 <= beam <= %d, got beam=%d" % (MAX_BEAM, beam))
        if batch < 1 or max_frames < 1 or blank < 0:
            raise ValueError("need batch >= 1, max_frames >= 1 and blank >= 0, got %d, %d, %d" % (batch, max_frames, blank))
        candidates = min(2 * beam, MAX_BEAM) if candidates is None else int(candidates)
        if not beam <= candidates <= MAX_BEAM:
            raise ValueError("need beam <= candidates <= %d, got beam=%d, candidates=%d" % (MAX_BEAM, beam, candidates))
        v = _Search(lm, lm_weight, length_bonus, need_lm)           # (TypeError unless an LM or a pair)
        for name, w in (("lm_weight", v.lm_weight), ("bias_weight", v.bias_weight),
                        ("length_bonus", v.length_bonus)) + tuple(more):
            if w != w or w in (float("inf"), -float("inf")):
                raise ValueError("%s must be finite" % name)
        if device is None and v.lm is not None:
            device = v.lm.device
        self.device = _hip_device(device, "cuda", type(self).__name__)
        v.check_against(0, self.device, "the state")                # (no class yet: the devices alone)
        self.batch, self.max_frames, self.beam, self.blank, self.candidates = batch, max_frames, beam, blank, candidates
        self.dtype, self.native, self._v = torch.float32, True, v
        self._dims = (batch, beam, candidates, max_frames)
        nbytes = _lib.lib().pika_msearch_lm_state_bytes(*self._dims)
        if nbytes == 0:
            raise ValueError("(batch,max_frames,beam,candidates) = (%d,%d,%d,%d) not supported"
                             % (batch, max_frames, beam, candidates))
        with torch.cuda.device(self.device):
            self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        BK = batch * beam           # the layout of include/pika_msearch_lm.h
        self._scores = self._state[8 * BK:12 * BK].view(torch.float32).view(batch, beam)
        self._am = self._state[12 * BK:16 * BK].view(torch.float32).view(batch, beam)
        self._frames = self._state[32 * BK:32 * BK + 4 * batch].view(torch.int32)
        self._over = self._state[32 * BK + 4 * batch:32 * BK + 8 * batch].view(torch.int32)
        self._bonus = self._state[:8 * BK].view(torch.float64).view(batch, beam)

    @property
    def am_scores(self):
        return self._am

    def _fsts(self, start):
        """The automata as the C ABI takes them; "none" for those there are not."""
        none = (None,) * 5 + (0, 0) + ((0,) if start else ()) + (0, 0)
        return self._v.fsts(start) + none * (2 - len(self._v.automata))

    def _weights(self):
        return (self._v.lm_weight, self._v.bias_weight if self._v.bias is not None else 0.0)

    def reset(self, which=None):
        which = self._which(which)
        starts = self._v.starts() + (0, 0) * (2 - len(self._v.automata))
        name = self._abi + "reset"
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib(), name)(*((_ptr(self._state),) + self._dims + starts
                                                   + (_ptr(which), _stream()))), name)

    _abi = "pika_msearch_lm_"          # the entry points of reset, advance and results

    def advance(self, logits, num_frames, sm_scale=1.0, blank_penalty=0.0):
        return self._advance(logits, num_frames, sm_scale, blank_penalty, ())

    def _advance(self, logits, num_frames, sm_scale, blank_penalty, dense):
        """dense: what the step takes between length_bonus and the outputs (the rows of a neural LM, or nothing)."""
        sm_scale, blank_penalty = self._finite(sm_scale, blank_penalty)
        logits, num_frames = self._check_logits(logits, num_frames)
        B, K, V = self.batch, self.beam, logits.shape[1]
        self._v.check_against(V, self.device, "the state")
        name = self._abi + "advance"
        with torch.cuda.device(self.device):
            parent = torch.empty((B, K), dtype=torch.int64, device=self.device)
            token = torch.empty((B, K), dtype=torch.int64, device=self.device)
            _lib.check(getattr(_lib.lib(), name)(*(
                (_ptr(self._state), _ptr(logits), logits.stride(0), _ptr(num_frames)) + self._dims
                + (V, self.blank, sm_scale, blank_penalty) + self._fsts(False) + self._weights()
                + (self._v.length_bonus,) + dense + (_ptr(parent), _ptr(token), _stream()))), name)
        return parent, token

    def results(self, nbest=1, max_len=None, use_final=True):
        nbest = self._nbest(nbest)
        tokens, lengths, L = self._read(nbest, max_len)
        with torch.cuda.device(self.device):
            scores = torch.empty((self.batch, nbest), dtype=torch.float32, device=self.device)
            am_scores = torch.empty((self.batch, nbest), dtype=torch.float32, device=self.device)
            _lib.check(getattr(_lib.lib(), self._abi + "results")(*(
                (_ptr(self._state),) + self._dims + self._fsts(True) + self._weights()
                + (1 if use_final else 0, nbest, L, _ptr(tokens), _ptr(lengths), _ptr(scores), _ptr(am_scores),
                   _stream()))), self._abi + "results")
        return tokens, lengths, scores, am_scores

    def hyps(self, max_len=None):
        tokens, lengths, L = self._read(self.beam, max_len)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().pika_msearch_lm_hyps(*((_ptr(self._state),) + self._dims
                                                         + (L, _ptr(tokens), _ptr(lengths), _stream()))),
                       "pika_msearch_lm_hyps")
        return tokens, lengths


class ModifiedNnLmBeamState(ModifiedLmBeamState):
    """`ModifiedLmBeamState` with a NEURAL LM fused into the ranking (include/pika_msearch_nn.h): per step the caller
    hands `advance` a dense row of LM logits for every slot, as it hands it the joint network's; the LM's own state lives
    with the caller, as the prediction network's does.

    nn_weight, nn_scale, nn_label_offset   a pre-selected label v of slot k adds nn_weight * log_softmax(nn_scale *
         lm_logits[k])[v + nn_label_offset] to the slot's bonus; a label whose class falls outside the LM's vocabulary or
         whose term is not finite (a -inf or NaN logit, a row of -inf) is dropped whatever the weights are, as a label an
         automaton does not reach.  Blank is untouched.  The LM does not enter the pre-selection (`candidates`).
    lm   optional: what `ModifiedLmBeamState` takes, fused beside the neural LM with `lm_weight`.  A low-order n-gram
         with a NEGATIVE weight -- `lm=CtcBiasedLm(ngram, low_order, bias_weight=-0.2)`, or the low-order LM alone with
         lm_weight < 0 -- is LODR (icefall's modified_beam_search_LODR).
    Equal token sequences merge and the group takes its best-ranked member's bonus: give equal rows to equal sequences
    (an LM that is a function of the tokens does).  With nn_weight = 0 the step is `ModifiedLmBeamState`'s bit for bit.

    advance(logits, lm_logits, num_frames, sm_scale=1.0, blank_penalty=0.0) -> (parent, token)   lm_logits
        (batch * beam, V_lm) float32, row b * beam + k for slot k as it stands BEFORE the step; any row stride >= V_lm.
    results(nbest=1, max_len=None, use_final=True) -> (tokens, lengths, scores, am_scores)   use_final adds the final
        terms of the automata there are; the neural LM has none.
    hyps(max_len=None), reset(which=None)   as `ModifiedLmBeamState`'s
    frames, scores (F), am_scores, bonus (float64: scores = float32(am_scores + bonus)), overflowed   live views.

    HIP float32 only: there is no CPU path (RuntimeError).  Every call is a kernel launch with no host synchronisation,
    capturable in a `torch.cuda.graph`; `ModifiedBeamTimes` takes the state as it takes a `ModifiedLmBeamState`."""

    _abi = "pika_msearch_nn_"

    def __init__(self, batch, max_frames, beam=4, blank=0, nn_weight=0.3, nn_scale=1.0, nn_label_offset=0, lm=None,
                 lm_weight=0.5, length_bonus=0.0, candidates=None, device=None):
        self.nn_weight, self.nn_scale, self.nn_label_offset = float(nn_weight), float(nn_scale), int(nn_label_offset)
        self._setup(batch, max_frames, lm, beam, blank, lm_weight, length_bonus, candidates, device, False,
                    (("nn_weight", self.nn_weight), ("nn_scale", self.nn_scale)))
        self.reset()

    @property
    def bonus(self):
        return self._bonus

    def advance(self, logits, lm_logits, num_frames, sm_scale=1.0, blank_penalty=0.0):
        if not isinstance(lm_logits, torch.Tensor):
            raise TypeError("lm_logits must be a tensor")
        if lm_logits.dtype != torch.float32:
            raise TypeError("lm_logits must be float32, got %s" % lm_logits.dtype)
        if lm_logits.device != self.device:
            raise ValueError("the state lives on %s, lm_logits on %s" % (self.device, lm_logits.device))
        if lm_logits.dim() != 2 or lm_logits.shape[0] != self.batch * self.beam or lm_logits.shape[1] < 1:
            raise ValueError("lm_logits must be (batch * beam, V_lm) = (%d, V_lm), got %s" % (self.batch * self.beam,
                                                                                          tuple(lm_logits.shape)))
        if lm_logits.stride(1) != 1 or lm_logits.stride(0) < lm_logits.shape[1]:
            raise ValueError("lm_logits rows must be contiguous (class stride 1, row stride >= V_lm), got strides %s"
                             % (tuple(lm_logits.stride()),))
        return self._advance(logits, num_frames, sm_scale, blank_penalty,
                             (_ptr(lm_logits), lm_logits.stride(0), lm_logits.shape[1], self.nn_label_offset,
                              self.nn_scale, self.nn_weight))


class ModifiedBeamStream(object):
    """A one-symbol-per-frame beam search that outlives its buffer (include/pika_msearch_stream.h; DESIGN.md section 3,
    "Streaming modified beam search"): a `ModifiedBeamState` (lm is None) or a `ModifiedLmBeamState` (`lm`, `lm_weight`,
    `length_bonus`, `candidates` are its arguments), exposed as `.state`, with a side record per stream -- the frames the
    commits gave back and the fp64 offsets of the scores -- and `commit`.

    advance(logits, num_frames, sm_scale=1.0, blank_penalty=0.0) -> (parent, token)   the state's step; num_frames
        (batch,) is the ABSOLUTE number of frames offered to each stream so far (the stream passes num_frames - retired on,
        a device subtraction), and the rows of stream b are those of its frame consumed[b].
    commit(which=None, max_tail=None, rebase=False, max_len=None) -> (tokens (batch, L) int64, -1 beyond the length;
        lengths (batch,) int64; slot_map (batch, beam) int64).  The labels that every live hypothesis of a stream shares can
        never change again: they are returned, the trie is re-rooted below them and rebuilt with what the slots still
        need, and `frames` drops to what that takes, so `room` grows.  max_tail=m forces it: when the best hypothesis
        would keep more than m labels, everything but its last m is committed and the hypotheses that disagree are
        dropped; slot_map[b, j] is the old slot of new slot j (the identity otherwise): re-order a prediction network's
        state by it as by advance's `parent`.  rebase=True moves the best slot's score (LM: its am and its bonus) into
        `offset` (`bonus_offset`), float64: absolute scores are scores + offset (LM: am_scores + offset and
        scores + offset + bonus_offset).  Without rebase a stream equals the one-shot search bit for bit; a rebase changes
        the rounding of what follows.  Unselected streams (`which`) get length 0 and are not touched.
        L = max_len or max_frames.
    results(...), hyps(max_len=None)   the state's own: the UNCOMMITTED tails, scores relative to the offsets.
    reset(which=None)   the state and the side record.
    frames (held capacity), retired, consumed = frames + retired, room = max_frames - frames, offset, bonus_offset
        (float64, zero until a rebase), scores, overflowed   live views or device expressions, no host read.

    On a HIP device every call is a kernel launch with no host synchronisation, capturable in a `torch.cuda.graph`.  On
    the CPU or with dtype=torch.float64 (plain search only) `commit` runs in Python on the state's dict tries, by the
    same definition, in the state's dtype."""

    def __init__(self, batch, max_frames, beam=4, blank=0, lm=None, lm_weight=0.5, length_bonus=0.0, candidates=None,
                 device=None, dtype=None):
        if lm is None:
            if candidates is not None or lm_weight != 0.5 or length_bonus != 0.0:
                raise ValueError("candidates, lm_weight and length_bonus belong to the search with an LM (lm is None)")
            self.state = ModifiedBeamState(batch, max_frames, beam, blank, device, dtype)
        else:
            if dtype not in (None, torch.float32):
                raise TypeError("the search with an LM is float32 only, got dtype=%s" % dtype)
            self.state = ModifiedLmBeamState(batch, max_frames, lm, beam, blank, lm_weight, length_bonus, candidates,
                                             device)
        s = self.state
        self.batch, self.max_frames, self.beam, self.blank = s.batch, s.max_frames, s.beam, s.blank
        self.device, self.dtype, self.native, self.lm = s.device, s.dtype, s.native, lm is not None
        B = self.batch
        if self.native:
            lib = _lib.lib()
            self._dims = s._dims if self.lm else (B, self.beam, self.max_frames)
            o1 = (4 * B + 15) & ~15                   # the layout of include/pika_msearch_stream.h
            o2 = o1 + ((8 * B + 15) & ~15)
            with torch.cuda.device(self.device):
                self._side = torch.empty(lib.pika_msearch_stream_side_bytes(B), dtype=torch.uint8, device=self.device)
                self._scratch = torch.empty(lib.pika_msearch_commit_scratch_bytes(B, self.beam, self.max_frames),
                                            dtype=torch.uint8, device=self.device)
            self._retired = self._side[:4 * B].view(torch.int32)
            self._offset = self._side[o1:o1 + 8 * B].view(torch.float64)
            self._boff = self._side[o2:o2 + 8 * B].view(torch.float64)
        else:
            self._retired = torch.empty(B, dtype=torch.int32, device=self.device)
            self._offset = torch.empty(B, dtype=torch.float64, device=self.device)
            self._boff = torch.empty(B, dtype=torch.float64, device=self.device)
        self._reset_side(None)

    frames = property(lambda self: self.state.frames)
    retired = property(lambda self: self._retired)
    consumed = property(lambda self: self.state.frames + self._retired)
    room = property(lambda self: self.max_frames - self.state.frames)
    offset = property(lambda self: self._offset)
    bonus_offset = property(lambda self: self._boff)
    scores = property(lambda self: self.state.scores)
    overflowed = property(lambda self: self.state.overflowed)

    def _reset_side(self, which):
        if self.native:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().pika_msearch_stream_reset(_ptr(self._side), self.batch, _ptr(which), _stream()),
                           "pika_msearch_stream_reset")
            return
        sel = slice(None) if which is None else which.bool()
        self._retired[sel] = 0
        self._offset[sel] = 0.0
        self._boff[sel] = 0.0

    def reset(self, which=None):
        which = self.state._which(which)
        self.state.reset(which)
        self._reset_side(which)

    def advance(self, logits, num_frames, sm_scale=1.0, blank_penalty=0.0):
        num_frames = torch.as_tensor(num_frames)
        if num_frames.dtype not in (torch.int32, torch.int64) or num_frames.numel() != self.batch:
            raise ValueError("num_frames must be (batch,) int32 or int64")
        held = num_frames.reshape(-1).to(self.device, torch.int64) - self._retired.to(torch.int64)
        return self.state.advance(logits, held, sm_scale, blank_penalty)

    def results(self, *args, **kwargs):
        return self.state.results(*args, **kwargs)

    def hyps(self, max_len=None):
        return self.state.hyps(max_len)

    def commit(self, which=None, max_tail=None, rebase=False, max_len=None):
        which = self.state._which(which)
        max_tail = -1 if max_tail is None else int(max_tail)
        if max_tail < 0 and max_tail != -1:
            raise ValueError("max_tail must be None or >= 0, got %d" % max_tail)
        L = self.max_frames if max_len is None else int(max_len)
        if L < 1:
            raise ValueError("max_len must be >= 1, got %d" % L)
        B, K = self.batch, self.beam
        if not self.native:
            return self._commit_cpu(which, max_tail, bool(rebase), L)
        with torch.cuda.device(self.device):
            tokens = torch.empty((B, L), dtype=torch.int64, device=self.device)
            lengths = torch.empty(B, dtype=torch.int64, device=self.device)
            slot_map = torch.empty((B, K), dtype=torch.int64, device=self.device)
            fn, name = ((_lib.lib().pika_msearch_lm_commit, "pika_msearch_lm_commit") if self.lm else
                        (_lib.lib().pika_msearch_commit, "pika_msearch_commit"))
            _lib.check(fn(*((_ptr(self.state._state), _ptr(self._side)) + self._dims
                            + (_ptr(which), max_tail, 1 if rebase else 0, L, _ptr(tokens), _ptr(lengths), _ptr(slot_map),
                               _ptr(self._scratch), _stream()))), name)
        return tokens, lengths, slot_map

    def _commit_cpu(self, which, max_tail, rebase, L):
        """The commit's definition on the dict tries of `ModifiedBeamState`."""
        s, B, K, ninf = self.state, self.batch, self.beam, -float("inf")
        tokens = torch.full((B, L), -1, dtype=torch.int64)
        lengths = torch.zeros(B, dtype=torch.int64)
        slot_map = torch.arange(K, dtype=torch.int64).repeat(B, 1)
        sel = range(B) if which is None else [b for b, w in enumerate(which.tolist()) if w]
        for b in sel:
            nodes = s._tries[b][1]
            n = 0                                               # the live slots: the front slots with a score
            while n < K and s._scores[b, n] > ninf:
                n += 1
            seqs = []
            for j in range(n):
                seq, node = [], s._node[b][j]
                while node != 0:
                    node, tok = nodes[node]
                    seq.append(tok)
                seqs.append(seq[::-1])
            d = min(len(q) for q in seqs) if n else 0           # the depth of the common ancestor
            while d > 0 and any(q[:d] != seqs[0][:d] for q in seqs):
                d -= 1
            if max_tail >= 0 and n and len(seqs[0]) - d > max_tail:
                d = len(seqs[0]) - max_tail
            keep = [j for j in range(n) if seqs[j][:d] == seqs[0][:d] and len(seqs[j]) >= d]
            if n:
                lengths[b] = d
                tokens[b, :min(d, L)] = torch.tensor(seqs[0][:min(d, L)], dtype=torch.int64)
            index, new_nodes = {}, [(-1, -1)]                   # the trie again, parents first
            old = s._scores[b].clone()
            for jn, j in enumerate(keep):
                node = 0
                for tok in seqs[j][d:]:
                    nxt = index.get((node, tok))
                    if nxt is None:
                        nxt = index[(node, tok)] = len(new_nodes)
                        new_nodes.append((node, tok))
                    node = nxt
                s._node[b][jn] = node
                s._scores[b, jn] = old[j]
                slot_map[b, jn] = j
            for jn in range(len(keep), n):                      # vacated: as a reset leaves an empty slot
                s._node[b][jn] = 0
                s._scores[b, jn] = ninf
                slot_map[b, jn] = jn
            s._tries[b] = (index, new_nodes)
            frames = int(s._frames[b])
            tail = max([len(seqs[j]) - d for j in keep] + [0])
            fnew = min(frames, max((len(new_nodes) - 1 + K - 1) // K, tail))
            s._frames[b] = fnew
            self._retired[b] += frames - fnew
            if rebase and keep:
                c = s._scores[b, 0].clone()
                live = s._scores[b] > ninf
                s._scores[b] = torch.where(live, s._scores[b] - c, s._scores[b])
                self._offset[b] += c.double()
        return tokens.to(self.device), lengths.to(self.device), slot_map.to(self.device)


class ModifiedBeamTimes(object):
    """The token time stamps of a one-symbol-per-frame beam search (include/pika_msearch_times.h; DESIGN.md section 3,
    "Time stamps of the modified beam search"): a record kept NEXT TO `search` -- a `ModifiedBeamState`, a
    `ModifiedLmBeamState` or a `ModifiedBeamStream`, whose batch, beam, max_frames, blank and device it takes -- that
    holds, for every slot and every label of the slot's current token sequence, the ABSOLUTE index of the frame at which
    the slot's lineage emitted the label.  A slot's lineage is its representative's: the best-ranked member of every
    merged group, whose old slot and token `advance` returns as (parent, token).  Integers only: exact, bit for bit.

    step(parent, token)   after EVERY `advance` of the search, with what it returned.  An utterance that the advance left
        alone is left alone; an utterance whose `consumed` moved by anything but one frame since the last step -- a step
        was skipped, or the search was reset without the record -- is LOST: `lost[b]` is set and its read-outs give -1
        until `reset` selects it.
    hyps(max_len=None) -> (batch, beam, L) int64: the times of the current slots, in the order of the search's `hyps`;
        -1 beyond the length and for empty slots.
    results(tokens, lengths) -> (batch, N, L) int64: the times of the entries that any `results(...)` call of the search
        returned, each found by its tokens among the live slots (`ModifiedLmBeamState.results(use_final=True)` re-ranks
        and drops slots); -1 for a missing entry, for an entry longer than L and for one no live slot spells.
    commit(lengths, slot_map, which=None, max_len=None) -> (batch, L) int64: right after `ModifiedBeamStream.commit`,
        with that call's lengths, slot_map and `which`: the times of the committed labels, -1 beyond the length, and
        the record re-rooted as the search was.  The time of a committed label is the EARLIEST over the hypotheses that
        are live after the commit -- they share the labels, not necessarily their lineages --, which keeps a stream's
        committed times followed by any live tail's times strictly increasing under every schedule.
    reset(which=None)   with the search's reset.
    lost   live view, (batch,) bool.

    Tokens are bit for bit the one-shot search's under any commit schedule; times equal the one-shot search's without
    commits, under any chunking.  With commits the committed times are final by definition: the one-shot search's best
    hypothesis may carry another member's lineage for a label that a stream committed earlier.

    Where the search runs its HIP kernels so does the record (no host synchronisation, capturable in a
    `torch.cuda.graph`); where the search runs in plain torch (CPU, float64) the record runs in numpy by the same
    definition."""

    def __init__(self, search):
        if isinstance(search, ModifiedBeamStream):
            state = search.state
        elif isinstance(search, (ModifiedBeamState, ModifiedLmBeamState)):
            state = search
        else:
            raise TypeError("search must be a ModifiedBeamState, a ModifiedLmBeamState or a ModifiedBeamStream, got %s"
                            % type(search).__name__)
        self.search, self._st = search, state
        self._stream = search if state is not search else None
        self.batch, self.beam, self.max_frames, self.blank = state.batch, state.beam, state.max_frames, state.blank
        self.device, self.native = state.device, state.native
        B, K, mf = self.batch, self.beam, self.max_frames
        if self.native:
            self._C = state.candidates if isinstance(state, ModifiedLmBeamState) else 0
            nbytes = _lib.lib().pika_msearch_times_bytes(B, K, mf)
            if nbytes == 0:
                raise ValueError("(batch,max_frames,beam) = (%d,%d,%d) not supported" % (B, mf, K))
            with torch.cuda.device(self.device):
                self._rec = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._seen = self._rec[:4 * B].view(torch.int32)        # the layout of include/pika_msearch_times.h
            self._lost = self._rec[4 * B:8 * B].view(torch.int32)
            self._dims = (B, K, self._C, mf)
        else:
            import numpy as np
            self._seen = np.zeros(B, np.int64)
            self._lost = torch.zeros(B, dtype=torch.int32)
            self._rows = [[[] for _ in range(K)] for _ in range(B)]
        self.reset()

    @property
    def lost(self):
        return self._lost != 0

    def _side(self):
        return _ptr(self._stream._side) if self._stream is not None else None

    def _length(self, max_len):
        L = self.max_frames if max_len is None else int(max_len)
        if L < 1:
            raise ValueError("max_len must be >= 1, got %d" % L)
        return L

    def _pairs(self, a, b, shape, names):
        out = []
        for t, name in zip((a, b), names):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
                raise TypeError("%s must be an int64 tensor" % name)
            if t.device != self.device:
                raise ValueError("the record lives on %s, %s on %s" % (self.device, name, t.device))
            out.append(t.contiguous())
        if tuple(out[1].shape) != shape:
            raise ValueError("%s must be %s, got %s" % (names[1], shape, tuple(out[1].shape)))
        return out

    # ---- the plain spelling of the definition (CPU, float64) --------------------------------------------------------
    def _consumed(self):
        at = self._st.frames.cpu().long()
        if self._stream is not None:
            at = at + self._stream.retired.cpu().long()
        return at.tolist()

    def _lens(self, b):
        """len of every slot of utterance b: the depth of its node in the state's dict trie."""
        nodes, out = self._st._tries[b][1], []
        for node in self._st._node[b]:
            n = 0
            while node != 0:
                node, n = nodes[node][0], n + 1
            out.append(n)
        return out

    def _live(self, b):
        return [bool(s > -float("inf")) for s in self._st.scores[b].cpu()]

    def reset(self, which=None):
        which = self._st._which(which)
        if self.native:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().pika_msearch_times_reset(_ptr(self._rec), self.batch, self.beam, self.max_frames,
                                                               _ptr(which), _stream()), "pika_msearch_times_reset")
            return
        for b in (range(self.batch) if which is None else [b for b, w in enumerate(which.tolist()) if w]):
            self._seen[b], self._lost[b] = 0, 0
            self._rows[b] = [[] for _ in range(self.beam)]

    def step(self, parent, token):
        B, K = self.batch, self.beam
        parent, token = self._pairs(parent, token, (B, K), ("parent", "token"))
        if tuple(parent.shape) != (B, K):
            raise ValueError("parent must be (%d, %d), got %s" % (B, K, tuple(parent.shape)))
        if self.native:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().pika_msearch_times_step(*(
                    (_ptr(self._rec), _ptr(self._st._state), self._side()) + self._dims
                    + (_ptr(parent), _ptr(token), self.blank, _stream()))), "pika_msearch_times_step")
            return
        parent, token = parent.cpu().tolist(), token.cpu().tolist()
        for b, now in enumerate(self._consumed()):
            if self._lost[b] or now == self._seen[b]:
                continue
            if now != self._seen[b] + 1:
                self._lost[b] = 1
                continue
            old, lens, new = self._rows[b], self._lens(b), []
            for j in range(K):
                label = token[b][j] != self.blank
                n = max(lens[j] - 1, 0) if label else lens[j]
                row = list(old[min(max(parent[b][j], 0), K - 1)][:n])
                if label and lens[j] > 0:
                    row.append(now - 1)
                new.append(row)
            self._rows[b], self._seen[b] = new, now

    def hyps(self, max_len=None):
        L = self._length(max_len)
        B, K = self.batch, self.beam
        if self.native:
            with torch.cuda.device(self.device):
                out = torch.empty((B, K, L), dtype=torch.int64, device=self.device)
                _lib.check(_lib.lib().pika_msearch_times_hyps(*(
                    (_ptr(self._rec), _ptr(self._st._state)) + self._dims + (L, _ptr(out), _stream()))),
                    "pika_msearch_times_hyps")
            return out
        out = torch.full((B, K, L), -1, dtype=torch.int64)
        for b in range(B):
            if not self._lost[b]:
                for k, (live, n) in enumerate(zip(self._live(b), self._lens(b))):
                    if live:
                        row = self._rows[b][k][:min(n, L)]
                        out[b, k, :len(row)] = torch.tensor(row, dtype=torch.int64)
        return out.to(self.device)

    def results(self, tokens, lengths):
        if not isinstance(tokens, torch.Tensor) or tokens.dim() != 3 or tokens.shape[0] != self.batch \
                or not 1 <= tokens.shape[1] <= self.beam or tokens.shape[2] < 1:
            raise ValueError("tokens must be (batch, N, L) with 1 <= N <= beam, as a results call returned them")
        B, N, L = tokens.shape
        tokens, lengths = self._pairs(tokens, lengths, (B, N), ("tokens", "lengths"))
        if self.native:
            with torch.cuda.device(self.device):
                out = torch.empty((B, N, L), dtype=torch.int64, device=self.device)
                _lib.check(_lib.lib().pika_msearch_times_results(*(
                    (_ptr(self._rec), _ptr(self._st._state)) + self._dims
                    + (N, L, _ptr(tokens), _ptr(lengths), _ptr(out), _stream()))), "pika_msearch_times_results")
            return out
        out = torch.full((B, N, L), -1, dtype=torch.int64)
        hyp, ln = (t.cpu() for t in self._st.hyps())
        tokens, lengths = tokens.cpu(), lengths.cpu().tolist()
        for b in range(B):
            for e in range(N):
                n = lengths[b][e]
                if self._lost[b] or not 0 <= n <= min(L, self.max_frames):
                    continue
                for k in range(self.beam):
                    if int(ln[b, k]) == n and torch.equal(hyp[b, k, :n], tokens[b, e, :n]):
                        out[b, e, :n] = torch.tensor(self._rows[b][k][:n], dtype=torch.int64)
                        break
        return out.to(self.device)

    def commit(self, lengths, slot_map, which=None, max_len=None):
        L = self._length(max_len)
        B, K = self.batch, self.beam
        which = self._st._which(which)
        lengths, slot_map = self._pairs(lengths, slot_map, (B, K), ("lengths", "slot_map"))
        if tuple(lengths.shape) != (B,):
            raise ValueError("lengths must be (%d,), got %s" % (B, tuple(lengths.shape)))
        if self.native:
            with torch.cuda.device(self.device):
                out = torch.empty((B, L), dtype=torch.int64, device=self.device)
                _lib.check(_lib.lib().pika_msearch_times_commit(*(
                    (_ptr(self._rec), _ptr(self._st._state)) + self._dims
                    + (_ptr(which), _ptr(lengths), _ptr(slot_map), L, _ptr(out), _stream()))),
                    "pika_msearch_times_commit")
            return out
        out = torch.full((B, L), -1, dtype=torch.int64)
        lengths, slot_map = lengths.cpu().tolist(), slot_map.cpu().tolist()
        for b in (range(B) if which is None else [b for b, w in enumerate(which.tolist()) if w]):
            if self._lost[b]:
                continue
            d, old, live = min(max(lengths[b], 0), self.max_frames), self._rows[b], self._live(b)
            n = live.index(False) if False in live else K          # the live slots: the front slots with a score
            src = [min(max(s, 0), K - 1) for s in slot_map[b]]
            for i in range(min(d, L)):
                out[b, i] = min(old[src[j]][i] for j in range(n)) if n else -1
            self._rows[b] = [list(old[src[j]][d:d + m]) for j, m in enumerate(self._lens(b))]
        return out.to(self.device)


class ModifiedStreamDecoder(object):
    """`modified_beam_search` chunk by chunk, for audio without an end: a transducer model (`pika_amd.model.transducer.
    Net`) with the LSTM prediction network (`decoder_type == 'rnn'`) or the stateless one (`'stateless'`: a
    `StatelessContext` stands where `(h, c)` does below, followed by one kernel per step, re-ordered by a commit's slot_map
    and reset with the streams; the conv-transformer raises NotImplementedError -- its cache is its own item) around a
    `ModifiedBeamStream` (`.stream`) of `batch` streams.  `lm`,
    `lm_weight`, `length_bonus`, `candidates` are the stream's.

    advance(enc_chunk (batch, Tc, H), lengths=None)   Tc frame steps on a chunk of ENCODER output; lengths (batch,): the
        chunk's frames that count for each stream (None: Tc).  The joint's encoder halves are computed once per chunk;
        per step the rows are gathered by consumed - chunk start, `(h, c)` is re-ordered by `parent` and stepped where
        token != blank.  Between two commits a stream takes at most `room` frames (`stream.overflowed` otherwise).
    commit(which=None, max_tail=None, rebase=False) -> (tokens, lengths, slot_map)   the stream's commit; `(h, c)` is
        re-ordered by slot_map and the new labels join the streams' committed text (one host read).
    results(nbest=1, max_len=None, **kw) -> (committed tokens (batch, Lc) int64, -1 beyond the length; committed lengths
        (batch,); tail tokens (batch, nbest, L); tail lengths (batch, nbest); scores (batch, nbest), relative to the
        stream's offsets): a hypothesis is the committed text followed by its tail.
    reset(which=None)   the stream, `(h, c)` and the committed text of the selected streams.
    track_times()   before the first `advance`: keeps a `ModifiedBeamTimes` (`.times`) next to the stream.  The step loop
        then steps it, `commit` (same return value) appends the committed labels' times to the streams' text times, and
    results_timed(nbest=1, max_len=None, **kw) -> `results(...)`'s tuple + (committed times (batch, Lc) int64, -1 beyond
        the length; tail times (batch, nbest, L)): absolute encoder frames; committed followed by any tail is strictly
        increasing.  With tracking off nothing changes."""

    def __init__(self, model, batch, max_frames, beam=4, lm=None, lm_weight=0.5, length_bonus=0.0, candidates=None,
                 sm_scale=1.0, blank_penalty=0.0, blank=0, precision="fp16x2"):
        from .. import gemm as G
        if getattr(model, "decoder_type", None) not in ('rnn', 'stateless'):
            raise NotImplementedError("ModifiedStreamDecoder steps the LSTM prediction network (decoder_type == 'rnn') "
                                      "and the stateless one ('stateless') only; the conv-transformer cache is not "
                                      "wired in")
        if precision not in G.PRECISIONS:
            raise ValueError("unknown precision %r" % (precision,))
        p = next(model.parameters())
        self.model, self.precision = model, precision
        self.sm_scale, self.blank_penalty = _BeamState._finite(sm_scale, blank_penalty)
        self.stream = ModifiedBeamStream(batch, max_frames, beam, blank, lm, lm_weight, length_bonus, candidates,
                                         p.device, None if lm is not None else p.dtype)
        s = self.stream
        self.batch, self.beam, self.blank, self.device = s.batch, s.beam, s.blank, s.device
        w1, wg = model.fc1, model.fc_gate
        stateless = model.decoder_type == 'stateless'
        H = self.H = w1.weight.shape[1] - (model.decoder.dim if stateless else model.decoder.hidden_size)   # the encoder's
        #                                                                                         share of the joint's input
        self.J = w1.weight.shape[0]
        self._we = torch.cat((w1.weight[:, :H], wg.weight[:, :H]), dim=0).contiguous()    # enc -> [e1 | eg]
        self._be = torch.cat((w1.bias, wg.bias), dim=0).contiguous()
        self._wp = torch.cat((w1.weight[:, H:], wg.weight[:, H:]), dim=0).contiguous()    # pred -> [p1 | pg]
        self._flat0 = (torch.arange(self.batch, device=self.device) * self.beam).unsqueeze(1)
        self._offered = torch.zeros(self.batch, dtype=torch.int64, device=self.device)
        self._pred = None
        self._context = None            # the stateless network's (h, c): every slot's last tokens and the rows for them
        if stateless:
            from ..model.stateless import StatelessContext
            self._context = StatelessContext(model.decoder, self.batch, self.beam, self.blank)
        self._text = [[] for _ in range(self.batch)]
        self.times, self._ttext, self._started = None, None, False
        self.reset()

    def track_times(self):
        if self._started:
            raise RuntimeError("track_times() comes before the first advance")
        if self.times is None:
            self.times = ModifiedBeamTimes(self.stream)
            self._ttext = [[] for _ in range(self.batch)]
        return self.times

    def _precision(self):
        from .. import gemm as G
        old = G.PRECISION
        if self.device.type == "cuda":
            G.PRECISION = self.precision
        return G, old

    @torch.no_grad()
    def reset(self, which=None):
        which = self.stream.state._which(which)
        self.stream.reset(which)
        if self.times is not None:
            self.times.reset(which)
            for b, w in enumerate([1] * self.batch if which is None else which.tolist()):
                if w:
                    self._ttext[b] = []
        if self._context is not None:
            self._context.reset(which)
            fresh = []
        else:
            G, old = self._precision()
            try:
                sos = torch.full((self.batch * self.beam, 1), self.blank, dtype=torch.long, device=self.device)
                _, st = self.model.decoder(self.model.embed(sos))
            finally:
                G.PRECISION = old
            fresh = [st[0].contiguous(), st[1].contiguous()]
        if which is None or self._pred is None:
            self._pred = fresh
            self._offered.zero_()
            self._text = [[] for _ in range(self.batch)]
            self._started = False
            return
        rows = which.bool().repeat_interleave(self.beam).view(1, -1, 1)
        for cur, new in zip(self._pred, fresh):
            cur.copy_(torch.where(rows, new, cur))
        self._offered.masked_fill_(which.bool(), 0)
        for b, w in enumerate(which.tolist()):
            if w:
                self._text[b] = []

    @torch.no_grad()
    def advance(self, enc_chunk, lengths=None):
        from ..model import ops
        B, K, H, model = self.batch, self.beam, self.H, self.model
        if enc_chunk.dim() != 3 or enc_chunk.shape[0] != B or enc_chunk.shape[2] != H:
            raise ValueError("enc_chunk must be (batch, Tc, H) = (%d, Tc, %d), got %s" % (B, H, tuple(enc_chunk.shape)))
        Tc = enc_chunk.shape[1]
        if Tc == 0:
            return
        self._started = True
        if lengths is None:
            lengths = torch.full((B,), Tc, dtype=torch.int64, device=self.device)
        else:
            lengths = torch.as_tensor(lengths)
            if lengths.dtype not in (torch.int32, torch.int64) or lengths.numel() != B:
                raise ValueError("lengths must be (batch,) int32 or int64")
            lengths = lengths.reshape(-1).to(self.device, torch.int64).clamp(0, Tc)
        G, old = self._precision()
        try:
            start = self._offered.clone()
            self._offered += lengths
            J = self.J
            e_all = ops.linear(enc_chunk.contiguous(), self._we, self._be).reshape(B * Tc, 2 * J)   # row b*Tc + t
            brow = torch.arange(B, device=self.device) * Tc
            context = self._context
            if context is None:
                hh, cc = self._pred
            for _ in range(Tc):
                tg = (self.stream.consumed.long() - start).clamp(0, Tc - 1)
                rows = (brow + tg).unsqueeze(1).expand(B, K).reshape(-1)
                z = e_all.index_select(0, rows) + ops.linear(hh[-1] if context is None else context.rows, self._wp)
                h = torch.tanh(z[:, :J]) * torch.sigmoid(z[:, J:])
                logits = ops.linear(h, model.fc2.weight, model.fc2.bias).contiguous()
                parent, token = self.stream.advance(logits, self._offered, self.sm_scale, self.blank_penalty)
                if self.times is not None:
                    self.times.step(parent, token)
                if context is not None:
                    context.follow(parent, token)
                    continue
                flat = (self._flat0 + parent).reshape(-1)
                hh.copy_(hh.index_select(1, flat))
                cc.copy_(cc.index_select(1, flat))
                _, (h2, c2) = model.decoder(model.embed(token.reshape(-1, 1)), (hh, cc))
                m = token.reshape(-1).ne(self.blank).view(1, -1, 1)
                hh.copy_(torch.where(m, h2, hh))
                cc.copy_(torch.where(m, c2, cc))
        finally:
            G.PRECISION = old

    @torch.no_grad()
    def commit(self, which=None, max_tail=None, rebase=False):
        tokens, lengths, slot_map = self.stream.commit(which, max_tail, rebase)
        if self._context is not None:
            self._context.reorder(slot_map)
        flat = (self._flat0 + slot_map).reshape(-1)
        for s_ in self._pred:
            s_.copy_(s_.index_select(1, flat))
        for b, (row, n) in enumerate(zip(tokens.tolist(), lengths.tolist())):
            self._text[b] += row[:n]
        if self.times is not None:
            when = self.times.commit(lengths, slot_map, which)
            for b, (row, n) in enumerate(zip(when.tolist(), lengths.tolist())):
                self._ttext[b] += row[:n]
        return tokens, lengths, slot_map

    def results(self, nbest=1, max_len=None, **kwargs):
        out = self.stream.results(nbest, max_len, **kwargs)
        Lc = max([len(t) for t in self._text] + [1])
        committed = torch.tensor([t + [-1] * (Lc - len(t)) for t in self._text], dtype=torch.int64, device=self.device)
        clen = torch.tensor([len(t) for t in self._text], dtype=torch.int64, device=self.device)
        return committed, clen, out[0], out[1], out[2]

    def results_timed(self, nbest=1, max_len=None, **kwargs):
        if self.times is None:
            raise RuntimeError("results_timed() needs track_times() before the first advance")
        out = self.results(nbest, max_len, **kwargs)
        Lc = out[0].shape[1]
        when = torch.tensor([t + [-1] * (Lc - len(t)) for t in self._ttext], dtype=torch.int64, device=self.device)
        return out + (when, self.times.results(out[2], out[3]))


@torch.no_grad()
def modified_beam_search(model, x, x_len, beam=4, nbest=1, sm_scale=1.0, blank_penalty=0.0, use_graph=True, blank=0,
                         precision="fp16x2"):
    """Decode a batch with a transducer model (`pika_amd.model.transducer.Net`) under the modified topology: at most --
    exactly -- one symbol per frame.  -> (tokens (B, nbest, T) int64, lengths (B, nbest) int64, scores (B, nbest) f32,
    enc_out (B, T, H)) with the conventions of `ModifiedBeamState.results`.

    x (B, T_in, D) features; x_len (B,) the utterances' numbers of ENCODER frames (as `TransducerDecoder.decode_batch`
    takes them), host or device, clamped to [0, T].  The encoder runs once; the joint's encoder halves are computed
    once; per frame step the rows of the frame frames[b] are gathered, the prediction half is added, gate and fc2 give
    the (B * beam, V) logits, `ModifiedBeamState.advance` cuts and merges, the prediction-network state is re-ordered by
    `parent` and stepped on the rows whose token is a label (every row is computed and masked: fixed shapes).  The
    loop runs exactly min(max(x_len), T) steps and reads nothing back.  use_graph (HIP only): two steps run eagerly,
    the next is captured once and replayed for the rest.

    Prediction networks: the LSTM of the shipped recipes (`decoder_type == 'rnn'`) is stepped on its (h, c) state.  The
    stateless network (`'stateless'`, `pika_amd.model.stateless`) keeps a `StatelessContext`: one kernel per step turns
    (parent, token) into the next prediction rows; there is no state to re-order.  The
    conv-transformer prediction network is re-run every step on [blank] + hyps() padded to T + 1 positions: correct, not
    fast (the incremental cache of `TransducerDecoder` is not wired in).

    Scores are the summed log-probabilities of the paths the beam kept, NOT length-normalised, and the entries come in
    the beam's order by that score; normalising by length and picking the entry to return is the caller's:
    nbest=beam gives every entry's score and length.  Token time stamps: `modified_beam_search_timed` returns the frames
    at which this search emitted the labels.  precision: `pika_amd.gemm.PRECISION` for the products of the call on a HIP device ("fp32": exact)."""
    return _drive(model, x, x_len, beam, sm_scale, blank_penalty, use_graph, blank, precision,
                  lambda B, T, dev, dtype: ModifiedBeamState(B, T, int(beam), int(blank), dev, dtype),
                  lambda state: state.results(nbest=nbest))


@torch.no_grad()
def modified_beam_search_lm(model, x, x_len, lm, beam=4, nbest=1, sm_scale=1.0, blank_penalty=0.0, use_graph=True,
                            blank=0, precision="fp16x2", lm_weight=0.5, length_bonus=0.0, candidates=None,
                            use_final=True):
    """`modified_beam_search` with an n-gram LM, a hotword list or both fused into the ranking: `lm`, `lm_weight`,
    `length_bonus` and `candidates` are `ModifiedLmBeamState`'s, `use_final` its `results`'.  HIP only.
    -> (tokens, lengths, scores, am_scores, enc_out): scores are the fused scores the entries are ordered by, am_scores
    the summed log-probabilities of the paths kept alone (what `modified_beam_search` calls scores)."""
    return _drive(model, x, x_len, beam, sm_scale, blank_penalty, use_graph, blank, precision,
                  lambda B, T, dev, dtype: ModifiedLmBeamState(B, T, lm, int(beam), int(blank), lm_weight, length_bonus,
                                                               candidates, dev),
                  lambda state: state.results(nbest=nbest, use_final=use_final))


@torch.no_grad()
def modified_beam_search_timed(model, x, x_len, lm=None, beam=4, nbest=1, sm_scale=1.0, blank_penalty=0.0,
                               use_graph=True, blank=0, precision="fp16x2", lm_weight=0.5, length_bonus=0.0,
                               candidates=None, use_final=True):
    """`modified_beam_search` -- `modified_beam_search_lm` when `lm` is given, with its `lm_weight`, `length_bonus`,
    `candidates` and `use_final`; they must be left alone otherwise -- with token time stamps.
    -> (tokens, lengths, scores[, am_scores], times, enc_out): times (B, nbest, T) int64, times[b, j, i] the encoder
    frame at which this search emitted label i of entry j (the lineage of the hypothesis' representative, see
    `ModifiedBeamTimes`), -1 beyond the length and for a missing entry.  Tokens, lengths and scores are those of the
    untimed call bit for bit: the record's step sits behind the search's in the same captured graph and only reads."""
    if lm is None:
        if candidates is not None or lm_weight != 0.5 or length_bonus != 0.0 or use_final is not True:
            raise ValueError("lm_weight, length_bonus, candidates and use_final belong to the search with an LM")

        def make_state(B, T, dev, dtype):
            return ModifiedBeamState(B, T, int(beam), int(blank), dev, dtype)
        kw = {}
    else:
        def make_state(B, T, dev, dtype):
            return ModifiedLmBeamState(B, T, lm, int(beam), int(blank), lm_weight, length_bonus, candidates, dev)
        kw = {"use_final": use_final}
    rec = []

    def hook(state):
        rec.append(ModifiedBeamTimes(state))
        return rec[0].step

    def results(state):
        out = tuple(state.results(nbest=nbest, **kw))
        return out + (rec[0].results(out[0], out[1]),)
    return _drive(model, x, x_len, beam, sm_scale, blank_penalty, use_graph, blank, precision, make_state, results,
                  hook=hook)


@torch.no_grad()
def modified_beam_search_nnlm(model, x, x_len, nnlm, beam=4, nbest=1, sm_scale=1.0, blank_penalty=0.0, use_graph=True,
                              blank=0, precision="fp16x2", nn_weight=0.3, nn_scale=1.0, nn_label_offset=0, lm=None,
                              lm_weight=0.5, length_bonus=0.0, candidates=None, use_final=True):
    """`modified_beam_search` with a neural LM fused into the ranking (icefall's modified_beam_search_lm_shallow_fusion):
    `nnlm` is a `pika_amd.model.lm.LstmLm` or any object with its four methods (the protocol is in that module's
    docstring), on the model's device; `nn_weight`, `nn_scale`, `nn_label_offset`, `lm`, `lm_weight`, `length_bonus` and
    `candidates` are `ModifiedNnLmBeamState`'s, `use_final` its `results`'.  HIP only.
    -> (tokens, lengths, scores, am_scores, enc_out) as `modified_beam_search_lm`.

    Per frame step `nnlm.logits` is computed fresh on the LM's output for all B * beam rows, the step takes it beside the
    joint network's logits, the LM's state is re-ordered by `parent` with the prediction network's, and the LM is stepped
    on every row with token + nn_label_offset and kept where the token is a label: fixed shapes, nothing read back, two
    eager steps and one captured step replayed for the rest, as for the prediction network.

    LODR (icefall's modified_beam_search_LODR): give the low-order n-gram as `lm` with a negative weight -- alone with
    lm_weight < 0, or as the `bias` of a `CtcBiasedLm(ngram, low_order, bias_weight < 0)` beside a full n-gram."""
    def make_state(B, T, dev, dtype):
        return ModifiedNnLmBeamState(B, T, int(beam), int(blank), nn_weight, nn_scale, nn_label_offset, lm, lm_weight,
                                     length_bonus, candidates, dev)
    return _drive(model, x, x_len, beam, sm_scale, blank_penalty, use_graph, blank, precision, make_state,
                  lambda state: state.results(nbest=nbest, use_final=use_final),
                  side=lambda rows: _LmRows(nnlm, rows, int(nn_label_offset)))


class _LmRows(object):
    """A neural LM beside the loop of `_drive`: its output and state for the B * beam rows, in buffers that stay where
    they are (a captured step reads and writes the same memory at every replay)."""

    def __init__(self, nnlm, rows, offset):
        for name in ("start", "step", "logits", "select"):
            if not callable(getattr(nnlm, name, None)):
                raise TypeError("nnlm must have start, step, logits and select (pika_amd.model.lm), got %s"
                                % type(nnlm).__name__)
        self.nnlm, self.offset = nnlm, offset
        out, state = nnlm.start(rows)
        self.out, self.state = out.clone(), tuple(s.clone() for s in state)

    def rows(self):
        """What `advance` takes behind the joint's logits: the LM's logits for the slots as they stand."""
        self.last = self.nnlm.logits(self.out).float().contiguous()
        return (self.last,)

    def follow(self, flat, token, label):
        """flat (rows,): the old row of every new row; token (rows,); label (rows,) bool: the token is a label."""
        out = self.out.index_select(0, flat)
        state = self.nnlm.select(self.state, flat)
        ids = (token + self.offset).clamp(0, self.last.shape[1] - 1)      # (blank's class may lie outside: masked below)
        out2, state2 = self.nnlm.step(ids, state)
        self.out.copy_(torch.where(label.view(-1, 1), out2, out))
        for buf, new, old in zip(self.state, state2, state):
            buf.copy_(torch.where(label.view((1, -1) + (1,) * (buf.dim() - 2)), new, old))


def _drive(model, x, x_len, beam, sm_scale, blank_penalty, use_graph, blank, precision, make_state, results, side=None,
           reduce=None, hook=None):
    """The loop of `modified_beam_search` around a search state: make_state(B, T, device, dtype) -> the state,
    results(state) -> what the call returns ahead of enc_out, side(B * beam) -> a `_LmRows`: what `advance` takes behind
    the logits, re-ordered and stepped with the prediction network (None: nothing), hook(state) -> a callable that every
    step hands its (parent, token) right after the advance (None: there is none), reduce(enc_out, x_len) -> (frames, lengths):
    what the step loop runs on instead of the encoder's output and x_len, of the same (B, T, H) shape (None: those
    themselves; `pika_amd.frame_skip.modified_beam_search_skip`).  The call returns the encoder's own output either way."""
    from .. import gemm as G
    from ..model import ops
    K, blank = int(beam), int(blank)
    old = G.PRECISION
    if x.is_cuda:
        if precision not in G.PRECISIONS:
            raise ValueError("unknown precision %r" % (precision,))
        G.PRECISION = precision
    try:
        if model.pack_seq and x_len is not None:
            enc_out = model.encode(x, x_len)
        else:
            enc_out = model.encoder(x)
        frames = enc_out
        if reduce is not None:
            frames, x_len = reduce(enc_out, x_len)
        B, T, H = frames.shape
        dev = frames.device
        x_len = torch.as_tensor(x_len)
        steps = min(max(int(x_len.max()), 0), T)               # (the one host read, before the first launch)
        num_frames = x_len.to(dev).long().clamp(0, T)
        rnn = model.decoder_type == 'rnn'
        stateless = model.decoder_type == 'stateless'
        state = make_state(B, T, dev, enc_out.dtype)
        after = hook(state) if hook is not None else None
        beside = side(B * K) if side is not None else None

        w1, wg = model.fc1, model.fc_gate
        e1_all = ops.linear(frames, w1.weight[:, :H].contiguous(), w1.bias)
        eg_all = ops.linear(frames, wg.weight[:, :H].contiguous(), wg.bias)
        e_all = torch.cat((e1_all, eg_all), dim=2).reshape(B * T, 2 * H)          # row b*T + t = [e1 | eg]
        wp = torch.cat((w1.weight[:, H:], wg.weight[:, H:]), dim=0).contiguous()  # (2H, H)
        brow = torch.arange(B, device=dev) * T
        flat0 = (torch.arange(B, device=dev) * K).unsqueeze(1)

        sos = torch.full((B * K, 1), blank, dtype=torch.long, device=dev)
        if stateless:
            from ..model.stateless import StatelessContext
            context = StatelessContext(model.decoder, B, K, blank)
            pred = [context.rows]                   # the joint's prediction half: rewritten in place by every follow
        elif rnn:
            _, st = model.decoder(model.embed(sos))
            pred = [st[0].contiguous(), st[1].contiguous()]
        else:
            pred = [model.decoder(sos)[:, -1, :].contiguous()]
            pad = model.embed.padding_idx
            pos = torch.arange(1, T + 1, device=dev).unsqueeze(0)

        def step():
            tg = state.frames.long().clamp(max=T - 1)
            rows = (brow + tg).unsqueeze(1).expand(B, K).reshape(-1)
            dec_hid = pred[0][-1] if rnn else pred[0]
            z = e_all.index_select(0, rows) + ops.linear(dec_hid, wp)
            h = torch.tanh(z[:, :H]) * torch.sigmoid(z[:, H:])
            logits = ops.linear(h, model.fc2.weight, model.fc2.bias).contiguous()
            extra = beside.rows() if beside is not None else ()
            parent, token = state.advance(logits, *(extra + (num_frames, sm_scale, blank_penalty)))
            if after is not None:
                after(parent, token)
            flat = (flat0 + parent).reshape(-1)
            label = token.reshape(-1).ne(blank)
            if stateless:                           # one launch: no state to re-order, no hyps() walk
                context.follow(parent, token)
            else:
                for s_ in pred:
                    s_.copy_(s_.index_select(1 if rnn else 0, flat))
            if beside is not None:
                beside.follow(flat, token.reshape(-1), label)
            if rnn:
                hh, cc = pred
                _, (h2, c2) = model.decoder(model.embed(token.reshape(-1, 1)), (hh, cc))
                m = label.view(1, -1, 1)
                hh.copy_(torch.where(m, h2, hh))
                cc.copy_(torch.where(m, c2, cc))
            elif not stateless:
                hyp, ln = state.hyps(max_len=T)
                hyp, ln = hyp.view(B * K, T), ln.view(-1).clamp(min=0)
                body = torch.where(pos <= ln.unsqueeze(1), hyp, torch.full_like(hyp, pad))
                out = model.decoder(torch.cat((sos, body), dim=1))
                last = out.gather(1, ln.view(-1, 1, 1).expand(-1, 1, out.shape[2])).squeeze(1)
                pred[0].copy_(torch.where(label.unsqueeze(1), last, pred[0]))

        graph = None
        for i in range(steps):
            if use_graph and enc_out.is_cuda and i >= 2:
                if graph is None:
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        step()
                graph.replay()
            else:
                step()
        out = tuple(results(state))
    finally:
        G.PRECISION = old
    return out + (enc_out,)
