"""Neural language models for shallow fusion in the one-symbol-per-frame beam search (`pika_amd.
modified_beam_search_nnlm`, `ModifiedNnLmBeamState`; include/pika_msearch_nn.h).

The PROTOCOL the search's driver uses -- any object with these four methods is accepted; `rows` is batch * beam:

    start(rows) -> (out, state)        the LM after the start-of-sentence symbol alone, for `rows` hypotheses
    step(ids, state) -> (out, state)   one token per row, ids (rows,) int64 classes of the LM
    logits(out) -> (rows, V_lm)        the unnormalised scores of the next token (the search takes the log-softmax)
    select(state, index) -> state      the state of the rows index (rows,) int64, in that order

`out` is a tensor with the rows on dimension 0.  `state` is a tuple of tensors with the rows on dimension 1 (nn.LSTM's
(h, c) layout): the driver keeps a stepped row where the row's token is a label and the old row otherwise with a
`torch.where` over that dimension, in buffers it allocates once -- shapes and dtypes must not change from step to step,
and nothing may be read back on the host, so that a step can be captured in a `torch.cuda.graph`.  The LM must be a
function of the tokens alone (eval mode, no dropout): hypotheses that spell the same sequence merge and the group keeps
one member's LM score.  The search has no end-of-sentence term.

`LstmLm` is the plain one: embedding, `nn.LSTM`, output linear -- the shape of icefall's RnnLmModel.
"""
import torch
import torch.nn as nn


class LstmLm(nn.Module):
    """LstmLm(vocab, embed_dim, hidden, layers=1, sos=0): token ids in [0, vocab); `sos` starts every sentence.

    forward(tokens (N, L) int64) -> logits (N, L + 1, vocab): position i scores token i given sos and the tokens before
    it (position L: what would follow) -- for training and for scoring whole sentences.  start / step / logits / select
    are the protocol above."""

    def __init__(self, vocab, embed_dim, hidden, layers=1, sos=0):
        super().__init__()
        vocab, embed_dim, hidden, layers, sos = int(vocab), int(embed_dim), int(hidden), int(layers), int(sos)
        if vocab < 1 or embed_dim < 1 or hidden < 1 or layers < 1:
            raise ValueError("need vocab, embed_dim, hidden and layers >= 1, got %d, %d, %d, %d"
                             % (vocab, embed_dim, hidden, layers))
        if not 0 <= sos < vocab:
            raise ValueError("need 0 <= sos < vocab = %d, got sos=%d" % (vocab, sos))
        self.vocab, self.sos = vocab, sos
        self.embed = nn.Embedding(vocab, embed_dim)
        self.rnn = nn.LSTM(embed_dim, hidden, layers, batch_first=True)
        self.out = nn.Linear(hidden, vocab)

    def forward(self, tokens):
        sos = torch.full((tokens.shape[0], 1), self.sos, dtype=torch.long, device=tokens.device)
        o, _ = self.rnn(self.embed(torch.cat((sos, tokens), dim=1)))
        return self.out(o)

    def start(self, rows):
        ids = torch.full((int(rows),), self.sos, dtype=torch.long, device=self.embed.weight.device)
        return self.step(ids, None)

    def step(self, ids, state):
        o, (h, c) = self.rnn(self.embed(ids.view(-1, 1)), state)
        return o[:, 0], (h, c)

    def logits(self, out):
        return self.out(out)

    def select(self, state, index):
        return tuple(s.index_select(1, index) for s in state)
