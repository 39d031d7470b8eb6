"""Reference of the one-symbol-per-frame beam search with a neural LM fused in (include/pika_msearch_nn.h), built on
`msearch_lm_common` (ML): the dense term is a third source of the increment that ML's walk adds up, so a neural LM is
handed to `ML.step` / `ML.search` as one more entry of `lms`, LAST (the order of the sum: lm, bias, nn, length_bonus),
in the shape of an automaton whose state is the token sequence itself:

    DenseLm(row_of, scale, offset, dtype).step(prefix, v, _) -> (inc_nn, prefix + (v,)) or None (the candidate does not
    exist: class outside the row, a row without a finite maximum, a non-finite increment);  .final(...) = 0: no term.

dtype=np.float64 is the reference; dtype=np.float32 evaluates y, M, S and inc_nn in numpy float32: the YARDSTICK of the
header's definition (numpy's own summation order -- the header's order is one of many equally valid ones).  ML's walk
rounds the increment to fp32 once, as the device does.  Columns that are -inf or NaN take no part in M and S.

`table_lm` is the LM of the tests: row = table[last token], table[-1] for the empty sequence -- equal sequences get
equal rows, so the members of a group agree on their bonus bit for bit.  `lm_rows` are the rows the device gets for a
beam (NaN for the empty slots: the kernel must not read them).  `lstm_reference` is the float64 CPU loop of
`modified_beam_search_nnlm` on a model's and an `LstmLm`'s own weights."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msearch_lm_common as ML  # noqa: E402

NINF = -np.inf


def log_softmax_row(row, scale, dtype):
    """(lp (V_lm,), ok): lp = (y - M) - S of y = scale * row in `dtype`; ok False when M is not finite."""
    with np.errstate(all="ignore"):
        y = (dtype(scale) * np.asarray(row).astype(dtype)).astype(dtype)
        part = ~np.isnan(y) & (y > NINF)
        if not part.any():
            return y, False
        M = y[part].max()
        if not np.isfinite(M):
            return y, False
        S = np.log(np.exp((y[part] - M).astype(dtype)).sum(dtype=dtype)).astype(dtype)
        return ((y - M).astype(dtype) - S).astype(dtype), True


class DenseLm(object):
    def __init__(self, row_of, scale=1.0, offset=0, dtype=np.float64):
        self.row_of, self.scale, self.offset, self.dtype = row_of, scale, int(offset), dtype
        self.start, self._lp = (), {}

    def step(self, prefix, v, _dtype=None):
        if prefix not in self._lp:
            self._lp[prefix] = log_softmax_row(self.row_of(prefix), self.scale, self.dtype)
        lp, ok = self._lp[prefix]
        c = v + self.offset
        if not ok or not 0 <= c < len(lp) or not np.isfinite(lp[c]):
            return None
        return lp[c], prefix + (v,)

    def final(self, prefix, _dtype=None):
        return 0.0

    def score(self, tokens):
        """sum of the increments of a token sequence in `dtype`, unrounded; None: some token does not exist."""
        total, prefix = 0.0, ()
        for v in tokens:
            st = self.step(prefix, v)
            if st is None:
                return None
            total, prefix = total + float(st[0]), st[1]
        return total


def table_lm(table, scale=1.0, offset=0, dtype=np.float64):
    """table (rows, V_lm) float32: row v for a sequence that ends in token v, the last row for the empty sequence."""
    return DenseLm(lambda prefix: table[prefix[-1] if prefix else -1], scale, offset, dtype)


def make_table(V, V_lm, seed, scale=2.0):
    return (scale * np.random.RandomState(seed).randn(V + 1, V_lm)).astype(np.float32)


def lm_rows(table, tokens_of_slots, live):
    """(K, V_lm) float32 for the device: the table's row per live slot, NaN for the others."""
    rows = np.full((len(live), table.shape[1]), np.nan, np.float32)
    for k, (tok, alive) in enumerate(zip(tokens_of_slots, live)):
        if alive:
            rows[k] = table[tok[-1] if tok else -1]
    return rows


def lstm_reference(net64, lm64, enc, x_len, K, C, sm_scale, nn_weight, nn_scale, offset, lms, weights, lb):
    """Per utterance ([(tokens, score, am)] with use_final, the smallest margin of the float64 run): the float64 fused
    search on the model's own weights -- prediction network and joint as tests/test_msearch_gpu.reference_search -- and
    on the LstmLm's (`lm64`: the module in double on the CPU), re-run on the prefix."""
    import torch
    out = []
    with torch.no_grad():
        def lm_row(prefix):
            ids = torch.tensor([[c + offset for c in prefix]], dtype=torch.long).reshape(1, len(prefix))
            return lm64(ids)[0, -1].numpy()
        for b in range(enc.shape[0]):
            cache = {}

            def logits_of(tok, t, b=b, cache=cache):
                if tok not in cache:
                    o, _ = net64.decoder(net64.embed(torch.tensor([[0] + list(tok)])))
                    cache[tok] = o[0, -1]
                z = torch.cat((enc[b, t], cache[tok]))
                h = torch.tanh(net64.fc1(z)) * torch.sigmoid(net64.fc_gate(z))
                return net64.fc2(h).numpy()
            all_lms = list(lms) + [DenseLm(lm_row, nn_scale, offset)]
            all_w = list(weights) + [nn_weight]
            beam, infos = ML.search(logits_of, int(x_len[b]), net64.output_dim, K, C, all_lms, all_w, lb, 0, sm_scale, 0.0)
            fin = ML.results(beam, all_lms, all_w, True)
            out.append((fin, ML.margins(infos, fin)))
    return out
