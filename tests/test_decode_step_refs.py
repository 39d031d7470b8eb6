"""tests/decode_step_common.py on its own, without a GPU: the references agree with the product's tensor-op bookkeeping and
with torch's own float64 operators, and every mutant is far outside the bound the GPU test applies
(tests/test_decode_step_kernels_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decode_step_common as R  # noqa: E402


@pytest.mark.parametrize("step", [2, 3])
def test_prep_reference_reproduces_the_tensor_op_bookkeeping(step):
    """One random step through decoder/prednet_cache.py (`reorder` by parent, then `step`: ancestry with the new node, the
    layer-0 cache row of the new label) and the state / frame-index lines of decoder/transducer_decoder.py's `step`
    (index_select by parent, t_idx += (y == blank)) against prep_ref."""
    from test_decode import build
    from pika_amd.decoder.prednet_cache import IncrementalPredNet
    net = build("transformer", "cpu").decoder
    emb = net.embeddings.weight.detach().float().numpy()
    B, beam, L = 3, 4, 12
    c = R.prep_case(B, beam, L, net.linear_out.weight.shape[0], (emb.shape[1],), 0, step, vocab=emb.shape[0] - 1, seed=step)
    c["emb"] = emb.copy()
    rows = c["rows"]
    with torch.no_grad():
        inc = IncrementalPredNet(net, rows, step + 1, L, torch.device("cpu"), 0)
        assert inc.dump_node >= c["nan_node"]
        inc.anc.copy_(torch.from_numpy(c["anc"][c["src"]]))
        inc.X[0][:c["cap"]] = torch.from_numpy(np.nan_to_num(c["X"][0]))
        state = torch.from_numpy(c["state"][c["src"]]).clone()
        t_idx = torch.from_numpy(c["t_idx"]).clone()
        tok = torch.from_numpy(c["y"])
        flat = (torch.arange(rows) // beam) * beam + torch.from_numpy(c["prev_k"])
        # transducer_decoder.py `step`: frame indices, then the re-order by parent of the step before
        t_idx.add_(tok.eq(0).long())
        state.copy_(state.index_select(0, flat))
        inc.reorder(flat)
        inc.step(state, tok, torch.from_numpy(c["hyp_len"]), torch.tensor(step), L)
    order = R.committing_rows(c)
    w = R.prep_ref(c, order)
    dst = c["src"] ^ 1
    commit = c["y"] > 0
    assert commit.any() and (~commit).any()
    assert np.array_equal(w["t_idx"], t_idx.numpy())
    assert np.array_equal(w["state"][dst][~commit], state.numpy()[~commit])      # (committing rows: the net's new state)
    v = w["anc_valid"]
    assert np.array_equal(w["anc"][dst][v], inc.anc.numpy()[v])
    pos = np.minimum(c["hyp_len"], L - 1)
    X0 = inc.X[0].numpy()
    for slot, r in enumerate(order):
        assert inc.anc[r, pos[r]] == w["node"][slot] == 1 + step * rows + r
        assert np.array_equal(X0[w["node"][slot]], w["X"][0][w["node"][slot]])
        C = c["Cs"][0]
        for j in range(4):
            q = pos[r] - 4 + j
            want = np.zeros(C, np.float32) if q < 0 else X0[inc.anc[r, q]]
            assert np.array_equal(w["A"][0][slot, j * C:(j + 1) * C], want)
        assert np.array_equal(w["A"][0][slot, 4 * C:5 * C], emb[c["y"][r]])


def test_cell_reference_is_torch_lstm_cell():
    g = torch.Generator().manual_seed(3)
    H, m = 20, 9
    cell = torch.nn.LSTMCell(5, H).double()
    with torch.no_grad():
        cell.weight_ih.zero_()
        cell.weight_hh.zero_()
        cell.bias_hh.zero_()
        for scale in (1.0, 30.0):
            gates = torch.randn(m, 4 * H, generator=g, dtype=torch.float64) * scale
            c0 = torch.randn(m, H, generator=g, dtype=torch.float64)
            h1 = torch.empty(m, H, dtype=torch.float64)
            c1 = torch.empty(m, H, dtype=torch.float64)
            for r in range(m):                   # the gate pre-activations enter as the bias: one row at a time
                cell.bias_ih.copy_(gates[r])
                h1[r], c1[r] = cell(torch.zeros(5, dtype=torch.float64), (torch.zeros(H, dtype=torch.float64), c0[r]))
            h, c = R.lstm_cell(gates.numpy(), c0.numpy())
            assert np.abs(h - h1.numpy()).max() < 1e-14 and np.abs(c - c1.numpy()).max() < 1e-14
            assert np.isfinite(h).all() and np.isfinite(c).all()


def test_attention_reference_is_torch_sdpa():
    c = R.attention_case(64, 4, rows=9, seed=1)
    c["pos"][:] = c["L"] - 1                      # a dense prefix for every row
    anc = np.random.default_rng(0).integers(0, 61, size=(9, c["L"])).astype(np.int64)
    out, Kc, Vc = R.attention_ref(c, anc, None, 9)
    d, heads, L = c["d"], c["heads"], c["L"]
    k = torch.from_numpy(c["Kc"]).double()[torch.from_numpy(anc)]                 # (rows, L, d)
    v = torch.from_numpy(c["Vc"]).double()[torch.from_numpy(anc)]
    kvq = torch.from_numpy(c["kvq"]).double()
    k[:, L - 1], v[:, L - 1] = kvq[:, :d], kvq[:, d:2 * d]

    def heads_first(t):
        return t.view(9, -1, heads, d // heads).transpose(1, 2)
    want = torch.nn.functional.scaled_dot_product_attention(heads_first(kvq[:, 2 * d:].unsqueeze(1)), heads_first(k),
                                                            heads_first(v)).transpose(1, 2).reshape(9, d)
    assert np.abs(out - want.numpy()).max() < 1e-13
    assert np.array_equal(Kc[c["node"]], c["kvq"][:, :d]) and np.array_equal(Vc[c["node"]], c["kvq"][:, d:2 * d])


@pytest.mark.parametrize("mutant", R.PREP_MUTANTS)
def test_prep_mutants_are_caught(mutant):
    c = R.prep_case(3, 4, 12, 64, (48, 300), 64, 3, seed=1)
    order = R.committing_rows(c)
    want = R.prep_ref(c, order)
    assert R.prep_mismatches(want, want, c) == []
    got = R.prep_ref(c, order, mutant)
    bad = R.prep_mismatches(got, want, c)
    expect = {"child_taps": "A[0]", "pos_unclamped": "pos", "node_off_row": "node", "frame_before_increment": "h"}[mutant]
    assert expect in bad, bad
    if mutant == "frame_before_increment":        # the one bounded (not exact) comparison: ten times outside, at least
        assert R.h_error(got, want) > 10 * R.H_TOL
    cl = R.prep_lstm_case(3, 4, 2, 260, 48, True, 3, seed=1)
    if mutant in ("child_taps", "frame_before_increment"):
        wl = R.prep_lstm_ref(cl, R.committing_rows(cl))
        gl = R.prep_lstm_ref(cl, R.committing_rows(cl), mutant)
        assert R.prep_lstm_mismatches(wl, wl, cl) == []
        assert ("A[0]" if mutant == "child_taps" else "h") in R.prep_lstm_mismatches(gl, wl, cl)


@pytest.mark.parametrize("mutant", R.ATT_MUTANTS)
@pytest.mark.parametrize("d,heads", [(64, 4), (512, 8), (1024, 4)])
def test_attention_mutants_are_caught(mutant, d, heads):
    c = R.attention_case(d, heads)
    want, _, _ = R.attention_ref(c, c["anc_perm"], c["rowmap"], c["rows"])
    got, _, _ = R.attention_ref(c, c["anc_perm"], c["rowmap"], c["rows"], mutant)
    assert R.att_error(got, want) > 10 * R.att_bound(want, c["rows"])


def test_cell_gate_order_mutant_is_caught():
    rng = np.random.default_rng(5)
    gates, c0 = rng.standard_normal((12, 4 * 260)), rng.standard_normal((12, 260))
    h, c = R.lstm_cell(gates, c0)
    hm, cm = R.lstm_cell(gates, c0, order="ifog")
    assert np.abs(hm - h).max() > 10 * R.cell_bound(h).max() and np.abs(cm - c).max() > 10 * R.cell_bound(c).max()
    # the fp32 restatement of the same five lines stays inside the bound's order of magnitude
    h32, c32 = R.lstm_cell(gates, c0, dtype=np.float32)
    assert np.abs(h32 - h).max() < 1e-6 and np.abs(c32 - c).max() < 2e-6


def test_gate_slot_row_mutant_is_caught_and_the_models_are_inside_the_tolerances():
    g = torch.Generator().manual_seed(2)
    B, beam, T, H, K, m = 4, 16, 11, 40, 512, 33
    A = torch.randn(B * beam, K, generator=g)
    W = torch.randn(2 * H, K, generator=g) / K ** 0.5
    e_all = torch.randn(B * T, 2 * H, generator=g)
    t_idx = torch.randint(-1, T + 2, (B * beam,), generator=g)
    rows = torch.randperm(B * beam, generator=g)[:m]
    z = A[rows].double() @ W.double().t()
    want = R.gate(z, e_all, t_idx, rows, beam, T)
    assert R.err(R.gate(z, e_all, t_idx, rows, beam, T, slot_rows=True), want) > 10 * R.H_TOL
    assert torch.equal(R.interleave(z)[:, 0::2], z[:, :H]) and torch.equal(R.interleave(z)[:, 1::2], z[:, H:])
    scale = float(z.abs().max())
    for terms, tol in R.GEMM_TOL.items():         # what the term count costs is inside the tolerance it is tested at
        e = R.err(R.model_product(A[rows], W, terms).float(), z)
        assert e <= tol * scale / R.MARGIN, (terms, e)
    parts = R.split_terms(A, 3)
    assert R.err(sum(parts), A) == 0.0            # three bf16 terms hold an fp32 value exactly
