"""CPU-side checks of the one-symbol-per-frame beam search: the float64 step reference against an independently written
k2-style search, against the modified RNN-T loss it decodes for, and the plain-torch route of `ModifiedBeamState`
against the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msearch_common as M  # noqa: E402
import rnnt_modified_common as R  # noqa: E402


@pytest.mark.parametrize("T,V,K,blank,sm_scale,penalty", [(6, 5, 4, 0, 1.0, 0.0), (9, 7, 3, 2, 0.8, 0.5),
                                                          (5, 3, 8, 0, 1.0, 0.0), (7, 4, 1, 0, 1.3, 0.0),
                                                          (4, 2, 64, 1, 1.0, -0.3)])
def test_step_reference_equals_the_k2_style_search(T, V, K, blank, sm_scale, penalty):
    for seed in range(5):
        model = M.TableModel(T, V, seed, blank)
        beam, _ = M.search(model, T, V, K, blank, sm_scale, penalty)
        want = M.k2_search(model, T, V, K, blank, sm_scale, penalty)
        got = {tok: s for s, tok in beam if s > M.NINF}
        assert set(got) == set(want) and len(got) == sum(s > M.NINF for s, _ in beam)
        for tok in got:
            assert abs(got[tok] - want[tok]) < 1e-12
        scores = [s for s, _ in beam if s > M.NINF]
        assert scores == sorted(scores, reverse=True)


@pytest.mark.parametrize("T,V,K", [(4, 3, 64), (3, 4, 64)])
def test_unpruned_scores_are_the_modified_loss(T, V, K):
    """Nothing is pruned at these sizes (at most 15 * 3 and 13 * 4 candidates), so a hypothesis's score is the
    log-probability the modified loss gives its token sequence."""
    for seed, (sm_scale, penalty) in enumerate([(1.0, 0.0), (0.7, 0.4)]):
        model = M.TableModel(T, V, 100 + seed)
        beam, infos = M.search(model, T, V, K, 0, sm_scale, penalty)
        live = [(s, tok) for s, tok in beam if s > M.NINF]
        assert len(live) == sum((V - 1) ** u for u in range(T + 1))
        assert all(len(i["selected"]) == np.sum(i["cand"] > M.NINF) for i in infos)      # no candidate was cut
        for s, tok in live:
            pb, pl = M.planes_for(model, tok, T, 0, sm_scale, penalty)
            cost, _, _ = R.planes_loss_ref(pb, pl, np.array([T]), np.array([len(tok)]))
            assert abs(s + cost[0]) < 1e-12, (tok, s, cost)


def drive(state, model, T, V, num_frames, sm_scale, penalty):
    """Frame steps of a `ModifiedBeamState` on a table model per utterance; -> per-step (parent, token)."""
    B, K = state.batch, state.beam
    out = []
    for _ in range(T):
        hyp, ln = state.hyps()
        fr = state.frames.tolist()
        rows = np.zeros((B * K, V))
        for b in range(B):
            for k in range(K):
                if ln[b, k] >= 0:
                    tok = tuple(int(v) for v in hyp[b, k, :int(ln[b, k])])
                    rows[b * K + k] = model[b](tok, min(fr[b], model[b].T - 1))
        logits = torch.from_numpy(rows).to(state.dtype)
        out.append(state.advance(logits, num_frames, sm_scale, penalty))
    return out


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,V,blank", [(4, 6, 0), (1, 5, 1), (8, 3, 2), (64, 2, 0)])
def test_torch_route_equals_the_reference(dtype, K, V, blank):
    from pika_amd import ModifiedBeamState
    T, B = 7, 3
    lens = [0, 3, T]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    tol = 1e-12 if dtype == torch.float64 else 2e-5
    models = [M.TableModel(T, V, 7 * K + b, blank) for b in range(B)]
    state = ModifiedBeamState(B, T, K, blank, "cpu", dtype)
    assert not state.native and state.frames.tolist() == [0] * B
    steps = drive(state, models, T, V, torch.tensor(lens), 0.9, 0.25)
    assert state.frames.tolist() == lens and not state.overflowed.any()
    tokens, lengths, scores = state.results(nbest=K)
    for b in range(B):
        beam = M.start(K, npdt)
        for t in range(lens[b]):
            rows = M.rows_of(models[b], beam, t, V).astype(npdt)
            beam, parent, token, _ = M.step(beam, rows, blank, 0.9, 0.25, npdt)
            assert steps[t][0][b].tolist() == parent.tolist() and steps[t][1][b].tolist() == token.tolist()
        for t in range(lens[b], T):                      # inactive: the identity
            assert steps[t][0][b].tolist() == list(range(K)) and steps[t][1][b].tolist() == [blank] * K
        for j, (s, tok) in enumerate(beam):
            if s > M.NINF:
                assert int(lengths[b, j]) == len(tok) and tokens[b, j, :len(tok)].tolist() == list(tok)
                assert (tokens[b, j, len(tok):] == -1).all() and abs(float(scores[b, j]) - float(s)) <= tol
            else:
                assert int(lengths[b, j]) == -1 and float(scores[b, j]) == -np.inf and (tokens[b, j] == -1).all()


def test_torch_route_state_handling():
    from pika_amd import ModifiedBeamState
    T, V, K, B = 3, 4, 2, 2
    models = [M.TableModel(8, V, b) for b in range(B)]
    state = ModifiedBeamState(B, T, K, 0, "cpu", torch.float64)
    drive(state, models, 5, V, torch.tensor([8, 2]), 1.0, 0.0)
    assert state.frames.tolist() == [3, 2] and state.overflowed.tolist() == [True, False]
    before = state.results(nbest=K)
    state.reset(which=[False, True])
    after = state.results(nbest=K)
    assert state.frames.tolist() == [3, 0] and state.overflowed.tolist() == [True, False]
    assert all(torch.equal(a[0], c[0]) for a, c in zip(before, after))
    assert after[1][1].tolist() == [0, -1] and after[2][1].tolist() == [0.0, -np.inf]
    tok, ln, _ = state.results(nbest=1, max_len=1)
    assert tok.shape == (B, 1, 1)
