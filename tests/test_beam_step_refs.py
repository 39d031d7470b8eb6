"""tests/beam_step_common.py on its own, without a GPU: the float64 reference of one beam-search step agrees with
`BeamState._advance` (the restatement pinned by the reference-decoder goldens) run in float64, every case of the table is
decisive and holds the state classes it names, and every mutant of the reference is caught by some case of the table --
the cases tests/test_beam_step_gpu.py runs the two advance kernels on."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import beam_step_common as R  # noqa: E402

NO_TIES = [c["name"] for c in R.CASES if "ties" not in c["tags"]]


def beamstate_advance(case, s0, logits):
    """BeamState._advance on the CPU with its tensors promoted to float64 -> the compared fields as numpy."""
    from pika_amd.decoder.beam_search import BeamState
    B, K, V, L = case["B"], case["K"], case["V"], case["L"]
    bs = BeamState(B, K, case["blk"], R.N_BEST, s0["max_len"].tolist(), V, torch.device("cpu"), beam_prune=bool(case["beam_prune"]))
    t = {k: torch.from_numpy(v.copy()) for k, v in s0.items()}
    bs.scores, bs.lm_scores = t["scores"].double(), t["lm_scores"].double()
    bs.y, bs.hyp, bs.hyp_len = t["y"], t["hyp"], t["hyp_len"]
    bs.ks_hist, bs.ys_hist, bs.step_t = t["ks_hist"], t["ys_hist"], t["step_t"]
    bs.eos_top = t["eos_top"].bool()
    bs.fin_cap = s0["fin_score"].shape[1]
    bs.fin_score, bs.fin_step, bs.fin_k, bs.fin_n = t["fin_score"].double(), t["fin_step"], t["fin_k"], t["fin_n"]
    bs._pos = torch.arange(L).view(1, 1, L)
    bs._brow = (torch.arange(B) * bs.fin_cap).unsqueeze(1)
    x = torch.from_numpy((np.float32(R.SM_SCALE) * logits).astype(np.float32)).double()
    prev_k = bs._advance(torch.log_softmax(x, dim=2), t["t_idx"], t["num_frames"], float(np.float32(R.LM_SCALE)), case["first"])
    got = dict(scores=bs.scores, y=bs.y, hyp=bs.hyp, hyp_len=bs.hyp_len, ks_hist=bs.ks_hist, ys_hist=bs.ys_hist,
               eos_top=bs.eos_top.to(torch.uint8), fin_score=bs.fin_score, fin_step=bs.fin_step, fin_k=bs.fin_k, fin_n=bs.fin_n,
               prev_k=prev_k, t_idx=t["t_idx"].gather(1, prev_k))
    return {k: v.numpy() for k, v in got.items()}, int(bs.step_t)


def test_the_table_covers_what_it_claims():
    ks = {c["K"] for c in R.CASES}
    vs = {c["V"] for c in R.CASES}
    assert ks == {1, 2, 3, 5, 16, 17, 33, 64}
    assert vs >= {64, 65, 191, 192, 193, 333, 1000, 6268, 8192, 12288} and any(c["V"] == c["K"] for c in R.CASES)
    assert {c["B"] for c in R.CASES} >= {1, 3, 5}
    k64 = {(c["V"], c["L"]) for c in R.CASES if c["K"] == 64}
    assert {v for v, _ in k64} >= {8192, 64, 193} and {l for _, l in k64} >= {100, 160, 200}
    named = {u for c in R.CASES for u in c["utts"]}
    assert named == set(R.STATE_CLASSES), set(R.STATE_CLASSES) ^ named
    assert any(c["beam_prune"] == 0 for c in R.CASES) and any("no_y_raw" in c["tags"] for c in R.CASES)
    assert any("misaligned" in c["tags"] and c["V"] % 4 == 0 for c in R.CASES)
    assert any("ldl_pad" in c["tags"] for c in R.CASES)
    assert any(c["L"] > 64 and "long70" in c["utts"] for c in R.CASES)


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_case_is_decisive_and_holds_its_state_classes(name):
    """make_state asserts decisiveness (it raises otherwise); the `ties` tag says exactly whether an exact tie sits among
    some utterance's top K + 1; and each named class does what the table says of it, read off the reference's result."""
    case = R.CASE_BY_NAME[name]
    state, logits, tie, want, want_l, yard = R.case_data(name)
    assert tie == ("ties" in case["tags"])
    assert all(w.intact() for w in state.values()) and logits.intact()
    s0 = R.plain(state)
    K, V, blk = case["K"], case["V"], case["blk"]
    step = int(s0["step_t"][0])
    for b, cls in enumerate(case["utts"]):
        fin = want["y"][b] == R.EOS
        par, sym = want["prev_k"][b], want["y_raw"][b]
        dead = R.disabled_rows(s0["y"][b], s0["hyp"][b], s0["hyp_len"][b], case["beam_prune"])
        if case["first"]:
            assert (par == 0).all() and s0["scores"][b].any() and s0["lm_scores"][b].any() and s0["hyp_len"][b].any()
            continue
        if cls == "all_eos":
            assert (par == 0).all() and (sym == np.arange(K)).all() and (np.abs(want["scores"][b]) > 1e19).all()
        elif cls == "single_live":
            assert (s0["y"][b] != R.EOS).sum() == 1
        elif cls in ("dup_live", "three_way"):
            assert dead.sum() == (case["beam_prune"] and (2 if cls == "three_way" else 1)) and (s0["y"][b] != R.EOS).all()
            assert case["beam_prune"] == 0 or not np.isin(par, np.flatnonzero(dead)).any()
        elif cls == "dup_eos":
            k1, k2, k3 = R._three(K)
            assert dead[k1] and not dead[k2] and dead[k3] == bool(case["beam_prune"]) and (par == k2).any()
        elif cls in ("diff_first", "diff_last", "dup_empty"):
            assert not dead[list(R._three(K)) if cls == "dup_empty" else [0, K - 1]].any() and (par == K - 1).any()    # (K - 1: the boosted slot)
        elif cls == "long70":
            k1, k2, k3 = R._three(K)
            assert s0["hyp_len"][b, k2] == 70 and (s0["hyp"][b, k1, :70] != s0["hyp"][b, k2, :70]).nonzero()[0].tolist() == [65]
            assert not dead[k2] and dead[k3] == bool(case["beam_prune"])
        elif cls == "blank_parent_last":
            p = par[0]
            assert sym[0] == blk and s0["t_idx"][b, p] == R.NF - 1 and s0["t_idx"][b, 0] != R.NF - 1 and fin[0] and p != 0
        elif cls == "blank_parent_conv":
            p = par[0]
            assert sym[0] == blk and s0["t_idx"][b, p] != R.NF - 1 and s0["t_idx"][b, 0] == R.NF - 1 and not fin[0] and p != 0
        elif cls == "only_nonzero_finish":
            assert not fin[0] and fin[1:].any() and want["eos_top"][b] == 0
        elif cls in ("maxlen", "fin_clamp"):
            assert fin.all() and step + 2 > s0["max_len"][b]
            if cls == "fin_clamp":
                cap = s0["fin_score"].shape[1]
                assert K >= 4 and s0["fin_n"][b] == cap - 4 and want["fin_n"][b] == cap - 4 + K and want["fin_k"][b, cap - 2] == K - 1
        elif cls == "maxlen_next":
            assert step + 2 == s0["max_len"][b]
        elif cls == "eos_top_set":
            assert s0["eos_top"][b] == 1 and want["eos_top"][b] == 1
        elif cls == "pool_tie":
            x = logits.view[b, K // 2]
            assert (x == 1.0).sum() == 300 and (x > 1.0).sum() < K and (par == K // 2).all()
        elif cls in ("tie_kth", "all_equal"):
            assert (par == K // 2).all()
        elif cls == "cross_row_tie":
            k1, k2 = (0, K - 1) if K < 5 else (1, K - 2)
            assert (par == k1).any() and (par == k2).any()
    if name == "k17_v193":
        assert (want["y"][0] == R.EOS).all() and not (want["y"][1:] == R.EOS).all(axis=1).any()   # by max_len: utterance 0 only
    if name in ("k2_v65_stop", "k5_v65_alldone"):
        assert want_l["stop"][0] == 1
    else:
        assert want_l["stop"][0] == 0


@pytest.mark.parametrize("name", NO_TIES)
def test_reference_agrees_with_beamstate_advance(name):
    case = R.CASE_BY_NAME[name]
    state, logits, tie, want, want_l, yard = R.case_data(name)
    s0 = R.plain(state)
    got, step_after = beamstate_advance(case, s0, logits.view)
    got["y_raw"] = want["y_raw"]                     # (_advance does not keep the symbol before the eos substitution)
    assert R.compare(got, want, s0, R.close64) == []
    assert step_after == want_l["step_t"][0]


def test_every_tie_free_case_is_cross_checked_and_no_other():
    assert set(NO_TIES) == {c["name"] for c in R.CASES if not R.case_data(c["name"])[2]}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_caught_by_some_case(mutant):
    caught = []
    for case in R.CASES:
        if case["V"] > 1000:                         # (the wide cases add nothing the small ones lack here)
            continue
        state, logits, tie, want, want_l, yard = R.case_data(case["name"])
        s0 = R.plain(state)
        got = R.advance_logits_ref(s0, logits.view, R.SM_SCALE, R.LM_SCALE, case["beam_prune"], case["blk"], R.N_BEST, mutant)
        bad = R.compare(got, want_l, s0, R.close64, logits_entry=True)
        if bad:
            caught.append((case["name"], bad))
    assert caught, "no case of the table notices the mutant %s" % mutant


def test_unmutated_reference_equals_itself_and_the_step_entry_point_adds_only_its_fields():
    for name in ("k3_v191", "k5_v65_alldone"):
        case = R.CASE_BY_NAME[name]
        state, logits, tie, want, want_l, yard = R.case_data(name)
        s0 = R.plain(state)
        again = R.advance_logits_ref(s0, logits.view, R.SM_SCALE, R.LM_SCALE, case["beam_prune"], case["blk"], R.N_BEST)
        assert R.compare(again, want_l, s0, R.close64, logits_entry=True) == []
        assert R.compare(want_l, want, s0, R.close64) == []
        s0["stop"][0] = 1                            # a call after the search has ended writes sync[4] and nothing else
        skipped = R.advance_logits_ref(s0, logits.view, R.SM_SCALE, R.LM_SCALE, case["beam_prune"], case["blk"], R.N_BEST)
        assert skipped["sync"][4] == 1 and all(np.array_equal(skipped[k], s0[k]) for k in s0 if k != "sync")


@pytest.mark.parametrize("cfg", R.MULTI_STEP, ids=lambda c: c["name"])
def test_multi_step_reference_against_beamstate_advance(cfg):
    """Six consecutive steps from the clean start, each side carrying its own state (BeamState in float64)."""
    case = dict(cfg, blk=0, beam_prune=1, first=False)
    s = R.plain(R.multi_step_start(cfg))
    finished_any = False
    for step_no in range(cfg["steps"]):
        logits, lm = R.multi_step_logits(cfg, s, step_no)
        s["lm_scores"] = lm
        want = R.advance_logits_ref(s, logits, R.SM_SCALE, R.LM_SCALE, 1, 0, R.N_BEST)
        _, tie = zip(*[R.top_is_decisive((np.float32(R.SM_SCALE) * logits[b]).astype(np.float32),
                                         dict(y=s["y"][b], hyp=s["hyp"][b], hyp_len=s["hyp_len"][b], scores=s["scores"][b],
                                              lm_scores=lm[b]), step_no == 0, 1) for b in range(cfg["B"])])
        if not any(tie):
            s32 = dict(s, scores=s["scores"].astype(np.float64), fin_score=s["fin_score"].astype(np.float64))
            got, _ = beamstate_advance(dict(case, first=step_no == 0), s32, logits)
            got["y_raw"] = want["y_raw"]
            assert R.compare(got, want, s, R.close64) == [], step_no
        finished_any |= bool((want["y"] == R.EOS).any())
        s = {k: v for k, v in want.items() if k != "new_len"}
        R.frame_rule(s, 0)
    assert finished_any and int(s["step_t"][0]) == cfg["steps"] and int(s["max_hyp"][0]) > 0
