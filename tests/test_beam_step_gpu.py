"""`pika_beam_advance` and `pika_beam_advance_logits` (pika_amd/csrc/decode.hip) against the float64 reference of one
search step (tests/beam_step_common.py), state by state, on every case of its table; six consecutive steps with each side
carrying its own state; the argument refusals; and after every call the sentinels around every buffer.

Integers (parents, symbols, frame indices, hypotheses on [0, hyp_len'), histories, finished lists, eos_top, counters,
stop / max_hyp / sync) are compared for equality.  Scores: per case the contract's formula is also evaluated in fp32 with
plain torch ops on the CPU (the yardstick); the kernel may deviate from the float64 reference by 4 x the yardstick's
largest deviation, at least 4 ulp of the score; dead candidates equal float32(reference) exactly.  Every figure is printed
(`BEAMSTEP ...`) before it is asserted; profiles/beam_step_parity.txt keeps those lines.

Measured on the MI355X: yardstick errors 9e-8 .. 1.7e-6, kernel errors 1.4e-7 .. 1.4e-6, largest ratio 3.2 (k5_v192_first),
most cases at 1.0 (the kernels evaluate the contract's formula in the yardstick's order).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_step_common as R  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ETOOBIG = -1, -2

STATE_ARGS = ["scores", "lm_scores", "lm_scale", "y", "t_idx", "num_frames", "max_len", "hyp", "hyp_len", "L", "ks_hist",
              "ys_hist", "step_t", "eos_top", "fin_score", "fin_step", "fin_k", "fin_n", "fin_cap", "prev_k", "y_raw"]
ADVANCE_ARGS = ["logits", "sm_scale", "first"] + STATE_ARGS + ["cand_ws", "B", "K", "V", "blk", "beam_prune"]
LOGITS_ARGS = ["pmax", "psum", "xpad", "ldl", "splits"] + STATE_ARGS + ["B", "K", "V", "blk", "beam_prune", "n_best", "stop",
                                                                        "max_hyp", "sync"]
SCALARS = {"sm_scale", "first", "lm_scale", "L", "fin_cap", "B", "K", "V", "blk", "beam_prune", "n_best", "ldl", "splits"}


class Dev:
    """The buffers of one call on the device, sentinels included."""

    def __init__(self, wins, dev):
        self.wins = dict(wins)
        self.t = {k: torch.from_numpy(w.full.copy()).to(dev) for k, w in self.wins.items()}

    def ptr(self, k):
        return self.t[k].data_ptr() + self.wins[k].lo * self.t[k].element_size()

    def put(self, k, arr):
        w = self.wins[k]
        self.t[k][w.lo:w.lo + w.n] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).to(self.t[k])

    def fetch(self):
        """name -> window after the call; asserts that no sentinel element changed."""
        torch.cuda.synchronize()
        out = {}
        for k, w in self.wins.items():
            full = self.t[k].cpu().numpy()
            assert w.intact(full), "sentinel around %s overwritten" % k
            out[k] = R.Win.window_of(w, full)
        return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def call(entry, d, dims, **override):
    from pika_amd import _lib
    lib = _lib.lib()
    names = ADVANCE_ARGS if entry == "advance" else LOGITS_ARGS
    vals = []
    for n in names:
        if n in override:
            vals.append(override[n])
        elif n in SCALARS:
            vals.append(dims[n])
        else:
            vals.append(d.ptr(n))
    fn = lib.pika_beam_advance if entry == "advance" else lib.pika_beam_advance_logits
    return fn(*vals, _stream())


def device_inputs(state, logits_win, dims, dev, entry, ldl_extra=0):
    wins = dict(state)
    if entry == "advance":
        wins["logits"] = logits_win
    else:
        x = (np.float32(R.SM_SCALE) * logits_win.view).astype(np.float32).reshape(-1, dims["V"])
        pmax, psum, xpad, splits, ldl = R.range_statistics(x, ldl_extra)
        wins.update(pmax=R.Win(pmax), psum=R.Win(psum), xpad=R.Win(xpad))
        dims.update(splits=splits, ldl=ldl)
    return Dev(wins, dev)


def case_dims(case, state):
    return dict(B=case["B"], K=case["K"], V=case["V"], L=case["L"], blk=case["blk"], beam_prune=case["beam_prune"],
                fin_cap=state["fin_score"].shape[1], sm_scale=R.SM_SCALE, lm_scale=R.LM_SCALE, first=int(case["first"]),
                n_best=R.N_BEST)


def report(name, entry, yard, got, want):
    err = max(R.kernel_error(got["scores"], want["scores"]), 0.0)
    print("BEAMSTEP %-22s %-8s yardstick err %.3g  kernel err %.3g  ratio %.3g  (allowed 4, floor 4 ulp)"
          % (name, entry, yard, err, err / yard if yard > 0 else float("nan")))


@pytest.mark.parametrize("entry", ["advance", "logits"])
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_one_step_against_float64(hip_device, name, entry):
    case = R.CASE_BY_NAME[name]
    state, logits, tie, want, want_l, yard = R.case_data(name)
    dims = case_dims(case, state)
    if entry not in case["entries"]:                 # the shape belongs to the other entry point: this one refuses it
        d = device_inputs(state, logits, dims, hip_device, entry)
        assert call(entry, d, dims) == ETOOBIG
        got = d.fetch()
        assert all(np.array_equal(got[k], w.view) for k, w in state.items())
        return
    d = device_inputs(state, logits, dims, hip_device, entry, 64 if "ldl_pad" in case["tags"] else 0)
    if entry == "advance":
        assert d.ptr("logits") % 16 == (4 if "misaligned" in case["tags"] else 0)
    elif "ldl_pad" in case["tags"]:
        assert dims["ldl"] > dims["splits"] * R.COLS
    no_y_raw = "no_y_raw" in case["tags"]
    rc = call(entry, d, dims, **({"y_raw": None} if no_y_raw else {}))
    assert rc == 0, rc
    got = d.fetch()
    ref = want_l if entry == "logits" else want
    report(name, entry, yard, got, ref)
    s0 = R.plain(state)
    assert R.compare(got, ref, s0, R.gpu_score_ok(yard), logits_entry=entry == "logits", y_raw=not no_y_raw) == []
    if no_y_raw:
        assert np.array_equal(got["y_raw"], s0["y_raw"])
    for k in ("lm_scores", "num_frames", "max_len"):                    # inputs stay as they were
        assert np.array_equal(got[k], s0[k]), k
    if entry == "advance":
        assert int(got["step_t"][0]) == int(s0["step_t"][0])           # (the caller counts the steps of this entry point)
    else:
        par = int(s0["step_t"][0]) & 1
        assert got["sync"][4] == 0 and got["sync"][7] == s0["sync"][7]
        assert (got["sync"][2 * par] & 0xffff) == case["B"]            # every utterance arrived once


@pytest.mark.parametrize("entry", ["advance", "logits"])
@pytest.mark.parametrize("cfg", R.MULTI_STEP, ids=lambda c: c["name"])
def test_six_steps_with_carried_state(hip_device, cfg, entry):
    """Fresh logits per step; the kernel, the float64 reference and the fp32 yardstick each carry their own state; between
    steps both sides get the caller's frame rule.  Compared after every step."""
    state = R.multi_step_start(cfg)
    dims = dict(B=cfg["B"], K=cfg["K"], V=cfg["V"], L=cfg["L"], blk=0, beam_prune=1, fin_cap=state["fin_score"].shape[1],
                sm_scale=R.SM_SCALE, lm_scale=R.LM_SCALE, n_best=R.N_BEST)
    s = R.plain(state)
    x0 = np.zeros((cfg["B"], cfg["K"], cfg["V"]), np.float32)
    d = device_inputs(state, R.Win(x0), dims, hip_device, entry)
    yard_scores = np.zeros((cfg["B"], cfg["K"]), np.float32)
    yard = 0.0
    for step_no in range(cfg["steps"]):
        logits, lm = R.multi_step_logits(cfg, s, step_no)
        s["lm_scores"] = lm
        if entry == "advance":
            s["stop"][0] = 0
        stopped = bool(s["stop"][0])
        want = R.advance_logits_ref(s, logits, R.SM_SCALE, R.LM_SCALE, 1, 0, R.N_BEST)
        if not stopped:
            yard_scores = R.yardstick_scores(dict(s, scores=yard_scores), logits, want, step_no == 0)
            live = np.abs(want["scores"]) < 1e19
            if live.any():
                yard = max(yard, float(np.abs(yard_scores.astype(np.float64) - want["scores"])[live].max()))
        d.put("lm_scores", lm)
        if entry == "advance":
            d.put("logits", logits)
            assert call(entry, d, dict(dims, first=int(step_no == 0))) == 0
            d.put("step_t", np.array([step_no + 1], np.int64))
        else:
            pmax, psum, xpad, _, _ = R.range_statistics((np.float32(R.SM_SCALE) * logits).astype(np.float32).reshape(-1, cfg["V"]))
            d.put("pmax", pmax)
            d.put("psum", psum)
            d.put("xpad", xpad)
            assert call(entry, d, dims) == 0
        got = d.fetch()
        report("%s[%d]" % (cfg["name"], step_no), entry, yard, got, want)
        assert R.compare(got, want, s, R.gpu_score_ok(yard), logits_entry=entry == "logits") == [], step_no
        s = {k: v for k, v in want.items() if k != "new_len"}
        R.frame_rule(s, 0)
        g = {"t_idx": got["t_idx"].copy(), "y": got["y"], "num_frames": got["num_frames"]}
        R.frame_rule(g, 0)
        d.put("t_idx", g["t_idx"])
    assert int(s["step_t"][0]) == cfg["steps"] or bool(s["stop"][0])


def test_a_call_after_the_search_ended_writes_sync4_only(hip_device):
    case = R.CASE_BY_NAME["k3_v191"]
    state, logits, *_ = R.case_data("k3_v191")
    dims = case_dims(case, state)
    d = device_inputs(state, logits, dims, hip_device, "logits")
    d.put("stop", np.array([1], np.int32))
    assert call("logits", d, dims) == 0
    got = d.fetch()
    s0 = R.plain(state)
    assert got["sync"][4] == 1 and got["stop"][0] == 1
    got["sync"][4] = 0
    assert all(np.array_equal(got[k], s0[k]) for k in s0 if k != "stop")


def _refusal_inputs(dev, entry, B, K, V, L, **dim_override):
    """Buffers large enough for the stated shape (nothing is launched, but nothing here relies on that)."""
    rng = np.random.default_rng(3)
    utts, xs = zip(*[R.build_utterance("generic", rng, K, V, L, 0, R.STEP_T) for _ in range(B)])
    state = R.assemble(list(utts), K, V, L, 0, R.STEP_T, 2 * K + 6)
    dims = dict(B=B, K=K, V=V, L=L, blk=0, beam_prune=1, fin_cap=2 * K + 6, sm_scale=R.SM_SCALE, lm_scale=R.LM_SCALE, first=0,
                n_best=R.N_BEST)
    d = device_inputs(state, R.Win(np.stack(xs)), dims, dev, entry)
    dims.update(dim_override)
    return state, d, dims


def _untouched(state, d):
    got = d.fetch()
    return all(np.array_equal(got[k], w.view) for k, w in state.items())


@pytest.mark.parametrize("what,B,K,V,L", [("K = 65", 1, 65, 70, 8), ("V = 8193", 1, 2, 8193, 8), ("V = K - 1", 1, 5, 4, 8),
                                          ("K*L*4 > 64 KiB", 1, 64, 64, 257)])
def test_advance_refuses_what_it_cannot_take(hip_device, what, B, K, V, L):
    state, d, dims = _refusal_inputs(hip_device, "advance", B, K, V, L)
    assert call("advance", d, dims) == ETOOBIG
    assert _untouched(state, d)


def test_advance_refuses_null_pointers(hip_device):
    state, d, dims = _refusal_inputs(hip_device, "advance", 1, 3, 9, 8)
    for n in ADVANCE_ARGS:
        if n not in SCALARS and n != "y_raw":
            assert call("advance", d, dims, **{n: None}) == EINVAL, n
    assert _untouched(state, d)


@pytest.mark.parametrize("what,B,K,V,L,over", [("K = 65", 1, 65, 70, 8, {}), ("splits = 65", 1, 2, 64 * 192 + 1, 8, {}),
                                               ("an L whose LDS does not fit", 1, 64, 64, 225, {}),
                                               ("V = K - 1", 1, 5, 4, 8, {})])
def test_advance_logits_refuses_what_it_cannot_take(hip_device, what, B, K, V, L, over):
    from pika_amd import _lib
    state, d, dims = _refusal_inputs(hip_device, "logits", B, K, V, L, **over)
    if what.startswith("an L"):
        assert _lib.lib().pika_beam_advance_logits_lds(K, L, dims["splits"]) == 0
        assert _lib.lib().pika_beam_advance_logits_lds(K, L - 1, dims["splits"]) > 0
    if what.startswith("splits"):
        assert dims["splits"] == 65
    assert call("logits", d, dims) == ETOOBIG
    assert _untouched(state, d)


def test_advance_logits_refuses_bad_arguments(hip_device):
    state, d, dims = _refusal_inputs(hip_device, "logits", 1, 3, 9, 8)
    assert call("logits", d, dict(dims, ldl=dims["V"] - 1)) == EINVAL
    assert call("logits", d, dict(dims, splits=0)) == EINVAL
    for n in LOGITS_ARGS:
        if n not in SCALARS and n != "y_raw":
            assert call("logits", d, dims, **{n: None}) == EINVAL, n
    assert _untouched(state, d)
