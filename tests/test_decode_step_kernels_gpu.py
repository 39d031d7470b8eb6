"""Every entry point of include/pika_decode_step.h that the launch chain of the batch beam search uses, one by one, against
the plain float64 / integer references of tests/decode_step_common.py -- driven through ctypes on buffers the test owns.

Every output buffer carries a sentinel where the contract says the launch must not write; indices a launch must never follow
point at in-bounds rows of NaN; every launch runs twice on the same inputs (the few-rows product promises sums in wave order:
the two results are bit-identical).  Every test prints the figures it asserts on (pytest -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import decode_step_common as R  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ETOOBIG = -1, -2


def _st():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from pika_amd import _lib as L
    return L


def _up(c, dev):
    t = {}
    for k, v in c.items():
        if isinstance(v, np.ndarray):
            t[k] = torch.from_numpy(v.copy()).to(dev)
        elif isinstance(v, list) and v and isinstance(v[0], np.ndarray):
            t[k] = [torch.from_numpy(x.copy()).to(dev) for x in v]
    return t


def _down(t):
    torch.cuda.synchronize()
    return {k: ([x.cpu().numpy() for x in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in t.items()}


def _same(a, b):
    """two downloads, bit for bit"""
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            if not R.bits_equal(x, y):
                return k
    return None


def _fill_joint(j, c, t):
    if c["JH"]:
        for i in range(2):
            j.pj[i] = t["pj"][i].data_ptr()
        j.h, j.e_all, j.rowmap32 = t["h"].data_ptr(), t["e_all"].data_ptr(), t["rowmap32"].data_ptr()
        j.T, j.JH = c["T"], c["JH"]


def _prep_struct(c, t, stop=None):
    from pika_amd.decoder.fused_step import DPrep
    p = DPrep()
    p.prev_k, p.y, p.hyp_len = t["prev_k"].data_ptr(), t["y"].data_ptr(), t["hyp_len"].data_ptr()
    p.step_t, p.t_idx, p.emb = t["step_t"].data_ptr(), t["t_idx"].data_ptr(), t["emb"].data_ptr()
    for i in range(2):
        p.state[i], p.anc[i] = t["state"][i].data_ptr(), t["anc"][i].data_ptr()
    for l in range(c["layers"]):
        p.X[l], p.A[l], p.C[l], p.lda[l] = t["X"][l].data_ptr(), t["A"][l].data_ptr(), c["Cs"][l], c["lda"][l]
    p.node, p.pos, p.rowmap, p.count = t["node"].data_ptr(), t["pos"].data_ptr(), t["rowmap"].data_ptr(), t["count"].data_ptr()
    p.dump_node, p.zero_node = c["dump_node"], c["zero_node"]
    p.layers, p.rows, p.beam, p.H, p.L, p.blk = c["layers"], c["rows"], c["beam"], c["H"], c["L"], c["blk"]
    p.stop = None if stop is None else stop.data_ptr()
    _fill_joint(p.joint, c, t)
    return p


def _prep_lstm_struct(c, t, stop=None):
    from pika_amd.decoder.fused_step import DPrepLSTM
    p = DPrepLSTM()
    p.prev_k, p.y, p.step_t, p.t_idx = t["prev_k"].data_ptr(), t["y"].data_ptr(), t["step_t"].data_ptr(), t["t_idx"].data_ptr()
    p.emb, p.rowmap, p.count = t["emb"].data_ptr(), t["rowmap"].data_ptr(), t["count"].data_ptr()
    for i in range(2):
        p.state[i] = t["state"][i].data_ptr()
    for l in range(c["layers"]):
        p.A[l], p.lda[l] = t["A"][l].data_ptr(), c["lda"][l]
    p.layers, p.rows, p.beam, p.H, p.E, p.blk = c["layers"], c["rows"], c["beam"], c["H"], c["E"], c["blk"]
    p.stop = None if stop is None else stop.data_ptr()
    _fill_joint(p.joint, c, t)
    return p


def _run_prep(c, dev, lstm=False, stop=None):
    L = _lib()
    t = _up(c, dev)
    p = (_prep_lstm_struct if lstm else _prep_struct)(c, t, stop)
    fn = L.lib().pika_dstep_prep_lstm if lstm else L.lib().pika_dstep_prep
    L.check(fn(ctypes.byref(p), _st()), "prep")
    return _down(t), (t, p, fn)


def _check_prep(c, got, lstm=False):
    src = c["src"]
    n = int(got["count"][src])
    commit = R.committing_rows(c)
    assert n == len(commit) and int(got["count"][src ^ 1]) == R.SENT_I
    order = got["rowmap"][:n]
    assert sorted(order.tolist()) == commit.tolist()                     # a permutation of the committing rows
    want = (R.prep_lstm_ref if lstm else R.prep_ref)(c, order)
    bad = (R.prep_lstm_mismatches if lstm else R.prep_mismatches)(got, want, c)
    e = R.h_error(got, want) if c["JH"] else 0.0
    print("prep%s rows %d commit %d: worst |h - float64| %.3g (bound %.1g)" % ("_lstm" if lstm else "", c["rows"], n, e, R.H_TOL))
    assert bad == [], bad
    return order


# (B, beam, L, H, C per layer, JH, step, tokens): every value of the lists in the issue of this file at least once --
# rows (3,4) (2,16) (1,1); step even / odd; tokens mixed / all blank / all label; L 5, 12, 300; H 64, 512, 1028; layers 1, 2, 4;
# C 48 (not a multiple of 64), 300 and 512 (4C > 256); joint off / JH 64, 640, 1280.  hyp_len and t_idx cycle through their
# lists inside every case (decode_step_common.prep_case).
PREP_CASES = [
    (3, 4, 12, 64, (48, 300), 64, 2, "mix"),
    (2, 16, 300, 1028, (48, 300, 64, 512), 1280, 3, "mix"),
    (3, 4, 300, 1028, (512, 64, 300, 48), 64, 2, "mix"),
    (2, 16, 12, 512, (300, 48), 640, 3, "mix"),
    (2, 16, 5, 512, (64,), 640, 2, "mix"),
    (1, 1, 5, 512, (64,), 0, 2, "label"),
    (1, 1, 12, 64, (48,), 640, 3, "blank"),
    (3, 4, 5, 512, (300, 64), 640, 3, "blank"),
    (2, 16, 12, 64, (512,), 0, 2, "label"),
    (3, 4, 12, 1028, (48, 64, 300, 512), 0, 3, "mix"),
]


@pytest.mark.parametrize("case", PREP_CASES, ids=lambda c: "B%dx%d-L%d-H%d-l%d-J%d-s%d-%s" % (c[0], c[1], c[2], c[3], len(c[4]), c[5], c[6], c[7]))
def test_prep_bit_for_bit(hip_device, case):
    B, beam, L, H, Cs, JH, step, tokens = case
    runs = []
    for _ in range(2):
        c = R.prep_case(B, beam, L, H, Cs, JH, step, tokens, seed=len(Cs))
        got, _ = _run_prep(c, hip_device)
        order = _check_prep(c, got)
        runs.append((got, order))
    # the slot order is free; whatever is indexed by row is the same in both runs
    for k in ("state", "anc", "t_idx", "X", "count") + (("pj", "h") if JH else ()):
        assert _same({k: runs[0][0][k]}, {k: runs[1][0][k]}) is None, k
    if tokens == "blank":
        assert len(runs[0][1]) == 0
    if L == 300:
        assert (np.minimum(c["hyp_len"], L - 1) >= 256).any()            # the second trip of the ancestry copy


LSTM_CASES = [      # (B, beam, layers, H, E, joint, step, tokens)
    (3, 4, 2, 260, 48, True, 2, "mix"),
    (2, 16, 4, 1024, 300, True, 3, "mix"),
    (1, 1, 1, 4, 48, False, 2, "label"),
    (3, 4, 1, 4, 300, True, 3, "blank"),
    (2, 16, 2, 260, 300, False, 2, "label"),
    (2, 16, 4, 4, 48, True, 2, "mix"),
]


@pytest.mark.parametrize("case", LSTM_CASES, ids=lambda c: "B%dx%d-l%d-H%d-E%d-j%d-s%d-%s" % c)
def test_prep_lstm_bit_for_bit(hip_device, case):
    runs = []
    for _ in range(2):
        c = R.prep_lstm_case(*case, seed=case[2])
        got, _ = _run_prep(c, hip_device, lstm=True)
        _check_prep(c, got, lstm=True)
        runs.append(got)
    for k in ("state", "t_idx", "count") + (("pj", "h") if c["JH"] else ()):
        assert _same({k: runs[0][k]}, {k: runs[1][k]}) is None, k


def test_prep_refusals(hip_device):
    """Return codes only: nothing is launched.  What the kernels cannot handle is refused (include/pika_decode_step.h)."""
    L = _lib()
    c = R.prep_case(3, 4, 12, 64, (48, 300), 64, 2)
    t = _up(c, hip_device)

    def rc(**kw):
        p = _prep_struct(c, t)
        for k, v in kw.items():
            obj, name = (p.joint, k[2:]) if k.startswith("j_") else (p, k)
            if isinstance(v, tuple):
                getattr(obj, name)[v[0]] = v[1]
            else:
                setattr(obj, name, v)
        return L.lib().pika_dstep_prep(ctypes.byref(p), _st())
    for L_ in (1, 4):
        assert rc(L=L_) == EINVAL
    assert rc(H=62) == EINVAL and rc(H=0) == EINVAL
    assert rc(j_JH=62) == EINVAL and rc(j_JH=0) == EINVAL and rc(j_T=0) == EINVAL
    assert rc(j_e_all=None) == EINVAL and rc(j_h=None) == EINVAL and rc(j_pj=(1, None)) == EINVAL
    for k in ("prev_k", "y", "hyp_len", "step_t", "t_idx", "emb", "node", "pos", "rowmap", "count"):
        assert rc(**{k: None}) == EINVAL, k
    assert rc(state=(1, None)) == EINVAL and rc(anc=(0, None)) == EINVAL and rc(X=(1, None)) == EINVAL and rc(A=(0, None)) == EINVAL
    assert rc(lda=(1, 5 * 300 - 4)) == EINVAL and rc(C=(0, 0)) == EINVAL
    assert rc(layers=0) == EINVAL and rc(layers=5) == EINVAL and rc(rows=0) == EINVAL and rc(beam=0) == EINVAL
    torch.cuda.synchronize()
    got = _down(t)
    assert _same(got, {k: v for k, v in _down(_up(c, hip_device)).items()}) is None     # and nothing was touched
    cl = R.prep_lstm_case(3, 4, 2, 260, 48, True, 2)
    tl = _up(cl, hip_device)

    def rcl(**kw):
        p = _prep_lstm_struct(cl, tl)
        for k, v in kw.items():
            obj, name = (p.joint, k[2:]) if k.startswith("j_") else (p, k)
            if isinstance(v, tuple):
                getattr(obj, name)[v[0]] = v[1]
            else:
                setattr(obj, name, v)
        return L.lib().pika_dstep_prep_lstm(ctypes.byref(p), _st())
    assert rcl(H=258) == EINVAL and rcl(lda=(0, 48 + 260 - 4)) == EINVAL and rcl(lda=(1, 2 * 260 - 4)) == EINVAL
    assert rcl(j_JH=258) == EINVAL and rcl(j_T=0) == EINVAL and rcl(j_e_all=None) == EINVAL and rcl(rowmap=None) == EINVAL


# ---- the LSTM cell ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("H", [4, 260])
def test_lstm_cell_against_float64(hip_device, H, scale):
    """c' = sigmoid(f) c + sigmoid(i) tanh(g), h' = sigmoid(o) tanh(c') within 4 ulp of the rounded float64 result + 1e-7;
    saturated gates (scale 30) stay finite; nothing but the blocks (2 layer, 2 layer + 1) of the rows rowmap[:m] changes."""
    L = _lib()
    layers, rows = 3, 12
    n_state, SP, ldg, ldn = rows + 2, layers * 2 * H, 4 * H + 4, 2 * H + 8
    rng = np.random.default_rng(H + int(scale))
    gates = np.full((rows, ldg), np.nan, dtype=np.float32)
    gates[:, :4 * H] = (rng.standard_normal((rows, 4 * H)) * scale).astype(np.float32)
    state0 = rng.standard_normal((n_state, SP)).astype(np.float32)
    rowmap = rng.permutation(n_state)[:rows].astype(np.int64)
    g_d, rm_d = torch.from_numpy(gates).to(hip_device), torch.from_numpy(rowmap).to(hip_device)
    worst = {"h": 0.0, "c": 0.0, "h32": 0.0, "c32": 0.0}
    for layer in (0, layers - 1):
        for m in (0, 1, rows - 3, rows + 5, None):
            for with_next in (False, True):
                mm = rows if m is None else min(m, rows)
                outs = []
                for _ in range(2):
                    st = torch.from_numpy(state0).to(hip_device)
                    nxt = torch.full((rows, ldn), R.SENT_F, device=hip_device)
                    md = None if m is None else torch.tensor([m], dtype=torch.int32, device=hip_device)
                    L.check(L.lib().pika_dstep_lstm_cell(g_d.data_ptr(), ldg, st.data_ptr(), SP, layer, rm_d.data_ptr(),
                                                         None if md is None else md.data_ptr(),
                                                         nxt.data_ptr() if with_next else None, ldn, rows, H, _st()), "cell")
                    torch.cuda.synchronize()
                    outs.append((st.cpu().numpy(), nxt.cpu().numpy()))
                assert R.bits_equal(outs[0][0], outs[1][0]) and R.bits_equal(outs[0][1], outs[1][1])
                st, nxt = outs[0]
                hs, cs = slice(2 * layer * H, (2 * layer + 1) * H), slice((2 * layer + 1) * H, (2 * layer + 2) * H)
                used = rowmap[:mm]
                h64, c64 = R.lstm_cell(gates[:mm, :4 * H], state0[used][:, cs])
                h32, c32 = R.lstm_cell(gates[:mm, :4 * H], state0[used][:, cs], dtype=np.float32)
                gh, gc = st[used][:, hs], st[used][:, cs]
                assert np.isfinite(gh).all() and np.isfinite(gc).all()
                if mm:
                    eh, ec = np.abs(gh - h64), np.abs(gc - c64)
                    worst["h"], worst["c"] = max(worst["h"], float((eh / R.cell_bound(h64)).max())), max(worst["c"], float((ec / R.cell_bound(c64)).max()))
                    worst["h32"] = max(worst["h32"], float((np.abs(h32 - h64) / R.cell_bound(h64)).max()))
                    worst["c32"] = max(worst["c32"], float((np.abs(c32 - c64) / R.cell_bound(c64)).max()))
                    assert (eh <= R.cell_bound(h64)).all() and (ec <= R.cell_bound(c64)).all(), (layer, m, eh.max(), ec.max())
                rest = state0.copy()
                rest[used, hs], rest[used, cs] = gh, gc
                assert R.bits_equal(st, rest)                            # other layers' blocks, other rows: untouched
                want_n = np.full((rows, ldn), R.SENT_F, dtype=np.float32)
                if with_next:
                    want_n[:mm, :H] = gh
                assert R.bits_equal(nxt, want_n)
    print("lstm_cell H %d scale %g: worst error / (4 ulp + 1e-7): h %.3f c %.3f (fp32 numpy restatement: h %.3f c %.3f)"
          % (H, scale, worst["h"], worst["c"], worst["h32"], worst["c32"]))
    lib = L.lib()
    assert lib.pika_dstep_lstm_cell(g_d.data_ptr(), 4 * H - 4, g_d.data_ptr(), SP, 0, rm_d.data_ptr(), None, None, 0, rows, H, _st()) == EINVAL
    assert lib.pika_dstep_lstm_cell(g_d.data_ptr(), ldg, g_d.data_ptr(), SP, layers, rm_d.data_ptr(), None, None, 0, rows, H, _st()) == EINVAL


# ---- attention -------------------------------------------------------------------------------------------------------------

def _attention(c, t, anc, rowmap, md, out, L_=None, d=None, heads=None, ldkvq=None):
    L = _lib()
    d = c["d"] if d is None else d
    return L.lib().pika_dstep_attention(t["kvq"].data_ptr(), 3 * c["d"] if ldkvq is None else ldkvq, t["Kc"].data_ptr(),
                                        t["Vc"].data_ptr(), anc.data_ptr(), c["L"], t["pos"].data_ptr(), t["node"].data_ptr(),
                                        None if rowmap is None else rowmap.data_ptr(), None if md is None else md.data_ptr(),
                                        c["rows"], c["L"] if L_ is None else L_, d, c["heads"] if heads is None else heads,
                                        out.data_ptr(), _st())


@pytest.mark.parametrize("d,heads", [(64, 4), (64, 16), (256, 4), (512, 8), (1024, 16), (1024, 4)])
def test_attention_against_float64(hip_device, d, heads):
    """Positions {0, 1, G-1, G, 8G-1, 8G, 8G+1, L-1, L+2} (groups without a position, one full unroll, one more, the clamp),
    rowmap NULL and a permutation, *m_dev < rows; the new keys / values land in the caches bit for bit, nothing else moves."""
    L = _lib()
    c = R.attention_case(d, heads)
    rows = c["rows"]
    G = R.att_group(d)
    assert 4 * (G * d + 2 * G * heads + c["L"]) <= 64 * 1024
    for which, m in (("id", None), ("perm", rows - 5), ("perm", rows + 4)):
        anc_np = c["anc_id"] if which == "id" else c["anc_perm"]
        rm_np = None if which == "id" else c["rowmap"]
        mm = rows if m is None else min(m, rows)
        want, Kw, Vw = R.attention_ref(c, anc_np, rm_np, mm)
        outs = []
        for _ in range(2):
            t = _up(c, hip_device)
            anc = torch.from_numpy(anc_np).to(hip_device)
            rm = None if rm_np is None else t["rowmap"]
            md = None if m is None else torch.tensor([m], dtype=torch.int32, device=hip_device)
            out = torch.full((rows, d), R.SENT_F, device=hip_device)
            L.check(_attention(c, t, anc, rm, md, out), "pika_dstep_attention")
            torch.cuda.synchronize()
            outs.append((out.cpu().numpy(), t["Kc"].cpu().numpy(), t["Vc"].cpu().numpy()))
        for a, b in zip(*outs):
            assert R.bits_equal(a, b)
        out, Kg, Vg = outs[0]
        e, bound = R.att_error(out[:mm], want[:mm]), R.att_bound(want, mm)
        print("attention d %d heads %d G %d %s m %s: worst %.3g bound %.3g" % (d, heads, G, which, m, e, bound))
        assert e <= bound
        assert (out[mm:] == R.SENT_F).all()
        assert R.bits_equal(Kg, Kw) and R.bits_equal(Vg, Vw)             # new rows = the k / v thirds; every other row untouched


def test_attention_refusals(hip_device):
    c = R.attention_case(64, 4)
    t = _up(c, hip_device)
    anc = torch.from_numpy(c["anc_id"]).to(hip_device)
    out = torch.full((c["rows"], 64), R.SENT_F, device=hip_device)
    assert _attention(c, t, anc, None, None, out, heads=5) == EINVAL               # d % heads
    assert _attention(c, t, anc, None, None, out, d=2048, heads=8) == EINVAL
    assert _attention(c, t, anc, None, None, out, d=96, heads=4) == EINVAL         # 256 % (d / 4)
    assert _attention(c, t, anc, None, None, out, ldkvq=3 * 64 + 2) == EINVAL
    assert _attention(c, t, anc, None, None, out, L_=20000) == ETOOBIG             # LDS: 4 (G d + 2 G heads + L) > 64 KB
    torch.cuda.synchronize()
    assert bool((out == R.SENT_F).all()) and R.bits_equal(t["Kc"].cpu().numpy(), c["Kc"])


# ---- pika_dgemm as the search launches it --------------------------------------------------------------------------------------

D_MODEL, D_FF, JH2, M_BUF = 512, 2048, 1280, 1024
M_DEVS = (0, 1, 31, 32, 33, 170)
FORMS = {      # FusedSearch._prednet / _joint_rows at the recipe's widths
    "conv": dict(N=D_MODEL, K=5 * D_MODEL, bias=1, relu=1),                             # PIPE rounds
    "qkv": dict(N=3 * D_MODEL, K=D_MODEL, ln=1, bias=1),                                # 32-column tiles
    "final": dict(N=D_MODEL, K=D_MODEL, bias=1, res=1),
    "w_1": dict(N=D_FF, K=D_MODEL, ln=1, bias=1, relu=1),
    "w_2_next": dict(N=D_MODEL, K=D_FF, bias=1, res=1, view=1, scatter=1),              # PIPE rounds
    "w_2_state": dict(N=D_MODEL, K=D_FF, bias=1, res=1, crow=1),
    "joint": dict(N=JH2, K=D_MODEL, gate=1, ln=1, rowlist=1),
    "k768": dict(N=D_MODEL, K=768, bias=1),                                             # one round on 8 waves, no LayerNorm
    "k1024": dict(N=D_MODEL, K=1024, bias=1),
    "w_1_all_rows": dict(N=D_FF, K=D_MODEL, ln=1, bias=1, relu=1, ms=(M_BUF,)),          # workgroups walk several tiles each
    "n1048": dict(N=1048, K=D_MODEL, bias=1, ms=(33, 170)),                             # tail column tile of a 2-tile group
    "n1032": dict(N=1032, K=D_MODEL, bias=1, ms=(33, 170)),                             # a group whose second tile does not exist
}
GEMM_CASES = [(f, t) for f in ("conv", "final", "joint") for t in (1, 2, 3, 4)] + \
             [(f, 3) for f in FORMS if f not in ("conv", "final", "joint")]


@pytest.mark.parametrize("form,terms", GEMM_CASES, ids=lambda v: str(v))
def test_dgemm_as_the_search_launches_it(hip_device, form, terms):
    from pika_amd.decoder.fused_step import DGemm, PackedWeight, DG_RELU, DG_GATE, DG_FEW_ROWS
    L = _lib()
    dev = hip_device
    f = FORMS[form]
    N, K, M = f["N"], f["K"], M_BUF
    ms = f.get("ms", M_DEVS)
    top = max(ms)
    g = torch.Generator().manual_seed(N + K + terms)
    lda = K + 32
    A_all = torch.randn(M, K, generator=g)
    if f.get("ln"):
        A_all = A_all * 3 + 0.7
    A_all = A_all.to(dev)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(N, generator=g).to(dev) if f.get("bias") else None
    res_all = torch.randn(M, N, generator=g).to(dev) if f.get("res") else None
    gamma = (1 + 0.2 * torch.randn(K, generator=g)).to(dev)
    beta = (0.1 * torch.randn(K, generator=g)).to(dev)
    perm = torch.randperm(M, generator=g)
    B, beam, T = M // 16, 16, 11
    e_all = torch.randn(B * T, N, generator=g).to(dev)
    t_idx = torch.randint(-1, T + 2, (M,), generator=g)
    t_idx[perm[:4]] = torch.tensor([-1, T + 1, 0, T - 1])
    t_idx = t_idx.to(dev)
    crow = torch.randperm(M, generator=g).to(dev) if f.get("crow") else None
    cap = M + 7
    node = torch.randperm(cap, generator=g)[:M].to(dev)
    nan_row = int(perm[M - 1])
    # launch row e stands for buffer row rows_of[e]
    rows_of = (perm if f.get("rowlist") else torch.arange(M)).to(dev)
    pw = PackedWeight(W, terms, interleave2=bool(f.get("gate")))
    # ---- float64 once, for the first `top` launch rows
    used = rows_of[:top]
    a64 = A_all[used].double()
    if f.get("ln"):
        a64 = R.layer_norm(A_all[used], gamma, beta, 1e-6)
    z = a64 @ W.double().t()
    if f.get("gate"):
        want = R.gate(z, e_all, t_idx, used, beam, T)
        want2 = R.interleave(z)
        zm = R.model_product(a64.float(), W, terms).float().double()         # the arithmetic model: accumulators in fp32
        e_model = R.err(R.gate(zm, e_all, t_idx, used, beam, T).float(), want)
        assert R.err(R.gate(z, e_all, t_idx, used, beam, T, slot_rows=True), want) > 10 * R.H_TOL      # (the rowlist mutant)
    else:
        if bias is not None:
            z = z + bias.double()
        if f.get("relu"):
            z = torch.relu(z)
        if res_all is not None:
            z = z + res_all[used].double()
        want = z
    ldc = (N // 2 if f.get("gate") else N) + 8
    Nc = N // 2 if f.get("gate") else N
    worst, worst2 = 0.0, 0.0
    for m in ms:
        act = rows_of[:m]
        A = torch.full((M, lda), float("nan"), device=dev)               # rows outside the launch, pad columns: NaN
        A[act, :K] = A_all[act]
        res = None
        if res_all is not None:
            res = torch.full((M, N), float("nan"), device=dev)
            res[act] = res_all[act]
        rl = None
        if f.get("rowlist"):
            off = 5
            rl = torch.full((off + M,), nan_row, dtype=torch.int32, device=dev)      # never followed: before rowoff, beyond m
            rl[off:off + m] = act.to(torch.int32)
            off_d = torch.tensor([off], dtype=torch.int32, device=dev)
        md = torch.tensor([m], dtype=torch.int32, device=dev)
        outs = []
        for _ in range(2):
            if f.get("view"):
                buf = torch.full((M, 5 * D_MODEL), R.SENT_F, device=dev)   # the next layer's conv matrix: its fifth tap block
                C, ldc_ = buf[:, 4 * D_MODEL:], 5 * D_MODEL
            else:
                buf = torch.full((M, ldc), R.SENT_F, device=dev)
                C, ldc_ = buf, ldc
            C2 = None
            d = DGemm()
            if f.get("scatter"):
                C2 = torch.full((cap, N), R.SENT_F, device=dev)
                d.C2, d.ldc2, d.node, d.skip_node = C2.data_ptr(), N, node.data_ptr(), -1
            if f.get("gate"):
                C2 = torch.full((M, N + 8), R.SENT_F, device=dev)
                d.C2, d.ldc2 = C2.data_ptr(), N + 8
                d.e_all, d.t_idx, d.T, d.beam = e_all.data_ptr(), t_idx.data_ptr(), T, beam
            d.A, d.lda, d.W = A.data_ptr(), lda, pw.buf.data_ptr()
            d.bias = None if bias is None else bias.data_ptr()
            if res is not None:
                d.res, d.ldr = res.data_ptr(), N
            d.C, d.ldc = C.data_ptr(), ldc_
            d.M, d.N, d.K, d.terms = M, N, K, terms
            d.flags = DG_FEW_ROWS | (DG_RELU if f.get("relu") else 0) | (DG_GATE if f.get("gate") else 0)
            d.m_dev = md.data_ptr()
            d.crow = None if crow is None else crow.data_ptr()
            if rl is not None:
                d.rowlist, d.rowoff_dev = rl.data_ptr(), off_d.data_ptr()
            if f.get("ln"):
                d.ln_gamma, d.ln_beta, d.ln_eps = gamma.data_ptr(), beta.data_ptr(), 1e-6
            L.check(L.lib().pika_dgemm(ctypes.byref(d), _st()), "pika_dgemm %s" % form)
            torch.cuda.synchronize()
            outs.append((buf, C, C2))
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))      # summed in wave order
        if C2 is not None:
            assert torch.equal(outs[0][2].view(torch.int32), outs[1][2].view(torch.int32))
        buf, C, C2 = outs[0]
        out_rows = act if crow is None else crow[act]
        if m:
            scale = float(want[:m].abs().max())
            e = R.err(C[out_rows][:, :Nc], want[:m])
            if f.get("gate"):
                bound = R.H_TOL if terms == 3 else R.MARGIN * e_model
                worst = max(worst, e / bound)
                assert e < bound, (form, terms, m, e, bound)
                s2 = float(want2[:m].abs().max())
                e2 = R.err(C2[out_rows][:, :N], want2[:m])
                worst2 = max(worst2, e2 / s2)
                assert e2 <= R.GEMM_TOL[terms] * s2, (form, terms, m, e2 / s2)
            else:
                worst = max(worst, e / scale)
                assert e <= R.GEMM_TOL[terms] * scale, (form, terms, m, e / scale)
                if f.get("scatter"):
                    e2 = R.err(C2[node[act]], want[:m])
                    assert e2 <= R.GEMM_TOL[terms] * scale
        # nothing else was written: the rows outside the launch, the pad columns, the rest of a wider buffer
        keep = torch.ones_like(buf, dtype=torch.bool)
        c_lo = 4 * D_MODEL if f.get("view") else 0
        if m:
            keep[out_rows, c_lo:c_lo + Nc] = False
        assert bool((buf[keep] == R.SENT_F).all()), (form, m)
        if C2 is not None:
            keep2 = torch.ones_like(C2, dtype=torch.bool)
            if m:
                keep2[node[act] if f.get("scatter") else out_rows, :N] = False
            assert bool((C2[keep2] == R.SENT_F).all()), (form, m)
    if f.get("gate"):
        print("dgemm %s terms %d: model error %.3g, worst h error / bound %.3f, worst raw accumulator error %.3g (tolerance %.1g)"
              % (form, terms, e_model, worst, worst2, R.GEMM_TOL[terms]))
    else:
        print("dgemm %s terms %d: worst error / |want|max %.3g (tolerance %.1g)" % (form, terms, worst, R.GEMM_TOL[terms]))


# ---- every host route of pika_dgemm, at the smallest shape that reaches it ------------------------------------------------
# (M, N, K); no m_dev and no PIKA_DG_FEW_ROWS: the route follows from the shape alone.  KT = ceil(K / 32).
ROUTES = {
    "sk_kw4": (16, 48, 512),                    # split reduction, 4 waves, one request round (KT = 16)
    "sk_kw8": (16, 48, 544),                    # 8 waves, one round (KT = 17)
    "sk_kw8_pipelined": (16, 48, 1056),         # 8 waves, rounds of 2 k-tiles each (KT = 33 > 32)
    "sk_wn2": (16, 1024, 64),                   # 32-column tiles
    "sk_ln": (16, 48, 1024),                    # LayerNorm inside the launch, at the largest K it accepts
    "tiled32": (257, 48, 64),                   # more than 256 rows: the 32-row tiles
    "tiled64": (1024, 2032, 32),                # 16 row tiles x 32 column groups = 512: the 64-row tiles
    "wide": (257, 2048, 32),                    # N >= 2048: 64 x 128 tiles
    "sk_too_long": (16, 48, 4128),              # KT = 129 > 128: few rows, but the tiled kernel
    "k_padded": (16, 48, 30),                   # K % 4 != 0: the reduction runs over ceil32(K) zero-padded columns
}
ROUTE_CASES = [("sk_kw4", t) for t in (1, 2, 3, 4)] + [(r, t) for r in ROUTES if r != "sk_kw4" for t in (3, 4)]


def run_route(dev, route, terms, K=None):
    """One launch on the route's shape with fixed seeds -> (return code, the whole output buffer, its C view, float64 want)."""
    from pika_amd.decoder.fused_step import PackedWeight, dgemm_args
    M, N, K0 = ROUTES[route]
    K = K or K0
    ln = route == "sk_ln"
    g = torch.Generator().manual_seed(M + N + K + terms)
    Kp = (K + 31) // 32 * 32
    A = torch.full((M, Kp + 32), float("nan"))                      # beyond the columns a launch may read: NaN
    A[:, :K] = torch.randn(M, K, generator=g) * (3 if ln else 1) + (0.7 if ln else 0)
    if K % 4:
        A[:, K:Kp] = 0                                               # (the caller zero-pads, as the header says)
    A = A.to(dev)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(K, generator=g)).to(dev), (0.1 * torch.randn(K, generator=g)).to(dev)
    a64 = R.layer_norm(A[:, :K], gamma, beta, 1e-6) if ln else A[:, :K].double()
    want = a64 @ W.double().t() + bias.double()
    pw = PackedWeight(W, terms)
    buf = torch.full((M + 2, N + 8), R.SENT_F, device=dev)          # a sentinel row above and below, 8 pad columns
    C = buf[1:M + 1]
    d = dgemm_args(A, Kp + 32, pw, bias, C, N + 8, M, ln=(gamma, beta, 1e-6) if ln else None)
    rc = _lib().lib().pika_dgemm(ctypes.byref(d), _st())
    torch.cuda.synchronize()
    return rc, buf, C, want


@pytest.mark.parametrize("route,terms", ROUTE_CASES, ids=lambda v: str(v))
def test_dgemm_host_routes(hip_device, route, terms):
    M, N, K = ROUTES[route]
    outs = []
    for _ in range(2):
        rc, buf, C, want = run_route(hip_device, route, terms)
        assert rc == 0
        outs.append(buf)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    scale = float(want.abs().max())
    e = R.err(C[:, :N], want)
    print("dgemm route %s terms %d: error / |want|max %.3g (tolerance %.1g)" % (route, terms, e / scale, R.GEMM_TOL[terms]))
    assert e <= R.GEMM_TOL[terms] * scale, (route, terms, e / scale)
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[1:M + 1, :N] = False
    assert bool((buf[keep] == R.SENT_F).all()), route


def test_dgemm_ln_refuses_k_beyond_1024(hip_device):
    rc, buf, _, _ = run_route(hip_device, "sk_ln", 3, K=1056)
    assert rc == EINVAL and bool((buf == R.SENT_F).all())


# ---- stop ------------------------------------------------------------------------------------------------------------------

def test_stop_leaves_every_buffer_alone(hip_device):
    """*stop != 0: prep, the LSTM prep and the advance return without touching anything (the advance sets sync[4], as the
    header says); with stop cleared the same calls do their work."""
    from test_decode_step_gpu import _beam_inputs
    from pika_amd.decoder.fused_step import PackedWeight
    L = _lib()
    lib = L.lib()
    dev = hip_device
    stop = torch.ones(1, dtype=torch.int32, device=dev)
    for lstm, c in ((False, R.prep_case(3, 4, 12, 64, (48, 300), 64, 2)), (True, R.prep_lstm_case(3, 4, 2, 260, 48, True, 2))):
        stop.fill_(1)
        before = _down(_up(c, dev))
        got, (t, p, fn) = _run_prep(c, dev, lstm=lstm, stop=stop)
        assert _same(got, before) is None
        stop.zero_()
        L.check(fn(ctypes.byref(p), _st()), "prep")
        after = _down(t)
        assert int(after["count"][c["src"]]) == len(R.committing_rows(c)) > 0
        _check_prep(c, after, lstm=lstm)
    # the advance, on the inputs of the smallest case of test_fc2_logits_advance_equals_the_materialised_logits_advance
    V, K, Hd, terms, B, L_, blk, S_steps, sm = 100, 4, 64, 3, 3, 12, 0, 40, 0.8
    g = torch.Generator().manual_seed(V + K + terms)
    R_ = B * K
    h = torch.randn(R_, Hd, generator=g).to(dev)
    W = (torch.randn(V, Hd, generator=g) * 0.5).to(dev)
    bias = torch.randn(V, generator=g).to(dev)
    pw = PackedWeight(W, terms)
    splits = lib.pika_dfc2_splits(V)
    ldl = splits * lib.pika_dfc2_cols_per_split()
    b = dict(pmax=torch.empty(R_ * splits, device=dev), psum=torch.empty(R_ * splits, device=dev),
             slog=torch.full((R_, ldl), 7.0, device=dev))
    L.check(lib.pika_dfc2_logits(h.data_ptr(), Hd, pw.buf.data_ptr(), bias.data_ptr(), R_, V, Hd, terms, sm, b["pmax"].data_ptr(),
                                 b["psum"].data_ptr(), b["slog"].data_ptr(), ldl, _st()), "pika_dfc2_logits")
    b.update(_beam_inputs(B, K, V, L_, torch.Generator().manual_seed(9), dev, False))
    fin_cap = K * S_steps + 1
    i64 = dict(dtype=torch.long, device=dev)
    b.update(ks_hist=torch.zeros(S_steps, B, K, **i64), ys_hist=torch.zeros(S_steps + 1, B, K, **i64),
             step_t=torch.full((1,), 3, **i64), fin_score=torch.zeros(B, fin_cap, device=dev),
             fin_step=torch.zeros(B, fin_cap, **i64), fin_k=torch.zeros(B, fin_cap, **i64), fin_n=torch.zeros(B, **i64),
             prev_k=torch.full((B, K), R.SENT_I, **i64), y_raw=torch.full((B, K), R.SENT_I, **i64),
             max_hyp=torch.zeros(1, **i64),                              # (an atomic max: the caller zeroes it)
             sync=torch.tensor([0, 0, 0, 0, 0, 3, 4, 0], dtype=torch.int32, device=dev))
    stop.fill_(1)

    def advance():
        L.check(lib.pika_beam_advance_logits(
            b["pmax"].data_ptr(), b["psum"].data_ptr(), b["slog"].data_ptr(), ldl, splits, b["scores"].data_ptr(),
            b["lm_scores"].data_ptr(), 1.0, b["y"].data_ptr(), b["t_idx"].data_ptr(), b["num_frames"].data_ptr(),
            b["max_len"].data_ptr(), b["hyp"].data_ptr(), b["hyp_len"].data_ptr(), L_, b["ks_hist"].data_ptr(),
            b["ys_hist"].data_ptr(), b["step_t"].data_ptr(), b["eos"].data_ptr(), b["fin_score"].data_ptr(),
            b["fin_step"].data_ptr(), b["fin_k"].data_ptr(), b["fin_n"].data_ptr(), fin_cap, b["prev_k"].data_ptr(),
            b["y_raw"].data_ptr(), B, K, V, blk, 1, K, stop.data_ptr(), b["max_hyp"].data_ptr(), b["sync"].data_ptr(), _st()),
            "pika_beam_advance_logits")
        torch.cuda.synchronize()
    before = {k: v.clone() for k, v in b.items()}
    advance()
    assert int(stop) == 1
    for k, v in b.items():
        if k == "sync":
            assert v.tolist() == [0, 0, 0, 0, 1, 3, 4, 0]                # the one permitted change: sync[4]
        else:
            assert R.bits_equal(v.cpu().numpy(), before[k].cpu().numpy()), k
    stop.zero_()
    advance()
    assert int(b["step_t"]) == 4 and int(b["max_hyp"]) == int(b["hyp_len"].max()) > 0 and not torch.equal(b["prev_k"], before["prev_k"])
    assert b["sync"][5:7].tolist() in ([0, 4], [3, 0])                   # the next step's compact-row counter was zeroed
