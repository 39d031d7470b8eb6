"""The per-step kernels of the batch beam search (include/pika_decode_step.h) restated in plain numpy / torch on the CPU, for
tests/test_decode_step_kernels_gpu.py.  Imports nothing from pika_amd.

  prep_case / prep_ref            pika_dstep_prep: the header comment ("prediction-network bookkeeping of one step"), exact
  prep_lstm_case / prep_lstm_ref  pika_dstep_prep_lstm, exact
  lstm_cell                       c' = sigmoid(f) c + sigmoid(i) tanh(g), h' = sigmoid(o) tanh(c'), float64 or fp32
  attention_case / attention_ref  softmax attention of the new position over anc[row, 0:pos] + the new position, float64
  layer_norm / split_terms / model_product / gate   the products of pika_dgemm: float64, and the ARITHMETIC MODEL of a term
                                  count (operands split into the kernel's terms, the kernel's set of products, summed in float64)
  MUTANTS                         each one line away from a reference: what a subtly wrong kernel would compute

Buffers a launch must not write carry a sentinel (SENT_F / SENT_I); indices a launch must never follow point at an in-bounds
row of NaN (`nan_node`), so that a forbidden read shows in the result without any fault.  The comparators (`*_mismatches`)
are shared by the GPU test (kernel output against reference) and the CPU test (mutant against reference).
tests/test_decode_step_refs.py checks all of this without a GPU."""
import numpy as np
import torch

SENT_F = 7.0
SENT_I = -77
H_TOL = 2e-6                # joint hidden of prep / the gate epilogue at 3 terms against float64 (tests/test_decode_step_gpu.py)
ATT_TOL = 2e-5              # x max(1, |want|max): tests/test_decode.py test_incremental_attention_kernel
GEMM_TOL = {1: 2e-2, 2: 2e-4, 3: 3e-6, 4: 5e-6}     # x |want|max, per term count (tests/test_decode_step_gpu.py)
MARGIN = 4.0                # kernel against the arithmetic model: the order of the fp32 sums differs (tests/lstm_common.py)

PREP_MUTANTS = ("child_taps", "pos_unclamped", "node_off_row", "frame_before_increment")
ATT_MUTANTS = ("no_new_pos", "no_scale")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def hyp_lens(L):
    """every number of real taps (0..4), one beyond, and the clamp at L - 1"""
    return [0, 1, 2, 3, 4, 5, L - 1, L, L + 3]


def _tokens(rng, rows, mode, blk, vocab):
    lab = rng.integers(blk + 1, vocab + 1, size=rows)
    if mode == "blank":
        return np.full(rows, blk, dtype=np.int64)
    if mode == "label":
        return lab.astype(np.int64)
    kind = np.array([(i + int(rng.integers(0, 3))) % 3 for i in range(rows)])
    if rows >= 3:
        kind[:3] = rng.permutation(3)           # every kind at least once
    return np.where(kind == 0, blk, np.where(kind == 1, lab, -1)).astype(np.int64)


def _parents(rng, B, beam):
    """several children per parent, parents nobody inherits: only the lower half of a beam is ever a parent"""
    return rng.integers(0, max(1, (beam + 1) // 2), size=B * beam).astype(np.int64)


def _joint_buffers(rng, c, rows, B, JH, T, src):
    c["JH"], c["T"] = JH, T
    if not JH:
        return
    pj = [None, None]
    pj[src] = rng.standard_normal((rows, 2 * JH)).astype(np.float32)
    pj[src ^ 1] = np.full((rows, 2 * JH), SENT_F, dtype=np.float32)
    c["pj"] = pj
    c["h"] = np.full((rows, JH), SENT_F, dtype=np.float32)
    c["e_all"] = rng.standard_normal((B * T, 2 * JH)).astype(np.float32)
    c["rowmap32"] = np.full(rows, SENT_I, dtype=np.int32)


def prep_case(B, beam, L, H, Cs, JH, step, tokens="mix", seed=0, T=7, vocab=23, blk=0, pad=12):
    """Every buffer of one pika_dstep_prep launch as numpy arrays (inputs random, outputs at their sentinels)."""
    rng = np.random.default_rng(1000 * seed + 10 * L + H + B)
    rows, layers = B * beam, len(Cs)
    src = step & 1
    n_old = 1 + step * rows                      # node ids of earlier steps: [0, n_old); this step's: n_old + r
    cap = n_old + rows + 3
    c = dict(B=B, beam=beam, rows=rows, L=L, H=H, Cs=tuple(Cs), layers=layers, blk=blk, step=step, src=src, cap=cap,
             zero_node=cap - 3, dump_node=cap - 2, nan_node=cap - 1, n_old=n_old)
    c["prev_k"] = _parents(rng, B, beam)
    c["y"] = _tokens(rng, rows, tokens, blk, vocab)
    hl = hyp_lens(L)
    c["hyp_len"] = np.array([hl[(i + seed) % len(hl)] for i in range(rows)], dtype=np.int64)
    if tokens == "mix" and rows >= len(hl):      # the clamp meets a committing row and a blank one
        c["y"][np.nonzero(c["hyp_len"] == L + 3)[0][0]] = blk + 1
        c["y"][np.nonzero(c["hyp_len"] == L)[0][0]] = blk
    tl = [-1, 0, T - 1, T + 2]
    c["t_idx"] = np.array([tl[(i // 2 + seed) % 4] for i in range(rows)], dtype=np.int64)
    c["step_t"] = np.array([step], dtype=np.int64)
    state = [None, None]
    state[src] = rng.standard_normal((rows, H)).astype(np.float32)
    state[src ^ 1] = np.full((rows, H), SENT_F, dtype=np.float32)
    c["state"] = state
    # ancestry of the parents: valid nodes up to the largest position one of the parent's children reads, NaN rows beyond
    pos = np.minimum(c["hyp_len"], L - 1)
    pr = (np.arange(rows) // beam) * beam + c["prev_k"]
    reach = np.full(rows, -1, dtype=np.int64)
    np.maximum.at(reach, pr, pos)
    a_src = rng.integers(0, n_old, size=(rows, L)).astype(np.int64)
    a_src[np.arange(L)[None, :] > reach[:, None]] = c["nan_node"]
    anc = [None, None]
    anc[src] = a_src
    anc[src ^ 1] = np.full((rows, L), SENT_I, dtype=np.int64)
    c["anc"] = anc
    c["emb"] = rng.standard_normal((vocab + 1, Cs[0])).astype(np.float32)
    c["X"], c["A"], c["lda"] = [], [], []
    for C in Cs:
        X = rng.standard_normal((cap, C)).astype(np.float32)
        X[n_old:n_old + rows] = SENT_F           # this step's nodes
        X[c["zero_node"]] = 0.0
        X[c["nan_node"]] = np.nan
        c["X"].append(X)
        c["lda"].append(5 * C + pad)
        c["A"].append(np.full((rows, 5 * C + pad), SENT_F, dtype=np.float32))
    for k in ("node", "pos", "rowmap"):
        c[k] = np.full(rows, SENT_I, dtype=np.int64)
    cnt = np.full(2, SENT_I, dtype=np.int32)
    cnt[src] = 0                                 # the caller zeroes the counter of this parity
    c["count"] = cnt
    _joint_buffers(rng, c, rows, B, JH, T, src)
    return c


def committing_rows(c):
    return np.nonzero(c["y"] > c["blk"])[0]


def _carry_joint(c, w, pr, t_frame, commit):
    """pj[dst][r] = pj[src][parent]; h for the rows that did not commit (float64), from the frame t_frame[r]"""
    if not c["JH"]:
        return
    JH, T, beam, src = c["JH"], c["T"], c["beam"], c["src"]
    rows = c["rows"]
    pj = [p.copy() for p in c["pj"]]
    pj[src ^ 1] = c["pj"][src][pr]
    w["pj"] = pj
    z = pj[src ^ 1].astype(np.float64)
    e = c["e_all"][(np.arange(rows) // beam) * T + np.clip(t_frame, 0, T - 1)].astype(np.float64)
    h = np.tanh(z[:, 0::2] + e[:, :JH]) * _sigmoid(z[:, 1::2] + e[:, JH:])
    h[commit] = SENT_F
    w["h64"] = h


def prep_ref(c, order, mutant=None):
    """The buffers after the launch, slots handed out in `order` (the committing rows in the order the launch took them)."""
    rows, beam, L, src = c["rows"], c["beam"], c["L"], c["src"]
    dst = src ^ 1
    r_ = np.arange(rows)
    pr = (r_ // beam) * beam + c["prev_k"]
    tok = c["y"]
    commit = tok > c["blk"]
    pos = c["hyp_len"].copy() if mutant == "pos_unclamped" else np.minimum(c["hyp_len"], L - 1)
    node = 1 + c["step"] * rows + r_ + (1 if mutant == "node_off_row" else 0)
    w = dict(state=[s.copy() for s in c["state"]], anc=[a.copy() for a in c["anc"]], X=[x.copy() for x in c["X"]],
             A=[a.copy() for a in c["A"]], node=c["node"].copy(), pos=c["pos"].copy(), rowmap=c["rowmap"].copy(),
             count=c["count"].copy())
    w["state"][dst] = c["state"][src][pr]
    a_src = c["anc"][src]
    flat = a_src.reshape(-1)                     # (the unclamped mutant walks off its row, like the kernel would)
    valid = np.zeros((rows, L), dtype=bool)
    for r in range(rows):
        p = int(min(pos[r], L - 1))
        w["anc"][dst][r, :p + 1] = a_src[pr[r], :p + 1]
        valid[r, :p + 1] = True
        if commit[r]:
            w["anc"][dst][r, p] = node[r]
    w["anc_valid"] = valid
    t_new = c["t_idx"] + (tok == c["blk"])
    w["t_idx"] = t_new
    order = np.asarray(order, dtype=np.int64)
    n = len(order)
    w["count"][src] += n
    w["rowmap"][:n] = order
    w["node"][:n] = node[order]
    w["pos"][:n] = pos[order]
    if c["JH"]:
        w["rowmap32"] = c["rowmap32"].copy()
        w["rowmap32"][:n] = order
    for slot, r in enumerate(order):
        via = r if mutant == "child_taps" else pr[r]
        taps = []
        for j in range(4):
            q = int(pos[r]) - 4 + j
            taps.append(c["zero_node"] if q < 0 else int(flat[min(via * L + q, flat.size - 1)]))
        x = c["emb"][tok[r]]
        for l, C in enumerate(c["Cs"]):
            for j in range(4):
                w["A"][l][slot, j * C:(j + 1) * C] = c["X"][l][taps[j]]
        w["A"][0][slot, 4 * c["Cs"][0]:5 * c["Cs"][0]] = x
        w["X"][0][node[r]] = x
    _carry_joint(c, w, pr, c["t_idx"] if mutant == "frame_before_increment" else t_new, commit)
    return w


def _exact(bad, name, got, want):
    if not bits_equal(got, want):
        bad.append(name)


def prep_mismatches(got, want, c):
    """Names of the buffers of `got` (kernel output, or a mutant's) that differ from the reference `want`."""
    bad = []
    src, dst = c["src"], c["src"] ^ 1
    _exact(bad, "state_src", got["state"][src], want["state"][src])
    _exact(bad, "state_dst", got["state"][dst], want["state"][dst])
    _exact(bad, "anc_src", got["anc"][src], want["anc"][src])
    v = want["anc_valid"]                        # positions > pos are documented as never read: not compared
    _exact(bad, "anc_dst", got["anc"][dst][v], want["anc"][dst][v])
    for k in ("t_idx", "node", "pos", "rowmap", "count"):
        _exact(bad, k, got[k], want[k])
    for l in range(c["layers"]):
        _exact(bad, "A[%d]" % l, got["A"][l], want["A"][l])
        _exact(bad, "X[%d]" % l, got["X"][l], want["X"][l])
    if c["JH"]:
        _exact(bad, "rowmap32", got["rowmap32"], want["rowmap32"])
        _exact(bad, "pj_src", got["pj"][src], want["pj"][src])
        _exact(bad, "pj_dst", got["pj"][dst], want["pj"][dst])
        if h_error(got, want) >= H_TOL:
            bad.append("h")
    return bad


def h_error(got, want):
    h = got["h64"] if "h64" in got else got["h"].astype(np.float64)
    e = np.abs(h - want["h64"])
    return float(np.where(np.isnan(e), np.inf, e).max())


# ---- LSTM prediction net ---------------------------------------------------------------------------------------------------

def prep_lstm_case(B, beam, layers, H, E, joint, step, tokens="mix", seed=0, T=7, vocab=23, blk=0, pad=8):
    rng = np.random.default_rng(1000 * seed + 10 * E + H + B)
    rows, src = B * beam, step & 1
    SP = layers * 2 * H
    c = dict(B=B, beam=beam, rows=rows, layers=layers, H=H, E=E, blk=blk, step=step, src=src, SP=SP)
    c["prev_k"] = _parents(rng, B, beam)
    c["y"] = _tokens(rng, rows, tokens, blk, vocab)
    tl = [-1, 0, T - 1, T + 2]
    c["t_idx"] = np.array([tl[(i // 2 + seed) % 4] for i in range(rows)], dtype=np.int64)
    c["step_t"] = np.array([step], dtype=np.int64)
    state = [None, None]
    state[src] = rng.standard_normal((rows, SP)).astype(np.float32)
    state[src ^ 1] = np.full((rows, SP), SENT_F, dtype=np.float32)
    c["state"] = state
    c["emb"] = rng.standard_normal((vocab + 1, E)).astype(np.float32)
    c["lda"] = [E + H + pad] + [2 * H + pad] * (layers - 1)
    c["A"] = [np.full((rows, w), SENT_F, dtype=np.float32) for w in c["lda"]]
    c["rowmap"] = np.full(rows, SENT_I, dtype=np.int64)
    cnt = np.full(2, SENT_I, dtype=np.int32)
    cnt[src] = 0
    c["count"] = cnt
    _joint_buffers(rng, c, rows, B, H if joint else 0, T, src)
    return c


def prep_lstm_ref(c, order, mutant=None):
    rows, beam, src, H, E = c["rows"], c["beam"], c["src"], c["H"], c["E"]
    dst = src ^ 1
    pr = (np.arange(rows) // beam) * beam + c["prev_k"]
    tok = c["y"]
    commit = tok > c["blk"]
    w = dict(state=[s.copy() for s in c["state"]], A=[a.copy() for a in c["A"]], rowmap=c["rowmap"].copy(),
             count=c["count"].copy())
    w["state"][dst] = c["state"][src][pr]
    t_new = c["t_idx"] + (tok == c["blk"])
    w["t_idx"] = t_new
    order = np.asarray(order, dtype=np.int64)
    n = len(order)
    w["count"][src] += n
    w["rowmap"][:n] = order
    if c["JH"]:
        w["rowmap32"] = c["rowmap32"].copy()
        w["rowmap32"][:n] = order
    for slot, r in enumerate(order):
        via = r if mutant == "child_taps" else pr[r]
        s = c["state"][src][via]
        w["A"][0][slot, :E] = c["emb"][tok[r]]
        w["A"][0][slot, E:E + H] = s[:H]
        for l in range(1, c["layers"]):
            w["A"][l][slot, H:2 * H] = s[2 * l * H:(2 * l + 1) * H]
    _carry_joint(c, w, pr, c["t_idx"] if mutant == "frame_before_increment" else t_new, commit)
    return w


def prep_lstm_mismatches(got, want, c):
    bad = []
    src, dst = c["src"], c["src"] ^ 1
    _exact(bad, "state_src", got["state"][src], want["state"][src])
    _exact(bad, "state_dst", got["state"][dst], want["state"][dst])
    for k in ("t_idx", "rowmap", "count"):
        _exact(bad, k, got[k], want[k])
    for l in range(c["layers"]):
        _exact(bad, "A[%d]" % l, got["A"][l], want["A"][l])
    if c["JH"]:
        _exact(bad, "rowmap32", got["rowmap32"], want["rowmap32"])
        _exact(bad, "pj_src", got["pj"][src], want["pj"][src])
        _exact(bad, "pj_dst", got["pj"][dst], want["pj"][dst])
        if h_error(got, want) >= H_TOL:
            bad.append("h")
    return bad


def lstm_cell(gates, c_prev, dtype=np.float64, order="ifgo"):
    """gates (m, 4H) pre-activations [i | f | g | o] (nn.LSTM order), c_prev (m, H) -> h', c' in `dtype` arithmetic."""
    g = gates.astype(dtype)
    c_prev = c_prev.astype(dtype)
    H = g.shape[1] // 4
    blk = {k: g[:, j * H:(j + 1) * H] for j, k in enumerate(order)}
    one = dtype(1)
    with np.errstate(over="ignore"):
        si, sf, so = (one / (one + np.exp(-blk[k])) for k in "ifo")
    cn = sf * c_prev + si * np.tanh(blk["g"])
    return so * np.tanh(cn), cn


def cell_bound(want64):
    """4 ulp of the float64 result rounded to fp32, plus 1e-7"""
    return 4.0 * np.spacing(np.abs(want64.astype(np.float32))).astype(np.float64) + 1e-7


# ---- attention -------------------------------------------------------------------------------------------------------------

def att_group(d):
    return 256 // (d // 4)


def att_positions(d):
    G = att_group(d)
    L = 8 * G + 40
    return L, [0, 1, G - 1, G, 8 * G - 1, 8 * G, 8 * G + 1, L - 1, L + 2]


def attention_case(d, heads, rows=27, seed=0, n_old=61):
    rng = np.random.default_rng(seed + d + heads)
    L, plist = att_positions(d)
    cap = n_old + rows + 1
    nan_node = cap - 1
    c = dict(d=d, heads=heads, rows=rows, L=L, cap=cap, nan_node=nan_node)
    c["pos"] = np.array([plist[i % len(plist)] for i in range(rows)], dtype=np.int64)
    c["node"] = (n_old + rng.permutation(rows)).astype(np.int64)          # distinct, not named by any ancestry prefix
    n_anc = rows + 3
    anc = rng.integers(0, n_old, size=(n_anc, L)).astype(np.int64)
    c["rowmap"] = rng.permutation(n_anc)[:rows].astype(np.int64)
    c["anc_perm"], c["anc_id"] = anc.copy(), anc.copy()                   # ancestry as read through rowmap / by identity
    p = np.minimum(c["pos"], L - 1)
    for s in range(rows):                        # positions >= pos are never followed (the new position comes from kvq)
        c["anc_perm"][c["rowmap"][s], p[s]:] = nan_node
        c["anc_id"][s, p[s]:] = nan_node
    free = np.ones(n_anc, dtype=bool)
    free[c["rowmap"]] = False
    c["anc_perm"][free] = nan_node
    c["anc_id"][rows:] = nan_node
    c["kvq"] = rng.standard_normal((rows, 3 * d)).astype(np.float32)
    for k in ("Kc", "Vc"):
        t = rng.standard_normal((cap, d)).astype(np.float32)
        t[n_old:n_old + rows] = SENT_F
        t[nan_node] = np.nan
        c[k] = t
    return c


def attention_ref(c, anc, rowmap, m, mutant=None):
    """out (rows, d) float64 (SENT_F beyond the first m slots) and the caches after the launch."""
    d, heads, L, rows = c["d"], c["heads"], c["L"], c["rows"]
    dh = d // heads
    scale = 1.0 if mutant == "no_scale" else 1.0 / np.sqrt(dh)
    out = np.full((rows, d), SENT_F, dtype=np.float64)
    Kc, Vc = c["Kc"].copy(), c["Vc"].copy()
    for s in range(min(m, rows)):
        r = s if rowmap is None else int(rowmap[s])
        p = int(min(c["pos"][s], L - 1))
        idx = anc[r, :p]
        k = np.concatenate([c["Kc"][idx], c["kvq"][s:s + 1, :d]]).astype(np.float64)
        v = np.concatenate([c["Vc"][idx], c["kvq"][s:s + 1, d:2 * d]]).astype(np.float64)
        if mutant == "no_new_pos" and p > 0:
            k, v = k[:-1], v[:-1]
        q = c["kvq"][s, 2 * d:].astype(np.float64)
        for hd in range(heads):
            sl = slice(hd * dh, (hd + 1) * dh)
            sc = (k[:, sl] @ q[sl]) * scale
            wgt = np.exp(sc - sc.max())
            out[s, sl] = (wgt / wgt.sum()) @ v[:, sl]
        Kc[c["node"][s]] = c["kvq"][s, :d]
        Vc[c["node"][s]] = c["kvq"][s, d:2 * d]
    return out, Kc, Vc


def att_error(got, want):
    e = np.abs(got.astype(np.float64) - want)
    return float(np.where(np.isnan(e), np.inf, e).max())


def att_bound(want, m):
    return ATT_TOL * max(1.0, float(np.abs(want[:m]).max())) if m else ATT_TOL


# ---- pika_dgemm ------------------------------------------------------------------------------------------------------------

def layer_norm(A, gamma, beta, eps):
    x = A.double()
    return (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + eps) * gamma.double() + beta.double()


def split_terms(x, terms):
    """fp32 tensor -> the planes the kernels multiply, as float64 (they sum to x up to what the term count drops)."""
    x = x.float()
    if terms == 4:                               # two fp16 terms: hi + 2^-11 lo'
        xc = x.clamp(-65504.0, 65504.0)
        hi = xc.half().float()
        lo = ((xc - hi) * 2048.0).half().float()
        return [hi.double(), lo.double() / 2048.0]
    out, r = [], x.clone()
    for _ in range(terms):
        h = r.bfloat16().float()
        out.append(h.double())
        r = r - h
    return out


# (plane of A, plane of W) of every product a kernel forms: 1 term hi.hi; 2 terms and two fp16 terms without lo.lo; three bf16
# terms without lo.lo, mid.lo, lo.mid (decode_step.hip, `compute`)
PRODUCTS = {1: [(0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 3: [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)],
            4: [(1, 0), (0, 1), (0, 0)]}


def model_product(A, W, terms):
    """A (m, K) . W (N, K)^T as the kernels form it, products and sums in float64 (the caller rounds to fp32).  A: the fp32
    operand as it is staged (after LayerNorm, rounded to fp32)."""
    a, w = split_terms(A, terms), split_terms(W, terms)
    y = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float64, device=A.device)
    for ia, iw in PRODUCTS[terms]:
        y += a[ia] @ w[iw].t()
    return y


def gate(z, e_all, t_idx, rows, beam, T, slot_rows=False):
    """z (m, 2H) float64 = [fc1 | fc_gate] prediction halves of the launch rows, `rows` (m,) the buffer rows they stand for:
    tanh(z1 + e1) * sigmoid(zg + eg), e = e_all[(r / beam) * T + clamp(t_idx[r], 0, T-1)].  slot_rows: the mutant that takes r
    as the launch row instead of the buffer row."""
    H = z.shape[1] // 2
    r = torch.arange(z.shape[0], device=z.device) if slot_rows else rows.long()
    g = torch.div(r, beam, rounding_mode="floor") * T + t_idx[r].clamp(0, T - 1)
    e = e_all[g].double()
    return torch.tanh(z[:, :H] + e[:, :H]) * torch.sigmoid(z[:, H:] + e[:, H:])


def interleave(z):
    """[fc1 | fc_gate] columns -> the raw accumulators' order (2j, 2j+1) = (fc1, fc_gate) of unit j"""
    H = z.shape[1] // 2
    return torch.stack((z[:, :H], z[:, H:]), dim=2).reshape(z.shape[0], 2 * H)


def err(a, b):
    e = (a.double() - b.double()).abs()
    return float(torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e).max()) if e.numel() else 0.0
