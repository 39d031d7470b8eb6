"""The joint-network kernels of include/pika_joint.h (pika_amd/csrc/joint.hip) as plain float64 restatements, the tables
of cases they are tested on, and the builders of padded / misaligned buffers.  Nothing here needs a GPU:
tests/test_joint_refs.py checks the restatements and the tables on their own, tests/test_joint_kernels_gpu.py runs the
kernels through the C ABI against them.

Fixed points of every reference: the inputs are the fp32 (or bf16) arrays the kernel gets, `scale` is the fp32 argument;
everything after that is float64 with explicit sums (no autograd).
"""
import functools

import numpy as np
import torch

F32, BF16 = 0, 1                       # PIKA_F32 / PIKA_BF16 (include/pika_gemm.h)
EINVAL, ETOOBIG = -1, -2

# tolerances of tests/test_joint_gpu.py / tests/test_mbr.py (the autograd-level tests of the same kernels)
GATE_H_TOL = 2e-6                      # |h - h64|
GRAD_REL_TOL = 1e-5                    # gate gradients: * max(1, max |ref|); log-softmax backward: * max(1, max_r sum_c |g|)
LSM_FWD_TOL = 1e-5
RISK_TOL = 1e-5


# ---- the references ------------------------------------------------------------------------------------------------
def _d(a):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).double()


def gate_ref(e1, p1, eg, pg):
    """h (B,T,U,H) float64 = tanh(e1[b,t] + p1[b,u]) * sigmoid(eg[b,t] + pg[b,u])."""
    z1 = _d(e1)[:, :, None, :] + _d(p1)[:, None, :, :]
    zg = _d(eg)[:, :, None, :] + _d(pg)[:, None, :, :]
    return torch.tanh(z1) * (1.0 / (1.0 + torch.exp(-zg)))


def gate_bwd_ref(dh, e1, p1, eg, pg):
    """(de1, dp1, deg, dpg) float64 from the formulas of include/pika_joint.h:
    dz1 = dh * sig(zg) * (1 - tanh(z1)^2), dzg = dh * tanh(z1) * sig(zg) * (1 - sig(zg)); de* = sum over u, dp* = sum over t."""
    z1 = _d(e1)[:, :, None, :] + _d(p1)[:, None, :, :]
    zg = _d(eg)[:, :, None, :] + _d(pg)[:, None, :, :]
    th, sg = torch.tanh(z1), 1.0 / (1.0 + torch.exp(-zg))
    dz1 = _d(dh) * sg * (1.0 - th * th)
    dzg = _d(dh) * th * sg * (1.0 - sg)
    return dz1.sum(2), dz1.sum(1), dzg.sum(2), dzg.sum(1)


def log_softmax_ref(x, scale):
    """(rows, cols) float64: z - (m + log(sum(exp(z - m)))), z = float32(scale) * x.  A row that is all -inf or holds a NaN
    comes out all NaN (m - m resp. the NaN reaches the sum), as torch.log_softmax gives on the CPU."""
    z = float(np.float32(scale)) * _d(x)
    m = z.max(dim=1, keepdim=True).values
    return z - (m + torch.log(torch.exp(z - m).sum(dim=1, keepdim=True)))


def log_softmax_bwd_ref(lp, g, scale):
    """(rows, cols) float64: scale * (g - exp(lp) * rowsum(g))."""
    g = _d(g)
    return float(np.float32(scale)) * (g - torch.exp(_d(lp)) * g.sum(dim=1, keepdim=True))


def risk_grad_ref(lp, sym, val, scale):
    """(rows, cols) float64: scale * val[r] * ((v == sym[r]) - exp(lp[r, v])); rows with val == 0 are zeros whatever lp holds."""
    lp, val = _d(lp), _d(val)
    onehot = torch.zeros_like(lp)
    onehot[torch.arange(lp.shape[0]), torch.as_tensor(np.asarray(sym)).long()] = 1.0
    out = float(np.float32(scale)) * val[:, None] * (onehot - torch.exp(lp))
    out[val == 0] = 0.0
    return out


# ---- padded / misaligned buffers -----------------------------------------------------------------------------------
LEAD = 64                              # sentinel elements in front of the operand (keeps a 256-byte aligned base aligned)
TAIL_ROWS = 2                          # sentinel rows behind the operand
SENT32 = np.uint32(0x7FC12345)         # a quiet NaN with a payload: whatever is read from the padding into a sum shows
SENT16 = np.uint16(0x7FC1)             # the same as bf16


class Padded:
    """A (rows, cols) operand as a view with pitch `ld` of a larger allocation filled with a sentinel bit pattern:
    LEAD + `offset` elements in front (offset = 1: the view starts one element past a 16-byte boundary), the columns
    [cols, ld) of every row, and TAIL_ROWS whole rows behind.  `bits` is the allocation as unsigned integers."""

    def __init__(self, rows, cols, ld, offset=0, itemsize=4, data=None):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.itemsize = rows, cols, ld, itemsize
        self.start = LEAD + offset
        self.utype = np.uint32 if itemsize == 4 else np.uint16
        self.bits = np.full(self.start + (rows + TAIL_ROWS) * ld, SENT32 if itemsize == 4 else SENT16, self.utype)
        if data is not None:
            self.window(self.bits)[...] = np.ascontiguousarray(data).view(self.utype).reshape(rows, cols)

    def window(self, bits):
        """The operand inside `bits` (the allocation, or a copy of it brought back from the device)."""
        return bits[self.start:self.start + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    def pad_mask(self):
        m = np.ones(self.bits.shape, bool)
        self.window(m)[...] = False
        return m

    def padding_intact(self, bits):
        """Every sentinel -- in front, in [cols, ld) of each row, in the rows behind -- bit-identical to before."""
        m = self.pad_mask()
        return bool(np.array_equal(bits[m], self.bits[m]))

    def byte_offset(self):
        return self.start * self.itemsize


# ---- gate cases ----------------------------------------------------------------------------------------------------
# (B,T,U,H): one thread; exactly one wave of threads; a partial second wave; 256 threads; exactly 1024 threads; the channel
# loop's second trip with a single active lane
GATE_SHAPES = [(1, 1, 1, 4), (2, 3, 2, 256), (1, 2, 3, 260), (2, 1, 5, 1024), (1, 3, 1, 4096), (1, 2, 2, 4100)]
SAT_Z1 = [-40.0, -15.5, -15.0, -9.0, 0.0, 9.0, 15.0, 15.5, 40.0]       # around the clamps at z1 = +-15 ...
SAT_ZG = [-100.0, -50.5, -50.0, -20.0, 0.0, 20.0, 100.0]               # ... and at zg = -50
SAT_MODERATE_ZG, SAT_MODERATE_Z1 = 0.5, 0.75
NAN, INF = float("nan"), float("inf")
INPUT_NAMES = ("e1", "p1", "eg", "pg")

# non-finite cases on shape (2,3,2,8): name -> [(input, index (b, t|u, c), value)]: the ONLY non-finite input elements
GATE_NONFINITE = {
    "nan_e1": [("e1", (1, 2, 5), NAN)],
    "nan_p1": [("p1", (0, 1, 0), NAN)],
    "nan_eg": [("eg", (0, 0, 7), NAN)],
    "nan_pg": [("pg", (1, 0, 3), NAN)],
    "posinf_e1": [("e1", (0, 1, 2), INF)],                 # tanh -> +1
    "neginf_p1": [("p1", (1, 1, 6), -INF)],                # tanh -> -1
    "posinf_pg": [("pg", (0, 0, 1), INF)],                 # sigmoid -> 1
    "neginf_eg": [("eg", (1, 0, 4), -INF)],                # sigmoid -> 0
    "inf_meet_z1": [("e1", (0, 2, 3), INF), ("p1", (0, 1, 3), -INF)],    # NaN at (0,2,1,3) only; +-1 along the rest
    "inf_meet_zg": [("eg", (1, 1, 2), -INF), ("pg", (1, 0, 2), INF)],
}
NONFINITE_SHAPE = (2, 3, 2, 8)


def _gate_random(shape, seed):
    B, T, U, H = shape
    g = torch.Generator().manual_seed(seed)
    ins = [torch.randn(B, n, H, generator=g) for n in (T, U, T, U)]
    dh = torch.randn(B, T, U, H, generator=g)
    return ins, dh


def gate_case_names():
    return ["shape_%dx%dx%dx%d" % s for s in GATE_SHAPES] + ["saturation"] + sorted(GATE_NONFINITE)


@functools.lru_cache(maxsize=None)
def gate_case(name):
    """One gate case, computed once and never modified: dict with the fp32 inputs e1, p1, eg, pg, `dh` (fp32), `dh16`
    (bf16), the float64 results h, `grads` (from dh) and `grads16` (from dh16 upcast), `finite` (no non-finite input) and
    `named` (the non-finite input elements)."""
    named = []
    if name.startswith("shape_"):
        shape = tuple(int(v) for v in name[6:].split("x"))
        ins, dh = _gate_random(shape, 100 * shape[0] + shape[3])
    elif name == "saturation":
        # channel c carries one chosen (z1, zg); e = z / 4 and p = 3 z / 4 are exact in fp32 for these values, so every
        # (t, u) of the channel sees exactly that pair
        z1 = SAT_Z1 + [SAT_MODERATE_Z1] * len(SAT_ZG)
        zg = [SAT_MODERATE_ZG] * len(SAT_Z1) + SAT_ZG
        B, T, U, H = shape = (1, 2, 3, len(z1))
        assert H % 4 == 0
        z1, zg = torch.tensor(z1), torch.tensor(zg)
        ins = [(0.25 * z1).expand(B, T, H).clone(), (0.75 * z1).expand(B, U, H).clone(),
               (0.25 * zg).expand(B, T, H).clone(), (0.75 * zg).expand(B, U, H).clone()]
        assert torch.equal(ins[0][0, 0] + ins[1][0, 0], z1) and torch.equal(ins[2][0, 0] + ins[3][0, 0], zg)
        dh = _gate_random(shape, 7)[1]
    else:
        named = GATE_NONFINITE[name]
        shape = NONFINITE_SHAPE
        ins, dh = _gate_random(shape, 11)
        for which, idx, value in named:
            ins[INPUT_NAMES.index(which)][idx] = value
    dh16 = dh.bfloat16()
    c = dict(zip(INPUT_NAMES, ins))
    c.update(name=name, shape=shape, dh=dh, dh16=dh16, named=named, finite=not named, h=gate_ref(*ins),
             grads=gate_bwd_ref(dh, *ins), grads16=gate_bwd_ref(dh16.float(), *ins))
    return c


# ---- log-softmax cases ---------------------------------------------------------------------------------------------
WAVE_MAX = 8192                        # 64 lanes * 4 floats * WQ 32
WQ20_MAX = 5120                        # 64 lanes * 4 floats * WQ 20
LSM_COLS = [4, 8, 13, 252, 256, 260, 5116, 5120, 5124, 8188, 8192, 8196, 8197]
# the row count of a case follows its cols (every layout of one cols shares its data): each of the three kernels sees
# fewer than four rows, and more than four that are no multiple of four
LSM_ROWS = {4: 1, 8: 3, 13: 2, 252: 4, 256: 5, 260: 9, 5116: 2, 5120: 3, 5124: 3, 8188: 9, 8192: 5, 8196: 3, 8197: 4}
LSM_SCALES = [1.0, 0.7]
LSM_LAYOUTS = ("eq", "pad4", "pad1", "off1")       # ld == cols; cols + 4; cols + 1; base one float past 16 bytes, ld = cols + 4
ROUTE_COLS = (5120, 5124, 8192, 8196)              # either side of both route boundaries: aligned layout vs block route


def lsm_route(cols, ld, offset):
    """The kernel pika_log_softmax_rows / _bwd_rows take (joint.hip: wave_row_ok, PIKA_WQ)."""
    if cols % 4 or ld % 4 or offset % 4 or cols > WAVE_MAX:
        return "block"
    return "wave20" if cols <= WQ20_MAX else "wave32"


def _lsm_layout(cols, layout):
    """(ld, offset in floats) of a layout."""
    return {"eq": (cols, 0), "pad4": (cols + 4, 0), "pad1": (cols + 1, 0), "off1": (cols + 4, 1)}[layout]


def _lsm_case(name, rows, cols, layout, scale, kind="finite", special=None):
    ld, offset = _lsm_layout(cols, layout)
    return dict(name=name, rows=rows, cols=cols, ld=ld, offset=offset, layout=layout, scale=scale, kind=kind,
                special=special, route=lsm_route(cols, ld, offset))


def _lsm_cases():
    cases = []
    for i, cols in enumerate(LSM_COLS):
        for j, layout in enumerate(LSM_LAYOUTS):
            if layout == "off1" and cols % 4:
                continue
            cases.append(_lsm_case("c%d_%s" % (cols, layout), LSM_ROWS[cols], cols, layout,
                                   LSM_SCALES[(i + j) % 2]))
    # masking and NaN: six rows = one full 4-row workgroup of the wave kernels and a partial one; once per route family
    for layout in ("eq", "pad1"):
        cases.append(_lsm_case("mask_%s" % layout, 6, 260, layout, 0.7, "mask", {1: (0, 3, 259), 4: (17, 18, 19, 20, 128)}))
        cases.append(_lsm_case("neginf_row_%s" % layout, 6, 260, layout, 1.0, "neginf_row", 2))
        cases.append(_lsm_case("nan_row_%s" % layout, 6, 260, layout, 0.7, "nan_row", (1, 77)))
    return cases


LSM_CASES = _lsm_cases()
LSM_BY_NAME = {c["name"]: c for c in LSM_CASES}


@functools.lru_cache(maxsize=None)
def _lsm_random(rows, cols):
    g = torch.Generator().manual_seed(rows * 31 + cols)
    x = torch.randn(rows, cols, generator=g) * 3
    w = torch.randn(rows, cols, generator=g)
    w[w.abs() < 1.0] = 0.0             # a sparse upstream gradient, like the RNN-T loss'
    return x, w


@functools.lru_cache(maxsize=None)
def lsm_data(name):
    """One log-softmax case, computed once and never modified: x, g (fp32), the float64 forward `want`, `lp` (= want
    rounded to fp32: the backward's input, so the backward does not depend on the forward kernel), the float64 backward
    `want_bwd` of (lp, g), `bad_rows` (rows whose reference is all NaN) and `neginf` (mask of exact -inf outputs)."""
    c = LSM_BY_NAME[name]
    x, g = (t.clone() for t in _lsm_random(c["rows"], c["cols"]))
    bad_rows, neginf = [], torch.zeros(x.shape, dtype=torch.bool)
    if c["kind"] == "mask":
        for r, cols in c["special"].items():
            x[r, list(cols)] = -INF
            g[r, list(cols)] = 0.0
            neginf[r, list(cols)] = True
    elif c["kind"] == "neginf_row":
        x[c["special"]] = -INF
        bad_rows = [c["special"]]
    elif c["kind"] == "nan_row":
        x[c["special"]] = NAN
        bad_rows = [c["special"][0]]
    with np.errstate(all="ignore"):
        want = log_softmax_ref(x, c["scale"])
    lp = want.float()
    return dict(x=x, g=g, want=want, lp=lp, want_bwd=log_softmax_bwd_ref(lp, g, c["scale"]), bad_rows=bad_rows,
                neginf=neginf, gsum=float(g.double().abs().sum(1).max()))


# bf16 backward: (cols, ld_out, rows); every case runs with ld == cols and ld = cols + 4.  WQ follows ld_out: (5000, 5184)
# runs the WQ = 32 kernel on rows the in-place kernel handles with WQ = 20
BF16_BWD_CASES = [(8, 64, 3), (5000, 5056, 5), (5000, 5184, 2), (5120, 5120, 1), (6268, 6272, 7), (8192, 8192, 6)]


@functools.lru_cache(maxsize=None)
def bf16_bwd_data(cols, rows, scale=0.7):
    x, g = _lsm_random(rows, cols)
    lp = log_softmax_ref(x, scale).float()
    return dict(lp=lp, g=g, scale=scale, want=log_softmax_bwd_ref(lp, g, scale), gsum=float(g.double().abs().sum(1).max()))


# ---- MBR risk gradient ---------------------------------------------------------------------------------------------
RISK_SCALE = 0.8
RISK_SHAPES = [(1, 4, 4), (5, 13, 16), (3, 300, 301), (4, 5000, 5000)]     # (rows, cols, ld)


@functools.lru_cache(maxsize=None)
def risk_data(rows, cols):
    """lp = log_softmax(0.8 * logits) fp32, sym (0 and cols - 1 among them), val (with an exact zero where rows > 1) and the
    float64 result.  The 5-row case also holds: row 1 with val == 0 whose lp has a -inf and a NaN (-> exact zeros) and row 3
    with val != 0 and lp = -inf away from sym (-> 0 there)."""
    g = torch.Generator().manual_seed(rows * 7 + cols)
    lp = log_softmax_ref(torch.randn(rows, cols, generator=g) * 2, RISK_SCALE).float()
    sym = torch.randint(0, cols, (rows,), generator=g).int()
    val = torch.randn(rows, generator=g)
    sym[0] = 0
    sym[-1] = cols - 1 if rows > 1 else 0
    zero_rows, neginf_at = [], []
    if rows > 1:
        val[1] = 0.0
        zero_rows = [1]
    if rows == 5:
        lp[1, 2], lp[1, 5] = -INF, NAN
        sym[3] = 4
        lp[3, 7] = -INF
        neginf_at = [(3, 7)]
    assert all(float(val[r]) != 0.0 for r in range(rows) if r not in zero_rows)
    return dict(lp=lp, sym=sym, val=val, want=risk_grad_ref(lp, sym, val, RISK_SCALE), zero_rows=zero_rows,
                neginf_at=neginf_at)
