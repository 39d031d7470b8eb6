"""The LSTM recurrence of training (include/pika_lstm.h:9-11,43-45) stated twice in plain torch on the CPU, for the
tests of pika_amd/csrc/lstm_train.hip.  Imports nothing from pika_amd.

  forward(gx, w_hh)                -> out, gates (ACTIVATED, order i|f|g|o), cells        zero initial state
  backward(dy, w_hh, gates, cells) -> dgates: the gradient of the PRE-activation gates

* the ORACLE (model=None): float64 throughout;
* the ARITHMETIC MODEL (model=MODEL): what the kernels are written to compute -- fp32, with h_{t-1} (forward), the gate
  gradients (backward) and W_hh each split into two bf16 terms, the products hi.hi + lo.hi + hi.lo (lo.lo dropped) summed
  in fp32, the activations by libm (evaluated in float64 and rounded once);
* MUTANTS of the model, each one line away from it: what a subtly wrong kernel would compute.

e_model = max |model - oracle| of a case is what the arithmetic costs there; the GPU test allows the kernels
max(4 * e_model, FLOOR) (tests/test_lstm_recurrence_gpu.py), and tests/test_lstm_oracle.py proves on the CPU that this
bound is inside 2e-5 and that every mutant is at least ten times outside it."""
import torch

MODEL = "model"
MUTANTS = ("drop_hi_lo", "drop_lo_hi", "one_term_w", "gate_order", "no_cell_carry", "forget_cell_now")
FORWARD_MUTANTS = ("drop_hi_lo", "drop_lo_hi", "one_term_w", "gate_order")       # the others differ in the backward only

# what the model leaves out of the kernel's arithmetic (the order of the fp32 sums, __expf / rcp at a few ulp)
MARGIN = 4.0
# the activations alone: libm is half an ulp, __expf (2 ulp) and rcp (1 ulp) are chained twice into h and meet the
# cancellation of 1 - 2 * rcp(..): 16 ulp of fp32 at the tensor's scale
FLOOR = 16 * 2.0 ** -24
# the bound of the same arithmetic in blstm.hip's test (tests/test_las_kernels_gpu.py): MARGIN * e_model stays inside it
CEILING = 2e-5

NOMINAL_CUS = 256       # MI355X; the GPU test reads the device's own count


def _split(a):
    hi = a.bfloat16().float()
    return hi, (a - hi).bfloat16().float()


def _product(a, w, variant):
    """a (B, K) . w (K, N) as the kernels form it: both operands as two bf16 terms, fp32 sums."""
    if variant is None:
        return a @ w
    ah, al = _split(a)
    wh, wl = _split(w)
    if variant == "one_term_w":
        return a @ wh
    y = ah @ wh
    if variant != "drop_lo_hi":
        y = y + al @ wh
    if variant != "drop_hi_lo":
        y = y + ah @ wl
    return y


def _act(fn, z, variant):
    return fn(z) if variant is None else fn(z.double()).float()


def forward(gx, w_hh, model=None):
    dt = torch.float64 if model is None else torch.float32
    gx, w_t = gx.to(dt), w_hh.to(dt).t().contiguous()
    B, S, H4 = gx.shape
    H = H4 // 4
    out, gates, cells = gx.new_empty(B, S, H), gx.new_empty(B, S, H4), gx.new_empty(B, S, H)
    h, c = gx.new_zeros(B, H), gx.new_zeros(B, H)
    for t in range(S):
        z = gx[:, t] + _product(h, w_t, model) if t else gx[:, t]
        zi, zf, zg, zo = z.chunk(4, dim=1)
        if model == "gate_order":
            zf, zg = zg, zf
        i, f, g, o = _act(torch.sigmoid, zi, model), _act(torch.sigmoid, zf, model), _act(torch.tanh, zg, model), \
            _act(torch.sigmoid, zo, model)
        c = f * c + i * g
        h = o * _act(torch.tanh, c, model)
        out[:, t], cells[:, t], gates[:, t] = h, c, torch.cat((i, f, g, o), dim=1)
    return out, gates, cells


def backward(dy, w_hh, gates, cells, model=None):
    dt = torch.float64 if model is None else torch.float32
    dy, w, gates, cells = dy.to(dt), w_hh.to(dt).contiguous(), gates.to(dt), cells.to(dt)
    B, S, H = dy.shape
    dgates = dy.new_empty(B, S, 4 * H)
    dc_next, dz = dy.new_zeros(B, H), None
    for t in range(S - 1, -1, -1):
        dh = dy[:, t] + _product(dz, w, model) if t + 1 < S else dy[:, t]
        i, f, g, o = gates[:, t].chunk(4, dim=1)
        if model == "gate_order":
            f, g = g, f
        c_prev = cells[:, t - 1] if t else torch.zeros_like(dc_next)
        if model == "forget_cell_now":
            c_prev = cells[:, t]
        tc = _act(torch.tanh, cells[:, t], model)
        dc = dh * o * (1 - tc * tc) + dc_next
        dz = torch.cat((dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), dim=1)
        dc_next = dc * f if model != "no_cell_carry" else torch.zeros_like(dc)
        dgates[:, t] = dz
    return dgates


def err(a, b):
    return float((a.double() - b.double()).abs().max())


def scale(want):
    return max(1.0, float(want.abs().max()))


def bound(e_model, want):
    """What a kernel may be away from the oracle tensor `want` where the model is e_model away."""
    return max(MARGIN * e_model, FLOOR * scale(want))


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of the GPU test: (B, S, H, gain, saturated).  B = "max": the largest batch the device admits; S = "long": 257
# or what keeps the backward scratch (S * ceil(B / 16) * (H / 16)^2 KB) under 1 GB.  Every H meets every S class
# {1, 2, 3, 51, long} and every B class {1, 15, 16, 17, 33, max}, both gains, and one saturated case.  (33 rows x 51 steps
# at gain 2 is 2.1e-5 on the gates, outside CEILING: that case runs at gain 1.5.)

def max_batch(H, cus=NOMINAL_CUS):
    return 16 * (cus // (H // 16))


def long_steps(B, H):
    per_step = ((B + 15) // 16) * (H // 16) ** 2 * 1024
    return min(257, (10 ** 9 - 256) // per_step)


def _table():
    cases = []
    for H in (256, 512, 768, 1024):
        cases += [(1, 1, H, 1, False), (15, 2, H, 2, False), (16, 3, H, 1, False), (17, 51, H, 1, False),
                  (33, 51, H, 1.5, False), ("max", 3, H, 2, False), ("max", 1, H, 1, False), (16, "long", H, 1, False),
                  (17, 20, H, 1, True)]
    cases += [(32, 51, 1024, 1, False), (33, 64, 768, 1, False), (17, 51, 512, 2, False), (5, 7, 256, 1, False)]
    return cases


CASES = _table()


def case_id(case):
    B, S, H, gain, sat = case
    return "B%s-S%s-H%d-g%g%s" % (B, S, H, gain, "-sat" if sat else "")


def resolve(case, cus=NOMINAL_CUS):
    B, S, H, gain, sat = case
    B = max_batch(H, cus) if B == "max" else B
    S = long_steps(B, H) if S == "long" else S
    return B, S, H, gain, sat


def inputs(B, S, H, gain, sat, seed=0):
    """fp32 gx (B, S, 4H), w_hh (4H, H) uniform in +-gain / sqrt(H), dy (B, S, H).  Saturated: a tenth of gx at +-30 and a
    few entries at +-1e4 (the ends of the fast activations)."""
    g = torch.Generator().manual_seed(1000 * H + 10 * S + B + seed)
    gx = torch.randn(B, S, 4 * H, generator=g)
    w = (torch.rand(4 * H, H, generator=g) * 2 - 1) * (gain / H ** 0.5)
    dy = torch.randn(B, S, H, generator=g)
    if sat:
        flat = gx.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)
        n = flat.numel() // 10
        sign = (torch.rand(n, generator=g) < 0.5).float() * 2 - 1
        flat[idx[:n]] = 30.0 * sign
        flat[idx[n:n + 16]] = 1e4 * sign[:16]
    return gx, w, dy
