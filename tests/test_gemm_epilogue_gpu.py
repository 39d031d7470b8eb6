"""The fused epilogues of the direct-to-LDS bf16 GEMM (pika_amd/csrc/gemm_glds.hip: launch_pp_epi<1>, <2>, <3>) through the C
ABI, element by element against the float64 formulas and the derived bounds of tests/gemm_epilogue_common.py: every entry
(pika_gemm_bf16_epilogue, pika_gemm_bf16_dropout_residual, pika_gemm_bf16_ex plain and over a time-delay view,
pika_dropout_mask_cast_bf16, pika_dropout_keep_mask with and without a salt), every store path of the 16-bit epilogues
(16-byte stores, 8-byte stores on an interior tile, the edge tile), at shapes that sit on the 256 x 256 x 64 tile edges,
into padded buffers whose sentinels must survive, and every argument refusal of the host entries.

Every case prints its largest error / bound ratio (`GEMMEPI ...`) before asserting it <= 1;
profiles/gemm_epilogue_parity.txt keeps one run.  The bound is derived (fp32 accumulation of exact products, one rounding
per output format); a ratio above 1 is a failure of the kernel, not a reason to touch the bound.

One formula differs from a flat relative form: a bf16 output is held to half a bf16 ulp OF THE OUTPUT (2^-9 .. 2^-8
relative) plus the accumulation bound, because round-to-nearest-even to 8 significant bits errs by up to 2^-8 |x| at a
significand of 1 (tests/test_gemm_epilogue_refs.py::test_bf16_checker_on_torch_rne_casts).

Measured on the MI355X (error / bound): fp32 outputs 0.017 at most, two-term outputs 0.35, bf16 outputs up to 1.0 -- rounding
ties, the half-ulp term on its own, not accumulation.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_epilogue_common as E  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 4711
GARBAGE = 1.0e30            # fills the pad columns of the operands: a kernel that read them could not pass
IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


def _lib():
    from pika_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(case, what, r):
    print("GEMMEPI %-44s %-14s ratio %.3f" % (case, what, r))


def _padded_copy(t, ld, dev, fill=GARBAGE):
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


_DEV = {}


def _on(c, dev):
    """Device copies of a case's operands: lda = K + 8, ldb = K + 16, ld_aux = ld_res = N rounded up to 4, plus 4."""
    key = (id(c), str(dev))
    if key not in _DEV:
        K, N4 = c["K"], E.round_up(c["N"], 4)
        d = dict(b=_padded_copy(c["b"], K + 16, dev), bias=c["bias"].to(dev))
        if "a" in c:
            d["a"] = _padded_copy(c["a"], K + 8, dev)
            d["aux"] = _padded_copy(c["aux"], N4 + 4, dev, fill=1.0)
            d["res"] = _padded_copy(c["res"], N4 + 4, dev)
        else:       # time-delay source (batch, T, C) with a padded row pitch
            x = c["x"]
            buf = torch.full((x.shape[0], x.shape[1], x.shape[2] + 8), GARBAGE, dtype=x.dtype, device=dev)
            buf[:, :, :x.shape[2]] = x.to(dev)
            d["x"] = buf[:, :, :x.shape[2]]
        _DEV[key] = d
    return _DEV[key]


def _keep(c, p, seed, dev):
    from pika_amd.model.hipops import dropout_keep_mask
    return dropout_keep_mask(c["M"], c["N"], p, seed, dev).cpu()


def _out(c, dtype, dev, mod8=None, base_off=0):
    N4 = E.round_up(c["N"], 4)
    return E.Padded(c["M"], c["N"], dtype, N4 + 4 if mod8 is None else E.ldo_for(c["N"], mod8), dev, base_off=base_off)


def _epilogue(c, d, o, mode, relu=0, p=0.0, seed=SEED, aux=None, scale=1.0, bias=True, **over):
    """pika_gemm_bf16_epilogue; returns the return code.  `over` replaces single arguments (the refusal cases)."""
    a, b = d["a"], d["b"]
    args = dict(A=a.data_ptr(), lda=a.stride(0), B=b.data_ptr(), ldb=b.stride(0), out=o.data_ptr(), ldo=o.stride(0),
                M=c["M"], N=c["N"], K=c["K"], bias=d["bias"].data_ptr() if bias else None, mode=mode, relu=relu, p=p, seed=seed,
                aux=None if aux is None else aux.data_ptr(), ld_aux=0 if aux is None else aux.stride(0), scale=scale)
    args.update(over)
    with torch.cuda.device(o.device):
        rc = _lib().pika_gemm_bf16_epilogue(*[args[k] for k in ("A", "lda", "B", "ldb", "out", "ldo", "M", "N", "K", "bias",
                                                                "mode", "relu", "p", "seed", "aux", "ld_aux", "scale")], _stream())
    torch.cuda.synchronize()
    return rc


def _residual(c, d, o, p=0.0, seed=SEED, bias=True, **over):
    a, b, res = d["a"], d["b"], d["res"]
    args = dict(A=a.data_ptr(), lda=a.stride(0), B=b.data_ptr(), ldb=b.stride(0), out=o.data_ptr(), ldo=o.stride(0),
                M=c["M"], N=c["N"], K=c["K"], bias=d["bias"].data_ptr() if bias else None, p=p, seed=seed,
                res=res.data_ptr(), ld_res=res.stride(0))
    args.update(over)
    with torch.cuda.device(o.device):
        rc = _lib().pika_gemm_bf16_dropout_residual(*[args[k] for k in ("A", "lda", "B", "ldb", "out", "ldo", "M", "N", "K",
                                                                        "bias", "p", "seed", "res", "ld_res")], _stream())
    torch.cuda.synchronize()
    return rc


def _ex(c, d, a_op, epi, out, **kw):
    from pika_amd import gemm as G
    G.gemm_ex(a_op, d["b"], c["M"], c["N"], c["K"], epi, out, **kw)
    torch.cuda.synchronize()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(x, y):
    return torch.equal(_bits(x), _bits(y))


# ---- the checks ------------------------------------------------------------------------------------------------------
def _check_dropout16(name, c, out, keep, p, relu, out_lo=None):
    """A PIKA_EPI_DROPOUT_BF16 result (CPU tensors) against x = keep * sc * relu?(v)."""
    sc = E.sc_of(p)
    x = E.expect_dropout(c, keep, p, relu)
    B = sc * E.acc_bound(c["K"], c["S"])
    r = E.bf16_error_ratio(out, x, B)
    _report(name, "bf16", r)
    assert r <= 1.0, (name, r)
    dropped = ~keep.bool()
    assert E.is_pos_zero(out)[dropped].all(), "%s: dropped elements must be +0" % name
    dec = E.decided(c)
    if relu:   # clipped by the ReLU: +0 exactly, never -0 (an order of ReLU and scale that leaves -0 shows here)
        assert E.is_pos_zero(out)[dec & (c["v"] < 0)].all(), "%s: clipped elements must be +0" % name
        assert ((out != 0) == keep.bool())[dec & (c["v"] > 0)].all()
    else:
        assert ((out != 0) == keep.bool())[dec].all(), "%s: zero pattern != keep mask" % name
    if p == 0:
        assert keep.all() and sc == 1.0
    if out_lo is not None:
        r2 = E.two_term_error_ratio(out, out_lo, x, B)
        _report(name, "bf16 hi+lo", r2)
        assert r2 <= 1.0, (name, r2)
        assert (out_lo.double().abs() <= 0.5 * E.bf16_ulp(out.double())).all(), "%s: |lo| > half an ulp of hi" % name
        assert E.is_pos_zero(out_lo)[dropped].all()
    return r


def _check_mask16(name, c, out, scale):
    x = E.expect_mask(c, scale)
    r = E.bf16_error_ratio(out, x, abs(scale) * E.acc_bound(c["K"], c["S0"]))
    _report(name, "bf16", r)
    assert r <= 1.0, (name, r)
    masked = ~(c["aux"].double() > 0)
    assert E.is_pos_zero(out)[masked].all(), "%s: masked elements must be +0" % name
    live = (c["v0"].abs() > E.acc_bound(c["K"], c["S0"])) & ~masked
    assert (out != 0)[live].all(), "%s: an element with aux > 0 came out zero" % name
    return r


def _check_residual(name, c, out, keep, p):
    x = E.expect_residual(c, keep, p)
    r = E.f32_error_ratio(out, x, E.sc_of(p) * E.acc_bound(c["K"], c["S"]) + E.U32 * x.abs())
    _report(name, "f32", r)
    assert r <= 1.0, (name, r)
    # a dropped element is the residual itself, bit for bit
    assert torch.equal(out[~keep.bool()], c["res"][~keep.bool()])
    return r


# ---- 1. pika_gemm_bf16_epilogue, DROPOUT_BF16 -------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_epilogue_dropout_bf16(hip_device, shape, relu, p):
    c = E.case(*shape)
    d = _on(c, hip_device)
    o = _out(c, torch.bfloat16, hip_device)
    assert _epilogue(c, d, o.view, E.EPI_DROPOUT_BF16, relu=relu, p=p) == 0
    assert o.intact()
    _check_dropout16("epilogue dropout %s relu%d p%g" % (IDS(shape), relu, p), c, o.cpu(), _keep(c, p, SEED, hip_device), p, relu)


@pytest.mark.parametrize("p", [1.0 / 65536, 0.999])
def test_epilogue_dropout_extreme_p(hip_device, p):
    """thr = 1 (one hash value in 65536 drops) and p = 0.999, where 65536 / (65536 - thr) = 992.97 and 1 / (1 - p) = 1000
    are 0.7 % apart: the scale belongs to the threshold."""
    c = E.case(257, 260, 128)
    d = _on(c, hip_device)
    keep = _keep(c, p, SEED, hip_device)
    assert E.thr_of(p) == (1 if p < 0.5 else 65470)
    for relu in (0, 1):
        o = _out(c, torch.bfloat16, hip_device)
        assert _epilogue(c, d, o.view, E.EPI_DROPOUT_BF16, relu=relu, p=p) == 0
        assert o.intact()
        _check_dropout16("epilogue dropout 257x260x128 relu%d p%g" % (relu, p), c, o.cpu(), keep, p, relu)
    kept = keep.double().mean().item()
    assert (kept > 0.999) if p < 0.5 else (0 < kept < 0.004)


def test_epilogue_null_bias(hip_device):
    c = dict(E.case(513, 520, 64))
    d = _on(E.case(513, 520, 64), hip_device)
    c["v"], c["S"] = c["v0"], c["S0"]
    o = _out(c, torch.bfloat16, hip_device)
    assert _epilogue(c, d, o.view, E.EPI_DROPOUT_BF16, relu=1, p=0.2, bias=False) == 0
    assert o.intact()
    _check_dropout16("epilogue dropout 513x520x64 no bias", c, o.cpu(), _keep(c, 0.2, SEED, hip_device), 0.2, 1)


# ---- 2. pika_gemm_bf16_epilogue, MASK_BF16 ----------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.25, -0.5])
@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_epilogue_mask_bf16(hip_device, shape, scale):
    c = E.case(*shape)
    d = _on(c, hip_device)
    o = _out(c, torch.bfloat16, hip_device)
    # (relu and p_drop are ignored by this mode; a bias is not added)
    assert _epilogue(c, d, o.view, E.EPI_MASK_BF16, relu=1, aux=d["aux"], scale=scale) == 0
    assert o.intact()
    _check_mask16("epilogue mask %s scale %g" % (IDS(shape), scale), c, o.cpu(), scale)


# ---- 3. pika_gemm_bf16_dropout_residual -------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_dropout_residual(hip_device, shape, p):
    c = E.case(*shape)
    d = _on(c, hip_device)
    o = _out(c, torch.float32, hip_device)
    assert _residual(c, d, o.view, p=p) == 0
    assert o.intact()
    keep = _keep(c, p, SEED, hip_device)
    _check_residual("residual %s p%g" % (IDS(shape), p), c, o.cpu(), keep, p)
    if p == 0:      # = the plain fp32 product + residual, to one fp32 rounding of the sum
        from pika_amd import gemm as G
        assert keep.all()
        f = _out(c, torch.float32, hip_device)
        _ex(c, d, G.matrix(d["a"])[0], E.EPI_F32, f.view, bias=d["bias"])
        assert f.intact()
        x = f.cpu().double() + c["res"].double()
        assert ((o.cpu().double() - x).abs() <= E.U32 * x.abs()).all()


# ---- 4. pika_gemm_bf16_ex over a plain operand: the same kernel as the dedicated entries ---------------------------------
@pytest.mark.parametrize("shape", E.SHAPES, ids=IDS)
def test_ex_plain_operand_is_the_dedicated_entry(hip_device, shape):
    from pika_amd import gemm as G
    c = E.case(*shape)
    d = _on(c, hip_device)
    a_op = G.matrix(d["a"])[0]
    assert a_op.seg == 0
    name = "ex plain %s" % IDS(shape)
    # EPI_F32 (+ ReLU) against float64, and without ReLU against pika_gemm_bf16_nt
    for relu in (0, 1):
        f = _out(c, torch.float32, hip_device)
        _ex(c, d, a_op, E.EPI_F32, f.view, bias=d["bias"], relu=bool(relu))
        assert f.intact()
        r = E.f32_error_ratio(f.cpu(), E.expect_f32(c, relu), E.acc_bound(c["K"], c["S"]))
        _report(name, "f32 relu%d" % relu, r)
        assert r <= 1.0
        if relu:
            assert E.is_pos_zero(f.cpu())[E.decided(c) & (c["v"] < 0)].all()
        else:
            nt = _out(c, torch.float32, hip_device)
            G.gemm_bf16_nt(d["a"], d["b"], bias=d["bias"], out=nt.view)
            torch.cuda.synchronize()
            assert nt.intact()
            if c["N"] > 128:     # pika_gemm_bf16_nt runs gemm_pp from N > 128 on: the same kernel, the same bits
                assert _same_bits(nt.view, f.view)
            else:                # ... and a kernel with another summation order below: held to the same bound
                assert E.f32_error_ratio(nt.cpu(), c["v"], E.acc_bound(c["K"], c["S"])) <= 1.0
    # DROPOUT_BF16, with and without the second plane
    for relu, p in ((0, 0.2), (1, 0.5)):
        ded = _out(c, torch.bfloat16, hip_device)
        assert _epilogue(c, d, ded.view, E.EPI_DROPOUT_BF16, relu=relu, p=p) == 0
        one = _out(c, torch.bfloat16, hip_device)
        _ex(c, d, a_op, E.EPI_DROPOUT_BF16, one.view, bias=d["bias"], relu=bool(relu), p_drop=p, seed=SEED)
        hi, lo = _out(c, torch.bfloat16, hip_device), _out(c, torch.bfloat16, hip_device)
        _ex(c, d, a_op, E.EPI_DROPOUT_BF16, hi.view, out_lo=lo.view, bias=d["bias"], relu=bool(relu), p_drop=p, seed=SEED)
        assert one.intact() and hi.intact() and lo.intact()
        assert _same_bits(one.view, ded.view) and _same_bits(hi.view, ded.view)
        _check_dropout16(name + " relu%d p%g" % (relu, p), c, hi.cpu(), _keep(c, p, SEED, hip_device), p, relu, out_lo=lo.cpu())
    # MASK_BF16
    ded = _out(c, torch.bfloat16, hip_device)
    assert _epilogue(c, d, ded.view, E.EPI_MASK_BF16, aux=d["aux"], scale=-0.5) == 0
    m = _out(c, torch.bfloat16, hip_device)
    _ex(c, d, a_op, E.EPI_MASK_BF16, m.view, bias=d["bias"], relu=True, aux=d["aux"], scale=-0.5)
    assert m.intact() and _same_bits(m.view, ded.view)
    _check_mask16(name + " mask", c, m.cpu(), -0.5)
    # DROPOUT_RESIDUAL with p_drop > 0
    ded = _out(c, torch.float32, hip_device)
    assert _residual(c, d, ded.view, p=0.2) == 0
    r3 = _out(c, torch.float32, hip_device)
    _ex(c, d, a_op, E.EPI_DROPOUT_RESIDUAL, r3.view, bias=d["bias"], p_drop=0.2, seed=SEED, residual=d["res"])
    assert r3.intact() and _same_bits(r3.view, ded.view)
    _check_residual(name + " residual p0.2", c, r3.cpu(), _keep(c, 0.2, SEED, hip_device), 0.2)


# ---- store paths of the 16-bit epilogues ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dropout", "dropout_two_term", "mask"])
@pytest.mark.parametrize("shape", E.STORE_PATH_SHAPES, ids=IDS)
def test_store_paths_give_the_same_bits(hip_device, shape, mode):
    """(a) ldo % 8 == 0 on a 16-byte aligned base: 16-byte stores of lane pairs (pp_pair16) on the interior tiles;
    (b) ldo % 8 == 4 and (c) a base 4 elements (8 bytes) further: 8-byte stores.  The edge tile stores 8 bytes or
    element-wise in all three.  Same values, same bits -- in `out` and in `out_lo`."""
    from pika_amd import gemm as G
    c = E.case(*shape)
    d = _on(c, hip_device)
    a_op = G.matrix(d["a"])[0]
    p, got = 0.2, []
    for path, (mod8, off) in (("a", (0, 0)), ("b", (4, 0)), ("c", (0, 4))):
        hi = _out(c, torch.bfloat16, hip_device, mod8, off)
        lo = _out(c, torch.bfloat16, hip_device, mod8, off) if mode == "dropout_two_term" else None
        assert hi.view.stride(0) % 8 == mod8 and hi.view.data_ptr() % 16 == 2 * off
        if mode == "mask":
            assert _epilogue(c, d, hi.view, E.EPI_MASK_BF16, aux=d["aux"], scale=1.25) == 0
        elif mode == "dropout":
            assert _epilogue(c, d, hi.view, E.EPI_DROPOUT_BF16, relu=0, p=p) == 0
        else:
            _ex(c, d, a_op, E.EPI_DROPOUT_BF16, hi.view, out_lo=lo.view, bias=d["bias"], p_drop=p, seed=SEED)
        assert hi.intact() and (lo is None or lo.intact()), "path (%s): a sentinel was overwritten" % path
        got.append((hi.cpu(), None if lo is None else lo.cpu()))
        name = "store path (%s) %s %s" % (path, mode, IDS(shape))
        if mode == "mask":
            _check_mask16(name, c, got[-1][0], 1.25)
        else:
            _check_dropout16(name, c, got[-1][0], _keep(c, p, SEED, hip_device), p, 0, out_lo=got[-1][1])
    for hi, lo in got[1:]:
        assert _same_bits(hi, got[0][0])
        assert lo is None or _same_bits(lo, got[0][1])
    if mode == "dropout_two_term":      # the first plane does not depend on the second being asked for
        one = _out(c, torch.bfloat16, hip_device, 0, 0)
        _ex(c, d, a_op, E.EPI_DROPOUT_BF16, one.view, bias=d["bias"], p_drop=p, seed=SEED)
        assert _same_bits(one.cpu(), got[0][0])


# ---- 5. pika_gemm_bf16_ex over a time-delay A -----------------------------------------------------------------------------
@pytest.mark.parametrize("td", E.TD_CASES, ids=IDS)
def test_ex_time_delay_operand(hip_device, td):
    from pika_amd import gemm as G
    dil, stride, pad, T = td
    c = E.td_case(*td)
    d = _on(c, hip_device)
    a_op, M, K, t_out = G.time_delay(d["x"], E.TD_TAPS, dil, stride, pad)
    assert (M, K, t_out) == (c["M"], c["K"], c["t_out"]) and a_op.ld == E.TD_C + 8
    name = "ex time-delay dil%d stride%d pad%d" % (dil, stride, pad)
    f = _out(c, torch.float32, hip_device)
    _ex(c, d, a_op, E.EPI_F32, f.view, bias=d["bias"], relu=True)
    assert f.intact()
    r = E.f32_error_ratio(f.cpu(), E.expect_f32(c, 1), E.acc_bound(K, c["S"]))
    _report(name, "f32 relu1", r)
    assert r <= 1.0
    p = 0.2
    hi, lo = _out(c, torch.bfloat16, hip_device, 0), _out(c, torch.bfloat16, hip_device, 0)
    _ex(c, d, a_op, E.EPI_DROPOUT_BF16, hi.view, out_lo=lo.view, bias=d["bias"], p_drop=p, seed=SEED)
    assert hi.intact() and lo.intact()
    _check_dropout16(name, c, hi.cpu(), _keep(c, p, SEED, hip_device), p, 0, out_lo=lo.cpu())
    one = _out(c, torch.bfloat16, hip_device, 0)
    _ex(c, d, a_op, E.EPI_DROPOUT_BF16, one.view, bias=d["bias"], p_drop=p, seed=SEED)
    assert _same_bits(one.view, hi.view)
    if pad:     # a padded view reaches the plain epilogues only: refused, nothing written
        aux = torch.ones(M, c["N"] + 4, dtype=torch.bfloat16, device=hip_device)[:, :c["N"]]
        res = torch.ones(M, c["N"], device=hip_device)
        o16, o32 = _out(c, torch.bfloat16, hip_device), _out(c, torch.float32, hip_device)
        with pytest.raises(RuntimeError, match=r"bad argument -1\)"):
            _ex(c, d, a_op, E.EPI_MASK_BF16, o16.view, aux=aux, scale=1.0)
        with pytest.raises(RuntimeError, match=r"bad argument -1\)"):
            _ex(c, d, a_op, E.EPI_DROPOUT_RESIDUAL, o32.view, bias=d["bias"], residual=res)
        torch.cuda.synchronize()
        assert o16.untouched() and o32.untouched()


# ---- 6. the keep mask ------------------------------------------------------------------------------------------------------
def test_keep_mask_is_a_function_of_seed_row_and_column(hip_device):
    import math
    from pika_amd.model.hipops import dropout_keep_mask as mask
    rows, cols, p = 257, 258, 0.2
    m = mask(rows, cols, p, SEED, hip_device)
    big = mask(rows + 300, cols + 260, p, SEED, hip_device)
    assert torch.equal(m, big[:rows, :cols])
    assert not torch.equal(m, mask(rows, cols, p, SEED + 1, hip_device))
    for q in (0.2, 0.5):
        k = mask(rows + 300, cols + 260, q, SEED, hip_device)
        n, rate = k.numel(), 1.0 - E.thr_of(q) / 65536.0
        assert abs(k.double().mean().item() - rate) <= 4.0 * math.sqrt(rate * (1.0 - rate) / n), q
    assert mask(rows, cols, 0.0, SEED, hip_device).all()


def test_dropout_salt_shifts_the_seed(hip_device):
    from pika_amd.model.hipops import dropout_keep_mask as mask
    c = E.case(257, 260, 128)
    d = _on(c, hip_device)
    p, w1, w2 = 0.2, 12345, 777

    def run(seed):
        o = _out(c, torch.bfloat16, hip_device)
        assert _epilogue(c, d, o.view, E.EPI_DROPOUT_BF16, p=p, seed=seed) == 0
        return mask(c["M"], c["N"], p, seed, hip_device).cpu(), o.cpu()

    plain1, plain2 = run(SEED + w1), run(SEED + w2)
    word = torch.tensor([w1], dtype=torch.int32, device=hip_device)
    try:
        assert _lib().pika_set_dropout_salt(word.data_ptr()) == 0
        salted1 = run(SEED)
        word.fill_(w2)
        salted2 = run(SEED)
    finally:
        assert _lib().pika_set_dropout_salt(None) == 0
    for s, q in ((salted1, plain1), (salted2, plain2)):
        assert torch.equal(s[0], q[0]) and _same_bits(s[1], q[1])
    assert not torch.equal(salted1[0], salted2[0]) and not _same_bits(salted1[1], salted2[1])
    # cleared: the seed alone again
    unsalted = run(SEED)
    assert not torch.equal(unsalted[0], salted1[0])
    _check_dropout16("salted epilogue 257x260x128", c, salted1[1], salted1[0], p, 0)


# ---- 7. pika_dropout_mask_cast_bf16 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("shape", E.MASK_CAST_SHAPES, ids=IDS)
def test_dropout_mask_cast_bf16(hip_device, shape, p):
    from pika_amd.model.hipops import dropout_keep_mask as mask
    rows, cols = shape
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, cols, generator=g) * torch.logspace(-2, 2, cols)
    xd = _padded_copy(x, cols + 4, hip_device)
    o = E.Padded(rows, cols, torch.bfloat16, cols + 8, hip_device, base_off=4)       # base 8-byte aligned only
    with torch.cuda.device(hip_device):
        rc = _lib().pika_dropout_mask_cast_bf16(xd.data_ptr(), xd.stride(0), rows, cols, p, SEED, o.view.data_ptr(),
                                                o.view.stride(0), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and o.intact()
    keep = mask(rows, cols, p, SEED, hip_device).cpu()
    out = o.cpu()
    want = keep.double() * E.sc_of(p) * x.double()
    r = E.bf16_error_ratio(out, want, E.U32 * want.abs())
    _report("mask_cast %s p%g" % (IDS(shape), p), "bf16", r)
    assert r <= 1.0
    assert E.is_pos_zero(out)[~keep].all() and torch.equal(out != 0, keep)
    if p == 0:
        assert _same_bits(out, x.bfloat16())


# ---- 8. refusals: argument checks of the host entries; nothing reaches the device ----------------------------------------------
def test_refusals_leave_the_output_untouched(hip_device):
    from pika_amd import gemm as G
    c = E.case(257, 260, 128)
    d = _on(c, hip_device)
    o16, o32 = _out(c, torch.bfloat16, hip_device), _out(c, torch.float32, hip_device)
    nan = float("nan")
    drop = dict(mode=E.EPI_DROPOUT_BF16, p=0.2)
    msk = dict(mode=E.EPI_MASK_BF16, aux=d["aux"])
    cases16 = [
        ("K % 64", dict(drop, K=c["K"] - 32)),
        ("ldo % 4", dict(drop, ldo=o16.view.stride(0) + 2)),
        ("ld_aux % 4", dict(msk, ld_aux=d["aux"].stride(0) + 2)),
        ("out 4-byte aligned", dict(drop, out=o16.view.data_ptr() + 4)),
        ("A 8-byte aligned", dict(drop, A=d["a"].data_ptr() + 8)),
        ("p_drop = 1", dict(drop, p=1.0)),
        ("p_drop = NaN", dict(drop, p=nan)),
        ("p_drop < 0", dict(drop, p=-0.25)),
        ("unknown epilogue", dict(drop, mode=7)),
        ("EPI_F32 is not a mode of this entry", dict(drop, mode=E.EPI_F32)),
        ("mask without aux", dict(mode=E.EPI_MASK_BF16)),
    ]
    for what, kw in cases16:
        assert _epilogue(c, d, o16.view, **kw) == E.EINVAL, what
        assert o16.untouched(), what
    cases32 = [
        ("K % 64", dict(K=c["K"] - 32)),
        ("ldo % 4", dict(ldo=o32.view.stride(0) + 2)),
        ("ld_res % 4", dict(ld_res=d["res"].stride(0) + 2)),
        ("out 8-byte aligned", dict(out=o32.view.data_ptr() + 8)),
        ("p_drop = 1", dict(p=1.0)),
        ("p_drop = NaN", dict(p=nan)),
        ("no residual", dict(res=None)),
    ]
    for what, kw in cases32:
        assert _residual(c, d, o32.view, p=kw.pop("p", 0.2), **kw) == E.EINVAL, what
        assert o32.untouched(), what
    # pika_gemm_bf16_ex
    a_op = G.matrix(d["a"])[0]
    bad = r"bad argument -1\)"
    odd = torch.full((c["M"], c["N"] + 6), E.SENTINEL, dtype=torch.bfloat16, device=hip_device)
    with pytest.raises(RuntimeError, match=bad):
        _ex(c, d, a_op, 7, o16.view, bias=d["bias"])
    with pytest.raises(RuntimeError, match=bad):
        _ex(c, d, a_op, E.EPI_MASK_BF16, o16.view, scale=1.0)                                    # aux == NULL
    with pytest.raises(RuntimeError, match=bad):
        _ex(c, d, a_op, E.EPI_DROPOUT_RESIDUAL, o32.view, bias=d["bias"], p_drop=0.2)            # residual == NULL
    with pytest.raises(RuntimeError, match=bad):
        _ex(c, d, a_op, E.EPI_DROPOUT_BF16, o16.view, bias=d["bias"], p_drop=1.0)
    with pytest.raises(RuntimeError, match=bad):
        _ex(c, d, a_op, E.EPI_DROPOUT_BF16, o16.view, bias=d["bias"], p_drop=nan)
    with pytest.raises(RuntimeError, match=bad):
        _ex(dict(c, K=c["K"] - 32), d, a_op, E.EPI_DROPOUT_BF16, o16.view, bias=d["bias"])
    with pytest.raises(RuntimeError, match=bad):
        _ex(c, d, a_op, E.EPI_DROPOUT_BF16, odd[:, :c["N"]], bias=d["bias"])                     # ldo % 4 == 2
    with pytest.raises(RuntimeError, match=bad):                                                # 4-byte aligned base
        _ex(c, d, a_op, E.EPI_DROPOUT_BF16, o16.buf[2: 2 + c["M"] * 264].view(c["M"], 264)[:, :c["N"]], bias=d["bias"])
    # pika_dropout_mask_cast_bf16: cols % 4, pitches, alignment, p_drop
    x = torch.ones(8, 16, device=hip_device)
    for what, kw in [("cols % 4", dict(cols=6)), ("ld % 4", dict(ld=18)), ("ld_out % 4", dict(ld_out=266)),
                     ("ld < cols", dict(ld=4)), ("p_drop = 1", dict(p=1.0)), ("p_drop = NaN", dict(p=nan)),
                     ("x 8-byte aligned", dict(x=x.data_ptr() + 8)), ("out 4-byte aligned", dict(out=o16.view.data_ptr() + 4))]:
        a = dict(x=x.data_ptr(), ld=16, rows=8, cols=8, p=0.2, seed=SEED, out=o16.view.data_ptr(), ld_out=o16.view.stride(0))
        a.update(kw)
        rc = _lib().pika_dropout_mask_cast_bf16(a["x"], a["ld"], a["rows"], a["cols"], a["p"], a["seed"], a["out"], a["ld_out"],
                                                _stream())
        assert rc == E.EINVAL, what
    torch.cuda.synchronize()
    assert o16.untouched() and o32.untouched() and bool((odd == E.SENTINEL).all())


def test_n_not_a_multiple_of_four_is_taken(hip_device):
    """N = 258 is accepted by every entry (the last group of four columns is stored element-wise); the shape runs in every
    table above.  Here: the two columns behind N in the same group of four keep their sentinel in every output type."""
    c = E.case(300, 258, 192)
    d = _on(c, hip_device)
    o = _out(c, torch.bfloat16, hip_device)
    assert _epilogue(c, d, o.view, E.EPI_DROPOUT_BF16, p=0.5) == 0
    full = o.buf[:301 * o.view.stride(0)].view(301, o.view.stride(0)).cpu()
    assert (full[:, 258:] == E.SENTINEL).all() and (full[300] == E.SENTINEL).all()
    assert (full[:300, :258] != E.SENTINEL).all()
