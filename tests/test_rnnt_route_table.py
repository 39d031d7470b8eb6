"""Route census of the RNN-T loss without a GPU: a plain restatement of the host's selection rules
(pika_amd/csrc/rnnt_loss.hip: lattice_width, PIKA_CQ, the 8-column d(logits) kernel's eligibility and NIT,
rows_per_wave) decides which instantiations every row of tests/test_rnnt_routes_gpu.ROUTES launches.  Each row must
name exactly those, and together the rows must reach every instantiation the source names -- a new width, NIT or CQ
cannot be added without a row that runs it on the GPU, and a row cannot silently drift to another route."""
import os
import re

import pytest

import test_rnnt_routes_gpu as R

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pika_amd", "csrc", "rnnt_loss.hip")

K_WAVES = (1, 2, 3, 4, 6, 8, 12, 16)


def lattice_width(U1):
    for nw in K_WAVES:
        if nw * 64 >= U1:
            return nw * 64
    return 0


def pika_cq(extent):
    return 20 if extent <= 64 * 4 * 20 else 32


def nit(ld_out):
    return 10 if ld_out <= 512 * 10 else (13 if ld_out <= 512 * 13 else 16)


def compact8_f32(V, ld_out):
    return V % 8 == 0 and ld_out % 8 == 0 and V > 512 * 9


def compact8_f16(V, ld_out, ld_in):
    return ld_out % 8 == 0 and ld_in % 8 == 0 and ld_in >= (V + 7) // 8 * 8 and V > 512 * 9


def rows_per_wave(rows):
    return min(64, max(4, rows // (4 * 2 * 256)))


def reached(row):
    """The shape-selected instantiations the calls of one ROUTES row launch (the test's buffers are 16-byte aligned)."""
    k = row["kind"]
    if k == "lattice":
        U1, V = row["U1"], row["V"]
        return {R.AB(lattice_width(U1) // 64), R.LG(pika_cq(V)), R.MG, R.FK(R.F32, pika_cq(V))}
    if k == "gathered":
        return {R.AB(lattice_width(row["U1"]) // 64), R.MGG}
    V = row["V"]
    out = {R.AB(lattice_width(row["U"] + 1) // 64)}
    for route in row["routes"]:
        kind = route[0]
        if kind in ("lp", "raw"):
            colsum, ld_out = route[1], route[2]
            if kind == "raw":
                out.add(R.LG(pika_cq(V)))
            if colsum and compact8_f32(V, ld_out):
                out.add(R.C8(nit(ld_out), R.F32))
            else:
                out.add(R.CK(colsum, R.F32, pika_cq(ld_out)))
        elif kind == "f16":
            colsum, ld_out, ld_in = route[1], route[2], route[3]
            out.add(R.MGG)
            if colsum and compact8_f16(V, ld_out, ld_in):
                out.add(R.C8(nit(ld_out), R.F16))
            else:
                out.add(R.CK(colsum, R.F16, pika_cq(ld_out)))
        else:
            out_dtype, ld_out = route[1], route[2]
            out.add(R.LG(pika_cq(V)))
            out.add(R.FK(R.F32 if out_dtype == 0 else R.BF16, pika_cq(ld_out)))
    return out


def source_instantiations():
    """Every shape-selected instantiation rnnt_loss.hip names, read from its host code."""
    src = open(SRC).read()
    lists = re.findall(r"std::integer_sequence<int, (\d[^>]*)>", src)
    assert len(lists) == 1, lists          # THE list: lattice_width searches it, dispatch_nw folds over it
    waves = tuple(int(w) for w in lists[0].split(","))
    assert waves == K_WAVES, waves
    assert not re.search(r"kWaves|launch_ab<\w+>\(|launch_align<\w+>\(|case \d+:", src)      # no second list, no ladder
    for kernel in ("rnnt_alpha_beta_kernel", "rnnt_align_kernel"):    # one launch each, under dispatch_nw over that list
        assert len(re.findall(r"dispatch_nw\(L\.Wp / 64, \[&\]\(auto nw\) \{\s*constexpr int NW = decltype\(nw\)::value;\s*"
                              r"hipLaunchKernelGGL\(\(%s<NW>\)," % kernel, src)) == 1, kernel
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s<" % kernel, src)) == 1, kernel
    assert re.search(r"return \(\(nw == NW && \(f\(std::integral_constant<int, NW>\{\}\), true\)\) \|\| \.\.\.\);", src)
    cq = {int(c) for c in re.findall(r"constexpr int CQ = (\d+);", src)}
    nits = {int(n) for n in re.findall(r"PIKA_C8\((\d+)\)", src)}
    # both compact d(logits) kernels are named once, in launch_dlogits_compact<TI>, for the input types it is called with
    in_types = set(re.findall(r"return launch_dlogits_compact<(\w+)>\(", src))
    assert in_types == {R.F32, R.F16}, in_types
    assert len(re.findall(r"rnnt_dlogits_compact8_kernel<NIT, TI>\)", src)) == 1
    assert not re.search(r"rnnt_dlogits_compact8_kernel<NIT, (?!TI>)", src)
    c8_types = in_types
    compact = {(cs, t) for cs in re.findall(r"rnnt_dlogits_compact_kernel<(true|false), TI, CQ>", src) for t in in_types}
    assert not re.search(r"rnnt_dlogits_compact_kernel<(true|false), (?!TI,)", src)
    fused = set(re.findall(r"rnnt_dlogits_fused_kernel<(\w+), CQ>", src))
    merge = set(re.findall(r"rnnt_lse_merge_gather_kernel<(true|false)>", src))
    assert "rnnt_lse_gather_kernel<CQ>" in src
    # one launch site for every layout; the padded layout of the regular topology -- the routes' -- is in its list
    assert len(re.findall(r"hipLaunchKernelGGL\(\(rnnt_lse_gather_kernel<CQ, P::layout, P::mod>\),", src)) == 1
    assert len(re.findall(r"hipLaunchKernelGGL\(\(?rnnt_lse_gather_kernel<", src)) == 1 and "LayoutOf<PADDED, false>{}" in src
    names = {R.AB(w) for w in waves}
    names |= {R.LG(c) for c in cq}
    names |= {"rnnt_lse_merge_gather_kernel<%s>" % m for m in merge}
    names |= {R.C8(n, t) for n in nits for t in c8_types}
    names |= {R.CK(cs == "true", t, c) for cs, t in compact for c in cq}
    names |= {R.FK(t, c) for t in fused for c in cq}
    return names


def test_selection_constants_match_the_source():
    """The numbers the restatement uses are the ones in the host code."""
    src = open(SRC).read()
    assert re.search(r"\(extent\) <= 64 \* 4 \* 20\) \{ constexpr int CQ = 20; CALL; \} else \{ constexpr int CQ = 32;", src)
    assert re.search(r"constexpr int CQ_MAX = 32, V_MAX = 64 \* 4 \* CQ_MAX;", src)
    assert len(re.findall(r"if \(ld_out <= 512 \* 10\) PIKA_C8\(10\); else if \(ld_out <= 512 \* 13\) PIKA_C8\(13\); "
                          r"else PIKA_C8\(16\);", src)) == 1
    assert len(re.findall(r"PIKA_C8\(\d+\)", src)) == 3 and src.count("#define PIKA_C8(NIT)") == 1
    # the two eligibility predicates of the 8-column kernel, each the whole condition of its input type
    assert re.search(r"bool compact8_ok_f32\(int V, long long ld_out, const void \*out\) \{\s*"
                     r"return !\(V & 7\) && !\(ld_out & 7\) && V > 512 \* 9 && !\(reinterpret_cast<uintptr_t>\(out\) & 15\);", src)
    assert re.search(r"bool compact8_ok_f16\(int V, long long ld_out, long long ld_in, const void \*out, const void \*logits16\) \{\s*"
                     r"return !\(ld_out & 7\) && !\(ld_in & 7\) && ld_in >= \(\(V \+ 7\) & ~7\) && V > 512 \* 9 &&\s*"
                     r"!\(reinterpret_cast<uintptr_t>\(out\) & 15\) && !\(reinterpret_cast<uintptr_t>\(logits16\) & 15\);", src)
    assert re.search(r"launch_dlogits_compact<float>\(log_probs, 0, compact8_ok_f32\(V, ld_out, out\),", src)
    assert re.search(r"launch_dlogits_compact<_Float16>\(static_cast<const _Float16 \*>\(logits16\), ld_in,\s*"
                     r"compact8_ok_f16\(V, ld_out, ld_in, out, logits16\),", src)
    assert re.search(r"if \(wide && !wide_off\) \{", src)
    assert re.search(r"const long long r = rows / \(4 \* 2 \* 256\);\s*return \(int\)\(r < 4 \? 4 : \(r > 64 \? 64 : r\)\);", src)
    assert re.search(r"if \(nw \* 64 >= U1\) return nw \* 64;", src)


@pytest.mark.parametrize("i", range(len(R.ROUTES)))
def test_row_names_what_it_selects(i):
    row = R.ROUTES[i]
    assert reached(row) == set(row["kernels"]), (row, sorted(reached(row) ^ set(row["kernels"])))


def test_rows_reach_every_instantiation_in_the_source():
    got = set().union(*(reached(r) for r in R.ROUTES))
    want = source_instantiations()
    assert got == want, ("missing", sorted(want - got), "unknown", sorted(got - want))


def test_boundaries_have_both_sides():
    """The lattice widths at both edges of NW = 4, 8, 12, 16 (and U1 = 1024); d(logits) rows on both sides of every
    V / pitch boundary; column sums with more than four rows per wave and a partly filled last block."""
    lat = [r["U1"] for r in R.ROUTES if r["kind"] == "lattice"]
    for lo, hi in ((193, 256), (385, 512), (513, 768), (769, 1024)):
        assert lo in lat and hi in lat
    gat = {(r["U1"], r["T"]) for r in R.ROUTES if r["kind"] == "gathered"}
    assert {u for u, _ in gat} == {1, 2, 15, 16, 17, 65, 1024} and {t for _, t in gat} == {1, 3, 20}
    assert {r["blank"] for r in R.ROUTES if r["kind"] == "gathered"} >= {0, 263}
    dl = [r for r in R.ROUTES if r["kind"] == "dlogits"]
    assert {r["V"] for r in dl} >= {4608, 4616, 5000, 5120, 5124, 6268, 6656, 6664, 8192}
    assert any(r["blank"] == 0 for r in dl) and any(r["blank"] == r["V"] - 1 for r in dl)
    assert any(r["scale"] != 1.0 for r in dl)
    routes = [(r, q) for r in dl for q in r["routes"]]
    assert any(q[0] in ("lp", "raw", "f16") and q[2] > r["V"] for r, q in routes)           # ld_out > V
    assert any(q[0] == "f16" and q[3] > r["V"] for r, q in routes)                           # ld_in > V
    assert any(r["U"] + 1 > 64 for r in dl)                                                  # multi-wave lattice
    big = [r for r in dl if rows_per_wave(r["B"] * r["T"] * (r["U"] + 1)) > 4]
    assert big
    for r in big:
        rows = r["B"] * r["T"] * (r["U"] + 1)
        assert rows % (4 * rows_per_wave(rows)) != 0
        hit = reached(r)
        assert {R.C8(10, R.F32), R.C8(10, R.F16), R.CK(True, R.F32, 20), R.CK(True, R.F16, 20)} <= hit
