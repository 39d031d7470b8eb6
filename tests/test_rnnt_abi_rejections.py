"""Every `pika_rnnt_*` and `pika_prnnt_*` entry point answers a bad call with the code it has always answered, before
any launch.

tests/golden/rnnt_abi_rejections.json is a table (entry point, arguments) -> return code, recorded from the library
BEFORE the host code of rnnt_loss.hip was folded into shared checks; only refusals are kept (a negative code, or 0
bytes from the two size queries, which never launch), so no row can start a kernel on its never-dereferenced pointers
(the convention of tests/test_rnnt_surface.py).  The sweep, from one valid call per entry point: every pointer null and
misaligned in turn; B, T, U1 in {0, 1, 1024, 1025}; blank in {-1, V}; V in {0, 3, 8196}; pitches below V and off their
granule; N in {0, rows + 1, 2^31}; n_part 0; lambdas < 0, NaN, inf; out_dtype 2; `gathered` without `g_labels`; and
each of those again under every PIKA_ETOOBIG condition (U1 = 1025, 2^32 rows, N = 2^31), which pins which of the two
codes wins.

The `pika_prnnt_*` rows (pruned, smoothed, modified) were recorded the same way from the library BEFORE the padded,
packed, banded and modified host paths became one.  Their sweep adds: S in {0, -1, 1, U1, U1 + 1}; `ranges` null with
S != U1, with S == U1 (legal for the `_mod_` entries only) and with S == U1 and null `labels`; the smoothed entries'
scales < 0, NaN, inf and summing to 1; and as further PIKA_ETOOBIG conditions B*T*S = 2^31 and 2^32 and the smoothed
entries' B = 65536.

    python tests/test_rnnt_abi_rejections.py --record     # rewrite the fixture from the library in the tree
"""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "rnnt_abi_rejections.json")

_FWD = "labels frames_lengths labels_lengths B T U1 V blank costs"
_PACKED = "labels frames_lengths labels_lengths row_offsets label_offsets B T U1 N V blank"
_BANDED = "frames_lengths labels_lengths labels ranges B T U1 S V blank"
ARGS = {name: names.split() for name, names in {
    "pika_rnnt_workspace_bytes": "B T U1",
    "pika_rnnt_align_scratch_bytes": "B T U1",
    "pika_rnnt_loss_forward": "log_probs " + _FWD + " workspace stream",
    "pika_rnnt_loss_backward": "labels frames_lengths labels_lengths B T U1 V blank grad_costs workspace grads stream",
    "pika_rnnt_loss_backward_fe": "labels frames_lengths labels_lengths B T U1 V blank grad_costs workspace grads "
                                  "fastemit_lambda stream",
    "pika_rnnt_loss_dense_grads": "workspace B T U1 V blank grads stream",
    "pika_rnnt_loss_fwd_bwd": "log_probs " + _FWD + " grads workspace stream",
    "pika_rnnt_export_lattice": "workspace frames_lengths labels_lengths B T U1 alphas betas stream",
    "pika_rnnt_dlogits_compact_bf16": "log_probs lse workspace B T U1 V blank out ld_out scale colsum stream",
    "pika_rnnt_dlogits_compact_bf16_f16in": "logits16 ld_in lse workspace B T U1 V blank out ld_out scale colsum gathered "
                                            "g_labels g_blank stream",
    "pika_rnnt_fused_forward": "logits " + _FWD + " lse workspace stream",
    "pika_rnnt_fused_forward_partials": "logits pmax psum n_part " + _FWD + " lse workspace stream",
    "pika_rnnt_fused_forward_gathered": "logits16 ld_in gathered g_labels g_blank pmax psum n_part " + _FWD
                                        + " lse workspace stream",
    "pika_rnnt_fused_backward": "logits lse labels frames_lengths labels_lengths B T U1 V blank grad_costs workspace "
                                "grad_logits out_dtype ld_out stream",
    "pika_rnnt_fused_backward_fe": "logits lse labels frames_lengths labels_lengths B T U1 V blank grad_costs workspace "
                                   "grad_logits out_dtype ld_out fastemit_lambda stream",
    "pika_rnnt_packed_forward": "log_probs " + _PACKED + " costs workspace stream",
    "pika_rnnt_packed_backward": _PACKED + " grad_costs workspace grads fastemit_lambda stream",
    "pika_rnnt_packed_fused_forward": "logits " + _PACKED + " costs lse workspace stream",
    "pika_rnnt_packed_fused_backward": "logits lse " + _PACKED + " grad_costs workspace grad_logits out_dtype ld_out "
                                       "fastemit_lambda stream",
    "pika_rnnt_align": "workspace frames_lengths labels_lengths label_offsets B T U1 scores emit_frames scratch stream",
    "pika_prnnt_smoothed_fwd": "am elm side labels B T U1 V blank lm_only_scale am_only_scale amax gathered sums blank_lp "
                               "label_lp stream",
    "pika_prnnt_smoothed_bwd": "am amax elm w sg labels B T U1 V blank lm_only_scale am_only_scale d_am m stream",
    "pika_prnnt_mod_workspace_bytes": "B T U1",
    **{"pika_prnnt_" + mod + fn: names for mod in ("", "mod_") for fn, names in {
        "forward": "log_probs " + _BANDED + " costs workspace stream",
        "backward": _BANDED + " grad_costs workspace grads fastemit_lambda stream",
        "fused_forward": "logits " + _BANDED + " costs lse workspace stream",
        "fused_backward": "logits lse " + _BANDED + " grad_costs workspace grad_logits out_dtype ld_out fastemit_lambda "
                          "stream",
        "planes_forward": "blank_lp label_lp frames_lengths labels_lengths B T U1 costs blank_occ label_occ workspace stream",
        "prune_ranges": "blank_occ label_occ frames_lengths labels_lengths B T U1 S ranges stream",
    }.items()},
}.items()}

BASE = dict(B=2, T=3, U1=4, V=8, blank=0, N=24, ld_out=8, ld_in=8, scale=1.0, n_part=1, g_blank=0, out_dtype=0,
            fastemit_lambda=0.0, stream=0, S=2, lm_only_scale=0.25, am_only_scale=0.25)
PTR = 256                                    # never dereferenced; 16-byte aligned
BIG = dict(B=1 << 12, T=1 << 10, U1=1 << 10)  # 2^32 rows
TOOBIG = [dict(U1=1025), BIG, dict(BIG, N=1 << 31)]
# what the pika_prnnt_* entries add: 2^32 and 2^31 band rows, and the smoothed calls' limit on B
PRUNED_TOOBIG = [dict(BIG, S=1 << 10), dict(B=1 << 11, T=1 << 10, U1=1 << 10, S=1 << 10), dict(B=1 << 16)]


def _mutations(fn, names, sig):
    ptrs = [n for n, t in zip(names, sig) if t is ctypes.c_void_p and n != "stream"]
    out = [{}]
    for p in ptrs:
        out += [{p: 0}, {p: PTR + 4}, {p: PTR + 8}]
    for d in ("B", "T", "U1"):
        out += [{d: v} for v in (0, 1, 1024, 1025)]
    out += [BIG, dict(blank=-1), dict(blank=BASE["V"]), dict(V=0), dict(V=3), dict(V=4, blank=3),
            dict(V=8196), dict(V=8196, ld_out=8196, ld_in=8196), dict(V=8192, ld_out=8192, ld_in=8192),
            dict(V=8192, ld_out=8196, ld_in=8192), dict(ld_out=4), dict(ld_out=10), dict(ld_out=12),
            dict(ld_in=4), dict(ld_in=10), dict(ld_in=12), dict(N=0), dict(N=-1), dict(N=25), dict(N=1 << 31),
            dict(BIG, N=1 << 31), dict(n_part=0), dict(n_part=-1), dict(out_dtype=2), dict(out_dtype=-1), dict(out_dtype=1),
            dict(fastemit_lambda=-1.0), dict(fastemit_lambda="nan"), dict(fastemit_lambda="inf"),
            dict(g_labels=0), dict(g_labels=0, gathered=0), dict(U1=1, labels=0), dict(U1=1, emit_frames=0),
            dict(U1=1, labels=0, label_offsets=0)]
    toobig = TOOBIG
    if fn.startswith("pika_prnnt_"):
        U1 = BASE["U1"]
        out += [dict(S=v) for v in (0, -1, 1, U1, U1 + 1)]
        out += [dict(ranges=0, S=U1 - 1), dict(ranges=0, S=U1), dict(ranges=0, S=U1, labels=0)]
        for k in ("lm_only_scale", "am_only_scale"):
            out += [{k: v} for v in (-1.0, "nan", "inf", 0.75)]
        toobig = TOOBIG + PRUNED_TOOBIG
    out += [dict(m, **big) for big in toobig for m in out]
    seen, rows = set(), []
    for m in out:
        m = {k: v for k, v in m.items() if k in names}
        row = tuple(m.get(n, BASE.get(n, PTR)) for n in names)
        if row not in seen:
            seen.add(row)
            rows.append(list(row))
    return rows


def _call(L, fn, sig, row):
    args = []
    for t, v in zip(sig, row):
        if t is ctypes.c_void_p:
            args.append(ctypes.c_void_p(v) if v else None)
        else:
            args.append(float(v) if t is ctypes.c_float else v)
    return getattr(L, fn)(*args)


def _signatures():
    from pika_amd import _lib
    return {k: v for k, v in _lib.SIGNATURES.items() if k.startswith(("pika_rnnt_", "pika_prnnt_"))}


def record():
    from pika_amd import _lib
    L, table = _lib.lib(), {}
    for fn, (res, sig) in sorted(_signatures().items()):
        names = ARGS[fn]
        assert len(names) == len(sig), fn
        rows = []
        for row in _mutations(fn, names, sig):
            rc = _call(L, fn, sig, row)
            if rc < 0 or (res is ctypes.c_size_t and rc == 0):
                rows.append(row + [rc])
        table[fn] = {"args": names, "rows": rows}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(
            '"%s": {"args": %s, "rows": [\n%s]}' % (fn, json.dumps(e["args"]), ",\n".join(json.dumps(r) for r in e["rows"]))
            for fn, e in table.items()) + "\n}\n")
    print("recorded %d rows over %d entry points" % (sum(len(e["rows"]) for e in table.values()), len(table)))


TABLE = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}


def test_table_covers_every_entry_point():
    sigs = _signatures()
    assert set(TABLE) == set(sigs) == set(ARGS)
    for fn, e in TABLE.items():
        assert e["args"] == ARGS[fn] and len(e["args"]) == len(sigs[fn][1]) and e["rows"], fn
        codes = {r[-1] for r in e["rows"]}
        assert codes <= ({0} if sigs[fn][0] is ctypes.c_size_t else {-1, -2}), (fn, codes)   # refusals only
    assert sum(len(e["rows"]) for e in TABLE.values()) >= 3881


@pytest.mark.parametrize("fn", sorted(ARGS))
def test_refusals_are_the_recorded_ones(fn):
    from pika_amd import _lib
    L, sig = _lib.lib(), _signatures()[fn][1]
    bad = []
    for row in TABLE[fn]["rows"]:
        got = _call(L, fn, sig, row[:-1])
        if got != row[-1]:
            bad.append((dict(zip(ARGS[fn], row[:-1])), "recorded", row[-1], "got", got))
    assert not bad, (len(bad), bad[:5])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    assert sys.argv[1:] == ["--record"], __doc__
    record()
