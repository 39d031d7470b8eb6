"""The gate on a pruned (banded) lattice (include/pika_joint.h: pika_joint_gate_banded_fwd / _bwd) restated in float64, and
the `ranges` its tests run on.  Nothing here needs a GPU or the product: tests/test_joint_banded_surface.py checks the two
formulations of the prediction-side sum against each other, tests/test_joint_banded_gpu.py runs the kernels against them.

Index contract (that of pika_amd.rnnt.rnnt_prune_lm): s_t = clamp(ranges[b,t], 0, U - S); row j of frame t pairs e*[b,t] with
p*[b, s_t + j].  U counts prediction rows (the loss's U + 1).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_common as J  # noqa: E402
import rnnt_pruned_common as P  # noqa: E402

# (B,T,U,S,H): smallest possible; a small band; 65 threads (crosses a wave); S = U with 257 threads; the channel loop wraps
# past 1024 threads
SHAPES = [(1, 1, 1, 1, 4), (2, 5, 4, 2, 8), (3, 33, 9, 4, 260), (2, 7, 6, 6, 1028), (1, 3, 5, 3, 4100)]
KINDS = ("valid", "nonmonotone", "clamped")
UNCOVERED_SHAPE = (3, 33, 9, 4, 260)       # its "nonmonotone" ranges leave row 4 of batch 0 outside every band


def band_rows(ranges, U, S):
    """(B,T,S) int64: the prediction row of every band row."""
    s = torch.as_tensor(np.asarray(ranges)).long().clamp(0, U - S)
    return s[:, :, None] + torch.arange(S)[None, None, :]


def make_ranges(shape, kind):
    """(B,T) int32 numpy.  valid: s_0 = 0, steps in [0, S-1], ending at U - S.  nonmonotone: in range, going down somewhere
    whenever T >= 2 and U > S.  clamped: entries -3 and U + 7 among in-range ones."""
    B, T, U, S, H = shape
    rng = np.random.default_rng(1000 * T + 10 * U + S)
    if kind == "valid":
        r = P.random_valid_ranges(np.full(B, T), np.full(B, U - 1), S, rng, T=T)
        d = np.diff(r, axis=1)
        assert (r[:, 0] == 0).all() and (r[:, -1] == U - S).all() and (d >= 0).all() and (d <= S - 1).all()
        return r
    r = rng.integers(0, U - S + 1, (B, T)).astype(np.int32)
    if kind == "nonmonotone":
        if shape == UNCOVERED_SHAPE:
            r[0] = np.where(rng.random(T) < 0.5, 0, U - S)       # batch 0: bands {0..3} and {5..8} only
        if T >= 2 and U > S:
            r[:, 0], r[:, 1] = U - S, 0
            assert (np.diff(r, axis=1) < 0).any()
        return r
    assert kind == "clamped"
    flat = r.reshape(-1)
    flat[::2] = -3
    flat[1::3] = U + 7
    return r


def covered(ranges, U, S):
    """(B,U) bool: row u lies in the band of at least one frame."""
    rows = band_rows(ranges, U, S)
    B = rows.shape[0]
    c = torch.zeros(B, U, dtype=torch.bool)
    for b in range(B):
        c[b, rows[b].reshape(-1)] = True
    return c


def _flat(e1, p1, eg, pg, ranges, S):
    """Every (b,t) as a one-frame batch of joint_common's references: e* (B*T,1,H), gathered p* (B*T,S,H)."""
    B, T, H = e1.shape
    U = p1.shape[1]
    rows = band_rows(ranges, U, S)                                             # (B,T,S)
    bidx = torch.arange(B)[:, None, None].expand(B, T, S)
    gp1, gpg = (p.double()[bidx, rows].reshape(B * T, S, H) for p in (p1, pg))
    return e1.double().reshape(B * T, 1, H), gp1, eg.double().reshape(B * T, 1, H), gpg, rows


def banded_gate_ref(e1, p1, eg, pg, ranges, S):
    """h (B,T,S,H) float64: joint_common.gate_ref on the gathered rows."""
    B, T, H = e1.shape
    fe1, gp1, feg, gpg, _ = _flat(e1, p1, eg, pg, ranges, S)
    return J.gate_ref(fe1, gp1, feg, gpg).reshape(B, T, S, H)


def banded_gate_bwd_ref(dh, e1, p1, eg, pg, ranges, S):
    """(de1, dp1, deg, dpg) float64: joint_common.gate_bwd_ref on the gathered rows (its "sum over u" is the sum over the
    band's rows, its "sum over t" has one term: dz of the row), the rows' dz summed back with index_add_ in float64."""
    B, T, H = e1.shape
    U = p1.shape[1]
    fe1, gp1, feg, gpg, rows = _flat(e1, p1, eg, pg, ranges, S)
    de1, dz1, deg, dzg = J.gate_bwd_ref(dh.double().reshape(B * T, 1, S, H), fe1, gp1, feg, gpg)
    out = []
    for dz in (dz1, dzg):
        dp = torch.zeros(B, U, H, dtype=torch.float64)
        dz = dz.reshape(B, T * S, H)
        for b in range(B):
            dp[b].index_add_(0, rows[b].reshape(-1), dz[b])
        out.append(dp)
    return de1.reshape(B, T, H), out[0], deg.reshape(B, T, H), out[1]


def pred_side_loop_ref(dz, ranges, U):
    """The definition of the prediction-side sum in plain loops: dp[b,u] = sum over t, in increasing t, of dz[b,t,u-s_t] for
    the frames with s_t <= u < s_t + S.  dz (B,T,S,H) float64."""
    B, T, S, H = dz.shape
    r = np.asarray(ranges)
    dp = torch.zeros(B, U, H, dtype=torch.float64)
    for b in range(B):
        for u in range(U):
            for t in range(T):
                s = min(max(int(r[b, t]), 0), U - S)
                if s <= u < s + S:
                    dp[b, u] += dz[b, t, u - s]
    return dp
