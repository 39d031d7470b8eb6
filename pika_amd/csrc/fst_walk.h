// pika_amd/csrc/fst_walk.h -- the device walk through an ilabel-sorted CSR back-off FST (the layout of pika_ctc_lm.h),
// shared by the searches that fuse one in (ctc_lm.hip: ctc_lm_kernel; msearch.hip: the fused frame step); not part of
// the C ABI.  Every loop has a fixed trip limit: a malformed table cannot spin a workgroup.
#ifndef PIKA_FST_WALK_H
#define PIKA_FST_WALK_H

#include <hip/hip_runtime.h>

namespace {

constexpr int MAX_HOPS = 8;

// ---------------------------------------------------------------------------------------------
// the LM: per-lane walks through the CSR table, vector loads (every lane its own state and label)
// ---------------------------------------------------------------------------------------------
struct Fst {
    const long long *off;
    const int *il;
    const float *w;
    const int *ns;
    const float *fin;
    int S, A, backoff, label_offset;
};

// the arcs of state s, clamped into the table; false: no such state
__device__ inline bool fst_range(const Fst &f, int s, int &lo, int &hi) {
    if ((unsigned)s >= (unsigned)f.S) return false;
    long long l = f.off[s], h = f.off[s + 1];
    l = l < 0 ? 0 : (l > f.A ? f.A : l);
    h = h < l ? l : (h > f.A ? f.A : h);
    lo = (int)l;
    hi = (int)h;
    return true;
}

// lower bound of `label` in [lo, hi): its arc, or -1.  hi - lo < 2^31: 32 halvings end it
__device__ inline int fst_find(const Fst &f, int lo, int hi, int label) {
    int a = lo, b = hi;
    for (int it = 0; it < 32 && a < b; ++it) {
        const int m = a + ((b - a) >> 1);
        if (f.il[m] < label) a = m + 1;
        else b = m;
    }
    return (a < hi && f.il[a] == label) ? a : -1;
}

// step(s, cls): false when the child does not exist
__device__ inline bool lm_step(const Fst &f, int s, int cls, float &inc, int &next) {
    const int label = cls + f.label_offset;
    double cost = 0.0;
    for (int hop = 0; hop <= MAX_HOPS; ++hop) {
        int lo, hi;
        if (!fst_range(f, s, lo, hi)) return false;
        const int a = fst_find(f, lo, hi, label);
        if (a >= 0) {
            next = f.ns[a];
            inc = (float)-(cost + (double)f.w[a]);
            return (unsigned)next < (unsigned)f.S;
        }
        const int b = fst_find(f, lo, hi, f.backoff);
        if (b < 0) return false;
        cost += (double)f.w[b];
        s = f.ns[b];
    }
    return false;
}

// final(s): the same walk to the first state with a finite final cost
__device__ inline bool lm_final(const Fst &f, int s, float &inc) {
    double cost = 0.0;
    for (int hop = 0; hop <= MAX_HOPS; ++hop) {
        int lo, hi;
        if (!fst_range(f, s, lo, hi)) return false;
        const float fw = f.fin[s];
        if (fw < __builtin_inff()) {  // false for +inf and NaN
            inc = (float)-(cost + (double)fw);
            return true;
        }
        const int b = fst_find(f, lo, hi, f.backoff);
        if (b < 0) return false;
        cost += (double)f.w[b];
        s = f.ns[b];
    }
    return false;
}

}  // namespace

#endif
