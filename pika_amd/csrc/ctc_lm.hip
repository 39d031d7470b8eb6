// pika_amd/csrc/ctc_lm.hip -- CTC prefix beam search with n-gram LM shallow fusion for gfx950 (MI355X), hand-written HIP
// (include/pika_ctc_lm.h).  The row pass of ctc_decode.hip is used as it is; this file holds the fused search.
//
//   search : one persistent 256-thread workgroup per utterance, the beam in LDS (double buffered), every slot with its
//            LM state (i32) and its bonus (fp64).  Per frame, wave 0 does the slot work of ctc_beam_kernel (lane = beam
//            slot: parent slot by node identity, the gather of the slot's own last label, the strike of classes whose
//            child is in the beam).  Then the n * candidates (+ n repeat) fresh children are spread over all lanes:
//            each is one FST lookup -- a bisection in global memory per state of the back-off chain -- whose fused
//            score, next state and increment go into LDS cells.  With an LM term a child's score is not monotone in
//            lp[c], so there is no "head of the class list": `beam` rounds of a workgroup arg-max over every open cell
//            and every stay follow, under the total order of the header; each thread keeps the best of its own cells
//            in registers and only the round's winner looks at its cells again.  Nodes, the trie table, the fp32
//            (p_b, p_nb) and the renormalisation are those of ctc_beam_kernel (helpers copied, that file is not
//            touched); the bonus is renormalised with tot.  The end applies the final cost, re-sorts by counting and
//            walks the table for the n-best.
//   Every loop over the FST has a fixed trip limit (header): a malformed table cannot spin the workgroup.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pika_ctc_lm.h"

namespace {

constexpr float NEG = -1.0e30f;  // "log zero": finite, so NEG+NEG / NEG-NEG never make NaN
constexpr float NEG_HALF = -0.5e30f;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_CAND = 128;
constexpr int MAX_BEAM = 64;
constexpr int MAX_HOPS = 8;
constexpr int RENORM = 8;
constexpr int CELLS_SMALL = 1024;                 // beam * candidates up to here: 12 KB of cells
constexpr int CELLS_LARGE = MAX_BEAM * MAX_CAND;  // 96 KB
constexpr int ROOT = 0x7ffffffe;                  // node of the empty prefix
constexpr int NONE = 0x7ffffffd;                  // its parent
constexpr int PENDING = -1;
constexpr unsigned NOKEY = 0xffffffffu;
constexpr unsigned long long EMPTY = ~0ull;

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline float addn(float a, float b) { return fmaxf(a + b, NEG); }

// log(exp(x)+exp(y)) on the transcendental pipe; NEG when both are "log zero"
__device__ inline float lse2(float x, float y) {
    const float m = fmaxf(x, y);
    if (!(m > NEG_HALF)) return NEG;
    const float e = __builtin_amdgcn_exp2f((x - m) * LOG2E) + __builtin_amdgcn_exp2f((y - m) * LOG2E);
    return m + LN2 * __builtin_amdgcn_logf(e);
}

__device__ inline unsigned long long trie_key(int parent, int token) {
    return ((unsigned long long)(unsigned)parent << 32) | (unsigned)token;
}

// insert-or-find: every probe is an atomic, so a slot is never seen through a stale cache line; only this workgroup
// touches the table
__device__ inline int trie_node(unsigned long long *table, unsigned mask, int parent, int token) {
    const unsigned long long key = trie_key(parent, token);
    unsigned h = ((unsigned)parent * 0x9E3779B1u) ^ ((unsigned)token * 0x85EBCA6Bu);
    h = (h ^ (h >> 15)) & mask;
    for (unsigned probes = 0; probes <= mask; ++probes) {  // at most T * beam <= (mask + 1) / 2 keys: it ends early
        const unsigned long long old = atomicCAS(&table[h], EMPTY, key);
        if (old == EMPTY || old == key) break;
        h = (h + 1) & mask;
    }
    return (int)h;
}

// (F, hi, lo) before (G, ghi, glo) in the total order: higher score, then the lower key
__device__ inline bool before(float F, unsigned hi, unsigned lo, float G, unsigned ghi, unsigned glo) {
    return F > G || (F == G && (hi < ghi || (hi == ghi && lo < glo)));
}

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

// ---------------------------------------------------------------------------------------------
// search.  grid = B, block = 256: wave 0's lane r owns beam slot r, every thread owns cells tid, tid + 256, ...
// ---------------------------------------------------------------------------------------------
struct Beam {
    int node[MAX_BEAM];   // the prefix: slot of its (parent, token) key in the utterance's table, ROOT for the empty one
    int last[MAX_BEAM];   // its last label, -1 for the empty prefix
    int pnode[MAX_BEAM];  // its parent's node
    int len[MAX_BEAM];
    int lmst[MAX_BEAM];   // its LM state
    float pb[MAX_BEAM], pnb[MAX_BEAM], tot[MAX_BEAM];
    double bonus[MAX_BEAM];  // lm_weight * LM + length_bonus * len, less the offset moved out
};

struct Args {
    const float *x;
    long long st, sb;
    const float *lse, *blank_lp, *top_val;
    const int *top_idx, *Tn;
    int B, T, beam, nbest, ncand, start, use_final;
    float lmw, lb;
    int *tokens, *lengths;
    float *scores, *am_scores;
    unsigned long long *table;
    unsigned mask;
};

template <int CELLS>
__global__ __launch_bounds__(THREADS) void ctc_lm_kernel(const Args a, const Fst f) {
    __shared__ Beam S[2];
    __shared__ float cv[MAX_CAND];
    __shared__ int ci[MAX_CAND];
    __shared__ unsigned excl[MAX_BEAM][MAX_CAND / 32];
    __shared__ int hasrep[MAX_BEAM];
    __shared__ float gs[MAX_BEAM];  // the value of the slot's own last label
    // fresh children: cell r * ncand + j is class ci[j] under slot r, cell n * ncand + r the repeat of slot r's last label
    __shared__ float cF[CELLS + MAX_BEAM];  // fused score, NEG: closed
    __shared__ int cN[CELLS + MAX_BEAM];    // next LM state
    __shared__ float cI[CELLS + MAX_BEAM];  // LM increment
    __shared__ float wF[2][WAVES];
    __shared__ unsigned wH[2][WAVES], wL[2][WAVES];
    __shared__ float fsc[MAX_BEAM];
    __shared__ int perm[MAX_BEAM];
    __shared__ int nlive_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool slots = w == 0;  // wave 0 does the slot work: its lane r owns beam slot r
    const int r = lane;
    const int B = a.B, T = a.T, beam = a.beam, ncand = a.ncand;
    const int Tn = clampi(a.Tn[b], 1, T);
    const double lmw = (double)a.lmw, lb = (double)a.lb;
    unsigned long long *table = a.table + (size_t)b * ((size_t)a.mask + 1);
    const unsigned mask = a.mask;
    const float *xb = a.x + (long long)b * a.sb;

    int cur = 0, n = 1;
    double off = 0.0, boff = 0.0;  // what was moved out of tot and of bonus (identical in every thread)
    if (tid == 0) {
        Beam &A = S[0];
        A.node[0] = ROOT; A.last[0] = -1; A.pnode[0] = NONE; A.len[0] = 0; A.lmst[0] = a.start;
        A.pb[0] = 0.0f; A.pnb[0] = NEG; A.tot[0] = 0.0f; A.bonus[0] = 0.0;
    }
    // the frame's compact row, fetched one frame ahead
    float pv = NEG, plb = NEG, pl = 0.0f;
    int pi = -1;
    auto fetch = [&](int t) __attribute__((always_inline)) {
        const size_t rb = (size_t)t * B + b;
        pv = tid < ncand ? a.top_val[rb * ncand + tid] : NEG;
        pi = tid < ncand ? a.top_idx[rb * ncand + tid] : -1;
        plb = a.blank_lp[rb];
        pl = a.lse ? a.lse[rb] : 0.0f;
    };
    fetch(0);
    for (int t = 0; t < Tn; ++t) {  // workgroup-uniform
        __syncthreads();            // the previous frame's beam is complete; cv / ci / excl / the cells are free
        const Beam &A = S[cur];
        Beam &N = S[cur ^ 1];
        if (tid < MAX_CAND) { cv[tid] = pv; ci[tid] = pi; }
        const float lpb = plb, l = pl;
        if (t + 1 < Tn) fetch(t + 1);
        // ---- slot work (wave 0; the other waves only meet the barriers)
        const bool act = slots && r < n;
        const int node_r = act ? A.node[r] : NONE, last_r = act ? A.last[r] : -1, pn_r = act ? A.pnode[r] : NONE;
        const float pb_r = act ? A.pb[r] : NEG, pnb_r = act ? A.pnb[r] : NEG, tot_r = act ? A.tot[r] : NEG;
        float g = NEG;  // the value of the slot's own last label: the one gather from the full row
        if (last_r >= 0) g = fmaxf(fmaxf(xb[(long long)t * a.st + last_r], NEG) - l, NEG);
        if (slots) {
            for (int q = 0; q < MAX_CAND / 32; ++q) excl[r][q] = 0;
            hasrep[r] = 0;
            gs[r] = g;
        }
        __syncthreads();
        float npb = NEG, npnb = NEG, s_stay = NEG;
        if (act) {
            int ps = -1;  // the parent's slot, if the parent is in the beam
            if (pn_r != NONE)
                for (int q = 0; q < n; ++q)
                    if (A.node[q] == pn_r) ps = q;
            int pos = -1;  // where the slot's last label stands in the frame's class list
            if (last_r >= 0)
                for (int j = 0; j < ncand; ++j)
                    if (ci[j] == last_r) pos = j;
            if (pos >= 0) {
                atomicOr(&excl[r][pos >> 5], 1u << (pos & 31));               // the repeat: its own cell, scored with p_b
                if (ps >= 0) atomicOr(&excl[ps][pos >> 5], 1u << (pos & 31));  // the parent's child that is in the beam
            }
            const bool rep_child = ps >= 0 && A.last[ps] == last_r;
            if (rep_child) hasrep[ps] = 1;
            npb = addn(lpb, tot_r);
            if (last_r >= 0) npnb = addn(g, pnb_r);
            if (ps >= 0) npnb = lse2(npnb, addn(g, rep_child ? A.pb[ps] : A.tot[ps]));
            s_stay = lse2(npb, npnb);
        }
        __syncthreads();  // excl, hasrep and gs are complete
        // ---- the fresh children: one FST lookup per open cell
        const int nl = n * ncand, ne = nl + n;
        float bF = NEG;  // the best of this thread's open candidates: (score, key); bE: its cell, -1 for the stay
        unsigned bH = NOKEY, bL = NOKEY;
        int bE = -1;
        bool stay_open = act && s_stay > NEG_HALF;
        const float F_stay = stay_open ? (float)((double)s_stay + A.bonus[r]) : NEG;
        if (stay_open) { bF = F_stay; bH = (unsigned)r; bL = 0; }
        // the slot, the class and the acoustic score of a cell
        auto cell = [&](int e, int &pr, int &cls, float &am) __attribute__((always_inline)) {
            bool ok;
            if (e < nl) {
                pr = e / ncand;
                const int j = e - pr * ncand;
                cls = ci[j];
                ok = cls >= 0 && !((excl[pr][j >> 5] >> (j & 31)) & 1u);
                am = addn(cv[j], A.tot[pr]);
            } else {
                pr = e - nl;
                cls = A.last[pr];
                ok = cls >= 0 && !hasrep[pr];
                am = addn(gs[pr], A.pb[pr]);
            }
            return ok && am > NEG_HALF;
        };
        for (int e = tid; e < ne; e += THREADS) {
            int pr, cls, next = -1;
            float am, inc = 0.0f, F = NEG;
            if (cell(e, pr, cls, am) && lm_step(f, A.lmst[pr], cls, inc, next)) {
                F = (float)((double)am + (A.bonus[pr] + lmw * (double)inc + lb));
                if (!(F > NEG_HALF)) F = NEG;  // also a NaN from a table that holds one
            }
            cF[e] = F;
            cN[e] = next;
            cI[e] = inc;
            if (F > NEG_HALF && before(F, 64u + (unsigned)pr, (unsigned)cls, bF, bH, bL)) {
                bF = F; bH = 64u + (unsigned)pr; bL = (unsigned)cls; bE = e;
            }
        }
        // ---- `beam` rounds of the workgroup's arg-max
        int k = 0;
        for (; k < beam; ++k) {  // workgroup-uniform
            float ws = bF;
            unsigned whi = bH, wlo = bL;
            for (int o = 32; o > 0; o >>= 1) {
                const float os = __shfl_xor(ws, o);
                const unsigned ohi = __shfl_xor(whi, o), olo = __shfl_xor(wlo, o);
                if (before(os, ohi, olo, ws, whi, wlo)) { ws = os; whi = ohi; wlo = olo; }
            }
            if (lane == 0) { wF[k & 1][w] = ws; wH[k & 1][w] = whi; wL[k & 1][w] = wlo; }
            __syncthreads();  // the one barrier of a round: round k + 1 writes the other buffer
            ws = wF[k & 1][0]; whi = wH[k & 1][0]; wlo = wL[k & 1][0];
            for (int v = 1; v < WAVES; ++v)
                if (before(wF[k & 1][v], wH[k & 1][v], wL[k & 1][v], ws, whi, wlo)) {
                    ws = wF[k & 1][v]; whi = wH[k & 1][v]; wlo = wL[k & 1][v];
                }
            if (!(ws > NEG_HALF)) break;  // nothing left: fewer prefixes exist than the beam holds
            if (bH != NOKEY && whi == bH && wlo == bL) {  // this thread's candidate won (keys are unique)
                if (bH < 64u) {
                    N.node[k] = node_r; N.last[k] = last_r; N.pnode[k] = pn_r; N.len[k] = A.len[r];
                    N.lmst[k] = A.lmst[r]; N.pb[k] = npb; N.pnb[k] = npnb; N.tot[k] = s_stay; N.bonus[k] = A.bonus[r];
                    stay_open = false;
                } else {
                    int pr, cls;
                    float am;
                    cell(bE, pr, cls, am);
                    N.node[k] = PENDING; N.last[k] = cls; N.pnode[k] = A.node[pr]; N.len[k] = A.len[pr] + 1;
                    N.lmst[k] = cN[bE]; N.pb[k] = NEG; N.pnb[k] = am; N.tot[k] = am;
                    N.bonus[k] = A.bonus[pr] + lmw * (double)cI[bE] + lb;
                    cF[bE] = NEG;
                }
                bF = NEG; bH = NOKEY; bL = NOKEY; bE = -1;  // the best of what this thread still has open
                if (stay_open) { bF = F_stay; bH = (unsigned)r; bL = 0; }
                for (int e = tid; e < ne; e += THREADS) {
                    const float F = cF[e];
                    if (!(F > NEG_HALF)) continue;
                    const int pr = e < nl ? e / ncand : e - nl;
                    const int cls = e < nl ? ci[e - pr * ncand] : A.last[pr];
                    if (before(F, 64u + (unsigned)pr, (unsigned)cls, bF, bH, bL)) {
                        bF = F; bH = 64u + (unsigned)pr; bL = (unsigned)cls; bE = e;
                    }
                }
            }
        }
        __syncthreads();  // the new beam's k slots are written
        if (slots && r < k && N.node[r] == PENDING) N.node[r] = trie_node(table, mask, N.pnode[r], N.last[r]);
        if (t % RENORM == RENORM - 1 && k > 0) {  // workgroup-uniform
            const float m = N.tot[0];             // slot 0 has the best fused score: its tot is finite
            const double mb = N.bonus[0];
            __syncthreads();
            if (slots && r < k) {
                N.pb[r] = N.pb[r] > NEG_HALF ? N.pb[r] - m : NEG;
                N.pnb[r] = N.pnb[r] > NEG_HALF ? N.pnb[r] - m : NEG;
                N.tot[r] = N.tot[r] - m;
                N.bonus[r] = N.bonus[r] - mb;
            }
            off += (double)m;
            boff += mb;
        }
        cur ^= 1;
        n = k;
    }
    __syncthreads();
    const Beam &A = S[cur];
    // ---- the end: the final cost, the order of the fp32 scores (ties: the rank before), the n-best
    float sc = -__builtin_inff();
    if (slots && r < n) {
        double s = off + boff + (double)A.tot[r] + A.bonus[r];
        bool live = true;
        if (a.use_final) {
            float inc;
            live = lm_final(f, A.lmst[r], inc);
            if (live) s += lmw * (double)inc;
        }
        if (live && (float)s > -__builtin_inff()) sc = (float)s;  // (a NaN is not alive)
    }
    if (slots) fsc[r] = sc;
    const unsigned long long alive = __ballot(sc > -__builtin_inff());
    if (tid == 0) nlive_s = __popcll(alive);  // wave 0 holds every slot
    __syncthreads();
    if (sc > -__builtin_inff()) {
        int rank = 0;
        for (int q = 0; q < n; ++q) rank += (fsc[q] > sc || (fsc[q] == sc && q < r)) ? 1 : 0;
        perm[rank] = r;
    }
    __syncthreads();
    const int nlive = nlive_s, nbest = a.nbest;
    if (slots && r < nbest) {
        const bool have = r < nlive;
        const int src = have ? perm[r] : 0;
        a.lengths[(size_t)b * nbest + r] = have ? A.len[src] : -1;
        a.scores[(size_t)b * nbest + r] = have ? fsc[src] : -__builtin_inff();
        a.am_scores[(size_t)b * nbest + r] = have ? (float)(off + (double)A.tot[src]) : -__builtin_inff();
    }
    for (int e = tid; e < nbest * T; e += THREADS) {
        const int kk = e / T, p = e - kk * T;
        if (kk >= nlive || p >= A.len[perm[kk]]) a.tokens[((size_t)b * nbest + kk) * T + p] = -1;
    }
    if (slots && r < nbest && r < nlive) {
        const int src = perm[r];
        int node = A.node[src];
        int *out = a.tokens + ((size_t)b * nbest + r) * T;
        for (int p = A.len[src] - 1; p >= 0 && node != ROOT; --p) {  // len <= T_n <= T: one label per frame at most
            const unsigned long long key =
                __hip_atomic_load(&table[(unsigned)node & mask], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            out[p] = (int)(unsigned)(key & 0xffffffffull);
            node = (int)(unsigned)(key >> 32);
        }
    }
}

int check_dims(int B, int T, int beam, int candidates) {
    if (B <= 0 || T <= 0 || beam <= 0 || candidates <= 0) return PIKA_EINVAL;
    if (beam > MAX_BEAM || candidates > MAX_CAND || B > 65535 || 2ll * T * beam > (1ll << 28)) return PIKA_ETOOBIG;
    return PIKA_OK;
}

size_t table_slots(int T, int beam) {
    size_t n = 64;
    while (n < 2 * (size_t)T * beam) n <<= 1;
    return n;
}

}  // namespace

extern "C" {

size_t pika_ctc_lm_scratch_bytes(int B, int T, int beam, int candidates) {
    if (check_dims(B, T, beam, candidates)) return 0;
    return 8 * (size_t)B * table_slots(T, beam);
}

int pika_ctc_lm_beam_search(const float *x, long long stride_t, long long stride_b, const float *lse,
                            const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths,
                            int B, int T, int C, int blank, int beam, int nbest, const long long *fst_offsets,
                            const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                            const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                            int label_offset, int candidates, float lm_weight, float length_bonus, int use_final,
                            int *tokens, int *lengths, float *scores, float *am_scores, void *scratch, void *stream) {
    if (B <= 0 || T <= 0 || C <= 0 || blank < 0 || blank >= C || nbest <= 0) return PIKA_EINVAL;
    if (num_states <= 0 || num_arcs < 0 || start < 0 || start >= num_states) return PIKA_EINVAL;
    if (int rc = check_dims(B, T, beam, candidates)) return rc;
    if (nbest > beam) return PIKA_ETOOBIG;
    if (!x || !blank_lp || !top_val || !top_idx || !input_lengths || !tokens || !lengths || !scores || !am_scores ||
        !scratch || !fst_offsets || !fst_final || (num_arcs > 0 && (!fst_ilabel || !fst_weight || !fst_nextstate)))
        return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t slots = table_slots(T, beam);
    if (hipError_t e = hipMemsetAsync(scratch, 0xff, 8 * (size_t)B * slots, s)) return (int)e;  // every key EMPTY
    const Args a = {x, stride_t, stride_b, lse, blank_lp, top_val, top_idx, input_lengths, B, T, beam, nbest,
                    candidates, start, use_final, lm_weight, length_bonus, tokens, lengths, scores, am_scores,
                    static_cast<unsigned long long *>(scratch), (unsigned)(slots - 1)};
    const Fst f = {fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                   label_offset};
    if (beam * candidates <= CELLS_SMALL)
        hipLaunchKernelGGL(ctc_lm_kernel<CELLS_SMALL>, dim3((unsigned)B), dim3(THREADS), 0, s, a, f);
    else
        hipLaunchKernelGGL(ctc_lm_kernel<CELLS_LARGE>, dim3((unsigned)B), dim3(THREADS), 0, s, a, f);
    return (int)hipGetLastError();
}

}  // extern "C"
