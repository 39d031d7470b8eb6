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
//            (p_b, p_nb) and the renormalisation are those of ctc_beam_kernel, shared through ctc_search_core.h;
//            the bonus is renormalised with tot.  The end applies the final cost, re-sorts by counting and
//            walks the table for the n-best.
//   stream : the search with its state in device memory between launches: reset (the one kernel of ctc_search_core.h,
//            here on the LM's records) writes the first beam and clears the table, advance runs a chunk's frames
//            through the frame body of the one-shot kernel (load, frames, store), results is the one-shot end -- final
//            cost and new order on the side -- on the stored beam, which it only reads.
//   bias   : the same kernel template with a second automaton (pika_ctc_lm2_*): a slot carries a second state, a fresh
//            child walks both FSTs and exists only when both reach it; the cells stay as they are -- the winners of a
//            frame (at most `beam`) walk the second FST again at node assignment, lane = slot, to get the state and to
//            complete the bonus.  The one-FST instantiations have no trace of it (if constexpr).
//   host   : the nine arguments of an automaton are packed once (make_fst, make_bias) and checked by one set of helpers
//            (check_fst and its halves); the one-shot search, the advance and the results are one template each over
//            "a Bias or none", so a pika_ctc_lm_* and a pika_ctc_lm2_* entry point differ in what they pack.
//   Every loop over the FST has a fixed trip limit (header): a malformed table cannot spin the workgroup.

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "pika_ctc_lm.h"
#include "ctc_search_core.h"
#include "fst_walk.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int CELLS_SMALL = 1024;                    // beam * candidates up to here: 12 KB of cells
constexpr int CELLS_LARGE = MAX_BEAM * MAX_CLASSES;  // 96 KB
constexpr unsigned NOKEY = 0xffffffffu;

// ---------------------------------------------------------------------------------------------
// search.  grid = B, block = 256: wave 0's lane r owns beam slot r, every thread owns cells tid, tid + 256, ...
// ---------------------------------------------------------------------------------------------
struct LmBeam : Beam {
    // (bonus before lmst: measured 2% faster than the other order, profiles/ctc_search_refactor.txt)
    double bonus[MAX_BEAM];  // lm_weight * LM + length_bonus * len, less the offset moved out
    int lmst[MAX_BEAM];      // its LM state
};

// the beam a search starts from: the empty prefix in slot 0, in the LM's start state
__device__ __forceinline__ void root_slot(LmBeam &A, int start) {
    A.node[0] = ROOT; A.last[0] = -1; A.pnode[0] = NONE; A.len[0] = 0; A.lmst[0] = start;
    A.pb[0] = 0.0f; A.pnb[0] = NEG; A.tot[0] = 0.0f; A.bonus[0] = 0.0;
}

__device__ __forceinline__ void copy_slot(LmBeam &D, const LmBeam &G, int r) {
    copy_slot(static_cast<Beam &>(D), static_cast<const Beam &>(G), r);
    D.lmst[r] = G.lmst[r];
    D.bonus[r] = G.bonus[r];
}

__device__ __forceinline__ void move_slot(LmBeam &D, int j, const LmBeam &G, int r) {
    move_slot(static_cast<Beam &>(D), j, static_cast<const Beam &>(G), r);
    D.lmst[j] = G.lmst[r];
    D.bonus[j] = G.bonus[r];
}

// the beam of the search with a second automaton; bonus holds both terms
struct Lm2Beam : LmBeam {
    int st2[MAX_BEAM];  // its state in the second FST
};

__device__ __forceinline__ void root_slot(Lm2Beam &A, int start, int start2) {
    root_slot(static_cast<LmBeam &>(A), start);
    A.st2[0] = start2;
}

__device__ __forceinline__ void copy_slot(Lm2Beam &D, const Lm2Beam &G, int r) {
    copy_slot(static_cast<LmBeam &>(D), static_cast<const LmBeam &>(G), r);
    D.st2[r] = G.st2[r];
}

__device__ __forceinline__ void move_slot(Lm2Beam &D, int j, const Lm2Beam &G, int r) {
    move_slot(static_cast<LmBeam &>(D), j, static_cast<const LmBeam &>(G), r);
    D.st2[j] = G.st2[r];
}

// the second automaton of a launch: a kernel takes none or one as its last argument
struct Bias {
    Fst f;
    int start;
    float w;
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

// ---------------------------------------------------------------------------------------------
// the state of a stream (pika_ctc_lm.h): reset writes it, the advance loads and stores it, the results only read it
// ---------------------------------------------------------------------------------------------
using Rec = StreamRec<LmBeam>;
using Rec2 = StreamRec<Lm2Beam>;
static_assert(sizeof(Rec) == PIKA_CTC_LM_STREAM_RECORD_BYTES && offsetof(StreamHdr, frames) == PIKA_CTC_STREAM_FRAMES_OFFSET &&
                  offsetof(StreamHdr, overflow) == PIKA_CTC_STREAM_OVERFLOW_OFFSET,
              "the record the header documents");
static_assert(sizeof(Rec2) == PIKA_CTC_LM2_STREAM_RECORD_BYTES && sizeof(Rec2) == sizeof(Rec) + MAX_BEAM * sizeof(int) &&
                  sizeof(Rec2) % 8 == 0,
              "the LM record, then the second states");

// the beam of a record into LDS (wave 0: lane r loads slot r); a label outside the classes (a record that was never
// reset) is no label
template <class BeamT>
__device__ __forceinline__ void load_beam(BeamT &A, const StreamRec<BeamT> &R, const StreamHdr &h, int tid, int C) {
    if (tid < h.n) {
        copy_slot(A, R.beam, tid);
        A.len[tid] = clampi(A.len[tid], 0, h.frames);
        if (A.last[tid] < -1 || A.last[tid] >= C) A.last[tid] = -1;
    }
}

// The search of utterance b = blockIdx.x in its three forms, one kernel template.  ONE_SHOT: the first beam, the frames t < T_n, the end.
// ADVANCE: the beam of the stream's record, the frames of the chunk (a.Tn its lengths, a.T its Tc; the outputs of `a`
// are not used), the beam back into the record.  RESULTS: the beam of the record, no frame, the end with a.T the token
// width; the record is only read -- the final term and the new order live in fsc / perm.  One body, so the forms cannot
// drift apart, and the one-shot kernel is the code it was before the other two existed.
enum Mode { ONE_SHOT, ADVANCE, RESULTS };

// BIAS: nothing, or one `Bias` -- the second automaton (TWO).
template <class... BIAS>
using BeamOf = std::conditional_t<sizeof...(BIAS) == 1, Lm2Beam, LmBeam>;

__device__ __forceinline__ const Bias *bias_of() { return nullptr; }
__device__ __forceinline__ const Bias *bias_of(const Bias &g) { return &g; }

// grid = B, block = 256.  recs, C and max_frames serve the two streaming forms only.
template <int CELLS, Mode MODE, class... BIAS>
__global__ __launch_bounds__(THREADS) void ctc_lm_kernel(const Args a, const Fst f, StreamRec<BeamOf<BIAS...>> *recs, int C,
                                                         int max_frames, const BIAS... bias) {
    static_assert(sizeof...(BIAS) <= 1, "none or one second automaton");
    constexpr bool TWO = sizeof...(BIAS) == 1;
    using BeamT = BeamOf<BIAS...>;
    const Bias *const second = bias_of(bias...);  // TWO: the kernel's own argument
    __shared__ BeamT S[2];
    __shared__ float cv[MAX_CLASSES];
    __shared__ int ci[MAX_CLASSES];
    __shared__ unsigned excl[MAX_BEAM][MAX_CLASSES / 32];
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
    StreamHdr h = {};
    int Tn = 0;
    if constexpr (MODE != ONE_SHOT) h = load_hdr(recs[b].h, beam, max_frames);
    if constexpr (MODE == ADVANCE) {
        bool cut;
        Tn = stream_frames(a.Tn, b, T, h.frames, max_frames, cut);
        // (not ordered against the other threads' load of the header above: nothing reads h.overflow)
        if (cut && tid == 0) recs[b].h.overflow = 1;
        if (Tn <= 0) return;  // workgroup-uniform: nothing of this chunk is the stream's, the state stays as it is
    }
    if constexpr (MODE == ONE_SHOT) Tn = clampi(a.Tn[b], 1, T);
    const double lmw = (double)a.lmw, lb = (double)a.lb;
    double bw = 0.0;
    if constexpr (TWO) bw = (double)second->w;
    unsigned long long *table = a.table + (size_t)b * ((size_t)a.mask + 1);
    const unsigned mask = a.mask;
    const float *xb = a.x + (long long)b * a.sb;

    int cur = 0, n = 1;
    double off = 0.0, boff = 0.0;  // what was moved out of tot and of bonus (identical in every thread)
    if constexpr (MODE != ONE_SHOT) {
        n = h.n; off = h.off; boff = h.boff;
        load_beam(S[0], recs[b], h, tid, C);
    } else {
        if constexpr (TWO) {
            if (tid == 0) root_slot(S[0], a.start, second->start);
        } else {
            if (tid == 0) root_slot(S[0], a.start);
        }
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
    if constexpr (MODE != RESULTS) fetch(0);
    for (int t = 0; t < Tn; ++t) {  // workgroup-uniform (RESULTS: no frame)
        __syncthreads();            // the previous frame's beam is complete; cv / ci / excl / the cells are free
        const BeamT &A = S[cur];
        BeamT &N = S[cur ^ 1];
        if (tid < MAX_CLASSES) { cv[tid] = pv; ci[tid] = pi; }
        const float lpb = plb, l = pl;
        if (t + 1 < Tn) fetch(t + 1);
        // ---- slot work (wave 0; the other waves only meet its barriers)
        const bool act = slots && r < n;
        const Slot me = load_slot(A, r, act);
        const int node_r = me.node, last_r = me.last, pn_r = me.pnode;
        float g = NEG;  // the value of the slot's own last label: the one gather from the full row
        if (last_r >= 0) g = fmaxf(fmaxf(xb[(long long)t * a.st + last_r], NEG) - l, NEG);
        if (slots) gs[r] = g;
        float npb, npnb, s_stay;
        slot_work(A, n, r, slots, me, ci, ncand, lpb, g, excl, hasrep, npb, npnb, s_stay);  // gs is complete too
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
                if constexpr (TWO) {  // the child exists when both automata reach it; the cell keeps the first's walk
                    float inc2;
                    int next2;
                    if (lm_step(second->f, A.st2[pr], cls, inc2, next2))
                        F = (float)((double)am + (A.bonus[pr] + lmw * (double)inc + bw * (double)inc2 + lb));
                } else {
                    F = (float)((double)am + (A.bonus[pr] + lmw * (double)inc + lb));
                }
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
                    if constexpr (TWO) N.st2[k] = A.st2[r];
                    stay_open = false;
                } else {
                    int pr, cls;
                    float am;
                    cell(bE, pr, cls, am);
                    N.node[k] = PENDING; N.last[k] = cls; N.pnode[k] = A.node[pr]; N.len[k] = A.len[pr] + 1;
                    N.lmst[k] = cN[bE]; N.pb[k] = NEG; N.pnb[k] = am; N.tot[k] = am;
                    if constexpr (TWO) {  // the parent's values: the slot's owner finishes both below
                        N.bonus[k] = A.bonus[pr] + lmw * (double)cI[bE];
                        N.st2[k] = A.st2[pr];
                    } else {
                        N.bonus[k] = A.bonus[pr] + lmw * (double)cI[bE] + lb;
                    }
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
        if constexpr (TWO) {
            // a fresh winner walks the second FST once more -- the walk its cell made, from the same state -- for the
            // state and the rest of its bonus: at most `beam` lookups side by side, next to the trie's atomics
            if (slots && r < k && N.node[r] == PENDING) {
                float inc2 = 0.0f;
                int next2 = -1;
                if (!lm_step(second->f, N.st2[r], N.last[r], inc2, next2)) next2 = -1;  // (it reached the child before)
                N.st2[r] = next2;
                N.bonus[r] = N.bonus[r] + bw * (double)inc2 + lb;
            }
        }
        assign_node(N, r, slots && r < k, table, mask);
        if (renorm_due(h.frames + t, k)) {  // (one-shot: h.frames is the constant 0)
            if constexpr (TWO) __syncthreads();  // slot 0's bonus is complete
            const double mb = N.bonus[0];  // slot 0 has the best fused score; read before renorm()'s barrier
            off += (double)renorm(N, r, slots && r < k);
            if (slots && r < k) N.bonus[r] = N.bonus[r] - mb;
            boff += mb;
        }
        cur ^= 1;
        n = k;
    }
    __syncthreads();
    const BeamT &A = S[cur];
    if constexpr (MODE == ADVANCE) {  // the beam and what was moved out of it, back into the record
        StreamRec<BeamT> &R = recs[b];
        if (tid < n) copy_slot(R.beam, A, tid);
        if (tid == 0) {
            R.h.n = n; R.h.frames = h.frames + Tn;
            R.h.off = off; R.h.boff = boff;
        }
        return;
    }
    // ---- the end: the final cost, the order of the fp32 scores (ties: the rank before), the n-best
    float sc = -__builtin_inff();
    if (slots && r < n) {
        double s = off + boff + (double)A.tot[r] + A.bonus[r];
        bool live = true;
        if (a.use_final) {
            float inc;
            live = lm_final(f, A.lmst[r], inc);
            if (live) s += lmw * (double)inc;
            if constexpr (TWO) {
                if (live) {
                    live = lm_final(second->f, A.st2[r], inc);
                    if (live) s += bw * (double)inc;
                }
            }
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
        a.scores[(size_t)b * nbest + r] = have ? fsc[src] : -__builtin_inff();
        a.am_scores[(size_t)b * nbest + r] = have ? (float)(off + (double)A.tot[src]) : -__builtin_inff();
    }
    write_nbest<THREADS, MODE == RESULTS>(A, nlive, [&](int q) { return perm[q]; }, tid, b, T, nbest, a.tokens, a.lengths, table, mask);
}

// ---------------------------------------------------------------------------------------------
// host: an entry point packs its automata (make_fst, make_bias) and is checks and one launch -- the three forms of the
// search as templates over "a Bias or none", the reset through reset_streams of ctc_search_core.h.  The checks of an
// automaton exist once: bad_start / fst_dims_bad for its sizes, fst_missing for its arrays, check_fst for both.
// ---------------------------------------------------------------------------------------------
static inline Fst make_fst(const long long *off, const int *il, const float *w, const int *ns, const float *fin, int S,
                           int A, int backoff, int label_offset) {
    return {off, il, w, ns, fin, S, A, backoff, label_offset};
}

// the second automaton of a pika_ctc_lm2_* call; a call without a start state passes 0
static inline Bias make_bias(const Fst &f, int start, float w) { return {f, start, w}; }

// S states and a start state among them.  A call that has no start state passes 0, which every table holds.
static inline bool bad_start(int S, int start) { return S <= 0 || start < 0 || start >= S; }

static inline bool fst_dims_bad(const Fst &f, int start) { return f.A < 0 || bad_start(f.S, start); }

static inline bool fst_missing(const Fst &f) { return !f.off || !f.fin || (f.A > 0 && (!f.il || !f.w || !f.ns)); }

// Sizes and arrays in one: the second automaton's check, ahead of everything else.  The first automaton's two halves
// stand apart in the forms below, the limits (PIKA_ETOOBIG) between them, as the entry points always answered.
static inline int check_fst(const Fst &f, int start) {
    return fst_dims_bad(f, start) || fst_missing(f) ? PIKA_EINVAL : PIKA_OK;
}

template <Mode MODE, class... BIAS>
static int launch(bool small, int B, hipStream_t s, const Args &a, const Fst &f, StreamRec<BeamOf<BIAS...>> *recs, int C,
                  int max_frames, const BIAS &...g) {
    if (MODE == RESULTS || small)  // (the results have no cells)
        hipLaunchKernelGGL((ctc_lm_kernel<CELLS_SMALL, MODE, BIAS...>), dim3((unsigned)B), dim3(THREADS), 0, s, a, f, recs,
                           C, max_frames, g...);
    else if constexpr (MODE != RESULTS)
        hipLaunchKernelGGL((ctc_lm_kernel<CELLS_LARGE, MODE, BIAS...>), dim3((unsigned)B), dim3(THREADS), 0, s, a, f, recs,
                           C, max_frames, g...);
    return (int)hipGetLastError();
}

template <class... BIAS>
static int beam_search(const float *x, long long stride_t, long long stride_b, const float *lse, const float *blank_lp,
                       const float *top_val, const int *top_idx, const int *input_lengths, int B, int T, int C, int blank,
                       int beam, int nbest, const Fst &f, int start, int candidates, float lm_weight, float length_bonus,
                       int use_final, int *tokens, int *lengths, float *scores, float *am_scores, void *scratch,
                       void *stream, const BIAS &...g) {
    if (B <= 0 || T <= 0 || C <= 0 || blank < 0 || blank >= C || nbest <= 0) return PIKA_EINVAL;
    if (fst_dims_bad(f, start)) return PIKA_EINVAL;
    if (int rc = check_search_dims(B, T, beam, candidates)) return rc;
    if (nbest > beam) return PIKA_ETOOBIG;
    if (!x || !blank_lp || !top_val || !top_idx || !input_lengths || !tokens || !lengths || !scores || !am_scores ||
        !scratch || fst_missing(f))
        return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = clear_tables(scratch, B, T, beam, s)) return (int)e;
    const Args a = {x, stride_t, stride_b, lse, blank_lp, top_val, top_idx, input_lengths, B, T, beam, nbest,
                    candidates, start, use_final, lm_weight, length_bonus, tokens, lengths, scores, am_scores,
                    static_cast<unsigned long long *>(scratch), (unsigned)(table_slots(T, beam) - 1)};
    return launch<ONE_SHOT, BIAS...>(beam * candidates <= CELLS_SMALL, B, s, a, f, nullptr, 0, 0, g...);
}

template <class... BIAS>
static int stream_advance(const float *x, long long stride_t, long long stride_b, const float *lse, const float *blank_lp,
                          const float *top_val, const int *top_idx, const int *chunk_lengths, int B, int Tc, int C,
                          int blank, int beam, const Fst &f, int candidates, float lm_weight, float length_bonus,
                          void *state, int max_frames, void *stream, const BIAS &...g) {
    if (B <= 0 || Tc <= 0 || C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (fst_dims_bad(f, 0)) return PIKA_EINVAL;
    if (int rc = check_search_dims(B, max_frames, beam, candidates)) return rc;
    if (2ll * Tc * beam > (1ll << 28)) return PIKA_ETOOBIG;  // the row arrays' index range, as in the one-shot search
    if (!x || !blank_lp || !top_val || !top_idx || !chunk_lengths || !state || fst_missing(f))
        return PIKA_EINVAL;
    const Args a = {x, stride_t, stride_b, lse, blank_lp, top_val, top_idx, chunk_lengths, B, Tc, beam, 0, candidates,
                    0, 0, lm_weight, length_bonus, nullptr, nullptr, nullptr, nullptr,
                    static_cast<unsigned long long *>(state), (unsigned)(table_slots(max_frames, beam) - 1)};
    return launch<ADVANCE, BIAS...>(beam * candidates <= CELLS_SMALL, B, static_cast<hipStream_t>(stream), a, f,
                                    stream_recs<StreamRec<BeamOf<BIAS...>>>(state, B, max_frames, beam), C, max_frames, g...);
}

template <class... BIAS>
static int stream_results(const void *state, int B, int max_frames, int beam, int candidates, const Fst &f,
                          float lm_weight, int use_final, int nbest, int L, int *tokens, int *lengths, float *scores,
                          float *am_scores, void *stream, const BIAS &...g) {
    if (fst_dims_bad(f, 0)) return PIKA_EINVAL;
    if (int rc = check_results_dims(B, max_frames, beam, candidates, nbest, L)) return rc;
    if (!state || !tokens || !lengths || !scores || !am_scores || fst_missing(f))
        return PIKA_EINVAL;
    const Args a = {nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, B, L, beam, nbest, candidates, 0, use_final,
                    lm_weight, 0.0f, tokens, lengths, scores, am_scores,
                    static_cast<unsigned long long *>(const_cast<void *>(state)),
                    (unsigned)(table_slots(max_frames, beam) - 1)};
    return launch<RESULTS, BIAS...>(true, B, static_cast<hipStream_t>(stream), a, f,
                                    stream_recs<StreamRec<BeamOf<BIAS...>>>(state, B, max_frames, beam), 0x7fffffff,
                                    max_frames, g...);
}

}  // namespace

extern "C" {

size_t pika_ctc_lm_scratch_bytes(int B, int T, int beam, int candidates) {
    if (check_search_dims(B, T, beam, candidates)) return 0;
    return table_bytes(B, T, beam);
}

int pika_ctc_lm_beam_search(const float *x, long long stride_t, long long stride_b, const float *lse,
                            const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths,
                            int B, int T, int C, int blank, int beam, int nbest, const long long *fst_offsets,
                            const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                            const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                            int label_offset, int candidates, float lm_weight, float length_bonus, int use_final,
                            int *tokens, int *lengths, float *scores, float *am_scores, void *scratch, void *stream) {
    const Fst f = make_fst(fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                           label_offset);
    return beam_search(x, stride_t, stride_b, lse, blank_lp, top_val, top_idx, input_lengths, B, T, C, blank, beam, nbest,
                       f, start, candidates, lm_weight, length_bonus, use_final, tokens, lengths, scores, am_scores,
                       scratch, stream);
}

size_t pika_ctc_lm_stream_state_bytes(int B, int max_frames, int beam, int candidates) {
    if (check_search_dims(B, max_frames, beam, candidates)) return 0;
    return table_bytes(B, max_frames, beam) + (size_t)B * sizeof(Rec);
}

int pika_ctc_lm_stream_reset(void *state, int B, int max_frames, int beam, int candidates, int num_states, int start,
                             const int *which, void *stream) {
    if (bad_start(num_states, start)) return PIKA_EINVAL;
    return reset_streams<LmBeam>(state, B, max_frames, beam, candidates, which, stream, start);
}

int pika_ctc_lm_stream_advance(const float *x, long long stride_t, long long stride_b, const float *lse,
                               const float *blank_lp, const float *top_val, const int *top_idx,
                               const int *chunk_lengths, int B, int Tc, int C, int blank, int beam,
                               const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                               const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                               int backoff_id, int label_offset, int candidates, float lm_weight, float length_bonus,
                               void *state, int max_frames, void *stream) {
    const Fst f = make_fst(fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                           label_offset);
    return stream_advance(x, stride_t, stride_b, lse, blank_lp, top_val, top_idx, chunk_lengths, B, Tc, C, blank, beam, f,
                          candidates, lm_weight, length_bonus, state, max_frames, stream);
}

int pika_ctc_lm_stream_results(const void *state, int B, int max_frames, int beam, int candidates,
                               const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                               const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                               int backoff_id, int label_offset, float lm_weight, int use_final, int nbest, int L,
                               int *tokens, int *lengths, float *scores, float *am_scores, void *stream) {
    const Fst f = make_fst(fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                           label_offset);
    return stream_results(state, B, max_frames, beam, candidates, f, lm_weight, use_final, nbest, L, tokens, lengths,
                          scores, am_scores, stream);
}

size_t pika_ctc_lm_stream_commit_scratch_bytes(int B, int max_frames, int beam, int candidates) {
    if (check_search_dims(B, max_frames, beam, candidates)) return 0;
    return commit_scratch_bytes(B, max_frames, beam);
}

int pika_ctc_lm_stream_commit(void *state, int B, int max_frames, int beam, int candidates, const int *which,
                              int max_tail, int L, int *tokens, int *lengths, void *scratch, void *stream) {
    return commit_streams<LmBeam>(state, B, max_frames, beam, candidates, which, max_tail, L, tokens, lengths, scratch,
                                  stream);
}

// ---- the same with a second automaton ----------------------------------------------------------------------------

size_t pika_ctc_lm2_scratch_bytes(int B, int T, int beam, int candidates) {
    return pika_ctc_lm_scratch_bytes(B, T, beam, candidates);
}

int pika_ctc_lm2_beam_search(const float *x, long long stride_t, long long stride_b, const float *lse,
                             const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths,
                             int B, int T, int C, int blank, int beam, int nbest, const long long *fst_offsets,
                             const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                             const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                             int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                             const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                             int num_states2, int num_arcs2, int start2, int backoff_id2, int label_offset2,
                             int candidates, float lm_weight, float bias_weight, float length_bonus, int use_final,
                             int *tokens, int *lengths, float *scores, float *am_scores, void *scratch, void *stream) {
    const Fst f = make_fst(fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                           label_offset);
    const Bias g = make_bias(make_fst(fst2_offsets, fst2_ilabel, fst2_weight, fst2_nextstate, fst2_final, num_states2,
                                      num_arcs2, backoff_id2, label_offset2), start2, bias_weight);
    if (int rc = check_fst(g.f, g.start)) return rc;
    return beam_search(x, stride_t, stride_b, lse, blank_lp, top_val, top_idx, input_lengths, B, T, C, blank, beam, nbest,
                       f, start, candidates, lm_weight, length_bonus, use_final, tokens, lengths, scores, am_scores,
                       scratch, stream, g);
}

size_t pika_ctc_lm2_stream_state_bytes(int B, int max_frames, int beam, int candidates) {
    if (check_search_dims(B, max_frames, beam, candidates)) return 0;
    return table_bytes(B, max_frames, beam) + (size_t)B * sizeof(Rec2);
}

int pika_ctc_lm2_stream_reset(void *state, int B, int max_frames, int beam, int candidates, int num_states, int start,
                              int num_states2, int start2, const int *which, void *stream) {
    if (bad_start(num_states, start) || bad_start(num_states2, start2)) return PIKA_EINVAL;
    return reset_streams<Lm2Beam>(state, B, max_frames, beam, candidates, which, stream, start, start2);
}

int pika_ctc_lm2_stream_advance(const float *x, long long stride_t, long long stride_b, const float *lse,
                                const float *blank_lp, const float *top_val, const int *top_idx,
                                const int *chunk_lengths, int B, int Tc, int C, int blank, int beam,
                                const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                                const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                                int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                                const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                                int num_states2, int num_arcs2, int backoff_id2, int label_offset2, int candidates,
                                float lm_weight, float bias_weight, float length_bonus, void *state, int max_frames,
                                void *stream) {
    const Fst f = make_fst(fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                           label_offset);
    const Bias g = make_bias(make_fst(fst2_offsets, fst2_ilabel, fst2_weight, fst2_nextstate, fst2_final, num_states2,
                                      num_arcs2, backoff_id2, label_offset2), 0, bias_weight);
    if (int rc = check_fst(g.f, g.start)) return rc;
    return stream_advance(x, stride_t, stride_b, lse, blank_lp, top_val, top_idx, chunk_lengths, B, Tc, C, blank, beam, f,
                          candidates, lm_weight, length_bonus, state, max_frames, stream, g);
}

int pika_ctc_lm2_stream_results(const void *state, int B, int max_frames, int beam, int candidates,
                                const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                                const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                                int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                                const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                                int num_states2, int num_arcs2, int backoff_id2, int label_offset2, float lm_weight,
                                float bias_weight, int use_final, int nbest, int L, int *tokens, int *lengths,
                                float *scores, float *am_scores, void *stream) {
    const Fst f = make_fst(fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                           label_offset);
    const Bias g = make_bias(make_fst(fst2_offsets, fst2_ilabel, fst2_weight, fst2_nextstate, fst2_final, num_states2,
                                      num_arcs2, backoff_id2, label_offset2), 0, bias_weight);
    if (int rc = check_fst(g.f, g.start)) return rc;
    return stream_results(state, B, max_frames, beam, candidates, f, lm_weight, use_final, nbest, L, tokens, lengths,
                          scores, am_scores, stream, g);
}

size_t pika_ctc_lm2_stream_commit_scratch_bytes(int B, int max_frames, int beam, int candidates) {
    return pika_ctc_lm_stream_commit_scratch_bytes(B, max_frames, beam, candidates);
}

int pika_ctc_lm2_stream_commit(void *state, int B, int max_frames, int beam, int candidates, const int *which,
                               int max_tail, int L, int *tokens, int *lengths, void *scratch, void *stream) {
    return commit_streams<Lm2Beam>(state, B, max_frames, beam, candidates, which, max_tail, L, tokens, lengths, scratch,
                                   stream);
}

}  // extern "C"
