// pika_amd/csrc/ctc_decode.hip -- CTC decoding for gfx950 (MI355X), hand-written HIP: best path and exact prefix beam
// search over the full vocabulary (include/pika_ctc_decode.h).
//
//   rows   : one workgroup per (t, b) row with t < T_n; the only pass that reads the (T,B,C) input, once.  Online
//            max / sum for the log-sum-exp of the from-logits form (the grouping and the fixed tree of ctc_loss.hip's
//            gather), the blank's value, and the K best non-blank classes ordered (value descending, class ascending).
//            K = 1 is a workgroup arg-max.  K > 1: the K-th largest of the 256 per-thread maxima is a lower bound on the
//            row's K-th largest value, so one more pass over the row (staged in LDS while it was read; rows wider than
//            the stage are read again through the cache) keeps the few dozen values at or above it; the survivors are
//            ranked by counting.  More survivors than the pool holds (rows of near-equal values): the exact K-th key by
//            bisection with counting passes, ties at it resolved by a second bisection on the class (lowest first).
//   greedy : one workgroup per utterance; ballot prefix scan over the "starts a new non-blank run" flags, compacted
//            tokens and frames stored in frame order; the score is summed in fp64 by a fixed tree.
//   search : one persistent 64-lane workgroup per utterance, lane = beam slot, the beam in LDS (double buffered).  Per
//            frame: every slot finds its parent's slot (node identity), the position of its own last label in the
//            frame's class list, and strikes that position from its own list (the repeat is scored with p_b, as a
//            candidate of its own) and from its parent's (that child is in the beam: the contribution is added to it).
//            Then `beam` rounds of "wave arg-max over every slot's best open candidate" -- the stay, the repeat child,
//            the head of the slot's class list -- under the total order of the header.  Fresh winners get their node by
//            insert-or-find in the utterance's open-addressing table of (parent node, token) keys: the node IS the
//            table slot, so a prefix that left the beam and comes back is the same node and its children merge with a
//            descendant that stayed.  Numerics as the loss: fp32 (p_b, p_nb), the best tot moved into an fp64 offset
//            every RENORM frames.  The n-best back-trace walks the table in the same launch.  What ctc_lm.hip's fused
//            search does the same way (beam, trie, slot work, order, renormalisation, tail) is in ctc_search_core.h.
//   stream : the search with its state in device memory between launches: reset (ctc_search_core.h: one kernel for
//            this search's records and ctc_lm.hip's) writes the first beam and clears the table, advance runs a chunk's
//            frames through the frame body of the one-shot kernel (load, frames, store), results is the one-shot tail on
//            the stored beam and modifies nothing.

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ctc_search_core.h"
#include "pika_ctc_decode.h"

namespace {

constexpr int ROW_THREADS = 256;
constexpr int ROW_STAGE = 8192;  // classes of a row staged in LDS for the second look
constexpr int POOL_CAP = 1024;   // survivors ranked by counting

// order-preserving integer image of a finite float; 0 is below every image
__device__ inline unsigned fkey(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float funkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// ---------------------------------------------------------------------------------------------
// rows.  grid = (T, B), block = 256.
// ---------------------------------------------------------------------------------------------
template <bool TOPK>
__global__ __launch_bounds__(ROW_THREADS) void ctc_rows_kernel(const float *__restrict__ x, long long st, long long sb,
                                                               const int *__restrict__ Tn_, int B, int T, int C,
                                                               int blank, int K, int logits,
                                                               float *__restrict__ blank_lp, float *__restrict__ top_val,
                                                               int *__restrict__ top_idx, float *__restrict__ lse_out) {
    __shared__ float rm[ROW_THREADS], rs[ROW_THREADS];
    __shared__ unsigned tk[ROW_THREADS];
    __shared__ int ti[ROW_THREADS];
    __shared__ float stage[TOPK ? ROW_STAGE : 1];
    __shared__ unsigned pool_k[TOPK ? POOL_CAP : 1];
    __shared__ int pool_i[TOPK ? POOL_CAP : 1];
    __shared__ int red[ROW_THREADS / 64];
    __shared__ int pool_n;
    __shared__ unsigned bound;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Tn = clampi(Tn_[b], 1, T);
    if (t >= Tn) return;  // workgroup-uniform; rows t >= T_n are never read
    const float *row = x + (long long)t * st + (long long)b * sb;
    const size_t rb = (size_t)t * B + b;
    const bool staged = TOPK && C <= ROW_STAGE;

    float m = NEG, s = 0.0f;  // online max / sum of exp
    unsigned bk = 0;          // the thread's best non-blank key (0: none) and its class
    int bi = -1;
    auto take = [&](float v, int c) __attribute__((always_inline)) {
        v = fmaxf(v, NEG);
        if (logits) {
            const float mn = fmaxf(m, v);
            s = s * __expf(m - mn) + __expf(v - mn);
            m = mn;
        }
        if (TOPK && staged) stage[c] = v;
        const unsigned k = fkey(v);
        if (c != blank && k > bk) {  // a thread's classes ascend: strict > keeps the lowest class of equal values
            bk = k;
            bi = c;
        }
    };
    // a thread takes the groups of four classes tid, tid + 256, ... whichever way they are loaded, so nothing below
    // depends on the alignment of the row
    const bool vec = C % 4 == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0;  // workgroup-uniform
    for (int i = tid; i < (C + 3) / 4; i += ROW_THREADS) {
        if (vec) {
            const v4f v = reinterpret_cast<const v4f *>(row)[i];
            take(v.x, 4 * i); take(v.y, 4 * i + 1); take(v.z, 4 * i + 2); take(v.w, 4 * i + 3);
        } else {
            for (int k = 4 * i; k < min(4 * i + 4, C); ++k) take(row[k], k);
        }
    }
    float l = 0.0f;
    if (logits) {
        rm[tid] = m;
        rs[tid] = s;
        __syncthreads();
        for (int h = ROW_THREADS / 2; h > 0; h >>= 1) {  // fixed tree: the same value on every run
            if (tid < h) {
                const float m0 = rm[tid], m1 = rm[tid + h], mn = fmaxf(m0, m1);
                rs[tid] = rs[tid] * __expf(m0 - mn) + rs[tid + h] * __expf(m1 - mn);
                rm[tid] = mn;
            }
            __syncthreads();
        }
        l = rm[0] + logf(rs[0]);
    }
    if (tid == 0) {
        blank_lp[rb] = fmaxf(fmaxf(row[blank], NEG) - l, NEG);
        if (logits) lse_out[rb] = l;
    }
    tk[tid] = bk;
    ti[tid] = bi;
    __syncthreads();

    if constexpr (!TOPK) {  // K == 1: the workgroup's arg-max, equal values to the lower class
        for (int h = ROW_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) {
                const unsigned k1 = tk[tid + h];
                const int i1 = ti[tid + h];
                if (k1 > tk[tid] || (k1 == tk[tid] && (unsigned)i1 < (unsigned)ti[tid])) {
                    tk[tid] = k1;
                    ti[tid] = i1;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const bool any = ti[0] >= 0;
            top_val[rb] = any ? fmaxf(funkey(tk[0]) - l, NEG) : NEG;
            top_idx[rb] = any ? ti[0] : -1;
        }
    } else {
        const int need = min(K, C - 1);
        float *ov = top_val + rb * K;
        int *oi = top_idx + rb * K;
        for (int k = need + tid; k < K; k += ROW_THREADS) {  // fewer non-blank classes than K: padding
            ov[k] = NEG;
            oi[k] = -1;
        }
        if (need <= 0) return;  // workgroup-uniform
        // the need-th largest thread maximum: at least `need` values of the row lie at or above it
        {
            int above = 0;
            for (int j = 0; j < ROW_THREADS; ++j) {
                const unsigned kj = tk[j];
                above += (kj > bk || (kj == bk && j < tid)) ? 1 : 0;
            }
            if (tid == 0) pool_n = 0;
            if (above == need - 1) bound = bk;  // exactly one thread (need <= 128 < 256 threads)
        }
        __syncthreads();
        const unsigned long long lt = (1ull << lane) - 1ull;
        // one look at every non-blank class: counts the classes pred(key, class) holds for and, with `collect`, appends
        // them to the pool (in any order: the ranking below does not depend on it).  Returns the workgroup's count.
        auto scan = [&](auto pred, bool collect) __attribute__((always_inline)) {
            int cnt = 0;
            for (int c0 = 0; c0 < C; c0 += ROW_THREADS) {  // workgroup-uniform trip count
                const int c = c0 + tid;
                bool sel = false;
                unsigned k = 0;
                if (c < C && c != blank) {
                    k = fkey(staged ? stage[c] : fmaxf(row[c], NEG));
                    sel = pred(k, (unsigned)c);
                }
                if (collect) {
                    const unsigned long long mk = __ballot(sel);
                    int base = 0;
                    if (lane == 0 && mk) base = atomicAdd(&pool_n, __popcll(mk));
                    base = __shfl(base, 0);
                    const int p = base + __popcll(mk & lt);
                    if (sel && p < POOL_CAP) {
                        pool_k[p] = k;
                        pool_i[p] = c;
                    }
                }
                cnt += sel ? 1 : 0;
            }
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
            __syncthreads();  // the previous total is read
            if (lane == 0) red[w] = cnt;
            __syncthreads();
            return red[0] + red[1] + red[2] + red[3];
        };
        const unsigned lo = bound;
        int n = scan([&](unsigned k, unsigned) { return k >= lo; }, true);
        if (n > POOL_CAP) {  // workgroup-uniform: the exact selection
            unsigned kth = 0;  // the largest key with at least `need` keys at or above it
            for (int bit = 31; bit >= 0; --bit) {
                const unsigned mid = kth | (1u << bit);
                if (scan([&](unsigned k, unsigned) { return k >= mid; }, false) >= need) kth = mid;
            }
            const int rem = need - scan([&](unsigned k, unsigned) { return k > kth; }, false);
            const int n_eq = scan([&](unsigned k, unsigned) { return k == kth; }, false);
            unsigned cut = 0xffffffffu;  // classes below `cut` among the ties: the `rem` lowest
            if (n_eq > rem) {
                cut = 0;
                for (int bit = 31; bit >= 0; --bit) {
                    const unsigned mid = cut | (1u << bit);
                    if (scan([&](unsigned k, unsigned c) { return k == kth && c < mid; }, false) <= rem) cut = mid;
                }
            }
            if (tid == 0) pool_n = 0;
            __syncthreads();
            n = scan([&](unsigned k, unsigned c) { return k > kth || (k == kth && c < cut); }, true);
        }
        n = min(n, POOL_CAP);
        for (int e = tid; e < n; e += ROW_THREADS) {  // rank by counting: classes are unique, so are the ranks
            const unsigned ke = pool_k[e];
            const int ie = pool_i[e];
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const unsigned kj = pool_k[j];
                rank += (kj > ke || (kj == ke && pool_i[j] < ie)) ? 1 : 0;
            }
            if (rank < need) {
                ov[rank] = fmaxf(funkey(ke) - l, NEG);
                oi[rank] = ie;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// greedy.  grid = B, block = 256.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float *__restrict__ blank_lp,
                                                         const float *__restrict__ top_val,
                                                         const int *__restrict__ top_idx, const int *__restrict__ Tn_,
                                                         int B, int T, int blank, int *__restrict__ tokens,
                                                         int *__restrict__ lengths, float *__restrict__ scores,
                                                         int *__restrict__ frames) {
    __shared__ int wcnt[4];
    __shared__ double acc_s[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Tn = clampi(Tn_[b], 1, T);
    const unsigned long long lt = (1ull << lane) - 1ull;
    // the frame's arg-max over all classes: the blank against the best non-blank class, equal values to the lower class
    auto best = [&](int t, float &v) __attribute__((always_inline)) {
        const size_t rb = (size_t)t * B + b;
        const float bv = blank_lp[rb], tv = top_val[rb];
        const int c = top_idx[rb];
        const bool is_blank = c < 0 || bv > tv || (bv == tv && blank < c);
        v = is_blank ? bv : tv;
        return is_blank ? blank : c;
    };
    int base = 0;
    double acc = 0.0;
    for (int t0 = 0; t0 < Tn; t0 += 256) {  // workgroup-uniform
        const int t = t0 + tid;
        bool flag = false;
        int c = blank;
        if (t < Tn) {
            float v, pv;
            c = best(t, v);
            acc += (double)v;
            const int prev = t > 0 ? best(t - 1, pv) : -1;
            flag = c != blank && c != prev;
        }
        const unsigned long long mk = __ballot(flag);
        if (lane == 0) wcnt[w] = __popcll(mk);
        __syncthreads();
        int off = base;
        for (int j = 0; j < w; ++j) off += wcnt[j];
        if (flag) {
            const int p = off + __popcll(mk & lt);  // p <= t < T
            tokens[(size_t)b * T + p] = c;
            frames[(size_t)b * T + p] = t;
        }
        base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    acc_s[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {  // fixed tree
        if (tid < h) acc_s[tid] += acc_s[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        scores[b] = (float)acc_s[0];
        lengths[b] = base;
    }
    for (int p = base + tid; p < T; p += 256) {
        tokens[(size_t)b * T + p] = -1;
        frames[(size_t)b * T + p] = -1;
    }
}

// ---------------------------------------------------------------------------------------------
// the state of a stream (pika_ctc_decode.h): reset writes it, the advance loads and stores it, the results only read it
// ---------------------------------------------------------------------------------------------
using Rec = StreamRec<Beam>;
static_assert(sizeof(Rec) == PIKA_CTC_STREAM_RECORD_BYTES && offsetof(StreamHdr, frames) == PIKA_CTC_STREAM_FRAMES_OFFSET &&
                  offsetof(StreamHdr, overflow) == PIKA_CTC_STREAM_OVERFLOW_OFFSET,
              "the record the header documents");

// the beam of a record into LDS; a label outside the classes (a record that was never reset) is no label
__device__ __forceinline__ void load_beam(Beam &A, const Rec &R, const StreamHdr &h, int r, int C) {
    if (r < h.n) {
        copy_slot(A, R.beam, r);
        A.len[r] = clampi(A.len[r], 0, h.frames);
        if (A.last[r] < -1 || A.last[r] >= C) A.last[r] = -1;
    }
}

// the n-best of a beam with n slots: scores here; lengths, tokens and the back-trace by the shared tail, slots in beam
// order
template <bool CLIP>
__device__ __forceinline__ void beam_tail(const Beam &A, int n, double off, int r, int b, int T, int nbest, int *tokens,
                                          int *lengths, float *scores, const unsigned long long *table, unsigned mask) {
    if (r < nbest) scores[(size_t)b * nbest + r] = r < n ? (float)(off + (double)A.tot[r]) : -__builtin_inff();
    write_nbest<64, CLIP>(A, n, [](int q) { return q; }, r, b, T, nbest, tokens, lengths, table, mask);
}

// ---------------------------------------------------------------------------------------------
// search.  grid = B, block = 64: lane r owns beam slot r.
// ---------------------------------------------------------------------------------------------
// The search of utterance b = blockIdx.x, as the one-shot kernel (STREAM false: the first beam, the frames t < T_n, the
// n-best) and as the streaming advance (STREAM true: the beam of the stream's record, the frames of the chunk -- Tn_ its
// lengths, T its Tc; the outputs are not used -- and the beam back into the record).  One body, so the two cannot drift
// apart.
template <bool STREAM>
__device__ __forceinline__ void beam_search(const float *__restrict__ x, long long st, long long sb,
                                            const float *__restrict__ lse, const float *__restrict__ blank_lp,
                                            const float *__restrict__ top_val, const int *__restrict__ top_idx,
                                            const int *__restrict__ Tn_, int B, int T, int blank, int beam, int nbest,
                                            int *__restrict__ tokens, int *__restrict__ lengths,
                                            float *__restrict__ scores, unsigned long long *table_, unsigned mask,
                                            Rec *recs, int C, int max_frames) {
    __shared__ Beam S[2];
    __shared__ float cv[MAX_CLASSES];
    __shared__ int ci[MAX_CLASSES];
    __shared__ unsigned excl[MAX_BEAM][MAX_CLASSES / 32];
    __shared__ int hasrep[MAX_BEAM];
    const int b = blockIdx.x, r = threadIdx.x, K = 2 * beam;
    StreamHdr h = {};
    int Tn;
    if constexpr (STREAM) {
        h = load_hdr(recs[b].h, beam, max_frames);
        bool cut;
        Tn = stream_frames(Tn_, b, T, h.frames, max_frames, cut);
        // (not ordered against the other threads' load of the header above: nothing reads h.overflow)
        if (cut && r == 0) recs[b].h.overflow = 1;
        if (Tn <= 0) return;  // workgroup-uniform: nothing of this chunk is the stream's, the state stays as it is
    } else {
        Tn = clampi(Tn_[b], 1, T);
    }
    unsigned long long *table = table_ + (size_t)b * ((size_t)mask + 1);
    const float *xb = x + (long long)b * sb;

    int cur = 0, n = 1;
    double off = 0.0;  // sum of the subtracted maxima (identical in every lane)
    if constexpr (STREAM) {
        n = h.n; off = h.off;
        load_beam(S[0], recs[b], h, r, C);
    } else {
        if (r == 0) root_slot(S[0]);
    }
    // the frame's compact row, fetched one frame ahead
    float pv0 = NEG, pv1 = NEG, plb = NEG, pl = 0.0f;
    int pi0 = -1, pi1 = -1;
    auto fetch = [&](int t) __attribute__((always_inline)) {
        const size_t rb = (size_t)t * B + b;
        pv0 = r < K ? top_val[rb * K + r] : NEG;
        pi0 = r < K ? top_idx[rb * K + r] : -1;
        pv1 = r + 64 < K ? top_val[rb * K + r + 64] : NEG;
        pi1 = r + 64 < K ? top_idx[rb * K + r + 64] : -1;
        plb = blank_lp[rb];
        pl = lse ? lse[rb] : 0.0f;
    };
    fetch(0);
    for (int t = 0; t < Tn; ++t) {  // workgroup-uniform
        __syncthreads();            // the previous frame's beam is complete; cv / ci / excl are free
        const Beam &A = S[cur];
        Beam &N = S[cur ^ 1];
        cv[r] = pv0; ci[r] = pi0; cv[r + 64] = pv1; ci[r + 64] = pi1;
        const float lpb = plb, l = pl;
        if (t + 1 < Tn) fetch(t + 1);
        const bool act = r < n;
        const Slot me = load_slot(A, r, act);
        const int node_r = me.node, last_r = me.last, pn_r = me.pnode, len_r = me.len;
        const float pb_r = me.pb, tot_r = me.tot;
        float g = NEG;  // the value of the slot's own last label: the one gather from the full row
        if (last_r >= 0) g = fmaxf(fmaxf(xb[(long long)t * st + last_r], NEG) - l, NEG);
        float npb, npnb, s_stay;
        slot_work(A, n, r, true, me, ci, K, lpb, g, excl, hasrep, npb, npnb, s_stay);
        const float s_rep = (last_r >= 0 && !hasrep[r]) ? addn(g, pb_r) : NEG;
        bool stay_open = s_stay > NEG_HALF, rep_open = s_rep > NEG_HALF;
        int j = -1;  // head of the slot's class list
        auto advance = [&]() __attribute__((always_inline)) {
            do ++j; while (j < K && ci[j] >= 0 && ((excl[r][j >> 5] >> (j & 31)) & 1u));
        };
        advance();
        int k = 0;
        for (; k < beam; ++k) {  // workgroup-uniform
            // the slot's best open candidate.  order key: (0, rank, 0) for the stay, (1, parent rank, class) for fresh
            float bs = NEG;
            unsigned bhi = 0xffffffffu, blo = 0xffffffffu;
            int kind = -1;
            if (stay_open) { bs = s_stay; bhi = (unsigned)r; blo = 0; kind = 0; }
            float fs = NEG;
            unsigned fc = 0xffffffffu;
            int fk = -1;
            if (rep_open) { fs = s_rep; fc = (unsigned)last_r; fk = 1; }
            if (act && j < K && ci[j] >= 0) {
                const float hs = addn(cv[j], tot_r);
                if (hs > NEG_HALF && (fk < 0 || hs > fs || (hs == fs && (unsigned)ci[j] < fc))) {
                    fs = hs; fc = (unsigned)ci[j]; fk = 2;
                }
            }
            if (fk >= 0 && fs > bs) { bs = fs; bhi = 64u + (unsigned)r; blo = fc; kind = fk; }
            float ws = bs;
            unsigned whi = bhi, wlo = blo;
            for (int o = 32; o > 0; o >>= 1) {
                const float os = __shfl_xor(ws, o);
                const unsigned ohi = __shfl_xor(whi, o), olo = __shfl_xor(wlo, o);
                if (before(os, ohi, olo, ws, whi, wlo)) { ws = os; whi = ohi; wlo = olo; }
            }
            if (!(ws > NEG_HALF)) break;  // nothing left: fewer prefixes exist than the beam holds
            if (whi == bhi && wlo == blo && kind >= 0) {  // this slot's candidate won (keys are unique)
                if (kind == 0) {
                    N.node[k] = node_r; N.last[k] = last_r; N.pnode[k] = pn_r; N.len[k] = len_r;
                    N.pb[k] = npb; N.pnb[k] = npnb;
                    stay_open = false;
                } else {
                    N.node[k] = PENDING; N.last[k] = (int)blo; N.pnode[k] = node_r; N.len[k] = len_r + 1;
                    N.pb[k] = NEG; N.pnb[k] = bs;
                    if (kind == 1) rep_open = false;
                    else advance();
                }
                N.tot[k] = bs;
            }
        }
        __syncthreads();  // the new beam's k slots are written
        assign_node(N, r, r < k, table, mask);
        if (renorm_due(h.frames + t, k)) off += (double)renorm(N, r, r < k);
        cur ^= 1;
        n = k;
    }
    __syncthreads();
    const Beam &A = S[cur];
    if constexpr (STREAM) {  // the beam and what was moved out of it, back into the record
        Rec &R = recs[b];
        if (r < n) copy_slot(R.beam, A, r);
        if (r == 0) {
            R.h.n = n; R.h.frames = h.frames + Tn;
            R.h.off = off;
        }
    } else {
        beam_tail<false>(A, n, off, r, b, T, nbest, tokens, lengths, scores, table, mask);
    }
}

__global__ __launch_bounds__(64) void ctc_beam_kernel(const float *__restrict__ x, long long st, long long sb,
                                                      const float *__restrict__ lse, const float *__restrict__ blank_lp,
                                                      const float *__restrict__ top_val, const int *__restrict__ top_idx,
                                                      const int *__restrict__ Tn_, int B, int T, int blank, int beam,
                                                      int nbest, int *__restrict__ tokens, int *__restrict__ lengths,
                                                      float *__restrict__ scores, unsigned long long *table_,
                                                      unsigned mask) {
    beam_search<false>(x, st, sb, lse, blank_lp, top_val, top_idx, Tn_, B, T, blank, beam, nbest, tokens, lengths, scores,
                       table_, mask, nullptr, 0, 0);
}

// grid = B, block = 64, as the one-shot search
__global__ __launch_bounds__(64) void ctc_stream_advance_kernel(
    const float *__restrict__ x, long long st, long long sb, const float *__restrict__ lse,
    const float *__restrict__ blank_lp, const float *__restrict__ top_val, const int *__restrict__ top_idx,
    const int *__restrict__ len_, int B, int Tc, int C, int beam, unsigned long long *table_, unsigned mask, Rec *recs,
    int max_frames) {
    beam_search<true>(x, st, sb, lse, blank_lp, top_val, top_idx, len_, B, Tc, 0, beam, 0, nullptr, nullptr, nullptr,
                      table_, mask, recs, C, max_frames);
}

// grid = B, block = 64; reads the state only
__global__ __launch_bounds__(64) void ctc_stream_results_kernel(const Rec *__restrict__ recs,
                                                                const unsigned long long *table_, unsigned mask,
                                                                int beam, int max_frames, int nbest, int L,
                                                                int *__restrict__ tokens, int *__restrict__ lengths,
                                                                float *__restrict__ scores) {
    __shared__ Beam A;
    const int b = blockIdx.x, r = threadIdx.x;
    const Rec &R = recs[b];
    const StreamHdr h = load_hdr(R.h, beam, max_frames);
    load_beam(A, R, h, r, 0x7fffffff);
    __syncthreads();
    beam_tail<true>(A, h.n, h.off, r, b, L, nbest, tokens, lengths, scores, table_ + (size_t)b * ((size_t)mask + 1),
                    mask);
}

int check_rows(int B, int T, int C, int blank) {
    if (B <= 0 || T <= 0 || C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (B > 65535) return PIKA_ETOOBIG;  // B is a grid's y extent
    return PIKA_OK;
}

}  // namespace

extern "C" {

int pika_ctc_decode_rows(const float *x, long long stride_t, long long stride_b, const int *input_lengths, int B, int T,
                         int C, int blank, int K, int logits, float *blank_lp, float *top_val, int *top_idx, float *lse,
                         void *stream) {
    if (int rc = check_rows(B, T, C, blank)) return rc;
    if (K <= 0) return PIKA_EINVAL;
    if (K > MAX_CLASSES) return PIKA_ETOOBIG;
    if (!x || !input_lengths || !blank_lp || !top_val || !top_idx || (logits && !lse)) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)T, (unsigned)B);
    if (K == 1)
        hipLaunchKernelGGL(ctc_rows_kernel<false>, grid, dim3(ROW_THREADS), 0, s, x, stride_t, stride_b, input_lengths,
                           B, T, C, blank, K, logits, blank_lp, top_val, top_idx, lse);
    else
        hipLaunchKernelGGL(ctc_rows_kernel<true>, grid, dim3(ROW_THREADS), 0, s, x, stride_t, stride_b, input_lengths,
                           B, T, C, blank, K, logits, blank_lp, top_val, top_idx, lse);
    return (int)hipGetLastError();
}

int pika_ctc_greedy(const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths, int B,
                    int T, int C, int blank, int *tokens, int *lengths, float *scores, int *frames, void *stream) {
    if (int rc = check_rows(B, T, C, blank)) return rc;
    if (!blank_lp || !top_val || !top_idx || !input_lengths || !tokens || !lengths || !scores || !frames)
        return PIKA_EINVAL;
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), blank_lp,
                       top_val, top_idx, input_lengths, B, T, blank, tokens, lengths, scores, frames);
    return (int)hipGetLastError();
}

size_t pika_ctc_beam_scratch_bytes(int B, int T, int beam) {
    if (check_search_dims(B, T, beam, 1)) return 0;
    return table_bytes(B, T, beam);
}

int pika_ctc_beam_search(const float *x, long long stride_t, long long stride_b, const float *lse,
                         const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths,
                         int B, int T, int C, int blank, int beam, int nbest, int *tokens, int *lengths, float *scores,
                         void *scratch, void *stream) {
    if (int rc = check_rows(B, T, C, blank)) return rc;
    if (nbest <= 0) return PIKA_EINVAL;
    if (int rc = check_search_dims(B, T, beam, 1)) return rc;
    if (nbest > beam) return PIKA_ETOOBIG;
    if (!x || !blank_lp || !top_val || !top_idx || !input_lengths || !tokens || !lengths || !scores || !scratch)
        return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = clear_tables(scratch, B, T, beam, s)) return (int)e;
    hipLaunchKernelGGL(ctc_beam_kernel, dim3((unsigned)B), dim3(64), 0, s, x, stride_t, stride_b, lse, blank_lp, top_val,
                       top_idx, input_lengths, B, T, blank, beam, nbest, tokens, lengths, scores,
                       static_cast<unsigned long long *>(scratch), (unsigned)(table_slots(T, beam) - 1));
    return (int)hipGetLastError();
}

size_t pika_ctc_stream_state_bytes(int B, int max_frames, int beam) {
    if (check_search_dims(B, max_frames, beam, 1)) return 0;
    return table_bytes(B, max_frames, beam) + (size_t)B * sizeof(Rec);
}

int pika_ctc_stream_reset(void *state, int B, int max_frames, int beam, const int *which, void *stream) {
    return reset_streams<Beam>(state, B, max_frames, beam, 1, which, stream);
}

int pika_ctc_stream_advance(const float *x, long long stride_t, long long stride_b, const float *lse,
                            const float *blank_lp, const float *top_val, const int *top_idx, const int *chunk_lengths,
                            int B, int Tc, int C, int blank, int beam, void *state, int max_frames, void *stream) {
    if (int rc = check_rows(B, Tc, C, blank)) return rc;
    if (int rc = check_search_dims(B, max_frames, beam, 1)) return rc;
    if (2ll * Tc * beam > (1ll << 28)) return PIKA_ETOOBIG;  // the row arrays' index range, as in the one-shot search
    if (!x || !blank_lp || !top_val || !top_idx || !chunk_lengths || !state) return PIKA_EINVAL;
    hipLaunchKernelGGL(ctc_stream_advance_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), x,
                       stride_t, stride_b, lse, blank_lp, top_val, top_idx, chunk_lengths, B, Tc, C, beam,
                       static_cast<unsigned long long *>(state), (unsigned)(table_slots(max_frames, beam) - 1),
                       stream_recs<Rec>(state, B, max_frames, beam), max_frames);
    return (int)hipGetLastError();
}

int pika_ctc_stream_results(const void *state, int B, int max_frames, int beam, int nbest, int L, int *tokens,
                            int *lengths, float *scores, void *stream) {
    if (int rc = check_results_dims(B, max_frames, beam, 1, nbest, L)) return rc;
    if (!state || !tokens || !lengths || !scores) return PIKA_EINVAL;
    hipLaunchKernelGGL(ctc_stream_results_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream),
                       stream_recs<Rec>(state, B, max_frames, beam), static_cast<const unsigned long long *>(state),
                       (unsigned)(table_slots(max_frames, beam) - 1), beam, max_frames, nbest, L, tokens, lengths,
                       scores);
    return (int)hipGetLastError();
}

size_t pika_ctc_stream_commit_scratch_bytes(int B, int max_frames, int beam) {
    if (check_search_dims(B, max_frames, beam, 1)) return 0;
    return commit_scratch_bytes(B, max_frames, beam);
}

int pika_ctc_stream_commit(void *state, int B, int max_frames, int beam, const int *which, int max_tail, int L,
                           int *tokens, int *lengths, void *scratch, void *stream) {
    return commit_streams<Beam>(state, B, max_frames, beam, 1, which, max_tail, L, tokens, lengths, scratch, stream);
}

}  // extern "C"
