// pika_amd/csrc/msearch.hip -- the one-symbol-per-frame ("modified") transducer beam search of include/pika_msearch.h:
// the state blob, the frame step, and the read-out of the beams through the trie of token sequences (the trie is the
// open-addressing table of ctc_search_core.h).
//
// The frame step is one 256-thread workgroup per utterance.  It has to find the K best of the K V candidates
// score[k] + lp[k,v] exactly, in a total order, with one pass over the rows from memory:
//   1  rows: wave w takes rows w, w + 4, ...; one pass gives the row's (max, sum exp) online and, per lane, the best
//      element among those the lane read.  The 64 lane maxima of a row are real candidates; they go to LDS in order.
//   2  threshold: wave 0 merges the K sorted lists for K rounds (lane r holds row r's head); the K-th pop is a
//      candidate with at least K candidates at or before it in the total order, so the K best are all at or before it.
//   3  collect: a second pass (the rows now come from the cache) keeps what is at or before the threshold, typically
//      between K and a few K elements, in an LDS list; each entry's rank is the number of entries before it.
//      When the list overflows -- the large values of the rows all sat on the elements of a few lanes -- the K best
//      are taken one at a time instead, K arg-max passes: slow, exact, bounded.
//   4  keys, merge, sort: at most 64 entries, wave 0.
// Every comparison is in the total order (value, k, v), so ties cost nothing and the result is a function of the input.
//
// The step with n-gram LM / hotword fusion (include/pika_msearch_lm.h) is the same kernel template with NFST = 1 or 2
// automata: stages 1-3 select C = candidates >= K entries by F[k] + lp[k,v]; in stage 4 thread j walks the automata for
// entry j (fst_walk.h), entries merge by key on their acoustic scores and the groups are ordered by the fused score.
// The plain instantiation (NFST = 0) has no trace of it (if constexpr).
//
// The step with a neural LM (include/pika_msearch_nn.h) is the same template again with DENSE: a row of LM logits per old
// slot.  The wave that takes acoustic row k in stage 1 takes LM row k right behind it, the same pass (row_stats) for the
// row's max and log-sum-exp; stage 4 adds the third increment.  The fused search's blob, with or without automata.
//
// Streaming (include/pika_msearch_stream.h): the side record and msearch_commit_kernel, one template for the two blobs,
// which emits the labels every slot shares, re-roots and rebuilds the trie and lowers `frames`.
//
// Time stamps (include/pika_msearch_times.h): a record of emission frames per slot that lives beside either blob and
// follows the (parent, token) pairs of the step; its kernels only read the blobs.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "ctc_search_core.h"
#include "fst_walk.h"
#include "pika_msearch.h"
#include "pika_msearch_lm.h"
#include "pika_msearch_nn.h"
#include "pika_msearch_stream.h"
#include "pika_msearch_times.h"

static_assert(ROOT == PIKA_MSEARCH_ROOT && MAX_BEAM == PIKA_MSEARCH_MAX_BEAM, "the constants the C ABI documents");

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int LIST_CAP = 1024;  // entries the collect pass can hold
constexpr float NINF = -INFINITY;

// where the parts of the blob lie; score is the value the step ranks by (the fused search's F).  The fused search's
// blob has am, bonus and the automata's states as well
struct Blob {
    float *score;
    int *node, *len, *frames, *overflowed;
    unsigned long long *tables;
    float *am;
    double *bonus;
    int *lmst, *lmst2;
};

__host__ __device__ inline size_t head_bytes(int B, int K) {
    return (12 * (size_t)B * K + 8 * (size_t)B + 15) & ~(size_t)15;
}

__host__ __device__ inline Blob blob_of(void *state, int B, int K) {
    char *p = static_cast<char *>(state);
    Blob s;
    s.score = reinterpret_cast<float *>(p);
    s.node = reinterpret_cast<int *>(p + 4 * (size_t)B * K);
    s.len = reinterpret_cast<int *>(p + 8 * (size_t)B * K);
    s.frames = reinterpret_cast<int *>(p + 12 * (size_t)B * K);
    s.overflowed = s.frames + B;
    s.tables = reinterpret_cast<unsigned long long *>(p + head_bytes(B, K));
    s.am = nullptr; s.bonus = nullptr; s.lmst = nullptr; s.lmst2 = nullptr;
    return s;
}

// the fused search's blob (pika_msearch_lm.h)
__host__ __device__ inline size_t lm_head_bytes(int B, int K) {
    return (32 * (size_t)B * K + 8 * (size_t)B + 15) & ~(size_t)15;
}

__host__ __device__ inline Blob lm_blob_of(void *state, int B, int K) {
    char *p = static_cast<char *>(state);
    const size_t BK = (size_t)B * K;
    Blob s;
    s.bonus = reinterpret_cast<double *>(p);
    s.score = reinterpret_cast<float *>(p + 8 * BK);
    s.am = reinterpret_cast<float *>(p + 12 * BK);
    s.node = reinterpret_cast<int *>(p + 16 * BK);
    s.len = reinterpret_cast<int *>(p + 20 * BK);
    s.lmst = reinterpret_cast<int *>(p + 24 * BK);
    s.lmst2 = reinterpret_cast<int *>(p + 28 * BK);
    s.frames = reinterpret_cast<int *>(p + 32 * BK);
    s.overflowed = s.frames + B;
    s.tables = reinterpret_cast<unsigned long long *>(p + lm_head_bytes(B, K));
    return s;
}

// what a launch of the fused search takes beside the plain one's arguments: the automata, the weights and C.  The plain
// search takes the empty one.
template <int NFST>
struct Fused {
    Fst f[NFST];
    float lmw, bw, lb;
    int C;
};

template <>
struct Fused<0> {};

// ... and with DENSE the rows of the neural LM (pika_msearch_nn.h).  lb and C are the dense launch's own -- there may be
// no automaton to carry them -- and hide Fused's: the kernel reads fu.lb and fu.C whatever the variant.
template <int NFST, bool DENSE>
struct Step : Fused<NFST> {};

template <int NFST>
struct Step<NFST, true> : Fused<NFST> {
    const float *rows;
    long long rld;
    int VL, off, rvec;
    float scale, nnw, lb;
    int C;
};

template <int NFST>
__host__ __device__ inline Blob blob_of(void *state, int B, int K) {
    if constexpr (NFST == 0) return blob_of(state, B, K);
    else return lm_blob_of(state, B, K);
}

// a candidate: its value and where it came from
struct Cand {
    float c;
    int k, v;
};

__device__ __forceinline__ bool cand_before(const Cand &a, const Cand &b) {
    return before(a.c, (unsigned)a.k, (unsigned)a.v, b.c, (unsigned)b.k, (unsigned)b.v);
}

// the better of two candidates over the wave; every lane ends with the wave's best
__device__ __forceinline__ Cand wave_best(Cand a) {
    for (int o = 32; o > 0; o >>= 1) {
        Cand p = {__shfl_xor(a.c, o), __shfl_xor(a.k, o), __shfl_xor(a.v, o)};
        if (cand_before(p, a)) a = p;
    }
    return a;
}

// f(v, logit) for the elements of a row that this lane owns; `vec`: 16-byte loads (wave-uniform)
template <class F>
__device__ __forceinline__ void for_row(const float *__restrict__ row, int V, int lane, bool vec, F f) {
    if (vec) {
        const int V4 = V >> 2;
        for (int i = lane; i < V4; i += 64) {
            const v4f q = reinterpret_cast<const v4f *>(row)[i];
            f(4 * i, q.x); f(4 * i + 1, q.y); f(4 * i + 2, q.z); f(4 * i + 3, q.w);
        }
        for (int v = 4 * V4 + lane; v < V; v += 64) f(v, row[v]);
    } else {
        for (int v = lane; v < V; v += 64) f(v, row[v]);
    }
}

// x[k,v]: the product and the difference are rounded apart wherever the value is formed
__device__ __forceinline__ float scaled(float l, int v, int blank, float sm_scale, float penalty) {
    const float x = __fmul_rn(sm_scale, l);
    return v == blank ? __fsub_rn(x, penalty) : x;
}

// cand[k,v] from x, the row's maximum and log(sum exp(x - max)); -inf for a masked class and for a dead row
__device__ __forceinline__ float cand_of(float score, float x, float m, float logs) {
    if (!(x > NINF) || !(m > NINF)) return NINF;
    return __fadd_rn(score, __fsub_rn(__fsub_rn(x, m), logs));
}

// One pass of a wave over a row: x = xf(v, logit) for every element, each(v, x) sees it behind the sums.  -> the row's
// max and log(sum exp(x - max)) in every lane: each lane folds its own elements online, in the order it reads them, the
// 64 lanes are combined by lane 0's xor tree.  Elements that are -inf or NaN take no part.
template <class X, class E>
__device__ __forceinline__ void row_stats(const float *__restrict__ row, int V, int lane, bool vec, X xf, E each,
                                          float &m_out, float &logs_out) {
    float m = NINF, s = 0.0f;
    for_row(row, V, lane, vec, [&](int v, float l) {
        const float x = xf(v, l);
        if (x > m) {
            s = __fadd_rn(__fmul_rn(s, expf(m - x)), 1.0f);
            m = x;
        } else if (x > NINF) {
            s += expf(x - m);
        }
        each(v, x);
    });
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        const float M = fmaxf(m, m2);
        if (M > NINF) {
            const float a = m > NINF ? __fmul_rn(s, expf(m - M)) : 0.0f;
            const float c = m2 > NINF ? __fmul_rn(s2, expf(m2 - M)) : 0.0f;
            s = __fadd_rn(a, c);
        }
        m = M;
    }
    m_out = __shfl(m, 0);
    logs_out = logf(__shfl(s, 0));
}

// LM: the fused search's blob; slot 0 starts in the automata's start states
template <bool LM>
__global__ __launch_bounds__(THREADS) void msearch_reset_kernel(void *state, int B, int K, size_t slots,
                                                                 const int *__restrict__ which, int start, int start2) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;  // workgroup-uniform
    const Blob s = blob_of<LM ? 1 : 0>(state, B, K);
    unsigned long long *table = s.tables + (size_t)b * slots;
    for (size_t i = (size_t)blockIdx.y * THREADS + threadIdx.x; i < slots; i += (size_t)gridDim.y * THREADS)
        table[i] = EMPTY;
    if (blockIdx.y == 0) {
        const int k = threadIdx.x;
        if (k < K) {
            s.score[(size_t)b * K + k] = k == 0 ? 0.0f : NINF;
            s.node[(size_t)b * K + k] = ROOT;
            s.len[(size_t)b * K + k] = 0;
            if constexpr (LM) {
                s.am[(size_t)b * K + k] = k == 0 ? 0.0f : NINF;
                s.bonus[(size_t)b * K + k] = 0.0;
                s.lmst[(size_t)b * K + k] = start;
                s.lmst2[(size_t)b * K + k] = start2;
            }
        }
        if (k == 0) { s.frames[b] = 0; s.overflowed[b] = 0; }
    }
}

// NFST: the automata fused in (0: the plain step of pika_msearch.h; 1, 2: the step of pika_msearch_lm.h); DENSE: the
// rows of a neural LM beside them (pika_msearch_nn.h; NFST = 0, 1, 2).  NSEL is the number of entries stages 1-3 select:
// K, or the fused step's C.
template <int NFST, bool DENSE>
__global__ __launch_bounds__(THREADS) void msearch_advance_kernel(void *state, const float *__restrict__ logits,
                                                                   long long ld, const long long *__restrict__ num_frames,
                                                                   int B, int K, int max_frames, int V, int blank,
                                                                   float sm_scale, float penalty, unsigned mask, int vec,
                                                                   long long *__restrict__ parent_out,
                                                                   long long *__restrict__ token_out,
                                                                   const Step<NFST, DENSE> fu) {
    constexpr bool LM = NFST > 0 || DENSE;
    constexpr int NL = LM ? MAX_BEAM : 1;  // the fused step's arrays: per old slot, and per selected entry
    __shared__ float s_am[NL], s_G[NL], s_nm[DENSE ? MAX_BEAM : 1], s_ns[DENSE ? MAX_BEAM : 1];
    __shared__ double s_bonus[NL], s_cbonus[NL];
    __shared__ int s_st[NL], s_st2[NL], s_cst[NL], s_cst2[NL];
    __shared__ float s_score[MAX_BEAM], s_m[MAX_BEAM], s_logs[MAX_BEAM];
    __shared__ int s_node[MAX_BEAM], s_len[MAX_BEAM];
    __shared__ float pool_c[MAX_BEAM][64];  // per row, the lane maxima in order
    __shared__ int pool_v[MAX_BEAM][64];
    __shared__ float list_c[LIST_CAP];
    __shared__ int list_kv[LIST_CAP][2];
    __shared__ Cand s_thr, s_sel[MAX_BEAM], s_part[WAVES];
    __shared__ int s_all, s_cnt, s_nsel, s_key[MAX_BEAM], s_klen[MAX_BEAM], s_lead[MAX_BEAM], s_from[MAX_BEAM];
    __shared__ float s_merged[MAX_BEAM];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Blob st = blob_of<LM ? 1 : 0>(state, B, K);
    const size_t bk = (size_t)b * K;
    int NSEL = K;
    if constexpr (LM) NSEL = clampi(fu.C, K, MAX_BEAM);
    const long long nf_raw = num_frames[b];
    const int nf = (int)(nf_raw < 0 ? 0 : (nf_raw > max_frames ? max_frames : nf_raw));
    const int frames = st.frames[b];
    if (!(frames >= 0 && frames < nf)) {  // workgroup-uniform: the utterance is not active
        if (tid < K) { parent_out[bk + tid] = tid; token_out[bk + tid] = blank; }
        if (tid == 0 && frames >= max_frames && nf_raw > max_frames) st.overflowed[b] = 1;
        return;
    }
    unsigned long long *table = st.tables + (size_t)b * ((size_t)mask + 1);
    if (tid < K) {
        s_score[tid] = st.score[bk + tid];
        s_node[tid] = st.node[bk + tid];
        s_len[tid] = clampi(st.len[bk + tid], 0, max_frames);
        if constexpr (LM) {  // (a state outside its table: lm_step finds no child; clamped all the same)
            s_am[tid] = st.am[bk + tid];
            s_bonus[tid] = st.bonus[bk + tid];
            if constexpr (NFST >= 1) s_st[tid] = clampi(st.lmst[bk + tid], 0, fu.f[0].S - 1);
            if constexpr (NFST == 2) s_st2[tid] = clampi(st.lmst2[bk + tid], 0, fu.f[1].S - 1);
        }
    }
    if (tid == 0) { s_cnt = 0; s_all = 0; }
    __syncthreads();

    // 1  the rows
    for (int k = wave; k < K; k += WAVES) {
        const float score = s_score[k];
        if (!(score > NINF)) continue;  // wave-uniform: an empty slot
        const float *row = logits + (bk + k) * ld;
        float m, logs, bx = NINF;
        int bv = 0x7fffffff;
        row_stats(
            row, V, lane, vec != 0, [&](int v, float l) { return scaled(l, v, blank, sm_scale, penalty); },
            [&](int v, float x) {
                if (x > bx) { bx = x; bv = v; }
            },
            m, logs);
        if (lane == 0) { s_m[k] = m; s_logs[k] = logs; }
        // the lane maxima in the total order, by counting; lanes that read nothing hold equal keys and keep their own
        // order, so the ranks are a permutation and every entry of the row's list is written
        const Cand mine = {cand_of(score, bx, m, logs), k, bv};
        int rank = 0;
        for (int j = 0; j < 64; ++j) {
            const Cand o = {__shfl(mine.c, j), k, __shfl(mine.v, j)};
            rank += (cand_before(o, mine) || (!cand_before(mine, o) && j < lane)) ? 1 : 0;
        }
        pool_c[k][rank] = mine.c;
        pool_v[k][rank] = mine.v;
        if constexpr (DENSE) {  // the LM's row of the same slot: M and S of y = nn_scale * lm_logits (a dead slot's is not read)
            float M, S;
            row_stats(
                fu.rows + (bk + k) * fu.rld, fu.VL, lane, fu.rvec != 0, [&](int, float l) { return __fmul_rn(fu.scale, l); },
                [](int, float) {}, M, S);
            if (lane == 0) { s_nm[k] = M; s_ns[k] = S; }
        }
    }
    __syncthreads();

    // 2  the threshold: the K-th of the lane maxima of all rows
    if (wave == 0) {
        const bool row_live = lane < K && s_score[lane] > NINF;
        int head = 0;
        Cand thr = {NINF, 0, 0};
        bool all = false;
        for (int r = 0; r < NSEL; ++r) {
            Cand h = {NINF, lane, 0x7fffffff};
            if (row_live && head < 64) { h.c = pool_c[lane][head]; h.v = pool_v[lane][head]; }
            const Cand w = wave_best(h);
            if (!(w.c > NINF)) { all = true; break; }  // fewer than K lane maxima exist: everything finite is kept
            thr = w;
            if (lane == w.k) ++head;
        }
        if (lane == 0) { s_thr = thr; s_all = all ? 1 : 0; }
    }
    __syncthreads();

    // 3  collect what is at or before the threshold
    const Cand thr = s_thr;
    const bool all = s_all != 0;
    for (int k = wave; k < K; k += WAVES) {
        const float score = s_score[k];
        if (!(score > NINF)) continue;
        const float m = s_m[k], logs = s_logs[k];
        if (!(m > NINF)) continue;  // a row of -inf: the slot dies
        const float *row = logits + (bk + k) * ld;
        for_row(row, V, lane, vec != 0, [&](int v, float l) {
            const Cand e = {cand_of(score, scaled(l, v, blank, sm_scale, penalty), m, logs), k, v};
            if (e.c > NINF && (all || !cand_before(thr, e))) {
                const int i = atomicAdd(&s_cnt, 1);
                if (i < LIST_CAP) { list_c[i] = e.c; list_kv[i][0] = k; list_kv[i][1] = v; }
            }
        });
    }
    __syncthreads();
    const int n = s_cnt;  // workgroup-uniform
    if (n <= LIST_CAP) {
        for (int i = tid; i < n; i += THREADS) {
            const Cand e = {list_c[i], list_kv[i][0], list_kv[i][1]};
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const Cand o = {list_c[j], list_kv[j][0], list_kv[j][1]};
                rank += cand_before(o, e) ? 1 : 0;
            }
            if (rank < NSEL) s_sel[rank] = e;
        }
        if (tid == 0) s_nsel = n < NSEL ? n : NSEL;
        __syncthreads();
    } else {
        // the list overflowed: the K best one at a time, each the best of what comes after the one before
        Cand prev = {INFINITY, -1, -1};
        int got = 0;
        for (int r = 0; r < NSEL; ++r) {
            Cand best = {NINF, 0x7fffffff, 0x7fffffff};
            for (int k = wave; k < K; k += WAVES) {
                const float score = s_score[k];
                if (!(score > NINF)) continue;
                const float m = s_m[k], logs = s_logs[k];
                if (!(m > NINF)) continue;
                const float *row = logits + (bk + k) * ld;
                for_row(row, V, lane, vec != 0, [&](int v, float l) {
                    const Cand e = {cand_of(score, scaled(l, v, blank, sm_scale, penalty), m, logs), k, v};
                    if (e.c > NINF && cand_before(prev, e) && cand_before(e, best)) best = e;
                });
            }
            best = wave_best(best);
            if (lane == 0) s_part[wave] = best;
            __syncthreads();
            best = s_part[0];
            for (int w = 1; w < WAVES; ++w)
                if (cand_before(s_part[w], best)) best = s_part[w];
            __syncthreads();              // s_part is read: the next round may write it
            if (!(best.c > NINF)) break;  // workgroup-uniform: nothing is left
            if (tid == 0) s_sel[r] = best;
            prev = best;
            got = r + 1;
        }
        if (tid == 0) s_nsel = got;
        __syncthreads();
    }

    // 4  keys, merge, order: entry j of the selection is thread j's
    const int nsel = s_nsel;
    if (tid < NSEL) { s_key[tid] = NONE; s_lead[tid] = 0; }
    __syncthreads();
    Cand me = {NINF, 0, blank};
    if (tid < nsel) {
        me = s_sel[tid];
        me.k = clampi(me.k, 0, K - 1);
        const int pn = s_node[me.k];
        bool exists = true;
        if constexpr (LM) {
            // the entry's acoustic score a' = am[k] + lp[k,v] (the one logit again, from the cache), then the walks: an
            // entry that an automaton does not reach keeps the key NONE and the value -inf, and makes no node
            me.v = clampi(me.v, 0, V - 1);
            const float x = scaled(logits[(bk + me.k) * ld + me.v], me.v, blank, sm_scale, penalty);
            me.c = __fadd_rn(s_am[me.k], __fsub_rn(__fsub_rn(x, s_m[me.k]), s_logs[me.k]));
            double bonus = s_bonus[me.k];
            int n1 = 0, n2 = 0;
            if constexpr (NFST >= 1) n1 = s_st[me.k];
            if constexpr (NFST == 2) n2 = s_st2[me.k];
            if (me.v != blank) {
                if constexpr (NFST >= 1) {
                    float inc = 0.0f;
                    exists = lm_step(fu.f[0], n1, me.v, inc, n1) && inc - inc == 0.0f;  // (false for +-inf and NaN)
                    bonus = __dadd_rn(bonus, __dmul_rn((double)fu.lmw, (double)inc));
                }
                if constexpr (NFST == 2) {
                    float inc2 = 0.0f;
                    exists = exists && lm_step(fu.f[1], n2, me.v, inc2, n2) && inc2 - inc2 == 0.0f;
                    bonus = __dadd_rn(bonus, __dmul_rn((double)fu.bw, (double)inc2));
                }
                if constexpr (DENSE) {
                    // the label's class in the LM's row: outside it, a row without a finite maximum or a non-finite
                    // increment and the entry does not exist; the one logit comes from the cache, the index clamped
                    const int c = me.v + fu.off;
                    const float M = s_nm[me.k];
                    const float y = __fmul_rn(fu.scale, fu.rows[(bk + me.k) * fu.rld + clampi(c, 0, fu.VL - 1)]);
                    const float inc3 = __fsub_rn(__fsub_rn(y, M), s_ns[me.k]);
                    exists = exists && c >= 0 && c < fu.VL && M - M == 0.0f && inc3 - inc3 == 0.0f;
                    bonus = __dadd_rn(bonus, __dmul_rn((double)fu.nnw, (double)inc3));
                }
                bonus = __dadd_rn(bonus, (double)fu.lb);
            }
            exists = exists && me.c > NINF;
            if (!exists) me.c = NINF;
            s_sel[tid].c = me.c;  // the merge below sums the acoustic scores
            s_cbonus[tid] = bonus;
            s_cst[tid] = n1;
            s_cst2[tid] = n2;
        }
        if (exists) {
            s_key[tid] = me.v == blank ? pn : trie_node(table, mask, pn, me.v);
            s_klen[tid] = s_len[me.k] + (me.v == blank ? 0 : 1);
        }
    }
    __syncthreads();
    if (tid < nsel && (!LM || me.c > NINF)) {  // (fused: an entry that does not exist joins no group)
        const int key = s_key[tid];
        int rep = tid;
        for (int i = tid - 1; i >= 0; --i)
            if (s_key[i] == key) rep = i;
        if (rep == tid) {  // the group's best-ranked member sums the group in rank order
            float s = 0.0f;
            for (int i = tid; i < nsel; ++i)
                if (s_key[i] == key) s += expf(s_sel[i].c - me.c);
            s_merged[tid] = __fadd_rn(me.c, logf(s));
            if constexpr (LM) s_G[tid] = (float)__dadd_rn((double)s_merged[tid], s_cbonus[tid]);
            s_lead[tid] = 1;
        }
    }
    __syncthreads();
    // the new beam: every group finds its place (s_from[j]: the entry that fills slot j), slot j's thread writes it
    if (tid < K) s_from[tid] = -1;
    __syncthreads();
    const float *s_order = s_merged;  // what orders the groups: the merged score, or the fused one
    if constexpr (LM) s_order = s_G;
    if (tid < nsel && s_lead[tid]) {
        const float mine = s_order[tid];
        int pos = 0;
        for (int i = 0; i < nsel; ++i)
            if (s_lead[i] && i != tid && (s_order[i] > mine || (s_order[i] == mine && i < tid))) ++pos;
        // (plain: pos < the number of groups <= K; fused: up to C groups, the K best stay)
        if (mine > NINF && (!LM || pos < K)) s_from[pos] = tid;
    }
    __syncthreads();
    if (tid < K) {
        const int j = s_from[tid];
        const bool full = j >= 0;
        st.score[bk + tid] = full ? s_order[j] : NINF;
        st.node[bk + tid] = full ? s_key[j] : ROOT;
        st.len[bk + tid] = full ? s_klen[j] : 0;
        if constexpr (LM) {
            st.am[bk + tid] = full ? s_merged[j] : NINF;
            st.bonus[bk + tid] = full ? s_cbonus[j] : 0.0;
            st.lmst[bk + tid] = full ? s_cst[j] : 0;
            st.lmst2[bk + tid] = full ? s_cst2[j] : 0;
        }
        parent_out[bk + tid] = full ? clampi(s_sel[j].k, 0, K - 1) : 0;
        token_out[bk + tid] = full ? s_sel[j].v : blank;
    }
    if (tid == 0) {
        st.frames[b] = frames + 1;
        if (frames + 1 >= max_frames && nf_raw > max_frames) st.overflowed[b] = 1;
    }
}

// the token sequences of `n` entries per utterance, entry j of the output from slot j of the beam.  The fused search's
// results with use_final (lane = slot) score every slot first -- am + bonus + the automata's final terms, no final state:
// the slot drops out -- and entry j is the j-th slot by that score, ties by the slot.  The state is only read.
template <int NFST, bool DENSE>
__global__ __launch_bounds__(64) void msearch_read_kernel(const void *state, int B, int K, int max_frames, unsigned mask,
                                                           int n, int L, long long *__restrict__ tokens,
                                                           long long *__restrict__ lengths, float *__restrict__ scores,
                                                           float *__restrict__ am_scores, const Fused<NFST> fu,
                                                           int use_final) {
    constexpr bool LM = NFST > 0 || DENSE;  // (DENSE: the fused search's blob, even with no automaton)
    __shared__ float s_sc[LM ? MAX_BEAM : 1];
    __shared__ int s_src[LM ? MAX_BEAM : 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const Blob st = blob_of<LM ? 1 : 0>(const_cast<void *>(state), B, K);
    const unsigned long long *table = st.tables + (size_t)b * ((size_t)mask + 1);
    const size_t bk = (size_t)b * K;
    if constexpr (LM) {
        float sc = NINF;
        if (lane < K) {
            sc = st.score[bk + lane];
            if constexpr (NFST > 0) if (use_final && sc > NINF) {
                double s = __dadd_rn((double)st.am[bk + lane], st.bonus[bk + lane]);
                float inc = 0.0f;
                bool live = lm_final(fu.f[0], clampi(st.lmst[bk + lane], 0, fu.f[0].S - 1), inc);
                if (live) s = __dadd_rn(s, __dmul_rn((double)fu.lmw, (double)inc));
                if constexpr (NFST == 2) {
                    if (live) {
                        live = lm_final(fu.f[1], clampi(st.lmst2[bk + lane], 0, fu.f[1].S - 1), inc);
                        if (live) s = __dadd_rn(s, __dmul_rn((double)fu.bw, (double)inc));
                    }
                }
                sc = live ? (float)s : NINF;
            }
            if (!(sc > NINF)) sc = NINF;  // (a NaN is not alive)
        }
        s_sc[lane] = sc;
        __syncthreads();
        if (lane < K) {
            int rank = lane;
            if (use_final) {
                rank = 0;
                for (int q = 0; q < K; ++q) rank += (s_sc[q] > sc || (s_sc[q] == sc && q < lane)) ? 1 : 0;
            }
            s_src[rank] = lane;
        }
        __syncthreads();
    }
    // entry j: its slot and its score
    auto slot_of = [&](int j) __attribute__((always_inline)) {
        if constexpr (LM) return s_src[j];
        else return j;
    };
    auto score_of = [&](int slot) __attribute__((always_inline)) {
        if constexpr (LM) return s_sc[slot];
        else return st.score[bk + slot];
    };
    for (int j = 0; j < n; ++j) {  // (no entry is longer than max_frames: the rows are short, the lanes pad them)
        const int src = slot_of(j);
        const float sc = score_of(src);
        const bool live = sc > NINF;
        const int len = live ? clampi(st.len[bk + src], 0, max_frames) : -1;
        long long *out = tokens + ((size_t)b * n + j) * L;
        for (int p = lane; p < L; p += 64)
            if (p >= len) out[p] = -1;
        if (lane == 0) {
            lengths[(size_t)b * n + j] = len;
            if (scores) scores[(size_t)b * n + j] = live ? sc : NINF;
            if constexpr (LM)
                if (am_scores) am_scores[(size_t)b * n + j] = live ? st.am[bk + src] : NINF;
        }
    }
    if (lane < n) {
        const int src = slot_of(lane);
        const bool live = score_of(src) > NINF;
        const int len = live ? clampi(st.len[bk + src], 0, max_frames) : 0;
        long long *out = tokens + ((size_t)b * n + lane) * L;
        int node = st.node[bk + src];
        for (int p = len - 1; p >= 0; --p) {  // bounded by len whatever the table holds
            long long tok = -1;
            if (node != ROOT) {
                const unsigned long long key = trie_load(table, mask, node);
                tok = (long long)(int)(unsigned)(key & 0xffffffffull);
                node = (int)(unsigned)(key >> 32);
            }
            if (p < L) out[p] = tok;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// streaming (pika_msearch_stream.h): the side record and the commit
// ---------------------------------------------------------------------------------------------
struct Side {
    int *retired;
    double *offset, *boff;
};

__host__ __device__ inline Side side_of(void *side, int B) {
    char *p = static_cast<char *>(side);
    Side s;
    s.retired = reinterpret_cast<int *>(p + PIKA_MSEARCH_STREAM_RETIRED_OFFSET(B));
    s.offset = reinterpret_cast<double *>(p + PIKA_MSEARCH_STREAM_OFFSET_OFFSET(B));
    s.boff = reinterpret_cast<double *>(p + PIKA_MSEARCH_STREAM_BONUS_OFFSET_OFFSET(B));
    return s;
}

__global__ __launch_bounds__(THREADS) void msearch_side_reset_kernel(Side sd, int B, const int *__restrict__ which) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B || (which && which[b] == 0)) return;
    sd.retired[b] = 0; sd.offset[b] = 0.0; sd.boff[b] = 0.0;
}

// Commit, one kernel for the two blobs; grid = B, block = 256, as ctc_stream_commit_kernel (ctc_search_core.h), whose walk
// this is: wave 0's lane r owns slot r and holds what the slot carries in its registers.  The lanes find the live slots'
// common ancestor -- every slot up to the depth of the shallowest, then all in step until they meet --, lane 0 writes the
// labels above it, every lane leaves the labels between the new root and its slot in paths[b][r][0, tail), root side
// first; the table is cleared by the workgroup; the lanes replay their labels through trie_node from ROOT (a node's
// identity is the table slot of its key, so the parents come first; lanes that share a prefix find each other's keys)
// and write their slot where it now stands.  Then the keys are counted and `frames` is lowered.  frames, every len and
// every node bound loops and index the table through its mask: a blob that was never reset ends inside its own memory.
// NSEL: the keys a step can add (K, or the fused search's C).
template <bool LM>
__global__ __launch_bounds__(THREADS) void msearch_commit_kernel(void *state, Side sd, int B, int K, int NSEL,
                                                                  int max_frames, unsigned mask,
                                                                  const int *__restrict__ which, int max_tail, int rebase,
                                                                  int L, long long *__restrict__ tokens,
                                                                  long long *__restrict__ lengths,
                                                                  long long *__restrict__ slot_map,
                                                                  int *__restrict__ paths) {
    __shared__ int s_depth, s_live, s_tail, s_n;
    const int b = blockIdx.x, tid = threadIdx.x, r = tid;
    const size_t bk = (size_t)b * K;
    long long *out = tokens + (size_t)b * L;
    if (which && which[b] == 0) {  // workgroup-uniform
        for (int p = tid; p < L; p += THREADS) out[p] = -1;
        if (tid < K) slot_map[bk + tid] = tid;
        if (tid == 0) lengths[b] = 0;
        return;
    }
    const Blob st = blob_of<LM ? 1 : 0>(state, B, K);
    unsigned long long *table = st.tables + (size_t)b * ((size_t)mask + 1);
    const int frames = clampi(st.frames[b], 0, max_frames);
    // one step towards the root; whatever a node holds, the load stays inside the table
    auto up = [&](int node) __attribute__((always_inline)) {
        return node == ROOT ? ROOT : (int)(unsigned)(trie_load(table, mask, node) >> 32);
    };
    int tail = -1, j = 0, n = 0;  // wave 0, lane r: the labels slot r keeps (-1: it does not stay), its slot afterwards
    float score = NINF, am = NINF;
    double bonus = 0.0;
    int st1 = 0, st2 = 0;
    if (tid < 64) {
        if (r < K) {
            score = st.score[bk + r];
            if constexpr (LM) {
                am = st.am[bk + r]; bonus = st.bonus[bk + r]; st1 = st.lmst[bk + r]; st2 = st.lmst2[bk + r];
            }
        }
        // the live slots: the front slots with a score (lanes at and beyond K have none)
        const unsigned long long dead = __ballot(!(r < K && score > NINF));
        n = dead ? __ffsll(dead) - 1 : 64;
        const bool act = r < n;
        const int node = act ? st.node[bk + r] : ROOT;
        const int len = act ? clampi(st.len[bk + r], 0, frames) : 0;
        int lmin = act ? len : 0x7fffffff;
        for (int o = 32; o > 0; o >>= 1) lmin = min(lmin, __shfl_xor(lmin, o));
        if (n == 0) lmin = 0;
        int cur = node;
        for (int k = len - lmin; k > 0; --k) cur = up(cur);  // (no slot: len = 0, no step)
        int steps = 0, first;
        bool same;
        for (;; ++steps) {  // wave-uniform
            first = __shfl(cur, 0);
            same = __all(!act || cur == first);
            if (same || steps >= lmin) break;
            cur = up(cur);
        }
        int depth = same ? lmin - steps : 0;  // labels from the root to the new root
        int root = same ? first : ROOT;       // (no meeting point within lmin steps: not a trie; nothing is shared)
        const int len0 = __shfl(len, 0);
        if (max_tail >= 0 && n > 0 && len0 - depth > max_tail) {  // wave-uniform: forced
            int c = node;
            if (r == 0)
                for (int k = 0; k < max_tail; ++k) c = up(c);  // max_tail < len0 <= frames
            root = __shfl(c, 0);
            depth = len0 - max_tail;
        }
        if (r == 0) {  // the committed labels, back from the new root; L may be narrower than the prefix
            int c = root;
            for (int p = depth - 1; p >= 0; --p) {
                long long tok = -1;
                if (c != ROOT) {
                    const unsigned long long key = trie_load(table, mask, c);
                    tok = (long long)(int)(unsigned)(key & 0xffffffffull);
                    c = (int)(unsigned)(key >> 32);
                }
                if (p < L) out[p] = tok;
            }
            lengths[b] = depth;
            s_depth = depth;
            s_live = 0;
        }
        // the labels between the new root and the slot; a slot stays if that walk ends at the new root
        if (act && len >= depth) {
            const int tl = len - depth;  // <= frames <= max_frames
            int *path = paths + (bk + r) * max_frames;
            int c = node;
            for (int k = 0; k < tl; ++k) {
                const unsigned long long key = trie_load(table, mask, c);
                path[tl - 1 - k] = (int)(unsigned)(key & 0xffffffffull);
                c = c == ROOT ? ROOT : (int)(unsigned)(key >> 32);
            }
            if (c == root) tail = tl;
        }
        const unsigned long long kept = __ballot(tail >= 0);
        j = __popcll(kept & ((1ull << r) - 1ull));
        int tmax = tail;
        for (int o = 32; o > 0; o >>= 1) tmax = max(tmax, __shfl_xor(tmax, o));
        if (r == 0) { s_n = __popcll(kept); s_tail = max(tmax, 0); }
    }
    __syncthreads();  // every walk through the old table is over; the slots are in wave 0's registers
    for (int p = s_depth + tid; p < L; p += THREADS) out[p] = -1;
    for (size_t i = tid; i <= (size_t)mask; i += THREADS) table[i] = EMPTY;
    __syncthreads();  // the table is empty
    if (tid < 64) {
        const int kept_n = s_n;
        int node = ROOT;
        if (tail >= 0) {
            const int *path = paths + (bk + r) * max_frames;
            for (int k = 0; k < tail; ++k) node = trie_node(table, mask, node, path[k]);
        }
        if (rebase && kept_n > 0) {  // wave-uniform: the new slot 0 is the first slot that stays
            const int r0 = __ffsll(__ballot(tail >= 0)) - 1;
            if constexpr (LM) {
                const float c = __shfl(am, r0);
                const double e = __shfl(bonus, r0);
                if (tail >= 0) {
                    am = __fsub_rn(am, c);
                    bonus = __dsub_rn(bonus, e);
                    score = (float)__dadd_rn((double)am, bonus);
                }
                if (r == 0) { sd.offset[b] += (double)c; sd.boff[b] += e; }
            } else {
                const float c = __shfl(score, r0);
                if (tail >= 0) score = __fsub_rn(score, c);
                if (r == 0) sd.offset[b] += (double)c;
            }
        }
        if (tail >= 0) {  // (j <= r, and every lane read its slot before the barrier)
            st.score[bk + j] = score; st.node[bk + j] = node; st.len[bk + j] = tail;
            if constexpr (LM) {
                st.am[bk + j] = am; st.bonus[bk + j] = bonus; st.lmst[bk + j] = st1; st.lmst2[bk + j] = st2;
            }
            slot_map[bk + j] = r;
        }
        if (r >= kept_n && r < K) {
            if (r < n) {  // vacated
                st.score[bk + r] = NINF; st.node[bk + r] = ROOT; st.len[bk + r] = 0;
                if constexpr (LM) {
                    st.am[bk + r] = NINF; st.bonus[bk + r] = 0.0; st.lmst[bk + r] = 0; st.lmst2[bk + r] = 0;
                }
            }
            slot_map[bk + r] = r;
        }
    }
    __syncthreads();  // the table holds the live keys
    int live = 0;
    for (size_t i = tid; i <= (size_t)mask; i += THREADS) live += trie_load(table, mask, (int)i) != EMPTY;
    if (live) atomicAdd(&s_live, live);
    __syncthreads();
    if (tid == 0) {
        // the fewest frames that account for the live keys (NSEL per frame) and for the longest tail; never more than before
        const int fnew = min(max((s_live + NSEL - 1) / NSEL, s_tail), frames);
        st.frames[b] = fnew;
        sd.retired[b] += frames - fnew;
    }
}

// ---------------------------------------------------------------------------------------------
// time stamps (pika_msearch_times.h): the record beside a blob.  The kernels read the blob -- score, len, node, frames,
// the table -- and never write it.
// ---------------------------------------------------------------------------------------------
struct Times {
    int *seen, *lost, *cur;
    int *planes;   // two planes of [B][K][max_frames]
    size_t plane;  // elements of one
};

__host__ __device__ inline Times times_of(void *times, int B, int K, int max_frames) {
    char *p = static_cast<char *>(times);
    Times t;
    t.seen = reinterpret_cast<int *>(p + PIKA_MSEARCH_TIMES_SEEN_OFFSET(B));
    t.lost = reinterpret_cast<int *>(p + PIKA_MSEARCH_TIMES_LOST_OFFSET(B));
    t.cur = reinterpret_cast<int *>(p + PIKA_MSEARCH_TIMES_CUR_OFFSET(B));
    t.planes = reinterpret_cast<int *>(p + PIKA_MSEARCH_TIMES_PLANES_OFFSET(B));
    t.plane = (size_t)B * K * max_frames;
    return t;
}

// row (b, k) of plane p
__device__ __forceinline__ int *times_row(const Times &t, int p, int b, int K, int k, int max_frames) {
    return t.planes + (size_t)p * t.plane + ((size_t)b * K + k) * max_frames;
}

__device__ __forceinline__ int clampll(long long v, int lo, int hi) {
    return v < lo ? lo : (v > hi ? hi : (int)v);
}

// n entries from src to dst by one wave; `vec` (wave-uniform): both rows are 16-byte aligned
__device__ __forceinline__ void times_copy(int *__restrict__ dst, const int *__restrict__ src, int n, int lane, bool vec) {
    int done = 0;
    if (vec) {
        const int n4 = n >> 2;
        for (int i = lane; i < n4; i += 64) reinterpret_cast<int4 *>(dst)[i] = reinterpret_cast<const int4 *>(src)[i];
        done = 4 * n4;
    }
    for (int p = done + lane; p < n; p += 64) dst[p] = src[p];
}

// grid = (B, y), block = 256: the workgroups (b, *) fill both planes of utterance b with -1, (b, 0) writes its head
__global__ __launch_bounds__(THREADS) void msearch_times_reset_kernel(Times tm, int K, int max_frames,
                                                                       const int *__restrict__ which) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;  // workgroup-uniform
    const size_t n = (size_t)K * max_frames;
    for (int p = 0; p < 2; ++p) {
        int *row = times_row(tm, p, b, K, 0, max_frames);
        for (size_t i = (size_t)blockIdx.y * THREADS + threadIdx.x; i < n; i += (size_t)gridDim.y * THREADS) row[i] = -1;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) { tm.seen[b] = 0; tm.lost[b] = 0; tm.cur[b] = 0; }
}

// The step; grid = B, block = 256: wave w moves the rows of the new slots w, w + 4, ...
template <bool LM>
__global__ __launch_bounds__(THREADS) void msearch_times_step_kernel(Times tm, const void *state,
                                                                      const int *__restrict__ retired, int B, int K,
                                                                      int max_frames, const long long *__restrict__ parent,
                                                                      const long long *__restrict__ token, int blank,
                                                                      int vec) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Blob st = blob_of<LM ? 1 : 0>(const_cast<void *>(state), B, K);
    const unsigned now = (unsigned)st.frames[b] + (retired ? (unsigned)retired[b] : 0u);  // consumed[b]
    const unsigned seen = (unsigned)tm.seen[b];
    const int lost = tm.lost[b], cur = tm.cur[b] & 1;
    __syncthreads();  // every thread has read the head that thread 0 writes below
    if (lost != 0 || now == seen) return;  // workgroup-uniform, as what follows
    if (now != seen + 1u) {
        if (tid == 0) tm.lost[b] = 1;
        return;
    }
    const int stamp = (int)(now - 1u);
    for (int j = wave; j < K; j += WAVES) {
        const size_t bk = (size_t)b * K + j;
        const int p = clampll(parent[bk], 0, K - 1);
        const bool label = token[bk] != (long long)blank;
        const int len = clampi(st.len[bk], 0, max_frames);
        const int n = label ? max(len - 1, 0) : len;
        int *dst = times_row(tm, cur ^ 1, b, K, j, max_frames);
        times_copy(dst, times_row(tm, cur, b, K, p, max_frames), n, lane, vec != 0);
        if (label && len > 0 && lane == 0) dst[len - 1] = stamp;
    }
    if (tid == 0) { tm.cur[b] = cur ^ 1; tm.seen[b] = (int)now; }
}

// The slots' times; grid = B, block = 256: a wave per slot
template <bool LM>
__global__ __launch_bounds__(THREADS) void msearch_times_hyps_kernel(Times tm, const void *state, int B, int K,
                                                                      int max_frames, int L, long long *__restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Blob st = blob_of<LM ? 1 : 0>(const_cast<void *>(state), B, K);
    const bool lost = tm.lost[b] != 0;
    const int cur = tm.cur[b] & 1;
    for (int j = wave; j < K; j += WAVES) {
        const size_t bk = (size_t)b * K + j;
        const bool live = !lost && st.score[bk] > NINF;
        const int len = live ? clampi(st.len[bk], 0, max_frames) : 0;
        const int *row = times_row(tm, cur, b, K, j, max_frames);
        long long *o = out + bk * L;
        for (int p = lane; p < L; p += 64) o[p] = p < len ? (long long)row[p] : -1ll;
    }
}

// The times of an entry of a results call; grid = (B, N), block = 64: lane k walks slot k's path up the trie against the
// entry's tokens, the first slot that spells them gives its row
template <bool LM>
__global__ __launch_bounds__(64) void msearch_times_results_kernel(Times tm, const void *state, int B, int K,
                                                                    int max_frames, unsigned mask, int N, int L,
                                                                    const long long *__restrict__ tokens,
                                                                    const long long *__restrict__ lengths,
                                                                    long long *__restrict__ out) {
    const int b = blockIdx.x, e = blockIdx.y, lane = threadIdx.x;
    const Blob st = blob_of<LM ? 1 : 0>(const_cast<void *>(state), B, K);
    const unsigned long long *table = st.tables + (size_t)b * ((size_t)mask + 1);
    const size_t bk = (size_t)b * K, be = (size_t)b * N + e;
    const long long *tok = tokens + be * L;
    const long long le = lengths[be];
    const bool ok = tm.lost[b] == 0 && le >= 0 && le <= (long long)L && le <= (long long)max_frames;  // wave-uniform
    const int n = ok ? (int)le : 0;
    bool match = false;
    if (ok && lane < K && st.score[bk + lane] > NINF && clampi(st.len[bk + lane], 0, max_frames) == n) {
        int node = st.node[bk + lane];
        match = true;
        for (int p = n - 1; p >= 0 && match; --p) {  // bounded by n <= max_frames whatever the table holds
            if (node == ROOT) { match = false; break; }
            const unsigned long long key = trie_load(table, mask, node);
            match = (long long)(int)(unsigned)(key & 0xffffffffull) == tok[p];
            node = (int)(unsigned)(key >> 32);
        }
        match = match && node == ROOT;
    }
    const unsigned long long found = __ballot(match);
    const int slot = found ? __ffsll(found) - 1 : -1;  // < K
    const int len = slot >= 0 ? n : 0;
    const int *row = times_row(tm, tm.cur[b] & 1, b, K, slot >= 0 ? slot : 0, max_frames);
    long long *o = out + be * L;
    for (int p = lane; p < L; p += 64) o[p] = p < len ? (long long)row[p] : -1ll;
}

// The commit; grid = B, block = 256.  The threads take the committed positions -- the minimum over the live slots' old
// rows, which the threads of a wave read side by side --, the waves move the tails.
template <bool LM>
__global__ __launch_bounds__(THREADS) void msearch_times_commit_kernel(Times tm, const void *state, int B, int K,
                                                                        int max_frames, const int *__restrict__ which,
                                                                        const long long *__restrict__ lengths,
                                                                        const long long *__restrict__ slot_map, int L,
                                                                        long long *__restrict__ out, int vec) {
    __shared__ int s_src[MAX_BEAM], s_len[MAX_BEAM], s_n;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t bk = (size_t)b * K;
    long long *o = out + (size_t)b * L;
    const int lost = tm.lost[b], cur = tm.cur[b] & 1;
    __syncthreads();  // every thread has read the head that thread 0 writes below
    if ((which && which[b] == 0) || lost != 0) {  // workgroup-uniform
        for (int p = tid; p < L; p += THREADS) o[p] = -1;
        return;
    }
    const Blob st = blob_of<LM ? 1 : 0>(const_cast<void *>(state), B, K);
    const int d = clampll(lengths[b], 0, max_frames);
    if (tid < 64) {
        // the live slots: the front slots with a score (lanes at and beyond K have none)
        const unsigned long long dead = __ballot(!(tid < K && st.score[bk + (tid < K ? tid : 0)] > NINF));
        if (tid < K) {
            s_src[tid] = clampll(slot_map[bk + tid], 0, K - 1);
            s_len[tid] = min(clampi(st.len[bk + tid], 0, max_frames), max_frames - d);
        }
        if (tid == 0) s_n = dead ? __ffsll(dead) - 1 : 64;
    }
    __syncthreads();
    const int n = s_n;  // <= K
    const int *old = times_row(tm, cur, b, K, 0, max_frames);
    for (int i = tid; i < min(d, L); i += THREADS) {
        int t = n > 0 ? 0x7fffffff : -1;
        for (int j = 0; j < n; ++j) t = min(t, old[(size_t)s_src[j] * max_frames + i]);
        o[i] = t;
    }
    for (int p = d + tid; p < L; p += THREADS) o[p] = -1;
    for (int j = wave; j < K; j += WAVES)
        times_copy(times_row(tm, cur ^ 1, b, K, j, max_frames), old + (size_t)s_src[j] * max_frames + d, s_len[j], lane,
                   vec != 0 && (d & 3) == 0);
    if (tid == 0) tm.cur[b] = cur ^ 1;
}

// ---------------------------------------------------------------------------------------------
// host.  C: what sizes the trie's tables -- the entries a step can select: K, or the fused search's candidates
// ---------------------------------------------------------------------------------------------
static inline int check_dims(int B, int K, int C, int max_frames) {
    if (B <= 0 || K <= 0 || C <= 0 || max_frames <= 0 || K > C) return PIKA_EINVAL;
    if (C > MAX_BEAM || B > 65535 || 2ll * max_frames * C > (1ll << 28)) return PIKA_ETOOBIG;
    return PIKA_OK;
}

static inline int check_dims(int B, int K, int max_frames) { return check_dims(B, K, K, max_frames); }

static inline int check_read(int B, int K, int C, int max_frames, int n, int L) {
    if (n <= 0 || L <= 0) return PIKA_EINVAL;
    if (int rc = check_dims(B, K, C, max_frames)) return rc;
    if (n > K || (long long)n * L > 0x7fffffffll) return PIKA_ETOOBIG;
    return PIKA_OK;
}

template <int NFST, bool DENSE = false>
static int read_out(const void *state, int B, int K, int C, int max_frames, int n, int L, long long *tokens,
                    long long *lengths, float *scores, float *am_scores, const Fused<NFST> &fu, int use_final,
                    void *stream) {
    hipLaunchKernelGGL((msearch_read_kernel<NFST, DENSE>), dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream),
                       state, B, K, max_frames, (unsigned)(table_slots(max_frames, C) - 1), n, L, tokens, lengths, scores,
                       am_scores, fu, use_final);
    return (int)hipGetLastError();
}

static int read_plain(const void *state, int B, int K, int max_frames, int n, int L, long long *tokens,
                      long long *lengths, float *scores, bool want_scores, void *stream) {
    if (int rc = check_read(B, K, K, max_frames, n, L)) return rc;
    if (!state || !tokens || !lengths || (want_scores && !scores)) return PIKA_EINVAL;
    return read_out<0>(state, B, K, K, max_frames, n, L, tokens, lengths, scores, nullptr, Fused<0>{}, 0, stream);
}

template <bool LM>
static int reset(void *state, int B, int K, int C, int max_frames, const int *which, int start, int start2, void *stream) {
    const size_t slots = table_slots(max_frames, C), y = slots / 4096;  // 16 keys per thread
    hipLaunchKernelGGL((msearch_reset_kernel<LM>), dim3((unsigned)B, (unsigned)(y < 1 ? 1 : (y > 256 ? 256 : y))),
                       dim3(THREADS), 0, static_cast<hipStream_t>(stream), state, B, K, slots, which, start, start2);
    return (int)hipGetLastError();
}

static inline int row_vec(const float *rows, long long ld) {
    return ld % 4 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0;
}

template <int NFST, bool DENSE = false>
static int advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K, int C,
                   int max_frames, int V, int blank, float sm_scale, float blank_penalty, long long *parent_out,
                   long long *token_out, const Step<NFST, DENSE> &fu, void *stream) {
    const int vec = row_vec(logits, ld);
    hipLaunchKernelGGL((msearch_advance_kernel<NFST, DENSE>), dim3((unsigned)B), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), state, logits, ld, num_frames, B, K, max_frames, V, blank,
                       sm_scale, blank_penalty, (unsigned)(table_slots(max_frames, C) - 1), vec, parent_out, token_out, fu);
    return (int)hipGetLastError();
}

static inline int check_streams(int B) { return B <= 0 ? PIKA_EINVAL : (B > 65535 ? PIKA_ETOOBIG : PIKA_OK); }

template <bool LM>
static int commit(void *state, void *side, int B, int K, int C, int max_frames, const int *which, int max_tail, int rebase,
                  int L, long long *tokens, long long *lengths, long long *slot_map, void *scratch, void *stream) {
    if (L <= 0) return PIKA_EINVAL;
    if (int rc = check_dims(B, K, C, max_frames)) return rc;
    if (!state || !side || !tokens || !lengths || !slot_map || !scratch) return PIKA_EINVAL;
    hipLaunchKernelGGL((msearch_commit_kernel<LM>), dim3((unsigned)B), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       state, side_of(side, B), B, K, C, max_frames, (unsigned)(table_slots(max_frames, C) - 1), which,
                       max_tail, rebase, L, tokens, lengths, slot_map, static_cast<int *>(scratch));
    return (int)hipGetLastError();
}

// ---- the automata of a fused call, checked as pika_ctc_lm.h states it
static inline bool bad_start(int S, int start) { return S <= 0 || start < 0 || start >= S; }

static inline int check_fst(const Fst &f, int start) {
    if (f.A < 0 || bad_start(f.S, start)) return PIKA_EINVAL;
    if (!f.off || !f.fin || (f.A > 0 && (!f.il || !f.w || !f.ns))) return PIKA_EINVAL;
    return PIKA_OK;
}

// the optional second automaton: 0 none (no states, no arcs, no arrays), 1 present and sound, < 0 refused
static inline int second_fst(const Fst &g, int start2) {
    if (g.S == 0) return (g.A == 0 && !g.off && !g.il && !g.w && !g.ns && !g.fin) ? 0 : PIKA_EINVAL;
    return check_fst(g, start2) ? PIKA_EINVAL : 1;
}

template <int NFST>
static inline Step<NFST, false> fused(const Fst &f, const Fst &g, float lmw, float bw, float lb, int C) {
    Step<NFST, false> fu;
    fu.f[0] = f;
    if constexpr (NFST == 2) fu.f[1] = g;
    fu.lmw = lmw; fu.bw = bw; fu.lb = lb; fu.C = C;
    return fu;
}

// the rows of a neural LM beside the automata that exist
struct NnRows {
    const float *rows;
    long long ld;
    int V, off;
    float scale, w;
};

template <int NFST>
static inline Step<NFST, true> dense(const Fst &f, const Fst &g, float lmw, float bw, float lb, int C, const NnRows &nn) {
    Step<NFST, true> fu;
    if constexpr (NFST >= 1) { fu.f[0] = f; fu.lmw = lmw; fu.bw = bw; }
    if constexpr (NFST == 2) fu.f[1] = g;
    fu.rows = nn.rows; fu.rld = nn.ld; fu.VL = nn.V; fu.off = nn.off; fu.rvec = row_vec(nn.rows, nn.ld);
    fu.scale = nn.scale; fu.nnw = nn.w; fu.lb = lb; fu.C = C;
    return fu;
}

// the automata of a call with a neural LM, either of which may be "none": the number present (0, 1, 2), < 0 refused
static inline int nn_fsts(const Fst &f, int start, const Fst &g, int start2) {
    const int one = second_fst(f, start), two = second_fst(g, start2);
    if (one < 0 || two < 0 || (two && !one)) return PIKA_EINVAL;
    return one + two;
}

// ---- the time record: C = 0 names the plain blob, K <= C the fused search's
static inline int check_times(int B, int K, int C, int max_frames) {
    if (C < 0) return PIKA_EINVAL;
    return check_dims(B, K, C == 0 ? K : C, max_frames);
}

static inline unsigned times_mask(int K, int C, int max_frames) {
    return (unsigned)(table_slots(max_frames, C == 0 ? K : C) - 1);
}

static inline int times_vec(const void *times, int max_frames) {
    return max_frames % 4 == 0 && reinterpret_cast<uintptr_t>(times) % 16 == 0;
}

}  // namespace

extern "C" {

size_t pika_msearch_state_bytes(int B, int K, int max_frames) {
    if (check_dims(B, K, max_frames)) return 0;
    return head_bytes(B, K) + table_bytes(B, max_frames, K);
}

int pika_msearch_reset(void *state, int B, int K, int max_frames, const int *which, void *stream) {
    if (int rc = check_dims(B, K, max_frames)) return rc;
    if (!state) return PIKA_EINVAL;
    return reset<false>(state, B, K, K, max_frames, which, 0, 0, stream);
}

int pika_msearch_advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K,
                         int max_frames, int V, int blank, float sm_scale, float blank_penalty, long long *parent_out,
                         long long *token_out, void *stream) {
    if (V < 2 || blank < 0 || blank >= V || ld < V || !std::isfinite(sm_scale) || !std::isfinite(blank_penalty)) return PIKA_EINVAL;
    if (int rc = check_dims(B, K, max_frames)) return rc;
    if (!state || !logits || !num_frames || !parent_out || !token_out) return PIKA_EINVAL;
    return advance<0>(state, logits, ld, num_frames, B, K, K, max_frames, V, blank, sm_scale, blank_penalty, parent_out,
                      token_out, Step<0, false>{}, stream);
}

int pika_msearch_results(const void *state, int B, int K, int max_frames, int nbest, int L, long long *tokens,
                         long long *lengths, float *scores, void *stream) {
    return read_plain(state, B, K, max_frames, nbest, L, tokens, lengths, scores, true, stream);
}

int pika_msearch_hyps(const void *state, int B, int K, int max_frames, int L, long long *tokens, long long *lengths,
                      void *stream) {
    return read_plain(state, B, K, max_frames, K, L, tokens, lengths, nullptr, false, stream);
}

// ---- the search with one or two automata fused in (pika_msearch_lm.h) ------------------------------------------------

size_t pika_msearch_lm_state_bytes(int B, int K, int C, int max_frames) {
    if (check_dims(B, K, C, max_frames)) return 0;
    return lm_head_bytes(B, K) + table_bytes(B, max_frames, C);
}

int pika_msearch_lm_reset(void *state, int B, int K, int C, int max_frames, int num_states, int start, int num_states2,
                          int start2, const int *which, void *stream) {
    if (bad_start(num_states, start) || num_states2 < 0 || (num_states2 > 0 && bad_start(num_states2, start2)))
        return PIKA_EINVAL;
    if (int rc = check_dims(B, K, C, max_frames)) return rc;
    if (!state) return PIKA_EINVAL;
    return reset<true>(state, B, K, C, max_frames, which, start, num_states2 > 0 ? start2 : 0, stream);
}

int pika_msearch_lm_advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K,
                            int C, int max_frames, int V, int blank, float sm_scale, float blank_penalty,
                            const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                            const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                            int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int backoff_id2, int label_offset2, float lm_weight,
                            float bias_weight, float length_bonus, long long *parent_out, long long *token_out,
                            void *stream) {
    const Fst f = {fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                   label_offset};
    const Fst g = {fst2_offsets, fst2_ilabel, fst2_weight, fst2_nextstate, fst2_final, num_states2, num_arcs2,
                   backoff_id2, label_offset2};
    if (V < 2 || blank < 0 || blank >= V || ld < V || !std::isfinite(sm_scale) || !std::isfinite(blank_penalty) ||
        !std::isfinite(lm_weight) || !std::isfinite(bias_weight) || !std::isfinite(length_bonus))
        return PIKA_EINVAL;
    const int two = second_fst(g, 0);
    if (two < 0 || check_fst(f, 0)) return PIKA_EINVAL;
    if (int rc = check_dims(B, K, C, max_frames)) return rc;
    if (!state || !logits || !num_frames || !parent_out || !token_out) return PIKA_EINVAL;
    if (two)
        return advance<2>(state, logits, ld, num_frames, B, K, C, max_frames, V, blank, sm_scale, blank_penalty,
                          parent_out, token_out, fused<2>(f, g, lm_weight, bias_weight, length_bonus, C), stream);
    return advance<1>(state, logits, ld, num_frames, B, K, C, max_frames, V, blank, sm_scale, blank_penalty, parent_out,
                      token_out, fused<1>(f, g, lm_weight, bias_weight, length_bonus, C), stream);
}

int pika_msearch_lm_results(const void *state, int B, int K, int C, int max_frames, const long long *fst_offsets,
                            const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                            const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                            int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int start2, int backoff_id2, int label_offset2,
                            float lm_weight, float bias_weight, int use_final, int nbest, int L, long long *tokens,
                            long long *lengths, float *scores, float *am_scores, void *stream) {
    const Fst f = {fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                   label_offset};
    const Fst g = {fst2_offsets, fst2_ilabel, fst2_weight, fst2_nextstate, fst2_final, num_states2, num_arcs2,
                   backoff_id2, label_offset2};
    if (!std::isfinite(lm_weight) || !std::isfinite(bias_weight)) return PIKA_EINVAL;
    const int two = second_fst(g, start2);
    if (two < 0 || check_fst(f, start)) return PIKA_EINVAL;
    if (int rc = check_read(B, K, C, max_frames, nbest, L)) return rc;
    if (!state || !tokens || !lengths || !scores || !am_scores) return PIKA_EINVAL;
    if (two)
        return read_out<2>(state, B, K, C, max_frames, nbest, L, tokens, lengths, scores, am_scores,
                           fused<2>(f, g, lm_weight, bias_weight, 0.0f, C), use_final != 0, stream);
    return read_out<1>(state, B, K, C, max_frames, nbest, L, tokens, lengths, scores, am_scores,
                       fused<1>(f, g, lm_weight, bias_weight, 0.0f, C), use_final != 0, stream);
}

int pika_msearch_lm_hyps(const void *state, int B, int K, int C, int max_frames, int L, long long *tokens,
                         long long *lengths, void *stream) {
    if (int rc = check_read(B, K, C, max_frames, K, L)) return rc;
    if (!state || !tokens || !lengths) return PIKA_EINVAL;
    // (the slots in the beam's order: no automaton is walked, the kernel takes an empty one)
    return read_out<1>(state, B, K, C, max_frames, K, L, tokens, lengths, nullptr, nullptr,
                       fused<1>(Fst{}, Fst{}, 0.0f, 0.0f, 0.0f, C), 0, stream);
}

// ---- the search with a neural LM's rows beside up to two automata (pika_msearch_nn.h) ---------------------------------

int pika_msearch_nn_reset(void *state, int B, int K, int C, int max_frames, int num_states, int start, int num_states2,
                          int start2, const int *which, void *stream) {
    if (num_states < 0 || num_states2 < 0 || (num_states2 > 0 && num_states == 0)) return PIKA_EINVAL;
    if ((num_states > 0 && bad_start(num_states, start)) || (num_states2 > 0 && bad_start(num_states2, start2)))
        return PIKA_EINVAL;
    if (int rc = check_dims(B, K, C, max_frames)) return rc;
    if (!state) return PIKA_EINVAL;
    return reset<true>(state, B, K, C, max_frames, which, num_states > 0 ? start : 0, num_states2 > 0 ? start2 : 0, stream);
}

int pika_msearch_nn_advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K,
                            int C, int max_frames, int V, int blank, float sm_scale, float blank_penalty,
                            const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                            const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                            int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int backoff_id2, int label_offset2, float lm_weight,
                            float bias_weight, float length_bonus, const float *lm_logits, long long lm_ld, int V_lm,
                            int nn_label_offset, float nn_scale, float nn_weight, long long *parent_out,
                            long long *token_out, void *stream) {
    const Fst f = {fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                   label_offset};
    const Fst g = {fst2_offsets, fst2_ilabel, fst2_weight, fst2_nextstate, fst2_final, num_states2, num_arcs2,
                   backoff_id2, label_offset2};
    if (V < 2 || blank < 0 || blank >= V || ld < V || !std::isfinite(sm_scale) || !std::isfinite(blank_penalty) ||
        !std::isfinite(lm_weight) || !std::isfinite(bias_weight) || !std::isfinite(length_bonus))
        return PIKA_EINVAL;
    if (V_lm < 1 || lm_ld < V_lm || !std::isfinite(nn_scale) || !std::isfinite(nn_weight)) return PIKA_EINVAL;
    const int n = nn_fsts(f, 0, g, 0);
    if (n < 0) return PIKA_EINVAL;
    if (int rc = check_dims(B, K, C, max_frames)) return rc;
    if (!state || !logits || !lm_logits || !num_frames || !parent_out || !token_out) return PIKA_EINVAL;
    const NnRows nn = {lm_logits, lm_ld, V_lm, nn_label_offset, nn_scale, nn_weight};
    if (n == 2)
        return advance<2, true>(state, logits, ld, num_frames, B, K, C, max_frames, V, blank, sm_scale, blank_penalty,
                                parent_out, token_out, dense<2>(f, g, lm_weight, bias_weight, length_bonus, C, nn), stream);
    if (n == 1)
        return advance<1, true>(state, logits, ld, num_frames, B, K, C, max_frames, V, blank, sm_scale, blank_penalty,
                                parent_out, token_out, dense<1>(f, g, lm_weight, bias_weight, length_bonus, C, nn), stream);
    return advance<0, true>(state, logits, ld, num_frames, B, K, C, max_frames, V, blank, sm_scale, blank_penalty,
                            parent_out, token_out, dense<0>(f, g, lm_weight, bias_weight, length_bonus, C, nn), stream);
}

int pika_msearch_nn_results(const void *state, int B, int K, int C, int max_frames, const long long *fst_offsets,
                            const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                            const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                            int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int start2, int backoff_id2, int label_offset2,
                            float lm_weight, float bias_weight, int use_final, int nbest, int L, long long *tokens,
                            long long *lengths, float *scores, float *am_scores, void *stream) {
    const Fst f = {fst_offsets, fst_ilabel, fst_weight, fst_nextstate, fst_final, num_states, num_arcs, backoff_id,
                   label_offset};
    const Fst g = {fst2_offsets, fst2_ilabel, fst2_weight, fst2_nextstate, fst2_final, num_states2, num_arcs2,
                   backoff_id2, label_offset2};
    if (!std::isfinite(lm_weight) || !std::isfinite(bias_weight)) return PIKA_EINVAL;
    const int n = nn_fsts(f, start, g, start2);
    if (n < 0) return PIKA_EINVAL;
    if (int rc = check_read(B, K, C, max_frames, nbest, L)) return rc;
    if (!state || !tokens || !lengths || !scores || !am_scores) return PIKA_EINVAL;
    if (n == 2)
        return read_out<2>(state, B, K, C, max_frames, nbest, L, tokens, lengths, scores, am_scores,
                           fused<2>(f, g, lm_weight, bias_weight, 0.0f, C), use_final != 0, stream);
    if (n == 1)
        return read_out<1>(state, B, K, C, max_frames, nbest, L, tokens, lengths, scores, am_scores,
                           fused<1>(f, g, lm_weight, bias_weight, 0.0f, C), use_final != 0, stream);
    // (no automaton: no final term, the beam as it stands)
    return read_out<0, true>(state, B, K, C, max_frames, nbest, L, tokens, lengths, scores, am_scores, Fused<0>{}, 0, stream);
}

// ---- streaming: the side record and the commit of either blob (pika_msearch_stream.h) --------------------------------

size_t pika_msearch_stream_side_bytes(int B) {
    if (check_streams(B)) return 0;
    return PIKA_MSEARCH_STREAM_BONUS_OFFSET_OFFSET(B) + PIKA_MSEARCH_STREAM_ROUND16(8 * (size_t)B);
}

int pika_msearch_stream_reset(void *side, int B, const int *which, void *stream) {
    if (int rc = check_streams(B)) return rc;
    if (!side) return PIKA_EINVAL;
    hipLaunchKernelGGL(msearch_side_reset_kernel, dim3((unsigned)((B + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), side_of(side, B), B, which);
    return (int)hipGetLastError();
}

size_t pika_msearch_commit_scratch_bytes(int B, int K, int max_frames) {
    if (check_dims(B, K, max_frames)) return 0;
    return sizeof(int) * (size_t)B * K * max_frames;
}

int pika_msearch_commit(void *state, void *side, int B, int K, int max_frames, const int *which, int max_tail,
                        int rebase, int L, long long *tokens, long long *lengths, long long *slot_map, void *scratch,
                        void *stream) {
    return commit<false>(state, side, B, K, K, max_frames, which, max_tail, rebase, L, tokens, lengths, slot_map, scratch,
                         stream);
}

int pika_msearch_lm_commit(void *state, void *side, int B, int K, int C, int max_frames, const int *which, int max_tail,
                           int rebase, int L, long long *tokens, long long *lengths, long long *slot_map, void *scratch,
                           void *stream) {
    return commit<true>(state, side, B, K, C, max_frames, which, max_tail, rebase, L, tokens, lengths, slot_map, scratch,
                        stream);
}

// ---- time stamps: the record beside either blob (pika_msearch_times.h) ------------------------------------------------

size_t pika_msearch_times_bytes(int B, int K, int max_frames) {
    if (check_dims(B, K, max_frames)) return 0;
    return PIKA_MSEARCH_TIMES_PLANES_OFFSET(B) + 2 * sizeof(int) * (size_t)B * K * max_frames;
}

int pika_msearch_times_reset(void *times, int B, int K, int max_frames, const int *which, void *stream) {
    if (int rc = check_dims(B, K, max_frames)) return rc;
    if (!times) return PIKA_EINVAL;
    const size_t y = ((size_t)K * max_frames) / 4096;  // 16 entries per thread and plane
    hipLaunchKernelGGL(msearch_times_reset_kernel, dim3((unsigned)B, (unsigned)(y < 1 ? 1 : (y > 256 ? 256 : y))),
                       dim3(THREADS), 0, static_cast<hipStream_t>(stream), times_of(times, B, K, max_frames), K,
                       max_frames, which);
    return (int)hipGetLastError();
}

int pika_msearch_times_step(void *times, const void *state, const void *side, int B, int K, int C, int max_frames,
                            const long long *parent, const long long *token, int blank, void *stream) {
    if (blank < 0) return PIKA_EINVAL;
    if (int rc = check_times(B, K, C, max_frames)) return rc;
    if (!times || !state || !parent || !token) return PIKA_EINVAL;
    const Times tm = times_of(times, B, K, max_frames);
    const int *retired = side ? side_of(const_cast<void *>(side), B).retired : nullptr;
    const int vec = times_vec(times, max_frames);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C)
        hipLaunchKernelGGL((msearch_times_step_kernel<true>), dim3((unsigned)B), dim3(THREADS), 0, s, tm, state, retired,
                           B, K, max_frames, parent, token, blank, vec);
    else
        hipLaunchKernelGGL((msearch_times_step_kernel<false>), dim3((unsigned)B), dim3(THREADS), 0, s, tm, state, retired,
                           B, K, max_frames, parent, token, blank, vec);
    return (int)hipGetLastError();
}

int pika_msearch_times_hyps(const void *times, const void *state, int B, int K, int C, int max_frames, int L,
                            long long *out, void *stream) {
    if (L <= 0) return PIKA_EINVAL;
    if (int rc = check_times(B, K, C, max_frames)) return rc;
    if ((long long)K * L > 0x7fffffffll) return PIKA_ETOOBIG;
    if (!times || !state || !out) return PIKA_EINVAL;
    const Times tm = times_of(const_cast<void *>(times), B, K, max_frames);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C)
        hipLaunchKernelGGL((msearch_times_hyps_kernel<true>), dim3((unsigned)B), dim3(THREADS), 0, s, tm, state, B, K,
                           max_frames, L, out);
    else
        hipLaunchKernelGGL((msearch_times_hyps_kernel<false>), dim3((unsigned)B), dim3(THREADS), 0, s, tm, state, B, K,
                           max_frames, L, out);
    return (int)hipGetLastError();
}

int pika_msearch_times_results(const void *times, const void *state, int B, int K, int C, int max_frames, int N, int L,
                               const long long *tokens, const long long *lengths, long long *out, void *stream) {
    if (N <= 0 || L <= 0) return PIKA_EINVAL;
    if (int rc = check_times(B, K, C, max_frames)) return rc;
    if (N > K || (long long)N * L > 0x7fffffffll) return PIKA_ETOOBIG;
    if (!times || !state || !tokens || !lengths || !out) return PIKA_EINVAL;
    const Times tm = times_of(const_cast<void *>(times), B, K, max_frames);
    const unsigned mask = times_mask(K, C, max_frames);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C)
        hipLaunchKernelGGL((msearch_times_results_kernel<true>), dim3((unsigned)B, (unsigned)N), dim3(64), 0, s, tm, state,
                           B, K, max_frames, mask, N, L, tokens, lengths, out);
    else
        hipLaunchKernelGGL((msearch_times_results_kernel<false>), dim3((unsigned)B, (unsigned)N), dim3(64), 0, s, tm,
                           state, B, K, max_frames, mask, N, L, tokens, lengths, out);
    return (int)hipGetLastError();
}

int pika_msearch_times_commit(void *times, const void *state, int B, int K, int C, int max_frames, const int *which,
                              const long long *lengths, const long long *slot_map, int L, long long *out, void *stream) {
    if (L <= 0) return PIKA_EINVAL;
    if (int rc = check_times(B, K, C, max_frames)) return rc;
    if (!times || !state || !lengths || !slot_map || !out) return PIKA_EINVAL;
    const Times tm = times_of(times, B, K, max_frames);
    const int vec = times_vec(times, max_frames);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (C)
        hipLaunchKernelGGL((msearch_times_commit_kernel<true>), dim3((unsigned)B), dim3(THREADS), 0, s, tm, state, B, K,
                           max_frames, which, lengths, slot_map, L, out, vec);
    else
        hipLaunchKernelGGL((msearch_times_commit_kernel<false>), dim3((unsigned)B), dim3(THREADS), 0, s, tm, state, B, K,
                           max_frames, which, lengths, slot_map, L, out, vec);
    return (int)hipGetLastError();
}

}  // extern "C"
