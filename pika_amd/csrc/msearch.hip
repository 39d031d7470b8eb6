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
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "ctc_search_core.h"
#include "pika_msearch.h"

static_assert(ROOT == PIKA_MSEARCH_ROOT && MAX_BEAM == PIKA_MSEARCH_MAX_BEAM, "the constants the C ABI documents");

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int LIST_CAP = 1024;  // entries the collect pass can hold
constexpr float NINF = -INFINITY;

// where the parts of the blob lie
struct Blob {
    float *score;
    int *node, *len, *frames, *overflowed;
    unsigned long long *tables;
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
    return s;
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

__global__ __launch_bounds__(THREADS) void msearch_reset_kernel(void *state, int B, int K, size_t slots,
                                                                 const int *__restrict__ which) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;  // workgroup-uniform
    const Blob s = blob_of(state, B, K);
    unsigned long long *table = s.tables + (size_t)b * slots;
    for (size_t i = (size_t)blockIdx.y * THREADS + threadIdx.x; i < slots; i += (size_t)gridDim.y * THREADS)
        table[i] = EMPTY;
    if (blockIdx.y == 0) {
        const int k = threadIdx.x;
        if (k < K) {
            s.score[(size_t)b * K + k] = k == 0 ? 0.0f : NINF;
            s.node[(size_t)b * K + k] = ROOT;
            s.len[(size_t)b * K + k] = 0;
        }
        if (k == 0) { s.frames[b] = 0; s.overflowed[b] = 0; }
    }
}

__global__ __launch_bounds__(THREADS) void msearch_advance_kernel(void *state, const float *__restrict__ logits,
                                                                   long long ld, const long long *__restrict__ num_frames,
                                                                   int B, int K, int max_frames, int V, int blank,
                                                                   float sm_scale, float penalty, unsigned mask, int vec,
                                                                   long long *__restrict__ parent_out,
                                                                   long long *__restrict__ token_out) {
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
    const Blob st = blob_of(state, B, K);
    const size_t bk = (size_t)b * K;
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
    }
    if (tid == 0) { s_cnt = 0; s_all = 0; }
    __syncthreads();

    // 1  the rows
    for (int k = wave; k < K; k += WAVES) {
        const float score = s_score[k];
        if (!(score > NINF)) continue;  // wave-uniform: an empty slot
        const float *row = logits + (bk + k) * ld;
        float m = NINF, s = 0.0f, bx = NINF;
        int bv = 0x7fffffff;
        for_row(row, V, lane, vec != 0, [&](int v, float l) {
            const float x = scaled(l, v, blank, sm_scale, penalty);
            if (x > m) {
                s = __fadd_rn(__fmul_rn(s, expf(m - x)), 1.0f);
                m = x;
            } else if (x > NINF) {
                s += expf(x - m);
            }
            if (x > bx) { bx = x; bv = v; }
        });
        // the row's (max, sum): lane 0's tree, handed to every lane
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
        m = __shfl(m, 0);
        s = __shfl(s, 0);
        const float logs = logf(s);
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
    }
    __syncthreads();

    // 2  the threshold: the K-th of the lane maxima of all rows
    if (wave == 0) {
        const bool row_live = lane < K && s_score[lane] > NINF;
        int head = 0;
        Cand thr = {NINF, 0, 0};
        bool all = false;
        for (int r = 0; r < K; ++r) {
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
            if (rank < K) s_sel[rank] = e;
        }
        if (tid == 0) s_nsel = n < K ? n : K;
        __syncthreads();
    } else {
        // the list overflowed: the K best one at a time, each the best of what comes after the one before
        Cand prev = {INFINITY, -1, -1};
        int got = 0;
        for (int r = 0; r < K; ++r) {
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
    if (tid < K) { s_key[tid] = NONE; s_lead[tid] = 0; }
    __syncthreads();
    Cand me = {NINF, 0, blank};
    if (tid < nsel) {
        me = s_sel[tid];
        me.k = clampi(me.k, 0, K - 1);
        const int pn = s_node[me.k];
        s_key[tid] = me.v == blank ? pn : trie_node(table, mask, pn, me.v);
        s_klen[tid] = s_len[me.k] + (me.v == blank ? 0 : 1);
    }
    __syncthreads();
    if (tid < nsel) {
        const int key = s_key[tid];
        int rep = tid;
        for (int i = tid - 1; i >= 0; --i)
            if (s_key[i] == key) rep = i;
        if (rep == tid) {  // the group's best-ranked member sums the group in rank order
            float s = 0.0f;
            for (int i = tid; i < nsel; ++i)
                if (s_key[i] == key) s += expf(s_sel[i].c - me.c);
            s_merged[tid] = __fadd_rn(me.c, logf(s));
            s_lead[tid] = 1;
        }
    }
    __syncthreads();
    // the new beam: every group finds its place (s_from[j]: the entry that fills slot j), slot j's thread writes it
    if (tid < K) s_from[tid] = -1;
    __syncthreads();
    if (tid < nsel && s_lead[tid]) {
        const float mine = s_merged[tid];
        int pos = 0;
        for (int i = 0; i < nsel; ++i)
            if (s_lead[i] && i != tid && (s_merged[i] > mine || (s_merged[i] == mine && i < tid))) ++pos;
        if (mine > NINF) s_from[pos] = tid;  // (pos < the number of groups <= K)
    }
    __syncthreads();
    if (tid < K) {
        const int j = s_from[tid];
        const bool full = j >= 0;
        st.score[bk + tid] = full ? s_merged[j] : NINF;
        st.node[bk + tid] = full ? s_key[j] : ROOT;
        st.len[bk + tid] = full ? s_klen[j] : 0;
        parent_out[bk + tid] = full ? clampi(s_sel[j].k, 0, K - 1) : 0;
        token_out[bk + tid] = full ? s_sel[j].v : blank;
    }
    if (tid == 0) {
        st.frames[b] = frames + 1;
        if (frames + 1 >= max_frames && nf_raw > max_frames) st.overflowed[b] = 1;
    }
}

// the token sequences of `n` slots per utterance, slot j of the output from slot j of the beam
__global__ __launch_bounds__(64) void msearch_read_kernel(const void *state, int B, int K, int max_frames, unsigned mask,
                                                           int n, int L, long long *__restrict__ tokens,
                                                           long long *__restrict__ lengths, float *__restrict__ scores) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const Blob st = blob_of(const_cast<void *>(state), B, K);
    const unsigned long long *table = st.tables + (size_t)b * ((size_t)mask + 1);
    const size_t bk = (size_t)b * K;
    for (int j = 0; j < n; ++j) {  // (no entry is longer than max_frames: the rows are short, the lanes pad them)
        const float sc = st.score[bk + j];
        const bool live = sc > NINF;
        const int len = live ? clampi(st.len[bk + j], 0, max_frames) : -1;
        long long *out = tokens + ((size_t)b * n + j) * L;
        for (int p = lane; p < L; p += 64)
            if (p >= len) out[p] = -1;
        if (lane == 0) {
            lengths[(size_t)b * n + j] = len;
            if (scores) scores[(size_t)b * n + j] = live ? sc : NINF;
        }
    }
    if (lane < n) {
        const bool live = st.score[bk + lane] > NINF;
        const int len = live ? clampi(st.len[bk + lane], 0, max_frames) : 0;
        long long *out = tokens + ((size_t)b * n + lane) * L;
        int node = st.node[bk + lane];
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

static inline int check_dims(int B, int K, int max_frames) {
    if (B <= 0 || K <= 0 || max_frames <= 0) return PIKA_EINVAL;
    if (K > MAX_BEAM || B > 65535 || 2ll * max_frames * K > (1ll << 28)) return PIKA_ETOOBIG;
    return PIKA_OK;
}

static int read_out(const void *state, int B, int K, int max_frames, int n, int L, long long *tokens, long long *lengths,
                    float *scores, bool want_scores, void *stream) {
    if (n <= 0 || L <= 0) return PIKA_EINVAL;
    if (int rc = check_dims(B, K, max_frames)) return rc;
    if (n > K || (long long)n * L > 0x7fffffffll) return PIKA_ETOOBIG;
    if (!state || !tokens || !lengths || (want_scores && !scores)) return PIKA_EINVAL;
    hipLaunchKernelGGL(msearch_read_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), state, B,
                       K, max_frames, (unsigned)(table_slots(max_frames, K) - 1), n, L, tokens, lengths, scores);
    return (int)hipGetLastError();
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
    const size_t slots = table_slots(max_frames, K), y = slots / 4096;  // 16 keys per thread
    hipLaunchKernelGGL(msearch_reset_kernel, dim3((unsigned)B, (unsigned)(y < 1 ? 1 : (y > 256 ? 256 : y))),
                       dim3(THREADS), 0, static_cast<hipStream_t>(stream), state, B, K, slots, which);
    return (int)hipGetLastError();
}

int pika_msearch_advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K,
                         int max_frames, int V, int blank, float sm_scale, float blank_penalty, long long *parent_out,
                         long long *token_out, void *stream) {
    if (V < 2 || blank < 0 || blank >= V || ld < V || !std::isfinite(sm_scale) || !std::isfinite(blank_penalty)) return PIKA_EINVAL;
    if (int rc = check_dims(B, K, max_frames)) return rc;
    if (!state || !logits || !num_frames || !parent_out || !token_out) return PIKA_EINVAL;
    const int vec = ld % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
    hipLaunchKernelGGL(msearch_advance_kernel, dim3((unsigned)B), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       state, logits, ld, num_frames, B, K, max_frames, V, blank, sm_scale, blank_penalty,
                       (unsigned)(table_slots(max_frames, K) - 1), vec, parent_out, token_out);
    return (int)hipGetLastError();
}

int pika_msearch_results(const void *state, int B, int K, int max_frames, int nbest, int L, long long *tokens,
                         long long *lengths, float *scores, void *stream) {
    return read_out(state, B, K, max_frames, nbest, L, tokens, lengths, scores, true, stream);
}

int pika_msearch_hyps(const void *state, int B, int K, int max_frames, int L, long long *tokens, long long *lengths,
                      void *stream) {
    return read_out(state, B, K, max_frames, K, L, tokens, lengths, nullptr, false, stream);
}

}  // extern "C"
