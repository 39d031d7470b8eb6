// pika_amd/csrc/ctc_loss.hip -- CTC loss, gradient and forced alignment for gfx950 (MI355X), hand-written HIP.
//
// The loss the reference's LAS trainer builds as nn.CTCLoss() (trainer/train_las_bmuf_otfaug.py:58-81).  Same shape
// as rnnt_loss.hip, on the CTC lattice: S = 2U+1 states (blank, y1, blank, ..., yU, blank) by T frames.
//
//   gather    : one workgroup per (t, b) row of the (T,B,C) input writes the row's S state log-probs into the plane
//               [B][T][Wp] (Wp = S_max rounded up to 64; -1e30 in invalid cells).  The from-logits form computes the
//               row's log-sum-exp in the same pass (online max/sum, one read) and stores logit - lse.  The t == 0
//               workgroups also write the per-state rows: class, "skip transition allowed", and the chain of states
//               of one class (next state with the same class), so nothing about the transcript is re-derived per frame.
//   alpha/beta: one workgroup per (utterance, direction), both directions concurrent; lane = state.  The s-1 and s-2
//               neighbours arrive by two DPP wave shifts; across waves the two edge lanes go through LDS with ONE
//               barrier per frame, and only when S > 64.  Plane rows are prefetched UNR frames ahead into registers.
//               Numerics: the scaled form.  Every RENORM frames the workgroup subtracts its running maximum and
//               accumulates it in an fp64 offset, so the fp32 state values stay O(RENORM * |lp|) however long the
//               utterance is; a plain fp32 log-space lattice carries |alpha| ~ 3.5 T (ulp 1.2e-4 at T = 600).
//               alpha and beta both INCLUDE the frame's own emission.
//   grad      : one workgroup per (t, b) row writes the dense row once with 16-byte stores (zeros, or grad_cost *
//               softmax for the from-logits form), then -- after the workgroup's barrier -- the first state of every
//               class walks its chain in increasing state order and stores the class's entry.  No atomics: the sum
//               order is fixed, two runs are bit-identical.
//   align     : max-plus over the same plane, one byte of back-pointer per cell in the caller's scratch; the
//               back-trace stages the scratch through LDS a chunk of frames at a time and is walked by one thread.
//   n-best    : for the n-best list of a search, one workgroup per hypothesis straight on the (T,B,C) input -- no plane,
//               no replicated input: the scaled sum and the max-plus in one sweep, two bits of back-pointer per cell,
//               and per token the frames and the summed value of its run on the best path.
//   n-best loss: the full-sum scores again, differentiable: one workgroup per (hypothesis, direction) leaves alpha, beta,
//               offsets and state rows per hypothesis; the backward, one workgroup per (t, b) row, writes the dense row
//               once and adds every hypothesis's weighted occupancies to it in increasing k -- no N dense gradients.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctc_numerics.h"
#include "pika_ctc.h"

namespace {

constexpr int UNR = 8;     // frames prefetched per register batch
constexpr int RENORM = 8;  // frames between renormalisations (== UNR: the last frame of a batch)
constexpr int MAX_WAVES = 16;

struct Ctc {
    float *lp;      // [B][T][Wp] log-prob of state s's class at frame t, NEG where invalid
    float *alpha;   // [B][T][Wp] alpha minus off_a[b][t]
    float *beta;    // [B][T][Wp] beta  minus off_b[b][t]
    double *off_a;  // [B][T]
    double *off_b;  // [B][T]
    double *ll;     // [B] log-likelihood (<= NEG_HALF: infeasible)
    int *cls;       // [B][Wp] class of state s, -1 for s >= S_n
    int *skp;       // [B][Wp] bit 0: the s-2 -> s transition is allowed; bit 1: first state of its class
    int *nxt;       // [B][Wp] next state of the same class, -1 at the last
    int Wp;
};

inline int state_width(int U) { return (2 * U + 1 + 63) / 64 * 64; }

inline Ctc carve(void *ws, int B, int T, int U) {
    Ctc L;
    L.Wp = state_width(U);
    const size_t n = (size_t)B * T * L.Wp;  // a multiple of 64: what follows stays 8-byte aligned
    float *p = static_cast<float *>(ws);
    L.lp = p;
    L.alpha = p + n;
    L.beta = p + 2 * n;
    double *q = reinterpret_cast<double *>(p + 3 * n);
    L.off_a = q;
    L.off_b = q + (size_t)B * T;
    L.ll = q + 2 * (size_t)B * T;
    L.cls = reinterpret_cast<int *>(L.ll + B);
    L.skp = L.cls + (size_t)B * L.Wp;
    L.nxt = L.skp + (size_t)B * L.Wp;
    return L;
}

inline size_t workspace_bytes(int B, int T, int U) {
    const size_t Wp = (size_t)state_width(U);
    return 12 * (size_t)B * T * Wp + 16 * (size_t)B * T + 8 * (size_t)B + 12 * (size_t)B * Wp;
}

// dimensions first (a bad C or blank is PIKA_EINVAL even where the state axis would be PIKA_ETOOBIG)
int check_lattice_dims(int B, int T, int U) {
    if (B <= 0 || T <= 0 || U < 0) return PIKA_EINVAL;
    if (U > 511 || B > 65535) return PIKA_ETOOBIG;  // 2U+1 <= 1024; B is a grid's y extent
    return PIKA_OK;
}
int check_dims(int B, int T, int U, int C, int blank) {
    if (C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    return check_lattice_dims(B, T, U);
}

// log(exp(x)+exp(y)+exp(z)) on the transcendental pipe (v_exp_f32 / v_log_f32); one term is exp2(0) = 1
__device__ inline float lse3(float x, float y, float z) {
    const float m = fmaxf(fmaxf(x, y), z);
    const float e = __builtin_amdgcn_exp2f((x - m) * LOG2E) + __builtin_amdgcn_exp2f((y - m) * LOG2E) +
                    __builtin_amdgcn_exp2f((z - m) * LOG2E);
    return m + LN2 * __builtin_amdgcn_logf(e);
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ inline float dpp(float v, float fill) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
// lane i <- lane i-1 across the whole 64-lane wave (DPP wave_shr:1); lane 0 <- fill.
__device__ inline float wave_shr1(float v, float fill) { return dpp<0x138>(v, fill); }
// lane i <- lane i+1 (DPP wave_shl:1); lane 63 <- fill.
__device__ inline float wave_shl1(float v, float fill) { return dpp<0x130>(v, fill); }
// max over the 64 lanes, broadcast (row_shr 1/2/4/8 + row_bcast 15/31, then readlane 63).
__device__ inline float wave_max(float v) {
    v = fmaxf(v, dpp<0x111>(v, NEG));
    v = fmaxf(v, dpp<0x112>(v, NEG));
    v = fmaxf(v, dpp<0x114>(v, NEG));
    v = fmaxf(v, dpp<0x118>(v, NEG));
    v = fmaxf(v, dpp<0x142, 0xa>(v, NEG));
    v = fmaxf(v, dpp<0x143, 0xc>(v, NEG));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---------------------------------------------------------------------------------------------
// gather.  grid = (T, B), block = 256.
// ---------------------------------------------------------------------------------------------
template <bool LOGITS>
__global__ __launch_bounds__(256) void ctc_gather_kernel(const float *__restrict__ x, const int *__restrict__ targets,
                                                         const int *__restrict__ toff, const int *__restrict__ Tn_,
                                                         const int *__restrict__ Un_, int B, int T, int U_max, int C,
                                                         int blank, float *__restrict__ lse, Ctc L) {
    __shared__ float rm[256], rs[256];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max);
    const int S = 2 * Un + 1, Wp = L.Wp;
    const int *tg = toff ? targets + toff[b] : targets + (size_t)b * U_max;  // read only below Un
    const float *row = x + ((size_t)t * B + b) * C;
    float l = 0.0f;
    if constexpr (LOGITS) {
        if (t < Tn) {  // workgroup-uniform; rows t >= T_n are never read
            float m = NEG, s = 0.0f;  // online max / sum of exp: one read of the row
            auto take = [&](float v) __attribute__((always_inline)) {
                v = fmaxf(v, NEG);
                const float mn = fmaxf(m, v);
                s = s * __expf(m - mn) + __expf(v - mn);
                m = mn;
            };
            // a thread takes the groups of four classes tid, tid + 256, ... whichever way they are loaded, so the
            // log-sum-exp (and with it costs and gradient) does not depend on the alignment of the base pointer
            const bool vec = C % 4 == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0;  // workgroup-uniform
            for (int i = tid; i < (C + 3) / 4; i += 256) {
                if (vec) {
                    const v4f v = reinterpret_cast<const v4f *>(row)[i];
                    take(v.x); take(v.y); take(v.z); take(v.w);
                } else {
                    for (int k = 4 * i; k < min(4 * i + 4, C); ++k) take(row[k]);
                }
            }
            rm[tid] = m;
            rs[tid] = s;
            __syncthreads();
            for (int h = 128; h > 0; h >>= 1) {  // fixed tree: the same value on every run
                if (tid < h) {
                    const float m0 = rm[tid], m1 = rm[tid + h], mn = fmaxf(m0, m1);
                    rs[tid] = rs[tid] * __expf(m0 - mn) + rs[tid + h] * __expf(m1 - mn);
                    rm[tid] = mn;
                }
                __syncthreads();
            }
            l = rm[0] + logf(rs[0]);
        }
        if (tid == 0) lse[(size_t)t * B + b] = l;
    }
    for (int s = tid; s < Wp; s += 256) {
        const int c = s < S ? ((s & 1) ? tg[s >> 1] : blank) : -1;
        const bool ok = t < Tn && c >= 0 && c < C;
        L.lp[((size_t)b * T + t) * Wp + s] = ok ? fmaxf(row[c] - l, NEG) : NEG;
        if (t == 0) {  // the state rows, once per utterance
            int skip = 0, first = s < S, next = -1;
            if (s < S) {
                if ((s & 1) && s >= 3 && c != blank && c != tg[(s >> 1) - 1]) skip = 1;
                for (int q = 0; q < s; ++q)
                    if (((q & 1) ? tg[q >> 1] : blank) == c) { first = 0; break; }
                for (int q = s + 1; q < S; ++q)
                    if (((q & 1) ? tg[q >> 1] : blank) == c) { next = q; break; }
            }
            L.cls[(size_t)b * Wp + s] = c;
            L.skp[(size_t)b * Wp + s] = skip | (first << 1);
            L.nxt[(size_t)b * Wp + s] = next;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The neighbour exchange both recurrences and the alignment share: thread s <- threads s-1 and s-2 (up), or s+1 and
// s+2 (down).  MULTI == false: one wave, pure DPP.  MULTI: DPP inside a wave + the two edge lanes through LDS, one
// barrier per frame, buffers alternating with the frame's parity.
// ---------------------------------------------------------------------------------------------
struct Edges {
    float e[2][MAX_WAVES + 1][2];  // up: e[.][w+1] = lanes 62, 63 of wave w; down: e[.][w] = lanes 0, 1 of wave w
    float red[2][MAX_WAVES];
    float fin[2];
};

__device__ inline void edges_init(Edges &E) {
    float *p = &E.e[0][0][0];
    constexpr int n = sizeof(Edges) / sizeof(float);
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = NEG;
    __syncthreads();
}

template <bool MULTI>
__device__ inline void shift_up(Edges &E, float v, int step, float &p1, float &p2) {
    float f63 = NEG, f62 = NEG;
    if constexpr (MULTI) {
        const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
        if (l >= 62 && w + 1 < nw) E.e[step & 1][w + 1][l - 62] = v;
        __syncthreads();
        f62 = E.e[step & 1][w][0];
        f63 = E.e[step & 1][w][1];
    }
    p1 = wave_shr1(v, f63);
    p2 = wave_shr1(p1, f62);
}

template <bool MULTI>
__device__ inline void shift_down(Edges &E, float v, int step, float &n1, float &n2) {
    float f0 = NEG, f1 = NEG;
    if constexpr (MULTI) {
        const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
        if (l < 2 && w > 0) E.e[step & 1][w][l] = v;
        __syncthreads();
        f0 = E.e[step & 1][w + 1][0];
        f1 = E.e[step & 1][w + 1][1];
    }
    n1 = wave_shl1(v, f0);
    n2 = wave_shl1(n1, f1);
}

template <bool MULTI>
__device__ inline float max_all(Edges &E, float v, int count) {  // workgroup-wide max
    float m = wave_max(v);
    if constexpr (MULTI) {
        const int nw = blockDim.x >> 6;
        float *r = E.red[count & 1];
        if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = m;
        __syncthreads();
        for (int w = 0; w < nw; ++w) m = fmaxf(m, r[w]);
    }
    return m;
}

// One frame of the scaled sum, shared by every sweep that carries it: v = the frame's value of the state's class, a its
// own previous value, q1 and q2 the neighbours' one and two states away.
__device__ inline float sum_step(float v, float a, float q1, float q2, bool skip, bool valid) {
    const float an = v + lse3(a, q1, skip ? q2 : NEG);
    return valid ? fmaxf(an, NEG) : NEG;
}
// ... and the renormalisation that follows every RENORM-th frame: the running maximum moves into the fp64 offset.
template <bool MULTI>
__device__ inline float renorm(Edges &E, float a, int count, double &off) {
    float m = max_all<MULTI>(E, a, count);
    m = m > NEG_HALF ? m : 0.0f;
    a = a > NEG_HALF ? a - m : NEG;
    off += (double)m;
    return a;
}

// ---------------------------------------------------------------------------------------------
// alpha / beta.  grid = (2, B): blockIdx.x 0 = alpha, 1 = beta.  block = Wp threads, thread s owns state s.
//   alpha_t(s) = lp_t(s) + lse(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if skip(s)]),  alpha_{-1} = [0, NEG, ...]
//   beta_t(s)  = lp_t(s) + lse(beta_{t+1}(s),  beta_{t+1}(s+1),  [beta_{t+1}(s+2) if skip(s+2)]), beta_{T_n} = [..., NEG, 0]
// (the virtual rows make frame 0 / frame T_n-1 ordinary steps: alpha_0 is non-NEG at s = 0, 1 and beta_{T_n-1} at
// s = S-1, S-2 only).  ll = lse(alpha_{T_n-1}(S-1), alpha_{T_n-1}(S-2)) in fp64, from the alpha side.
// ---------------------------------------------------------------------------------------------
template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_alpha_beta_kernel(Ctc L, const int *__restrict__ Tn_,
                                                                           const int *__restrict__ Un_,
                                                                           float *__restrict__ costs, int T, int U_max) {
    __shared__ Edges E;
    edges_init(E);
    const int b = blockIdx.y, s = threadIdx.x, Wp = L.Wp;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max);
    const int S = 2 * Un + 1;
    const bool valid = s < S;
    const size_t base = (size_t)b * T * Wp + s;
    const float *lp = L.lp + base;
    const bool fwd = blockIdx.x == 0;
    float *out = (fwd ? L.alpha : L.beta) + base;
    double *offs = (fwd ? L.off_a : L.off_b) + (size_t)b * T;
    // is the transition over two states into this state (alpha) / out of it (beta) allowed
    const int sk_at = fwd ? s : s + 2;
    const bool skip = sk_at < Wp && (L.skp[(size_t)b * Wp + sk_at] & 1);
    // frame of step j: alpha walks up from 0, beta down from T_n - 1
    auto frame = [&](int j) __attribute__((always_inline)) { return fwd ? j : Tn - 1 - j; };

    float cur[UNR], nx[UNR];
    auto load = [&](float *dst, int j0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) dst[i] = lp[(size_t)frame(min(j0 + i, Tn - 1)) * Wp];
    };
    float a = (fwd ? s == 0 : s == S - 1) ? 0.0f : NEG;
    double off = 0.0;  // sum of the subtracted maxima (identical in every thread)
    load(cur, 0);
    for (int j0 = 0; j0 < Tn; j0 += UNR) {
        load(nx, j0 + UNR);
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const int j = j0 + i;
            if (j < Tn) {  // workgroup-uniform
                float q1, q2;
                if (fwd) shift_up<MULTI>(E, a, j, q1, q2);
                else shift_down<MULTI>(E, a, j, q1, q2);
                a = sum_step(cur[i], a, q1, q2, skip, valid);
                if (i == UNR - 1) a = renorm<MULTI>(E, a, j / RENORM, off);  // j = RENORM - 1 (mod RENORM)
                out[(size_t)frame(j) * Wp] = a;
                if (s == 0) offs[frame(j)] = off;
            }
        }
#pragma unroll
        for (int i = 0; i < UNR; ++i) cur[i] = nx[i];
    }
    if (fwd) {
        if (s == S - 1) E.fin[0] = a;
        if (s == S - 2) E.fin[1] = a;  // S == 1: stays NEG
        __syncthreads();
        if (s == 0) {
            const float x = E.fin[0], y = E.fin[1], m = fmaxf(x, y);
            if (m > NEG_HALF) {
                const double ll = off + (double)m + log(exp((double)(x - m)) + exp((double)(y - m)));
                L.ll[b] = ll;
                costs[b] = (float)(-ll);
            } else {  // no path reaches the end: infeasible
                L.ll[b] = (double)NEG;
                costs[b] = __builtin_inff();
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// grad.  grid = (T, B), block = 256.  LOGITS: d/d logits = gc * (softmax - occ); else d/d log_probs = -gc * occ, with
// occ(c) = sum_{s : cls(s) = c} exp(alpha + beta - lp - ll), the exponent assembled in fp64 from the planes and offsets.
// ---------------------------------------------------------------------------------------------
template <bool LOGITS>
__global__ __launch_bounds__(256) void ctc_grad_kernel(Ctc L, const float *__restrict__ x, const float *__restrict__ lse,
                                                       const int *__restrict__ Tn_, const float *__restrict__ grad_costs,
                                                       int B, int T, int C, float *__restrict__ g) {
    __shared__ float e[MAX_WAVES * 64];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, Wp = L.Wp;
    const int Tn = clampi(Tn_[b], 1, T);
    const double ll = L.ll[b];
    const bool live = t < Tn && ll > (double)NEG_HALF;  // workgroup-uniform
    const float gc = grad_costs ? grad_costs[b] : 1.0f;
    const size_t r = ((size_t)t * B + b) * C;
    float *out = g + r;
    const float *in = LOGITS ? x + r : nullptr;
    const float l = (LOGITS && live) ? lse[(size_t)t * B + b] : 0.0f;
    const int *cls = L.cls + (size_t)b * Wp, *skp = L.skp + (size_t)b * Wp, *nxt = L.nxt + (size_t)b * Wp;
    if (live) {
        const double k = L.off_a[(size_t)b * T + t] + L.off_b[(size_t)b * T + t] - ll;
        for (int s = tid; s < Wp; s += 256) {
            const size_t o = ((size_t)b * T + t) * Wp + s;
            const int c = cls[s];
            const double arg = k + ((double)L.alpha[o] + (double)L.beta[o] - (double)L.lp[o]);
            e[s] = (c >= 0 && c < C) ? expf((float)fmax(arg, -1.0e30)) : 0.0f;
        }
    }
    // the whole row once: zeros, or gc * softmax
    auto fill = [&](float v) __attribute__((always_inline)) { return (LOGITS && live) ? gc * expf(v - l) : 0.0f; };
    if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
        (!LOGITS || (reinterpret_cast<uintptr_t>(in) & 15) == 0)) {
        v4f *out4 = reinterpret_cast<v4f *>(out);
        for (int i = tid; i < C / 4; i += 256) {
            v4f v = {0.f, 0.f, 0.f, 0.f};
            if (LOGITS && live) {
                const v4f u = reinterpret_cast<const v4f *>(in)[i];
                v.x = fill(u.x); v.y = fill(u.y); v.z = fill(u.z); v.w = fill(u.w);
            }
            out4[i] = v;
        }
    } else {
        for (int i = tid; i < C; i += 256) out[i] = (LOGITS && live) ? fill(in[i]) : 0.0f;
    }
    if (!live) return;
    __syncthreads();  // e[] is complete, and the row's fill is ordered before the entries stored below
    for (int s = tid; s < Wp; s += 256) {
        const int c = cls[s];
        if ((skp[s] & 2) && c >= 0 && c < C) {  // first state of its class: sums the class in state order
            float occ = 0.0f;
            for (int q = s; q >= 0; q = nxt[q]) occ += e[q];
            out[c] = LOGITS ? gc * (expf(in[c] - l) - occ) : 0.0f - gc * occ;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// forced alignment.  grid = B, block = Wp.  delta_t(s) = lp_t(s) + max(delta_{t-1}(s), delta_{t-1}(s-1),
// [delta_{t-1}(s-2) if skip(s)]), the predecessor chosen with strict > in that order (a tie keeps the earlier one:
// stay, then s-1, then s-2).  Back-pointer byte = how many states the path came up.
// ---------------------------------------------------------------------------------------------
constexpr int CHUNK_BYTES = 16384;  // >= 16 frames of back-pointers at the widest state axis

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_align_kernel(Ctc L, const int *__restrict__ Tn_,
                                                                      const int *__restrict__ Un_,
                                                                      float *__restrict__ scores,
                                                                      int *__restrict__ frame_labels,
                                                                      unsigned char *__restrict__ bp_, int T, int U_max) {
    __shared__ Edges E;
    __shared__ unsigned int chunk[CHUNK_BYTES / 4];
    __shared__ int clsL[MAX_WAVES * 64];
    __shared__ int endState;
    edges_init(E);
    const int b = blockIdx.x, s = threadIdx.x, Wp = L.Wp;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max);
    const int S = 2 * Un + 1;
    const bool valid = s < S;
    const float *lp = L.lp + (size_t)b * T * Wp + s;
    unsigned char *bp = bp_ + (size_t)b * T * Wp;
    const bool skip = L.skp[(size_t)b * Wp + s] & 1;
    clsL[s] = L.cls[(size_t)b * Wp + s];

    float cur[UNR], nx[UNR];
    auto load = [&](float *dst, int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) dst[i] = lp[(size_t)min(t0 + i, Tn - 1) * Wp];
    };
    float v = s == 0 ? 0.0f : NEG;
    load(cur, 0);
    for (int t0 = 0; t0 < Tn; t0 += UNR) {
        load(nx, t0 + UNR);
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const int t = t0 + i;
            if (t < Tn) {  // workgroup-uniform
                float p1, p2;
                shift_up<MULTI>(E, v, t, p1, p2);
                float best = v;
                unsigned char k = 0;
                if (s >= 1 && p1 > best) { best = p1; k = 1; }
                if (skip && p2 > best) { best = p2; k = 2; }
                v = valid ? fmaxf(cur[i] + best, NEG) : NEG;
                bp[(size_t)t * Wp + s] = k;
            }
        }
#pragma unroll
        for (int i = 0; i < UNR; ++i) cur[i] = nx[i];
    }
    if (s == S - 1) E.fin[0] = v;
    if (s == S - 2) E.fin[1] = v;
    __syncthreads();  // fin, clsL and (workgroup-scope) the back-pointers are written
    if (s == 0) {
        const bool second = S >= 2 && E.fin[1] > E.fin[0];  // a tie ends in the final blank
        scores[b] = second ? E.fin[1] : E.fin[0];
        endState = second ? S - 2 : S - 1;
    }
    for (int t = Tn + s; t < T; t += blockDim.x) frame_labels[(size_t)b * T + t] = -1;
    // back-trace, a chunk of frames at a time through LDS
    const int rows = CHUNK_BYTES / Wp;
    int cs = 0;
    for (int thi = Tn - 1; thi >= 0; thi -= rows) {  // workgroup-uniform
        const int tlo = max(thi - rows + 1, 0);
        const unsigned int *src = reinterpret_cast<const unsigned int *>(bp + (size_t)tlo * Wp);
        const int words = (thi - tlo + 1) * (Wp / 4);
        __syncthreads();  // the previous chunk is walked (first pass: endState is written)
        for (int i = s; i < words; i += blockDim.x) chunk[i] = src[i];
        __syncthreads();
        if (s == 0) {
            if (thi == Tn - 1) cs = endState;
            const unsigned char *cb = reinterpret_cast<const unsigned char *>(chunk);
            for (int t = thi; t >= tlo; --t) {
                frame_labels[(size_t)b * T + t] = clsL[cs];
                cs -= cb[(size_t)(t - tlo) * Wp + cs];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// n-best alignment.  grid = (N, B): one workgroup per hypothesis, block = Wp, thread s owns state s of ITS hypothesis.
// No plane: the workgroup derives class, skip and validity of its states from `tokens` (an LDS row) and reads every
// frame's value straight from x[t * stride_t + b * stride_b + cls(s)] (minus lse[t,b] for logits), UNR frames ahead.
// One sweep over t advances BOTH recurrences on that value -- the scaled sum of ctc_alpha_beta_kernel (same operations,
// same renormalisation frames, fp64 offset) and the max-plus of ctc_align_kernel (same comparison order) -- with one
// neighbour exchange: the edge lanes of both go through LDS behind the same barrier.  Back-pointers: TWO BITS per cell,
// four frames of one state to a byte (a lane packs its own four values in a register and stores one byte), rows of Wp
// bytes per group of four frames.  The back-trace is ctc_align_kernel's, chunked through LDS, and leaves the first and
// last frame of every visited state in LDS; lane 2j+1 then writes token j's times and sums its own run in time order.
// ---------------------------------------------------------------------------------------------
template <bool MULTI>
__device__ inline void shift_up2(Edges &Ea, Edges &Ev, float a, float v, int step, float &a1, float &a2, float &v1,
                                 float &v2) {
    float a63 = NEG, a62 = NEG, v63 = NEG, v62 = NEG;
    if constexpr (MULTI) {
        const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
        if (l >= 62 && w + 1 < nw) {
            Ea.e[step & 1][w + 1][l - 62] = a;
            Ev.e[step & 1][w + 1][l - 62] = v;
        }
        __syncthreads();
        a62 = Ea.e[step & 1][w][0];
        a63 = Ea.e[step & 1][w][1];
        v62 = Ev.e[step & 1][w][0];
        v63 = Ev.e[step & 1][w][1];
    }
    a1 = wave_shr1(a, a63);
    a2 = wave_shr1(a1, a62);
    v1 = wave_shr1(v, v63);
    v2 = wave_shr1(v1, v62);
}

__host__ __device__ inline int nbest_groups(int T) { return (T + 3) / 4; }  // back-pointer rows: four frames to a byte

template <bool MULTI, bool LOGITS>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_nbest_align_kernel(
    const float *__restrict__ x, long long stride_t, long long stride_b, const float *__restrict__ lse,
    const int *__restrict__ Tn_, const int *__restrict__ tokens, const int *__restrict__ lengths, int B, int N, int L,
    int T, int C, int blank, int U_max, float *__restrict__ full, float *__restrict__ best, int *__restrict__ starts,
    int *__restrict__ ends, float *__restrict__ tscores, unsigned char *__restrict__ bp_) {
    __shared__ Edges Ea, Ev;
    __shared__ unsigned int chunk[CHUNK_BYTES / 4];
    __shared__ int tokL[MAX_WAVES * 32];
    __shared__ int firstL[MAX_WAVES * 64], lastL[MAX_WAVES * 64];
    __shared__ int badToken;
    const int b = blockIdx.y, s = threadIdx.x, Wp = blockDim.x;
    const size_t h = (size_t)b * N + blockIdx.x;
    const int Tn = clampi(Tn_[b], 1, T);
    const int U = lengths[h];
    int *so = starts + h * L, *eo = ends + h * L;
    float *to = tscores + h * L;
    // an entry that has no alignment: times -1, token scores -inf, both scores `score`
    auto refuse = [&](float score) __attribute__((always_inline)) {
        for (int j = s; j < L; j += Wp) {
            so[j] = -1;
            eo[j] = -1;
            to[j] = -__builtin_inff();
        }
        if (s == 0) {
            full[h] = score;
            best[h] = score;
        }
    };
    if (U < 0 || U > min(U_max, L)) {  // workgroup-uniform: missing (-inf), or longer than the state axis (NaN)
        refuse(U < 0 ? -__builtin_inff() : __builtin_nanf(""));
        return;
    }
    const int S = 2 * U + 1;
    if (s == 0) badToken = 0;
    firstL[s] = -1;
    lastL[s] = -1;
    edges_init(Ea);
    edges_init(Ev);
    for (int j = s; j < U; j += Wp) {
        const int c = tokens[h * L + j];
        tokL[j] = c;
        if (c < 0 || c >= C || c == blank) badToken = 1;
    }
    __syncthreads();
    if (badToken) {  // workgroup-uniform; nothing was read through the token
        refuse(-__builtin_inff());
        return;
    }
    const bool valid = s < S;
    const int cls = (valid && (s & 1)) ? tokL[s >> 1] : blank;  // in [0,C) from here on
    const bool skip = valid && (s & 1) && s >= 3 && cls != tokL[(s >> 1) - 1];
    const float *xs = x + (long long)b * stride_b + cls;
    unsigned char *bp = bp_ + h * (size_t)nbest_groups(T) * Wp;
    auto value = [&](int t) __attribute__((always_inline)) {  // t in [0, T_n)
        float e = xs[(long long)t * stride_t];
        if constexpr (LOGITS) e -= lse[(size_t)t * B + b];
        return fmaxf(e, NEG);
    };

    float cur[UNR], nx[UNR];
    auto load = [&](float *dst, int t0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) dst[i] = value(min(t0 + i, Tn - 1));
    };
    float a = s == 0 ? 0.0f : NEG, v = a;
    double off = 0.0;  // sum of the subtracted maxima (identical in every thread)
    unsigned int pk = 0;
    load(cur, 0);
    for (int t0 = 0; t0 < Tn; t0 += UNR) {
        load(nx, t0 + UNR);
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const int t = t0 + i;
            if (t < Tn) {  // workgroup-uniform
                float a1, a2, v1, v2;
                shift_up2<MULTI>(Ea, Ev, a, v, t, a1, a2, v1, v2);
                a = sum_step(cur[i], a, a1, a2, skip, valid);
                float top = v;
                unsigned int k = 0;
                if (s >= 1 && v1 > top) { top = v1; k = 1; }
                if (skip && v2 > top) { top = v2; k = 2; }
                v = valid ? fmaxf(cur[i] + top, NEG) : NEG;
                pk |= k << (2 * (i & 3));  // t0 is a multiple of 4: i & 3 == t & 3
                if ((i & 3) == 3 || t == Tn - 1) {
                    bp[(size_t)(t >> 2) * Wp + s] = (unsigned char)pk;
                    pk = 0;
                }
                if (i == UNR - 1) a = renorm<MULTI>(Ea, a, t / RENORM, off);  // t = RENORM - 1 (mod RENORM)
            }
        }
#pragma unroll
        for (int i = 0; i < UNR; ++i) cur[i] = nx[i];
    }
    if (s == S - 1) { Ea.fin[0] = a; Ev.fin[0] = v; }
    if (s == S - 2) { Ea.fin[1] = a; Ev.fin[1] = v; }  // S == 1: stays NEG
    __syncthreads();  // fin and (workgroup-scope) the back-pointers are written
    const float fa0 = Ea.fin[0], fa1 = Ea.fin[1], fv0 = Ev.fin[0], fv1 = Ev.fin[1];
    const float ma = fmaxf(fa0, fa1);
    const bool second = S >= 2 && fv1 > fv0;  // a tie ends in the final blank
    const float vb = second ? fv1 : fv0;
    if (!(ma > NEG_HALF) || !(vb > NEG_HALF)) {  // workgroup-uniform: no path reaches the end
        refuse(-__builtin_inff());
        return;
    }
    if (s == 0) {
        full[h] = (float)(off + (double)ma + log(exp((double)(fa0 - ma)) + exp((double)(fa1 - ma))));
        best[h] = vb;
    }
    // back-trace, a chunk of four-frame rows at a time through LDS
    const int rows = CHUNK_BYTES / Wp;
    int cs = second ? S - 2 : S - 1, prev = -1;
    for (int ghi = (Tn - 1) >> 2; ghi >= 0; ghi -= rows) {  // workgroup-uniform
        const int glo = max(ghi - rows + 1, 0);
        const unsigned int *src = reinterpret_cast<const unsigned int *>(bp + (size_t)glo * Wp);
        const int words = (ghi - glo + 1) * (Wp / 4);
        __syncthreads();  // the previous chunk is walked
        for (int i = s; i < words; i += Wp) chunk[i] = src[i];
        __syncthreads();
        if (s == 0) {
            const unsigned char *cb = reinterpret_cast<const unsigned char *>(chunk);
            for (int t = min(4 * ghi + 3, Tn - 1); t >= 4 * glo; --t) {
                if (cs != prev) {
                    lastL[cs] = t;
                    prev = cs;
                }
                firstL[cs] = t;
                cs -= (cb[(size_t)((t >> 2) - glo) * Wp + cs] >> (2 * (t & 3))) & 3;
            }
        }
    }
    __syncthreads();
    for (int j = U + s; j < L; j += Wp) {
        so[j] = -1;
        eo[j] = -1;
        to[j] = -__builtin_inff();
    }
    if (valid && (s & 1)) {  // a label state: on the path of every feasible hypothesis
        const int t0 = clampi(firstL[s], 0, Tn - 1), t1 = clampi(lastL[s], t0, Tn - 1);
        float acc = 0.0f;
        for (int t = t0; t <= t1; ++t) acc += value(t);
        so[s >> 1] = t0;
        eo[s >> 1] = t1;
        to[s >> 1] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// n-best loss: the full-sum scores of an n-best list WITH their gradient.  The lattice of hypothesis (b, k) in the
// caller's workspace, what ctc_grad_kernel reads per utterance, per hypothesis -- and no lp plane: forward and backward
// both read the value of a state's class straight from the utterance's own rows of x.
// ---------------------------------------------------------------------------------------------
struct Nbl {
    float *alpha;   // [B][N][T][Wp] alpha minus off_a[b][k][t]
    float *beta;    // [B][N][T][Wp] beta  minus off_b[b][k][t]
    double *off_a;  // [B][N][T]
    double *off_b;  // [B][N][T]
    double *ll;     // [B][N] log-likelihood; NEG: a dead entry (missing, infeasible, too long) -- its planes are never read
    int *cls;       // [B][N][Wp] as Ctc::cls, skp, nxt
    int *skp;
    int *nxt;
    int Wp;
};

inline Nbl carve_nbest(void *ws, int B, int N, int T, int U) {
    Nbl W;
    W.Wp = state_width(U);
    const size_t hn = (size_t)B * N, n = hn * T * W.Wp;  // n: a multiple of 64, what follows stays 8-byte aligned
    float *p = static_cast<float *>(ws);
    W.alpha = p;
    W.beta = p + n;
    double *q = reinterpret_cast<double *>(p + 2 * n);
    W.off_a = q;
    W.off_b = q + hn * T;
    W.ll = q + 2 * hn * T;
    W.cls = reinterpret_cast<int *>(W.ll + hn);
    W.skp = W.cls + hn * W.Wp;
    W.nxt = W.skp + hn * W.Wp;
    return W;
}

// forward.  grid = (2, N, B): blockIdx.x 0 = alpha, 1 = beta, both concurrent; block = Wp, thread s owns state s of
// hypothesis (b, k).  The recurrences and their numerics are ctc_alpha_beta_kernel's (the alpha side is the scaled sum of
// ctc_nbest_align_kernel, operation for operation), the classification of an entry is ctc_nbest_align_kernel's and
// happens in both workgroups alike; the alpha workgroup also writes the state rows, ll and full_scores.
template <bool MULTI, bool LOGITS>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_nbest_loss_kernel(
    const float *__restrict__ x, long long stride_t, long long stride_b, const float *__restrict__ lse,
    const int *__restrict__ Tn_, const int *__restrict__ tokens, const int *__restrict__ lengths, int B, int N, int L,
    int T, int C, int blank, int U_max, float *__restrict__ full, Nbl W) {
    __shared__ Edges E;
    __shared__ int tokL[MAX_WAVES * 32];
    __shared__ int badToken;
    const bool fwd = blockIdx.x == 0;
    const int b = blockIdx.z, s = threadIdx.x, Wp = blockDim.x;
    const size_t h = (size_t)b * N + blockIdx.y;
    const int Tn = clampi(Tn_[b], 1, T);
    const int U = lengths[h];
    // a dead entry: ll as the loss marks an infeasible utterance, so the backward skips it
    auto refuse = [&](float score) __attribute__((always_inline)) {
        if (fwd && s == 0) {
            W.ll[h] = (double)NEG;
            full[h] = score;
        }
    };
    if (U < 0 || U > min(U_max, L)) {  // workgroup-uniform: missing (-inf), or longer than the state axis (NaN)
        refuse(U < 0 ? -__builtin_inff() : __builtin_nanf(""));
        return;
    }
    const int S = 2 * U + 1;
    if (s == 0) badToken = 0;
    edges_init(E);
    for (int j = s; j < U; j += Wp) {
        const int c = tokens[h * L + j];
        tokL[j] = c;
        if (c < 0 || c >= C || c == blank) badToken = 1;
    }
    __syncthreads();
    if (badToken) {  // workgroup-uniform; nothing was read through the token
        refuse(-__builtin_inff());
        return;
    }
    const bool valid = s < S;
    const int cls = (valid && (s & 1)) ? tokL[s >> 1] : blank;  // in [0,C) from here on
    // is the transition over two states into this state (alpha) / out of it (beta) allowed
    const bool skip_in = valid && (s & 1) && s >= 3 && cls != tokL[(s >> 1) - 1];
    const bool skip_out = (s & 1) && s + 2 < S && tokL[(s >> 1) + 1] != cls;
    const bool skip = fwd ? skip_in : skip_out;
    if (fwd) {  // the state rows: first of its class, next of its class (blank: the even states; a label: its repeats)
        int first = valid, next = -1;
        if (valid && (s & 1)) {
            for (int j = 0; j < (s >> 1); ++j)
                if (tokL[j] == cls) { first = 0; break; }
            for (int j = (s >> 1) + 1; j < U; ++j)
                if (tokL[j] == cls) { next = 2 * j + 1; break; }
        } else if (valid) {
            first = s == 0;
            next = s + 2 < S ? s + 2 : -1;
        }
        W.cls[h * Wp + s] = valid ? cls : -1;
        W.skp[h * Wp + s] = (int)skip_in | (first << 1);
        W.nxt[h * Wp + s] = next;
    }
    const float *xs = x + (long long)b * stride_b + cls;
    auto value = [&](int t) __attribute__((always_inline)) {  // t in [0, T_n)
        float e = xs[(long long)t * stride_t];
        if constexpr (LOGITS) e -= lse[(size_t)t * B + b];
        return fmaxf(e, NEG);
    };
    // frame of step j: alpha walks up from 0, beta down from T_n - 1
    auto frame = [&](int j) __attribute__((always_inline)) { return fwd ? j : Tn - 1 - j; };
    float *out = (fwd ? W.alpha : W.beta) + h * (size_t)T * Wp + s;
    double *offs = (fwd ? W.off_a : W.off_b) + h * (size_t)T;

    float cur[UNR], nx[UNR];
    auto load = [&](float *dst, int j0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) dst[i] = value(frame(min(j0 + i, Tn - 1)));
    };
    float a = (fwd ? s == 0 : s == S - 1) ? 0.0f : NEG;
    double off = 0.0;  // sum of the subtracted maxima (identical in every thread)
    load(cur, 0);
    for (int j0 = 0; j0 < Tn; j0 += UNR) {
        load(nx, j0 + UNR);
#pragma unroll
        for (int i = 0; i < UNR; ++i) {
            const int j = j0 + i;
            if (j < Tn) {  // workgroup-uniform
                float q1, q2;
                if (fwd) shift_up<MULTI>(E, a, j, q1, q2);
                else shift_down<MULTI>(E, a, j, q1, q2);
                a = sum_step(cur[i], a, q1, q2, skip, valid);
                if (i == UNR - 1) a = renorm<MULTI>(E, a, j / RENORM, off);  // j = RENORM - 1 (mod RENORM)
                out[(size_t)frame(j) * Wp] = a;
                if (s == 0) offs[frame(j)] = off;
            }
        }
#pragma unroll
        for (int i = 0; i < UNR; ++i) cur[i] = nx[i];
    }
    if (fwd) {
        if (s == S - 1) E.fin[0] = a;
        if (s == S - 2) E.fin[1] = a;  // S == 1: stays NEG
        __syncthreads();
        if (s == 0) {
            const float fa0 = E.fin[0], fa1 = E.fin[1], ma = fmaxf(fa0, fa1);
            if (ma > NEG_HALF) {
                const double ll = off + (double)ma + log(exp((double)(fa0 - ma)) + exp((double)(fa1 - ma)));
                W.ll[h] = ll;
                full[h] = (float)ll;
            } else {  // no path reaches the end: infeasible
                refuse(-__builtin_inff());
            }
        }
    }
}

// backward.  grid = (T, B), block = 256: row (t, b) of d sum_k g[b,k] * full[b,k] / d x, written once.  First the whole
// row -- zeros, or -(sum of the live g) * softmax for logits -- then, hypothesis by hypothesis in increasing k, the first
// state of every class walks its chain in increasing state order and adds g[b,k] * occ_k to the class's entry of the row,
// which the workgroup revisits in global memory: any C, no table of classes, no atomics.  One barrier per live
// hypothesis: e[] alternates, and the barrier that completes hypothesis k's e[] also orders every earlier store to the
// row (the fill, the entries of the hypotheses before) ahead of k's read-modify-writes.
template <bool LOGITS>
__global__ __launch_bounds__(256) void ctc_nbest_grad_kernel(Nbl W, const float *__restrict__ x, long long stride_t,
                                                             long long stride_b, const float *__restrict__ lse,
                                                             const int *__restrict__ Tn_,
                                                             const float *__restrict__ grad_scores, int B, int N, int T,
                                                             int C, float *g) {
    __shared__ float e[2][MAX_WAVES * 64];
    __shared__ float gsum;
    __shared__ int nlive;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, Wp = W.Wp;
    const int Tn = clampi(Tn_[b], 1, T);
    const bool in_time = t < Tn;  // workgroup-uniform; rows t >= T_b of x are never read
    float *out = g + ((size_t)t * B + b) * C;
    const float *in = x + (long long)t * stride_t + (long long)b * stride_b;
    const double *lls = W.ll + (size_t)b * N;
    const float *gs = grad_scores + (size_t)b * N;
    if (in_time) {
        if (tid == 0) {  // in increasing k; the weight of a dead entry is never loaded
            float sum = 0.0f;
            int n = 0;
            for (int k = 0; k < N; ++k)
                if (lls[k] > (double)NEG_HALF) {
                    sum += gs[k];
                    ++n;
                }
            gsum = sum;
            nlive = n;
        }
        __syncthreads();
    }
    const bool live = in_time && nlive > 0;  // workgroup-uniform
    const float l = (LOGITS && live) ? lse[(size_t)t * B + b] : 0.0f;
    const float gt = live ? gsum : 0.0f;
    // the whole row once: zeros, or -gt * softmax
    auto fill = [&](float v) __attribute__((always_inline)) { return (LOGITS && live) ? 0.0f - gt * expf(v - l) : 0.0f; };
    if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
        (!LOGITS || (reinterpret_cast<uintptr_t>(in) & 15) == 0)) {
        v4f *out4 = reinterpret_cast<v4f *>(out);
        for (int i = tid; i < C / 4; i += 256) {
            v4f v = {0.f, 0.f, 0.f, 0.f};
            if (LOGITS && live) {
                const v4f u = reinterpret_cast<const v4f *>(in)[i];
                v.x = fill(u.x); v.y = fill(u.y); v.z = fill(u.z); v.w = fill(u.w);
            }
            out4[i] = v;
        }
    } else {
        for (int i = tid; i < C; i += 256) out[i] = (LOGITS && live) ? fill(in[i]) : 0.0f;
    }
    if (!live) return;
    int buf = 0;
    for (int k = 0; k < N; ++k) {
        const size_t h = (size_t)b * N + k;
        const double ll = lls[k];
        if (!(ll > (double)NEG_HALF)) continue;  // workgroup-uniform
        const float gk = gs[k];
        const int *cls = W.cls + h * Wp, *skp = W.skp + h * Wp, *nxt = W.nxt + h * Wp;
        const double off = W.off_a[h * T + t] + W.off_b[h * T + t] - ll;
        float *ek = e[buf];
        for (int s = tid; s < Wp; s += 256) {
            const size_t o = (h * T + t) * Wp + s;
            const int c = cls[s];
            float v = 0.0f;
            if (c >= 0 && c < C) {
                const float val = fmaxf(LOGITS ? in[c] - l : in[c], NEG);
                const double arg = off + ((double)W.alpha[o] + (double)W.beta[o] - (double)val);
                v = expf((float)fmax(arg, -1.0e30));
            }
            ek[s] = v;
        }
        __syncthreads();
        for (int s = tid; s < Wp; s += 256) {
            const int c = cls[s];
            if ((skp[s] & 2) && c >= 0 && c < C) {  // first state of its class: sums the class in state order
                float occ = 0.0f;
                for (int q = s; q >= 0; q = nxt[q]) occ += ek[q];
                out[c] += gk * occ;
            }
        }
        buf ^= 1;
    }
}

// what the n-best call refuses, dimensions first
int check_nbest_dims(int B, int N, int T, int U) {
    if (B <= 0 || N <= 0 || T <= 0 || U < 0) return PIKA_EINVAL;
    if (U > 511 || B > 65535 || N > 65535) return PIKA_ETOOBIG;  // 2U+1 <= 1024; N and B are the grid's extents
    size_t n;
    if (__builtin_mul_overflow((size_t)B * (size_t)N, (size_t)nbest_groups(T) * (size_t)state_width(U), &n))
        return PIKA_ETOOBIG;
    return PIKA_OK;
}

// the n-best loss's workspace: two planes, two offset rows, ll, three state rows
inline size_t nbest_loss_bytes(int B, int N, int T, int U) {
    const size_t hn = (size_t)B * N, Wp = (size_t)state_width(U);
    return 8 * hn * T * Wp + 16 * hn * T + 8 * hn + 12 * hn * Wp;
}
int check_nbest_loss_dims(int B, int N, int T, int U) {
    if (B <= 0 || N <= 0 || T <= 0 || U < 0) return PIKA_EINVAL;
    if (U > 511 || B > 65535 || N > 65535) return PIKA_ETOOBIG;  // 2U+1 <= 1024; N and B are the grid's extents
    size_t n;  // the small rows together stay below 24 times the cells of one plane
    if (__builtin_mul_overflow((size_t)B * (size_t)N, (size_t)T * (size_t)state_width(U), &n) || n > SIZE_MAX / 32)
        return PIKA_ETOOBIG;
    return PIKA_OK;
}

// gather + the two recurrences: what both forward calls enqueue
template <bool LOGITS>
int forward(const float *x, const int *targets, const int *toff, const int *Tn, const int *Un, int B, int T, int U, int C,
            int blank, float *costs, float *lse, void *workspace, void *stream) {
    if (int rc = check_dims(B, T, U, C, blank)) return rc;
    if (!x || !Tn || !Un || !costs || !workspace || (LOGITS && !lse) || (U > 0 && !targets)) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Ctc L = carve(workspace, B, T, U);
    hipLaunchKernelGGL(ctc_gather_kernel<LOGITS>, dim3((unsigned)T, (unsigned)B), dim3(256), 0, s, x, targets, toff, Tn,
                       Un, B, T, U, C, blank, lse, L);
    if (L.Wp == 64)
        hipLaunchKernelGGL(ctc_alpha_beta_kernel<false>, dim3(2, (unsigned)B), dim3(64), 0, s, L, Tn, Un, costs, T, U);
    else
        hipLaunchKernelGGL(ctc_alpha_beta_kernel<true>, dim3(2, (unsigned)B), dim3((unsigned)L.Wp), 0, s, L, Tn, Un,
                           costs, T, U);
    return (int)hipGetLastError();
}

template <bool LOGITS>
int backward(const float *x, const float *lse, const int *Tn, const int *Un, int B, int T, int U, int C, int blank,
             const float *grad_costs, const void *workspace, float *grads, void *stream) {
    if (int rc = check_dims(B, T, U, C, blank)) return rc;
    if (!Tn || !Un || !workspace || !grads || (LOGITS && (!x || !lse))) return PIKA_EINVAL;
    const Ctc L = carve(const_cast<void *>(workspace), B, T, U);
    hipLaunchKernelGGL(ctc_grad_kernel<LOGITS>, dim3((unsigned)T, (unsigned)B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), L, x, lse, Tn, grad_costs, B, T, C, grads);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t pika_ctc_workspace_bytes(int B, int T, int U_max) {
    if (check_lattice_dims(B, T, U_max)) return 0;
    return workspace_bytes(B, T, U_max);
}

size_t pika_ctc_align_scratch_bytes(int B, int T, int U_max) {
    if (check_lattice_dims(B, T, U_max)) return 0;
    return (size_t)B * T * state_width(U_max);
}

int pika_ctc_loss_forward(const float *log_probs, const int *targets, const int *target_offsets,
                          const int *input_lengths, const int *target_lengths, int B, int T, int U_max, int C,
                          int blank, float *costs, void *workspace, void *stream) {
    return forward<false>(log_probs, targets, target_offsets, input_lengths, target_lengths, B, T, U_max, C, blank,
                          costs, nullptr, workspace, stream);
}

int pika_ctc_loss_backward(const int *input_lengths, const int *target_lengths, int B, int T, int U_max, int C,
                           int blank, const float *grad_costs, const void *workspace, float *grads, void *stream) {
    return backward<false>(nullptr, nullptr, input_lengths, target_lengths, B, T, U_max, C, blank, grad_costs,
                           workspace, grads, stream);
}

int pika_ctc_fused_forward(const float *logits, const int *targets, const int *target_offsets,
                           const int *input_lengths, const int *target_lengths, int B, int T, int U_max, int C,
                           int blank, float *costs, float *lse, void *workspace, void *stream) {
    return forward<true>(logits, targets, target_offsets, input_lengths, target_lengths, B, T, U_max, C, blank, costs,
                         lse, workspace, stream);
}

int pika_ctc_fused_backward(const float *logits, const float *lse, const int *input_lengths,
                            const int *target_lengths, int B, int T, int U_max, int C, int blank,
                            const float *grad_costs, const void *workspace, float *grad_logits, void *stream) {
    return backward<true>(logits, lse, input_lengths, target_lengths, B, T, U_max, C, blank, grad_costs, workspace,
                          grad_logits, stream);
}

int pika_ctc_align(const void *workspace, const int *input_lengths, const int *target_lengths, int B, int T, int U_max,
                   float *scores, int *frame_labels, void *scratch, void *stream) {
    if (int rc = check_lattice_dims(B, T, U_max)) return rc;
    if (!workspace || !input_lengths || !target_lengths || !scores || !frame_labels || !scratch) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Ctc L = carve(const_cast<void *>(workspace), B, T, U_max);
    unsigned char *bp = static_cast<unsigned char *>(scratch);
    if (L.Wp == 64)
        hipLaunchKernelGGL(ctc_align_kernel<false>, dim3((unsigned)B), dim3(64), 0, s, L, input_lengths, target_lengths,
                           scores, frame_labels, bp, T, U_max);
    else
        hipLaunchKernelGGL(ctc_align_kernel<true>, dim3((unsigned)B), dim3((unsigned)L.Wp), 0, s, L, input_lengths,
                           target_lengths, scores, frame_labels, bp, T, U_max);
    return (int)hipGetLastError();
}

size_t pika_ctc_nbest_align_scratch_bytes(int B, int N, int T, int U_max) {
    if (check_nbest_dims(B, N, T, U_max)) return 0;
    return (size_t)B * N * nbest_groups(T) * state_width(U_max);
}

int pika_ctc_nbest_align(const float *x, long long stride_t, long long stride_b, const float *lse,
                         const int *input_lengths, const int *tokens, const int *lengths, int B, int N, int L, int T,
                         int C, int blank, int U_max, float *full_scores, float *best_scores, int *starts, int *ends,
                         float *token_scores, void *scratch, void *stream) {
    if (L <= 0 || C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (int rc = check_nbest_dims(B, N, T, U_max)) return rc;
    if (!x || !input_lengths || !tokens || !lengths || !full_scores || !best_scores || !starts || !ends ||
        !token_scores || !scratch)
        return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Wp = state_width(U_max);
    const dim3 grid((unsigned)N, (unsigned)B), block((unsigned)Wp);
    unsigned char *bp = static_cast<unsigned char *>(scratch);
#define PIKA_NBEST_LAUNCH(MULTI, LOGITS)                                                                              \
    hipLaunchKernelGGL((ctc_nbest_align_kernel<MULTI, LOGITS>), grid, block, 0, s, x, stride_t, stride_b, lse,        \
                       input_lengths, tokens, lengths, B, N, L, T, C, blank, U_max, full_scores, best_scores, starts, \
                       ends, token_scores, bp)
    if (Wp == 64) {
        if (lse) PIKA_NBEST_LAUNCH(false, true);
        else PIKA_NBEST_LAUNCH(false, false);
    } else {
        if (lse) PIKA_NBEST_LAUNCH(true, true);
        else PIKA_NBEST_LAUNCH(true, false);
    }
#undef PIKA_NBEST_LAUNCH
    return (int)hipGetLastError();
}

size_t pika_ctc_nbest_loss_workspace_bytes(int B, int N, int T, int U_max) {
    if (check_nbest_loss_dims(B, N, T, U_max)) return 0;
    return nbest_loss_bytes(B, N, T, U_max);
}

int pika_ctc_nbest_loss_forward(const float *x, long long stride_t, long long stride_b, const float *lse,
                                const int *input_lengths, const int *tokens, const int *lengths, int B, int N, int L,
                                int T, int C, int blank, int U_max, float *full_scores, void *workspace, void *stream) {
    if (L <= 0 || C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (int rc = check_nbest_loss_dims(B, N, T, U_max)) return rc;
    if (!x || !input_lengths || !tokens || !lengths || !full_scores || !workspace) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Nbl W = carve_nbest(workspace, B, N, T, U_max);
    const dim3 grid(2, (unsigned)N, (unsigned)B), block((unsigned)W.Wp);
#define PIKA_NBEST_LAUNCH(MULTI, LOGITS)                                                                             \
    hipLaunchKernelGGL((ctc_nbest_loss_kernel<MULTI, LOGITS>), grid, block, 0, s, x, stride_t, stride_b, lse,        \
                       input_lengths, tokens, lengths, B, N, L, T, C, blank, U_max, full_scores, W)
    if (W.Wp == 64) {
        if (lse) PIKA_NBEST_LAUNCH(false, true);
        else PIKA_NBEST_LAUNCH(false, false);
    } else {
        if (lse) PIKA_NBEST_LAUNCH(true, true);
        else PIKA_NBEST_LAUNCH(true, false);
    }
#undef PIKA_NBEST_LAUNCH
    return (int)hipGetLastError();
}

int pika_ctc_nbest_loss_backward(const float *x, long long stride_t, long long stride_b, const float *lse,
                                 const int *input_lengths, int B, int N, int T, int C, int blank, int U_max,
                                 const float *grad_scores, const void *workspace, float *grads, void *stream) {
    if (C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (int rc = check_nbest_loss_dims(B, N, T, U_max)) return rc;
    if (!x || !input_lengths || !grad_scores || !workspace || !grads) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Nbl W = carve_nbest(const_cast<void *>(workspace), B, N, T, U_max);
    const dim3 grid((unsigned)T, (unsigned)B), block(256);
    if (lse)
        hipLaunchKernelGGL(ctc_nbest_grad_kernel<true>, grid, block, 0, s, W, x, stride_t, stride_b, lse, input_lengths,
                           grad_scores, B, N, T, C, grads);
    else
        hipLaunchKernelGGL(ctc_nbest_grad_kernel<false>, grid, block, 0, s, W, x, stride_t, stride_b, lse,
                           input_lengths, grad_scores, B, N, T, C, grads);
    return (int)hipGetLastError();
}

}  // extern "C"
