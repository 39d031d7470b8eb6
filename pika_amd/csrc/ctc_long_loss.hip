// pika_amd/csrc/ctc_long_loss.hip -- long-form CTC loss and gradient (include/pika_ctc.h: pika_ctc_long_loss_*): the full
// sum over alignments with the state axis TILED as in ctc_long.hip, so a transcript is not bound by the 1024 states of one
// workgroup, and both planes kept for a gradient writer that has no limit on the state axis either.
//
// Launches, all in stream order, none waiting on another from inside a kernel:
//   lloss_rows_kernel    grid (T, B): one read of row (t, b) of x -> its maximum r_t (clamped at -1e30).  The recurrences
//                        run on e_t(s) = fl32(x_t(l'_s) - r_t) <= 0; what that takes out, M_t = r_t (log-probs) or
//                        r_t - lse_t (logits), is summed in fp64 into the offsets.
//   lloss_sort_kernel    grid (ceil(U_max / 256), B), once per call: the labels of a transcript in the stable order
//                        (class, position), by counting ranks -- U^2 comparisons against the T U exp/log of the
//                        recurrences, any C, no table of classes.  The gradient sums the states of a class from it.
//   lloss_dp_kernel      one launch per block of QF = 64 frames, grid (tiles, B, 2): z = 0 is alpha on frame block k, z = 1
//                        beta on frame block nblk-1-k.  A tile OWNS QW = 896 states and recomputes QH = 2 QF = 128 more --
//                        below them for alpha, above them for beta: a state's value after k frames depends on the 2k
//                        states on that side k frames before, so the owned states are exact at every frame of the block.
//                        A tile needs only the state column at the block's edge, kept ping-pong in the workspace: launch k
//                        reads column k & 1 and writes the other, so no tile reads what a neighbour of the same launch
//                        writes.  Owned states store every frame's value into the plane.
//                        Numerics: log-space fp32, -1e30 "impossible".  At the start of a block every tile subtracts the
//                        SAME amount R, the largest of the per-tile maxima the launch before left (max is exact and order-
//                        free: all tiles agree to the bit), and tile 0 moves R and the M_t into the fp64 offset of every
//                        frame: true alpha_t(s) = plane + off_a[t].
//   lloss_finish_kernel  a thread per utterance: ll = off_a[T_b-1] + logsumexp(alpha(S-1), alpha(S-2)) in fp64; the cost.
//   lloss_grad_kernel    grid (T, B): writes row (t, b) of the dense gradient once (zeros, or gc * softmax), then the class
//                        entries: blank = the even states, thread-strided partial sums and a fixed tree; the labels in
//                        sorted order, a contiguous chunk per thread, the pieces of a class that spans chunks joined in
//                        chunk order by the thread that holds its first label.  No atomics; the order of every sum is a
//                        function of (t, T_b, U_b) alone.
// Lengths are clamped on the device; workgroups of frame blocks beyond T_b and of tiles beyond S_b return at once, so the
// launch sequence depends on (T, U_max) alone and can be captured.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctc_numerics.h"
#include "pika_ctc.h"

namespace {

constexpr int QW = 896;       // owned states per tile          (pika_amd.ctc.LONG_LOSS_TILE)
constexpr int QF = 64;        // frames per recurrence launch   (pika_amd.ctc.LONG_LOSS_FRAMES)
constexpr int QH = 2 * QF;    // recomputed states beside a tile
constexpr int QB = QW + QH;   // threads of a tile's workgroup
constexpr int QUNR = 8;       // frames prefetched per register batch
constexpr int QWAVES = QB / 64;
constexpr int MAX_LOSS_U = 1 << 28;
static_assert(QB == 1024 && QF % QUNR == 0 && QW % 64 == 0, "tile geometry");

struct LongLoss {
    float *alpha;   // [B][T][Sp] alpha minus off_a[b][t], the frame's own emission included
    float *beta;    // [B][T][Sp] beta  minus off_b[b][t], likewise
    double *off_a;  // [B][T]
    double *off_b;  // [B][T]
    double *ll;     // [B] log-likelihood (<= -0.5e30: infeasible)
    float *col;     // [2][2][B][Sp] direction, parity: the state column at a block's edge
    float *tmax;    // [2][2][B][NT] direction, parity: the largest owned value of every tile of that column
    float *rowmax;  // [B][T]
    int *sidx;      // [B][U_max] label positions in (class, position) order
    int *scls;      // [B][U_max] their classes
    int Sp, NT;
};

inline int loss_sp(int U) { return (int)(((2ll * U + 1 + QW - 1) / QW) * QW); }

// 0 when the size does not fit size_t
inline size_t loss_bytes(int B, int T, int U) {
    const size_t Sp = (size_t)loss_sp(U), b = (size_t)B, t = (size_t)T;
    size_t n;
    if (__builtin_mul_overflow(b * t, Sp, &n) || n > SIZE_MAX / 64) return 0;  // what follows the planes is below 56 n
    return 8 * n + 16 * b * t + 8 * b + 16 * b * Sp + 16 * b * (Sp / QW) + 4 * b * t + 8 * b * (size_t)U;
}

int check_loss_dims(int B, int T, int U) {
    if (B <= 0 || T <= 0 || U < 0) return PIKA_EINVAL;
    if (U > MAX_LOSS_U || B > 65535 || loss_bytes(B, T, U) == 0) return PIKA_ETOOBIG;
    return PIKA_OK;
}

inline LongLoss carve_loss(void *ws, int B, int T, int U) {
    LongLoss Z;
    Z.Sp = loss_sp(U);
    Z.NT = Z.Sp / QW;
    const size_t n = (size_t)B * T * Z.Sp, bt = (size_t)B * T;  // n is even: what follows stays 8-byte aligned
    Z.alpha = static_cast<float *>(ws);
    Z.beta = Z.alpha + n;
    Z.off_a = reinterpret_cast<double *>(Z.beta + n);
    Z.off_b = Z.off_a + bt;
    Z.ll = Z.off_b + bt;
    Z.col = reinterpret_cast<float *>(Z.ll + B);
    Z.tmax = Z.col + 4 * (size_t)B * Z.Sp;
    Z.rowmax = Z.tmax + 4 * (size_t)B * Z.NT;
    Z.sidx = reinterpret_cast<int *>(Z.rowmax + bt);
    Z.scls = Z.sidx + (size_t)B * U;
    return Z;
}

// log(exp(x)+exp(y)+exp(z)) on the transcendental pipe; all three "log zero": -1e30 + log 3 == -1e30
__device__ inline float lse3(float x, float y, float z) {
    const float m = fmaxf(fmaxf(x, y), z);
    const float e = __builtin_amdgcn_exp2f((x - m) * LOG2E) + __builtin_amdgcn_exp2f((y - m) * LOG2E) +
                    __builtin_amdgcn_exp2f((z - m) * LOG2E);
    return m + LN2 * __builtin_amdgcn_logf(e);
}

// the largest v of the workgroup, in every thread; red holds one float per wave and is free again after the call
__device__ inline float block_max(float v, float *red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = red[0];
    for (int w = 1; w < nw; ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    return m;
}

// grid (T, B), 256 threads: the maximum of row (t, b), NaN skipped, clamped at NEG
__global__ __launch_bounds__(256) void lloss_rows_kernel(const float *__restrict__ x, long long stride_t,
                                                         long long stride_b, const int *__restrict__ Tn_, int T, int C,
                                                         LongLoss Z) {
    __shared__ float red[4];
    const int t = blockIdx.x, b = blockIdx.y, i = threadIdx.x;
    if (t >= clampi(Tn_[b], 1, T)) return;  // workgroup-uniform; never read beyond T_b
    const float *row = x + (long long)t * stride_t + (long long)b * stride_b;
    float m = NEG;
    if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {  // workgroup-uniform
        for (int c = i; c < C / 4; c += 256) {
            const v4f v = reinterpret_cast<const v4f *>(row)[c];
            m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        }
    } else {
        for (int c = i; c < C; c += 256) m = fmaxf(m, row[c]);
    }
    m = block_max(m, red);
    if (i == 0) Z.rowmax[(size_t)b * T + t] = m;
}

// grid (ceil(U_max / 256), B), 256 threads: label u goes to position #{v : (y_v, v) < (y_u, u)} of the sorted rows
__global__ __launch_bounds__(256) void lloss_sort_kernel(const int *__restrict__ targets, const int *__restrict__ Un_,
                                                         int U_max, LongLoss Z) {
    __shared__ int yL[256];
    const int b = blockIdx.y, i = threadIdx.x, u = blockIdx.x * 256 + i;
    const int Un = clampi(Un_[b], 0, U_max);
    if ((int)blockIdx.x * 256 >= Un) return;  // workgroup-uniform
    const int *y = targets + (size_t)b * U_max;
    const bool live = u < Un;
    const int c = live ? y[u] : 0;
    int rank = 0;
    for (int v0 = 0; v0 < Un; v0 += 256) {  // workgroup-uniform
        __syncthreads();
        if (v0 + i < Un) yL[i] = y[v0 + i];
        __syncthreads();
        const int n = min(256, Un - v0);
        for (int k = 0; k < n; ++k) {
            const int cv = yL[k];
            rank += (cv < c || (cv == c && v0 + k < u)) ? 1 : 0;
        }
    }
    if (live) {  // rank counts labels other than u below U_b: rank <= U_b - 1
        Z.sidx[(size_t)b * U_max + rank] = u;
        Z.scls[(size_t)b * U_max + rank] = c;
    }
}

// grid (tiles, B, 2), QB threads.  z = 0: alpha over frames [blk QF, blk QF + QF) upwards, blk = step, thread i holds state
// tile QW - QH + i; z = 1: beta over the frames of block blk = nblk - 1 - step below T_b, downwards, thread i holds state
// tile QW + i.  The first block of a direction starts from the virtual row ([0, NEG, ...] below frame 0, [..., NEG, 0]
// above frame T_b - 1), which makes its first frame an ordinary step.
__global__ __launch_bounds__(QB) void lloss_dp_kernel(const float *__restrict__ x, long long stride_t, long long stride_b,
                                                      const float *__restrict__ lse, const int *__restrict__ Tn_,
                                                      const int *__restrict__ targets, const int *__restrict__ Un_,
                                                      int B, int T, int C, int blank, int U_max, LongLoss Z, int step,
                                                      int nblk) {
    __shared__ float vL[2][QB + 4];  // [.][i + 2] = v of local state i; two slots on either side stay NEG
    __shared__ float shiftL[QF];
    __shared__ double mL[QF];
    __shared__ float red[QWAVES];
    const int b = blockIdx.y, tile = blockIdx.x, i = threadIdx.x;
    const bool fwd = blockIdx.z == 0;
    const int blk = fwd ? step : nblk - 1 - step;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max), S = 2 * Un + 1;
    const int t0 = blk * QF;
    if (t0 >= Tn || (long long)tile * QW >= S) return;  // workgroup-uniform: nothing of this utterance lives here
    const int tEnd = min(t0 + QF, Tn), n = tEnd - t0;
    const bool first = fwd ? blk == 0 : tEnd == Tn;
    const int g = fwd ? tile * QW - QH + i : tile * QW + i;
    const bool valid = g >= 0 && g < S, owned = fwd ? i >= QH : i < QW;
    bool ok = valid, skip = false;
    int cls = blank;
    if (valid && (g & 1)) {
        const int *y = targets + (size_t)b * U_max + (g >> 1);
        const int c = y[0];
        ok = c >= 0 && c < C;  // a bad label: its state is impossible and nothing is read through it
        cls = ok ? c : blank;
        // the transition over two states INTO this state (alpha) / OUT of it (beta), as ctc_gather_kernel classifies it
        if (fwd) skip = g >= 3 && c != blank && c != y[-1];
        else skip = g + 2 < S && y[1] != blank && y[1] != c;
    }
    const float *xs = x + (long long)b * stride_b + cls;
    const int dir = fwd ? 0 : 1, par = step & 1;
    const size_t colB = (size_t)B * Z.Sp, tmB = (size_t)B * Z.NT;
    const float *colin = Z.col + (size_t)(2 * dir + par) * colB + (size_t)b * Z.Sp;
    float *colout = Z.col + (size_t)(2 * dir + (par ^ 1)) * colB + (size_t)b * Z.Sp;
    const float *tmin = Z.tmax + (size_t)(2 * dir + par) * tmB + (size_t)b * Z.NT;
    float *tmout = Z.tmax + (size_t)(2 * dir + (par ^ 1)) * tmB + (size_t)b * Z.NT;

    float R = 0.0f;  // what this block takes out of every state: the same value in every tile
    if (!first) {
        const int nt = (S + QW - 1) / QW;
        float m = NEG;
        for (int k = i; k < nt; k += QB) m = fmaxf(m, tmin[k]);
        m = block_max(m, red);
        R = m > NEG_HALF ? m : 0.0f;
    }
    float v;
    if (first) {
        v = (g == (fwd ? 0 : S - 1)) ? 0.0f : NEG;
    } else {
        v = valid ? colin[g] : NEG;
        v = v > NEG_HALF ? v - R : NEG;
    }
    if (i < 2) vL[0][i] = vL[1][i] = vL[0][QB + 2 + i] = vL[1][QB + 2 + i] = NEG;
    if (i < QF) {
        const int t = min(t0 + i, Tn - 1);
        const float r = Z.rowmax[(size_t)b * T + t];
        shiftL[i] = r;
        mL[i] = lse ? (double)r - (double)lse[(size_t)t * B + b] : (double)r;
    }
    __syncthreads();
    if (tile == 0 && i == 0) {  // the offsets of this block's frames, in the order the sweep visits them
        double *offs = (fwd ? Z.off_a : Z.off_b) + (size_t)b * T;
        double off = first ? 0.0 : offs[fwd ? t0 - 1 : tEnd];
        off += (double)R;
        for (int j = 0; j < n; ++j) {
            const int t = fwd ? t0 + j : tEnd - 1 - j;
            off += mL[t - t0];
            offs[t] = off;
        }
    }

    const int dn = fwd ? -1 : 1;
    const size_t pbase = (size_t)b * T * Z.Sp + (size_t)(valid ? g : 0);
    float *plane = (fwd ? Z.alpha : Z.beta) + pbase;
    auto frame = [&](int j) __attribute__((always_inline)) { return fwd ? t0 + j : tEnd - 1 - j; };
    float cur[QUNR], nx[QUNR];
    auto load = [&](float *dst, int j0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < QUNR; ++j)
            dst[j] = ok ? fmaxf(xs[(long long)frame(min(j0 + j, n - 1)) * stride_t], NEG) : NEG;
    };
    load(cur, 0);
    for (int j0 = 0; j0 < n; j0 += QUNR) {  // workgroup-uniform
        load(nx, j0 + QUNR);
#pragma unroll
        for (int j = 0; j < QUNR; ++j) {
            if (j0 + j < n) {  // workgroup-uniform
                const int buf = j & 1, t = frame(j0 + j);
                vL[buf][i + 2] = v;
                __syncthreads();
                const float q1 = vL[buf][i + 2 + dn], q2 = vL[buf][i + 2 + 2 * dn];
                const float e = ok ? cur[j] - shiftL[t - t0] : NEG;
                const float an = e + lse3(v, q1, skip ? q2 : NEG);
                v = valid ? fmaxf(an, NEG) : NEG;
                if (owned && valid) plane[(size_t)t * Z.Sp] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < QUNR; ++j) cur[j] = nx[j];
    }
    if (owned && valid) colout[g] = v;
    const float m = block_max((owned && valid) ? v : NEG, red);
    if (i == 0) tmout[tile] = m;
}

// a thread per utterance: ll in fp64 from the last column, S-1 and S-2 (state 0 alone at U = 0)
__global__ __launch_bounds__(64) void lloss_finish_kernel(const int *__restrict__ Tn_, const int *__restrict__ Un_, int B,
                                                          int T, int U_max, float *__restrict__ costs, LongLoss Z) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max), S = 2 * Un + 1;
    const float *a = Z.alpha + ((size_t)b * T + (Tn - 1)) * Z.Sp;
    const float f0 = a[S - 1], f1 = S >= 2 ? a[S - 2] : NEG, m = fmaxf(f0, f1);
    if (m > NEG_HALF) {
        const double ll = Z.off_a[(size_t)b * T + Tn - 1] + (double)m +
                          log(exp((double)(f0 - m)) + exp((double)(f1 - m)));
        Z.ll[b] = ll;
        costs[b] = (float)(-ll);
    } else {  // no path reaches the end: infeasible
        Z.ll[b] = (double)NEG;
        costs[b] = __builtin_inff();
    }
}

// grid (T, B), 256 threads.  LOGITS: d/d logits = gc (softmax - occ); else d/d log_probs = -gc occ, with
// occ(c) = sum_{s : l'_s = c} exp(alpha + beta - value - ll), the exponent assembled in fp64 from planes and offsets.
template <bool LOGITS>
__global__ __launch_bounds__(256) void lloss_grad_kernel(LongLoss Z, const float *__restrict__ x, long long stride_t,
                                                         long long stride_b, const float *__restrict__ lse,
                                                         const int *__restrict__ Tn_, const int *__restrict__ Un_,
                                                         const float *__restrict__ grad_costs, int B, int T, int C,
                                                         int blank, int U_max, float *__restrict__ g) {
    __shared__ float sumL[256], headL[256];
    __shared__ int stopL[256];
    __shared__ float oddBlank;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max), S = 2 * Un + 1;
    const double ll = Z.ll[b];
    const bool live = t < Tn && ll > (double)NEG_HALF;  // workgroup-uniform; rows t >= T_b of x are never read
    const float gc = grad_costs ? grad_costs[b] : 1.0f;
    float *out = g + ((size_t)t * B + b) * C;
    const float *in = x + (long long)t * stride_t + (long long)b * stride_b;
    const float l = (LOGITS && live) ? lse[(size_t)t * B + b] : 0.0f;
    // the whole row once: zeros, or gc * softmax
    auto fill = [&](float v) __attribute__((always_inline)) { return (LOGITS && live) ? gc * expf(v - l) : 0.0f; };
    if (C % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
        (!(LOGITS && live) || (reinterpret_cast<uintptr_t>(in) & 15) == 0)) {
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
    const float rm = Z.rowmax[(size_t)b * T + t];
    // alpha + beta - value - ll = (plane_a + plane_b - e) + (off_a + off_b - M_t - ll), value = e + M_t
    const double k = Z.off_a[(size_t)b * T + t] + Z.off_b[(size_t)b * T + t] - ((double)rm - (double)l) - ll;
    const float *ap = Z.alpha + ((size_t)b * T + t) * Z.Sp, *bp = Z.beta + ((size_t)b * T + t) * Z.Sp;
    // the states both sweeps can reach at this frame: s <= 2t + 1 from the start, S - 1 - s <= 2 (T_b - 1 - t) + 1 to the end
    const int lo = (int)max(0ll, (long long)S - 2ll * (Tn - t)), hi = (int)min((long long)S - 1, 2ll * t + 1);
    auto occ = [&](int s, int c) __attribute__((always_inline)) {
        const float e = fmaxf(in[c], NEG) - rm;
        const double arg = k + ((double)ap[s] + (double)bp[s] - (double)e);
        return expf((float)fmax(arg, -1.0e30));
    };
    // blank: the even states, a thread's in increasing order, then a fixed tree
    float part = 0.0f;
    for (long long s = ((lo + 1) & ~1) + 2ll * tid; s <= hi; s += 512) part += occ((int)s, blank);
    sumL[tid] = part;
    if (tid == 0) oddBlank = 0.0f;
    __syncthreads();  // also orders the row's fill before the entries stored below
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) sumL[tid] += sumL[tid + h];
        __syncthreads();
    }
    // the labels in (class, position) order, a contiguous chunk per thread
    const int *sidx = Z.sidx + (size_t)b * U_max, *scls = Z.scls + (size_t)b * U_max;
    auto emit = [&](int c, float o) __attribute__((always_inline)) {
        if (c == blank) oddBlank = o;  // a label equal to blank: one class, one writer; joins the even states below
        else if ((unsigned)c < (unsigned)C) out[c] = LOGITS ? gc * (expf(in[c] - l) - o) : 0.0f - gc * o;
    };
    const int per = (Un + 255) / 256, j0 = min(tid * per, Un), j1 = min(j0 + per, Un);
    float acc = 0.0f, head = 0.0f;
    int curc = -1;
    bool started = false;
    for (int j = j0; j < j1; ++j) {
        const int c = scls[j], s = 2 * sidx[j] + 1;
        if (j == 0 || scls[j - 1] != c) {  // the first label of class c
            if (started) emit(curc, acc);
            else head = acc;
            started = true;
            acc = 0.0f;
            curc = c;
        }
        if (s >= lo && s <= hi && (unsigned)c < (unsigned)C) acc += occ(s, c);
    }
    if (!started) head = acc;
    headL[tid] = head;
    stopL[tid] = started || j0 >= Un;  // the class that runs into this chunk ends in it
    __syncthreads();
    if (started) {  // the class still open at the end of the chunk: its pieces in chunk order
        for (int q = tid + 1; q < 256; ++q) {
            acc += headL[q];
            if (stopL[q]) break;
        }
        emit(curc, acc);
    }
    __syncthreads();
    if (tid == 0) {
        const float o = sumL[0] + oddBlank;
        out[blank] = LOGITS ? gc * (expf(in[blank] - l) - o) : 0.0f - gc * o;
    }
}

}  // namespace

extern "C" {

size_t pika_ctc_long_loss_workspace_bytes(int B, int T, int U_max) {
    if (check_loss_dims(B, T, U_max)) return 0;
    return loss_bytes(B, T, U_max);
}

int pika_ctc_long_loss_forward(const float *x, long long stride_t, long long stride_b, const float *lse,
                               const int *input_lengths, const int *targets, const int *target_lengths, int B, int T,
                               int C, int blank, int U_max, float *costs, void *workspace, void *stream) {
    if (B <= 0 || T <= 0 || U_max < 0 || C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (int rc = check_loss_dims(B, T, U_max)) return rc;
    if (!x || !input_lengths || !target_lengths || !costs || !workspace || (U_max > 0 && !targets)) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LongLoss Z = carve_loss(workspace, B, T, U_max);
    hipLaunchKernelGGL(lloss_rows_kernel, dim3((unsigned)T, (unsigned)B), dim3(256), 0, s, x, stride_t, stride_b,
                       input_lengths, T, C, Z);
    if (U_max > 0)
        hipLaunchKernelGGL(lloss_sort_kernel, dim3((unsigned)((U_max + 255) / 256), (unsigned)B), dim3(256), 0, s,
                           targets, target_lengths, U_max, Z);
    const int nblk = (T + QF - 1) / QF;
    const dim3 grid((unsigned)Z.NT, (unsigned)B, 2);
    for (int step = 0; step < nblk; ++step)
        hipLaunchKernelGGL(lloss_dp_kernel, grid, dim3(QB), 0, s, x, stride_t, stride_b, lse, input_lengths, targets,
                           target_lengths, B, T, C, blank, U_max, Z, step, nblk);
    hipLaunchKernelGGL(lloss_finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, input_lengths,
                       target_lengths, B, T, U_max, costs, Z);
    return (int)hipGetLastError();
}

int pika_ctc_long_loss_backward(const float *x, long long stride_t, long long stride_b, const float *lse,
                                const int *input_lengths, const int *target_lengths, int B, int T, int C, int blank,
                                int U_max, const float *grad_costs, const void *workspace, float *grads, void *stream) {
    if (B <= 0 || T <= 0 || U_max < 0 || C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (int rc = check_loss_dims(B, T, U_max)) return rc;
    if (!x || !input_lengths || !target_lengths || !workspace || !grads) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LongLoss Z = carve_loss(const_cast<void *>(workspace), B, T, U_max);
    const dim3 grid((unsigned)T, (unsigned)B), block(256);
    if (lse)
        hipLaunchKernelGGL(lloss_grad_kernel<true>, grid, block, 0, s, Z, x, stride_t, stride_b, lse, input_lengths,
                           target_lengths, grad_costs, B, T, C, blank, U_max, grads);
    else
        hipLaunchKernelGGL(lloss_grad_kernel<false>, grid, block, 0, s, Z, x, stride_t, stride_b, lse, input_lengths,
                           target_lengths, grad_costs, B, T, C, blank, U_max, grads);
    return (int)hipGetLastError();
}

}  // extern "C"
