// pika_amd/csrc/ctc_long.hip -- long-form CTC forced alignment (include/pika_ctc.h: pika_ctc_long_align): the Viterbi path
// of one transcript per recording with the state axis TILED, so neither the 1024 states of one workgroup nor an fp32 plane
// bound it -- an hour of audio (T ~ 1e5 frames) against its whole transcript (U ~ 1e4 labels).
//
// Four kinds of launch, all in stream order, none waiting on another from inside a kernel:
//   long_rows_kernel    grid (T, B): one read of row (t, b) of x -> its maximum (clamped at -1e30).  That is m_t for
//                       log-probs and maxlogit_t for logits; either way the recurrence subtracts it from the value it
//                       gathers, so e_t(s) <= 0 and a well-aligned path stays near 0 however long the recording.
//   long_dp_kernel      one launch per block of LF = 64 frames, grid (tiles, B), 1024 threads.  A tile OWNS LW = 896 states
//                       and recomputes the LH = 2 LF = 128 states below them: a state's value after k frames depends on the
//                       2k states below it k frames earlier, so after k steps everything from local index 2k up is exact
//                       and the owned states (local index >= 128) are exact at every frame of the block.  A tile therefore
//                       needs only the full state column at the block's first frame, which lives ping-pong in scratch:
//                       block n reads column n & 1 and writes the other, so a tile never reads what a neighbour of the same
//                       launch writes.  Only owned states write back-pointers (two bits per cell, four frames of one state
//                       to a byte, as ctc_nbest_align_kernel packs them) and the column.
//   long_trace_kernel   grid B, one wave: the end rule, the score (v_end + the sum of m_t, in fp64), and the back-trace.
//                       The path comes down at most two states per frame, so the wave fetches the back-pointer window of
//                       the next 64 frames -- 16 byte rows by at most 132 states -- in one go into LDS and lane 0 walks it
//                       there: T / 64 dependent global round trips instead of T.  Writes the state of every frame.
//   long_tokens_kernel  a thread per token: two binary searches in the (monotone) per-frame path give its run, which it
//                       sums in fp32 in increasing t.
// Lengths are clamped on the device; workgroups of frame blocks beyond T_b and of tiles beyond S_b return at once, so the
// launch sequence depends on (T, U_max) alone and can be captured.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctc_numerics.h"
#include "pika_ctc.h"

namespace {

constexpr int LW = 896;       // owned states per tile          (pika_amd.ctc.LONG_ALIGN_TILE)
constexpr int LF = 64;        // frames per recurrence launch   (pika_amd.ctc.LONG_ALIGN_FRAMES)
constexpr int LH = 2 * LF;    // recomputed states below a tile
constexpr int LB = LW + LH;   // threads of a tile's workgroup
constexpr int LUNR = 8;       // frames prefetched per register batch
constexpr int WIN_ROWS = LF / 4;           // back-pointer rows (four frames each) per trace window
constexpr int WIN_WORDS = (LH + 4) / 4 + 1;  // 32-bit words per window row: states [lo & ~3, cs], cs - lo <= 2 * 64
constexpr int MAX_LONG_U = 1 << 28;
static_assert(LB == 1024 && LF % 4 == 0 && LW % 64 == 0, "tile geometry");

struct LongScratch {
    unsigned char *bp;  // [B][G][Sp] two bits per cell
    float *col;         // [2][B][Sp]
    int *path;          // [B][Tp]
    float *rowmax;      // [B][Tp]
    int *meta;          // [B][4]: feasible, end state
    int Sp, G, Tp;
};

inline int long_sp(int U) { return (int)(((2ll * U + 1 + LW - 1) / LW) * LW); }

// 0 when the size does not fit size_t
inline size_t long_bytes(int B, int T, int U) {
    const size_t Sp = (size_t)long_sp(U), G = ((size_t)T + 3) / 4, Tp = 4 * G, b = (size_t)B;
    size_t bp, n;
    if (__builtin_mul_overflow(b * G, Sp, &bp)) return 0;
    if (__builtin_add_overflow(bp, 8 * b * Sp + 8 * b * Tp + 16 * b, &n)) return 0;
    return n;
}

int check_long_dims(int B, int T, int U) {
    if (B <= 0 || T <= 0 || U < 0) return PIKA_EINVAL;
    if (U > MAX_LONG_U || B > 65535 || long_bytes(B, T, U) == 0) return PIKA_ETOOBIG;
    return PIKA_OK;
}

inline LongScratch carve_long(void *scratch, int B, int T, int U) {
    LongScratch Z;
    Z.Sp = long_sp(U);
    Z.G = (T + 3) / 4;
    Z.Tp = 4 * Z.G;
    Z.bp = static_cast<unsigned char *>(scratch);  // B G Sp bytes: a multiple of 64
    Z.col = reinterpret_cast<float *>(Z.bp + (size_t)B * Z.G * Z.Sp);
    Z.path = reinterpret_cast<int *>(Z.col + 2 * (size_t)B * Z.Sp);
    Z.rowmax = reinterpret_cast<float *>(Z.path + (size_t)B * Z.Tp);
    Z.meta = reinterpret_cast<int *>(Z.rowmax + (size_t)B * Z.Tp);
    return Z;
}

// grid (T, B), 256 threads: the maximum of row (t, b), NaN skipped, clamped at NEG
__global__ __launch_bounds__(256) void long_rows_kernel(const float *__restrict__ x, long long stride_t, long long stride_b,
                                                        const int *__restrict__ Tn_, int T, int C, LongScratch Z) {
    __shared__ float red[256];
    const int t = blockIdx.x, b = blockIdx.y, i = threadIdx.x;
    if (t >= clampi(Tn_[b], 1, T)) return;  // workgroup-uniform; never read beyond T_b
    const float *row = x + (long long)t * stride_t + (long long)b * stride_b;
    float m = NEG;
    for (int c = i; c < C; c += 256) m = fmaxf(m, row[c]);
    red[i] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (i < w) red[i] = fmaxf(red[i], red[i + w]);
        __syncthreads();
    }
    if (i == 0) Z.rowmax[(size_t)b * Z.Tp + t] = red[0];
}

// grid (tiles, B), LB threads: frames [blk LF, blk LF + LF) of tile blockIdx.x; thread i holds state tile LW - LH + i
__global__ __launch_bounds__(LB) void long_dp_kernel(const float *__restrict__ x, long long stride_t, long long stride_b,
                                                     const int *__restrict__ Tn_, const int *__restrict__ targets,
                                                     const int *__restrict__ Un_, int B, int T, int C, int blank,
                                                     int U_max, LongScratch Z, int blk) {
    __shared__ float vL[2][LB + 2];  // [.][i + 2] = v of local state i; the two slots below stay NEG
    __shared__ float shiftL[LF];
    const int b = blockIdx.y, tile = blockIdx.x, i = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max), S = 2 * Un + 1;
    const int t0 = blk * LF;
    if (t0 >= Tn || (long long)tile * LW >= S) return;  // workgroup-uniform: nothing of this recording lives here
    const int g = tile * LW - LH + i;
    const bool valid = g >= 0 && g < S, owned = i >= LH;
    bool ok = valid, skip = false;
    int cls = blank;
    if (valid && (g & 1)) {
        const int *y = targets + (size_t)b * U_max + (g >> 1);
        const int c = y[0];
        ok = c >= 0 && c < C && c != blank;  // a bad token: its state is impossible and nothing is read through it
        cls = ok ? c : blank;
        skip = g >= 3 && c != y[-1];
    }
    const float *xs = x + (long long)b * stride_b + cls;
    const size_t colB = (size_t)B * Z.Sp;
    const float *colin = Z.col + (size_t)(blk & 1) * colB + (size_t)b * Z.Sp;
    float *colout = Z.col + (size_t)((blk + 1) & 1) * colB + (size_t)b * Z.Sp;
    unsigned char *bp = Z.bp + (size_t)b * Z.G * Z.Sp;
    float v = (blk > 0 && valid) ? colin[g] : NEG;
    if (i < 2) vL[0][i] = vL[1][i] = NEG;
    if (i < LF) shiftL[i] = Z.rowmax[(size_t)b * Z.Tp + min(t0 + i, Tn - 1)];
    __syncthreads();

    float cur[LUNR], nx[LUNR];
    auto load = [&](float *dst, int j0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < LUNR; ++j)
            dst[j] = ok ? fmaxf(xs[(long long)min(t0 + j0 + j, Tn - 1) * stride_t], NEG) : NEG;
    };
    unsigned int pk = 0;
    load(cur, 0);
    for (int j0 = 0; j0 < LF && t0 + j0 < Tn; j0 += LUNR) {  // workgroup-uniform
        load(nx, min(j0 + LUNR, LF - LUNR));
#pragma unroll
        for (int j = 0; j < LUNR; ++j) {
            const int t = t0 + j0 + j;
            if (t < Tn) {  // workgroup-uniform
                const int buf = j & 1;
                vL[buf][i + 2] = v;
                __syncthreads();
                const float p1 = vL[buf][i + 1], p2 = vL[buf][i];
                const float e = ok ? cur[j] - shiftL[j0 + j] : NEG;
                float top = v;
                unsigned int k = 0;
                if (g >= 1 && p1 > top) { top = p1; k = 1; }
                if (skip && p2 > top) { top = p2; k = 2; }
                if (t == 0) {
                    v = (valid && g <= 1) ? e : NEG;
                    k = 0;
                } else {
                    v = valid ? e + top : NEG;
                }
                pk |= k << (2 * (j & 3));  // t0 + j0 is a multiple of 4: j & 3 == t & 3
                if ((j & 3) == 3 || t == Tn - 1) {
                    if (owned) bp[(size_t)(t >> 2) * Z.Sp + g] = (unsigned char)pk;
                    pk = 0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LUNR; ++j) cur[j] = nx[j];
    }
    if (owned) colout[g] = v;
}

// grid B, one wave: end rule, score, back-trace through LDS windows
__global__ __launch_bounds__(64) void long_trace_kernel(const float *__restrict__ lse, const int *__restrict__ Tn_,
                                                        const int *__restrict__ Un_, int B, int T, int U_max,
                                                        float *__restrict__ scores, LongScratch Z) {
    __shared__ double red[64];
    __shared__ unsigned int win[WIN_ROWS * WIN_WORDS];
    __shared__ int pathL[LF];
    __shared__ int csL;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max), S = 2 * Un + 1;
    const int nblk = (Tn + LF - 1) / LF;  // the column the last frame block of this recording wrote
    const float *col = Z.col + (size_t)(nblk & 1) * B * Z.Sp + (size_t)b * Z.Sp;
    const float f0 = col[S - 1], f1 = S >= 2 ? col[S - 2] : NEG;
    const bool second = S >= 2 && f1 > f0;  // a tie ends in the final blank
    const float vend = second ? f1 : f0;
    const bool feasible = vend > -1.0e29f;
    double acc = 0.0;
    for (int t = lane; t < Tn; t += 64) {
        const float r = Z.rowmax[(size_t)b * Z.Tp + t];
        acc += (double)(lse ? fmaxf(r - lse[(size_t)t * B + b], NEG) : r);
    }
    red[lane] = acc;
    __syncthreads();
    if (lane == 0) {
        double total = 0.0;
        for (int l = 0; l < 64; ++l) total += red[l];
        scores[b] = feasible ? (float)((double)vend + total) : -__builtin_inff();
        Z.meta[4 * b] = feasible;
        Z.meta[4 * b + 1] = second ? S - 2 : S - 1;
        csL = second ? S - 2 : S - 1;
    }
    if (!feasible) return;  // workgroup-uniform; the token launch does not read the path of such a recording
    const unsigned char *bp = Z.bp + (size_t)b * Z.G * Z.Sp;
    for (int thi = Tn - 1; thi >= 0;) {  // workgroup-uniform
        const int ghi = thi >> 2, glo = ghi & ~(WIN_ROWS - 1), tlo = 4 * glo, rows = ghi - glo + 1;
        __syncthreads();  // csL is written; the previous window is walked and its frames are stored
        const int cs = csL;
        const int lo = max(cs - LH, 0) & ~3, nw = ((cs - lo) >> 2) + 1;  // nw <= WIN_WORDS; lo + 4 nw <= Sp
        for (int idx = lane; idx < rows * nw; idx += 64) {
            const int r = idx / nw, w = idx - r * nw;
            win[r * WIN_WORDS + w] = *reinterpret_cast<const unsigned int *>(bp + (size_t)(glo + r) * Z.Sp + lo + 4 * w);
        }
        __syncthreads();
        if (lane == 0) {
            const unsigned char *wb = reinterpret_cast<const unsigned char *>(win);
            int c = cs;
            for (int t = thi; t >= tlo; --t) {
                pathL[t - tlo] = c;
                const int k = (wb[((t >> 2) - glo) * (4 * WIN_WORDS) + (c - lo)] >> (2 * (t & 3))) & 3;
                c = max(c - k, lo);  // k <= 2 per frame keeps c inside the window; the clamp guards the LDS read
            }
            csL = c;
        }
        __syncthreads();
        if (lane <= thi - tlo) Z.path[(size_t)b * Z.Tp + tlo + lane] = pathL[lane];
        thi = tlo - 1;
    }
}

// grid (ceil(U_max / 256), B): token j's run by two binary searches in the monotone path, its score in time order
__global__ __launch_bounds__(256) void long_tokens_kernel(const float *__restrict__ x, long long stride_t,
                                                          long long stride_b, const float *__restrict__ lse,
                                                          const int *__restrict__ Tn_, const int *__restrict__ targets,
                                                          const int *__restrict__ Un_, int B, int T, int C, int U_max,
                                                          int *__restrict__ starts, int *__restrict__ ends,
                                                          float *__restrict__ tscores, LongScratch Z) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= U_max) return;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U_max);
    const size_t o = (size_t)b * U_max + j;
    if (j >= Un || !Z.meta[4 * b]) {
        starts[o] = -1;
        ends[o] = -1;
        tscores[o] = -__builtin_inff();
        return;
    }
    const int *p = Z.path + (size_t)b * Z.Tp;
    auto first_at_least = [&](int s) __attribute__((always_inline)) {  // the first t in [0, Tn] with p[t] >= s
        int lo = 0, hi = Tn;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p[mid] >= s) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    };
    const int s = 2 * j + 1;  // a label state: on the path of every feasible transcript
    const int ta = clampi(first_at_least(s), 0, Tn - 1), tb = clampi(first_at_least(s + 1) - 1, ta, Tn - 1);
    const int c = clampi(targets[o], 0, C - 1);  // in [0,C) already: the recording is feasible
    const float *xs = x + (long long)b * stride_b + c;
    float acc = 0.0f;
    for (int t = ta; t <= tb; ++t) {
        float e = xs[(long long)t * stride_t];
        if (lse) e -= lse[(size_t)t * B + b];
        acc += fmaxf(e, NEG);
    }
    starts[o] = ta;
    ends[o] = tb;
    tscores[o] = acc;
}

}  // namespace

extern "C" {

size_t pika_ctc_long_align_scratch_bytes(int B, int T, int U_max) {
    if (check_long_dims(B, T, U_max)) return 0;
    return long_bytes(B, T, U_max);
}

int pika_ctc_long_align(const float *x, long long stride_t, long long stride_b, const float *lse,
                        const int *input_lengths, const int *targets, const int *target_lengths, int B, int T, int C,
                        int blank, int U_max, float *scores, int *starts, int *ends, float *token_scores,
                        void *scratch, void *stream) {
    if (B <= 0 || T <= 0 || U_max < 0 || C <= 0 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (int rc = check_long_dims(B, T, U_max)) return rc;
    if (!x || !input_lengths || !target_lengths || !scores || !starts || !ends || !token_scores || !scratch ||
        (U_max > 0 && !targets))
        return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LongScratch Z = carve_long(scratch, B, T, U_max);
    hipLaunchKernelGGL(long_rows_kernel, dim3((unsigned)T, (unsigned)B), dim3(256), 0, s, x, stride_t, stride_b,
                       input_lengths, T, C, Z);
    const dim3 grid((unsigned)(Z.Sp / LW), (unsigned)B);
    for (int blk = 0; blk < (T + LF - 1) / LF; ++blk)
        hipLaunchKernelGGL(long_dp_kernel, grid, dim3(LB), 0, s, x, stride_t, stride_b, input_lengths, targets,
                           target_lengths, B, T, C, blank, U_max, Z, blk);
    hipLaunchKernelGGL(long_trace_kernel, dim3((unsigned)B), dim3(64), 0, s, lse, input_lengths, target_lengths, B, T,
                       U_max, scores, Z);
    if (U_max > 0)
        hipLaunchKernelGGL(long_tokens_kernel, dim3((unsigned)((U_max + 255) / 256), (unsigned)B), dim3(256), 0, s, x,
                           stride_t, stride_b, lse, input_lengths, targets, target_lengths, B, T, C, U_max, starts, ends,
                           token_scores, Z);
    return (int)hipGetLastError();
}

}  // extern "C"
