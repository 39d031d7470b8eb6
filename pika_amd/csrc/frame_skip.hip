// pika_amd/csrc/frame_skip.hip -- CTC-guided frame skipping for gfx950 (MI355X), hand-written HIP
// (include/pika_frame_skip.h; DESIGN.md section 3, "CTC-guided frame skipping").
//
//   rows  : from logits, one workgroup per (b, t) row with t < L: a single read of the C classes with an online max / sum
//           per thread (a thread takes the groups of four classes tid, tid + 256, ... whichever way they are loaded) and
//           a fixed tree over the 256 partials; blank_lp = (logit[blank] - max) - log(sum), so the log-sum-exp is never
//           rounded on its own.  From log-probs, a strided gather of the blank's column.  Cells t >= L get 0.
//   plan  : one workgroup per utterance, the frames' keys in LDS (0: kept as it stands; otherwise the order-preserving
//           integer image of the dropped frame's blank_lp).  The min_frames top-up finds the r-th smallest key by building
//           it bit by bit from exact counts, then the frame index that cuts the ties at it the same way: integers only,
//           so the choice is a function of the input.  The keep flags are compacted by ballot / popcount with a carry
//           across the waves and across the chunks of 256 frames.
//   apply : one workgroup per output row: the row index[b, j] of x, or zeros; 16-byte accesses where everything is
//           16-byte aligned, element-sized accesses otherwise.  Forward (frame_index) and backward (position) alike.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pika_frame_skip.h"

namespace {

constexpr int ROW_THREADS = 256;
constexpr int PLAN_THREADS = 256;
constexpr int APPLY_THREADS = 128;

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// order-preserving integer image of a non-NaN float (-0.0 counts as +0.0); never 0
__device__ inline unsigned fkey(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---------------------------------------------------------------------------------------------
// rows from logits.  grid = B * T, block = 256.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void fskip_rows_logits_kernel(const float *__restrict__ x, long long sb,
                                                                        long long st, const int *__restrict__ len,
                                                                        int T, int C, int blank,
                                                                        float *__restrict__ blank_lp) {
    __shared__ float rm[ROW_THREADS], rs[ROW_THREADS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / T, t = blockIdx.x - b * T;
    if (t >= clampi(len[b], 0, T)) {  // workgroup-uniform; the row is never read
        if (tid == 0) blank_lp[blockIdx.x] = 0.0f;
        return;
    }
    const float *row = x + (long long)b * sb + (long long)t * st;
    const float ninf = -INFINITY;
    float m = ninf, s = 0.0f;
    auto take = [&](float v) __attribute__((always_inline)) {
        if (v > m) {
            s = s * expf(m - v) + 1.0f;
            m = v;
        } else if (!(v == ninf)) {  // (a NaN lands here and makes the sum a NaN)
            s += expf(v - m);
        }
    };
    const bool vec = C % 4 == 0 && (reinterpret_cast<uintptr_t>(row) & 15) == 0;  // workgroup-uniform
    for (int i = tid; i < (C + 3) / 4; i += ROW_THREADS) {
        if (vec) {
            const float4 v = reinterpret_cast<const float4 *>(row)[i];
            take(v.x); take(v.y); take(v.z); take(v.w);
        } else {
            for (int k = 4 * i; k < min(4 * i + 4, C); ++k) take(row[k]);
        }
    }
    rm[tid] = m;
    rs[tid] = s;
    __syncthreads();
    for (int h = ROW_THREADS / 2; h > 0; h >>= 1) {  // fixed tree: the same value on every run
        if (tid < h) {
            const float m0 = rm[tid], m1 = rm[tid + h], mn = fmaxf(m0, m1);
            rs[tid] = mn == ninf ? rs[tid] + rs[tid + h] : rs[tid] * expf(m0 - mn) + rs[tid + h] * expf(m1 - mn);
            rm[tid] = mn;
        }
        __syncthreads();
    }
    if (tid == 0) blank_lp[blockIdx.x] = (row[blank] - rm[0]) - logf(rs[0]);
}

// ---------------------------------------------------------------------------------------------
// rows from log-probs: the blank's column.  grid = ceil(B * T / 256), block = 256.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_THREADS) void fskip_rows_gather_kernel(const float *__restrict__ x, long long sb,
                                                                        long long st, const int *__restrict__ len,
                                                                        int B, int T, int blank,
                                                                        float *__restrict__ blank_lp) {
    const long long r = (long long)blockIdx.x * ROW_THREADS + threadIdx.x;
    if (r >= (long long)B * T) return;
    const int b = (int)(r / T), t = (int)(r - (long long)b * T);
    blank_lp[r] = t < clampi(len[b], 0, T) ? x[(long long)b * sb + (long long)t * st + blank] : 0.0f;
}

// ---------------------------------------------------------------------------------------------
// plan.  grid = B, block = 256.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PLAN_THREADS) void fskip_plan_kernel(const float *__restrict__ blank_lp,
                                                                  const int *__restrict__ len,
                                                                  const int *__restrict__ min_frames, int T,
                                                                  float log_thr, int *__restrict__ kept_lengths,
                                                                  int *__restrict__ frame_index,
                                                                  int *__restrict__ position) {
    __shared__ unsigned key[PIKA_FSKIP_MAX_T];
    __shared__ int red[PLAN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int L = clampi(len[b], 0, T);
    const int m = L == 0 ? 0 : clampi(min_frames ? min_frames[b] : 1, 1, L);
    const float *lp = blank_lp + (size_t)b * T;
    int *fi = frame_index + (size_t)b * T;
    int *po = position + (size_t)b * T;

    // the workgroup's sum of one int per thread (every thread gets it)
    auto total = [&](int v) __attribute__((always_inline)) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        __syncthreads();  // the previous total is read; what was written to LDS before is visible behind it
        if (lane == 0) red[w] = v;
        __syncthreads();
        return red[0] + red[1] + red[2] + red[3];
    };
    // the dropped frames pred(key, t) holds for, counted
    auto count = [&](auto pred) __attribute__((always_inline)) {
        int c = 0;
        for (int t = tid; t < L; t += PLAN_THREADS) {
            const unsigned k = key[t];
            c += (k != 0 && pred(k, t)) ? 1 : 0;
        }
        return total(c);
    };

    int mine = 0;
    for (int t = tid; t < L; t += PLAN_THREADS) {
        const float v = lp[t];
        const bool drop = v >= log_thr;  // a NaN compares false: kept
        key[t] = drop ? fkey(v) : 0u;
        mine += drop ? 0 : 1;
    }
    const int natural = total(mine);

    // top-up: the r dropped frames that come first in (key, t) are put back: key < kth, or key == kth and t < cut
    unsigned kth = 0;
    int cut = 0;
    if (natural < m) {  // workgroup-uniform
        const int r = m - natural;  // 1 <= r <= the number of dropped frames, as m <= L
        for (int bit = 31; bit >= 0; --bit) {  // kth: the largest x with fewer than r keys below it = the r-th smallest key
            const unsigned mid = kth | (1u << bit);
            if (count([&](unsigned k, int) { return k < mid; }) < r) kth = mid;
        }
        const unsigned kk = kth;
        const int rem = r - count([&](unsigned k, int) { return k < kk; });  // >= 1 of the frames at kth
        // cut: the largest x with at most rem of the ties before it (every bit up to T's highest, >= T, if all of them fit)
        for (int bit = 31 - __clz(T); bit >= 0; --bit) {
            const int mid = cut | (1 << bit);
            if (count([&](unsigned k, int t) { return k == kk && t < mid; }) <= rem) cut = mid;
        }
    }

    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;  // kept frames before this chunk: workgroup-uniform
    for (int t0 = 0; t0 < T; t0 += PLAN_THREADS) {
        const int t = t0 + tid;
        bool keep = false;
        if (t < L) {
            const unsigned k = key[t];
            keep = k == 0 || k < kth || (k == kth && t < cut);
        }
        const unsigned long long mask = __ballot(keep);
        __syncthreads();  // the previous chunk's totals are read
        if (lane == 0) red[w] = __popcll(mask);
        __syncthreads();
        int before = base;
        for (int i = 0; i < w; ++i) before += red[i];
        const int pos = before + __popcll(mask & below);
        if (t < T) po[t] = keep ? pos : -1;
        if (keep) fi[pos] = t;  // pos < L <= T: the map is injective
        base += red[0] + red[1] + red[2] + red[3];
    }
    for (int j = base + tid; j < T; j += PLAN_THREADS) fi[j] = -1;
    if (tid == 0) kept_lengths[b] = base;
}

// ---------------------------------------------------------------------------------------------
// apply.  grid = B * T, block = 128.
// ---------------------------------------------------------------------------------------------
template <typename W>
__device__ inline void copy_row(const char *in, char *out, long long n, bool ok) {
    const W *src = reinterpret_cast<const W *>(in);
    W *dst = reinterpret_cast<W *>(out);
    for (long long i = threadIdx.x; i < n; i += APPLY_THREADS) dst[i] = ok ? src[i] : W{};
}

__global__ __launch_bounds__(APPLY_THREADS) void fskip_apply_kernel(const char *__restrict__ x, long long sb,
                                                                    long long st, const int *__restrict__ index, int T,
                                                                    long long row_bytes, int elem_bytes, int vec,
                                                                    char *__restrict__ out) {
    const int b = blockIdx.x / T;
    const int src = index[blockIdx.x];
    const bool ok = src >= 0 && src < T;  // anything else reads nothing
    const char *in = x + (long long)b * sb + (long long)(ok ? src : 0) * st;
    char *o = out + (long long)blockIdx.x * row_bytes;
    if (vec)
        copy_row<uint4>(in, o, row_bytes / 16, ok);
    else if (elem_bytes == 4)
        copy_row<unsigned>(in, o, row_bytes / 4, ok);
    else
        copy_row<unsigned short>(in, o, row_bytes / 2, ok);
}

int check_dims(int B, int T) {
    if (B < 1 || T < 1) return PIKA_EINVAL;
    if (T > PIKA_FSKIP_MAX_T || (long long)B * T > 0x7fffffffLL) return PIKA_ETOOBIG;
    return PIKA_OK;
}

}  // namespace

extern "C" {

int pika_fskip_rows(const float *x, long long stride_b, long long stride_t, const int *lengths, int B, int T, int C,
                    int blank, int logits, float *blank_lp, void *stream) {
    if (int rc = check_dims(B, T)) return rc;
    if (C < 1 || blank < 0 || blank >= C) return PIKA_EINVAL;
    if (!x || !lengths || !blank_lp) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long rows = (long long)B * T;
    if (logits)
        hipLaunchKernelGGL(fskip_rows_logits_kernel, dim3((unsigned)rows), dim3(ROW_THREADS), 0, s, x, stride_b,
                           stride_t, lengths, T, C, blank, blank_lp);
    else
        hipLaunchKernelGGL(fskip_rows_gather_kernel, dim3((unsigned)((rows + ROW_THREADS - 1) / ROW_THREADS)),
                           dim3(ROW_THREADS), 0, s, x, stride_b, stride_t, lengths, B, T, blank, blank_lp);
    return (int)hipGetLastError();
}

int pika_fskip_plan(const float *blank_lp, const int *lengths, const int *min_frames, int B, int T, float log_thr,
                    int *kept_lengths, int *frame_index, int *position, void *stream) {
    if (int rc = check_dims(B, T)) return rc;
    if (!blank_lp || !lengths || !kept_lengths || !frame_index || !position) return PIKA_EINVAL;
    hipLaunchKernelGGL(fskip_plan_kernel, dim3((unsigned)B), dim3(PLAN_THREADS), 0, static_cast<hipStream_t>(stream),
                       blank_lp, lengths, min_frames, T, log_thr, kept_lengths, frame_index, position);
    return (int)hipGetLastError();
}

int pika_fskip_apply(const void *x, long long stride_b, long long stride_t, const int *index, int B, int T,
                     long long row_bytes, int elem_bytes, void *out, void *stream) {
    if (int rc = check_dims(B, T)) return rc;
    if (!x || !index || !out || row_bytes < 1 || (elem_bytes != 2 && elem_bytes != 4)) return PIKA_EINVAL;
    if (row_bytes > 0x7fffffffLL) return PIKA_ETOOBIG;
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    const long long e = elem_bytes;
    if (row_bytes % e || stride_b % e || stride_t % e || xa % e || oa % e) return PIKA_EINVAL;
    const int vec = row_bytes % 16 == 0 && stride_b % 16 == 0 && stride_t % 16 == 0 && xa % 16 == 0 && oa % 16 == 0;
    hipLaunchKernelGGL(fskip_apply_kernel, dim3((unsigned)((long long)B * T)), dim3(APPLY_THREADS), 0,
                       static_cast<hipStream_t>(stream), static_cast<const char *>(x), stride_b, stride_t, index, T,
                       row_bytes, elem_bytes, vec, static_cast<char *>(out));
    return (int)hipGetLastError();
}

}  // extern "C"
