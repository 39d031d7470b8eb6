// pika_amd/csrc/stateless.hip -- the stateless prediction network (include/pika_stateless.h): embedding + grouped causal
// Conv1d over the last ctx labels + ReLU.  Training forward and backward, and the search's per-frame step.
//
// Everything here is bound by launches and by gathers of short rows, not by arithmetic: ctx * cpg (8 in the recipes)
// fused multiply-adds per output element.  The kernels are therefore plain: one thread per output element, E read in
// 16-byte pieces where a group's cpg inputs allow it, no atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pika_stateless.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_CTX = PIKA_STATELESS_MAX_CTX;
constexpr int MAX_BEAM = 64;
constexpr int DW_ROWS = 32;          // d_w: the least number of (b,u) rows a chunk sums
constexpr int DW_MAX_CHUNKS = 128;   // and the most chunks there are
constexpr int DW_TILE = 64;          // output channels per workgroup of the chunk sums
constexpr long long MAX_ROWS = 1ll << 30;

__device__ __forceinline__ int token_of(long long t, int V) {        // < 0: padding; clamped below V
    return t < 0 ? -1 : (int)(t < (long long)(V - 1) ? t : (long long)(V - 1));
}

// THE definition of z for output channel d; tok(j) is the token at context position j (negative: padding), already
// below V.  j ascending outside, c ascending inside, every product fused into the sum: the same bits whatever VEC is.
template <bool VEC, class Tok>
__device__ __forceinline__ float stateless_z(Tok tok, const float *__restrict__ E, const float *__restrict__ w, int D,
                                             int cpg, int ctx, int d) {
    const int g0 = (d / cpg) * cpg;
    const float *wd = w + (size_t)d * cpg * ctx;
    float acc = 0.0f;
    for (int j = 0; j < ctx; ++j) {
        const int t = tok(j);
        if (t < 0) continue;
        const float *e = E + (size_t)t * D + g0;
        if (VEC) {
            for (int c = 0; c < cpg; c += 4) {
                const float4 v = *reinterpret_cast<const float4 *>(e + c);
                acc = fmaf(wd[(c + 0) * ctx + j], v.x, acc);
                acc = fmaf(wd[(c + 1) * ctx + j], v.y, acc);
                acc = fmaf(wd[(c + 2) * ctx + j], v.z, acc);
                acc = fmaf(wd[(c + 3) * ctx + j], v.w, acc);
            }
        } else {
            for (int c = 0; c < cpg; ++c) acc = fmaf(wd[c * ctx + j], e[c], acc);
        }
    }
    return acc;
}

__device__ __forceinline__ float relu(float z) { return z > 0.0f ? z : 0.0f; }

template <bool VEC>
__global__ __launch_bounds__(THREADS) void stateless_forward_kernel(
    const long long *__restrict__ y, long long ldy, const float *__restrict__ E, const float *__restrict__ w,
    long long N, int U, int V, int D, int cpg, int ctx, float *__restrict__ out, long long ld) {
    const long long total = N * D;
    for (long long idx = (long long)blockIdx.x * THREADS + threadIdx.x; idx < total; idx += (long long)gridDim.x * THREADS) {
        const long long n = idx / D;
        const int d = (int)(idx - n * D);
        const long long b = n / U;
        const int first = (int)(n - b * U) - (ctx - 1);          // the position of context entry 0
        const long long *yr = y + b * ldy;
        const float z = stateless_z<VEC>([&](int j) { return first + j < 0 ? -1 : token_of(yr[first + j], V); }, E, w, D,
                                         cpg, ctx, d);
        out[n * ld + d] = relu(z);
    }
}

// One workgroup per utterance.  All K old contexts go to LDS before the first store, so a slot never reads a context
// that another slot has rewritten.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void stateless_step_kernel(
    int *__restrict__ ctx_tok, const long long *__restrict__ parent, const long long *__restrict__ token, int K, int ctx,
    int blank, const float *__restrict__ E, const float *__restrict__ w, int V, int D, int cpg, float *__restrict__ rows,
    long long ld) {
    __shared__ int s_old[MAX_BEAM * MAX_CTX];
    __shared__ int s_new[MAX_BEAM * MAX_CTX];
    const long long b = blockIdx.x;
    int *rec = ctx_tok + b * K * ctx;
    const int n = K * ctx;
    for (int i = threadIdx.x; i < n; i += THREADS) s_old[i] = rec[i];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const int j = i / ctx, q = i - j * ctx;
        long long p = parent[b * K + j];
        p = p < 0 ? 0 : (p > K - 1 ? K - 1 : p);
        const long long tk = token[b * K + j];
        int v;
        if (tk != (long long)blank)
            v = q + 1 < ctx ? s_old[(int)p * ctx + q + 1] : (tk < 0 ? -1 : (int)(tk > 0x7fffffffll ? 0x7fffffffll : tk));
        else
            v = s_old[(int)p * ctx + q];
        s_new[i] = v;
        rec[i] = v;
    }
    __syncthreads();
    const int total = K * D;
    for (int idx = threadIdx.x; idx < total; idx += THREADS) {
        const int j = idx / D, d = idx - j * D;
        const int *c = s_new + j * ctx;
        const float z = stateless_z<VEC>([&](int q) { return token_of(c[q], V); }, E, w, D, cpg, ctx, d);
        rows[(b * K + j) * ld + d] = relu(z);
    }
}

// Backward, first launch: go = dout * (out > 0) into the workspace (for d_E), and d_w summed over this chunk of rows.
// grid (chunks, ceil(D / DW_TILE)).
__global__ __launch_bounds__(THREADS) void stateless_dw_chunk_kernel(
    const long long *__restrict__ y, long long ldy, const float *__restrict__ E, const float *__restrict__ out,
    long long ld_out, const float *__restrict__ dout, long long ld_dout, long long N, int U, int V, int D, int cpg,
    int ctx, int rows_per_chunk, float *__restrict__ go, float *__restrict__ part) {
    const long long n0 = (long long)blockIdx.x * rows_per_chunk;
    const long long n1 = n0 + rows_per_chunk < N ? n0 + rows_per_chunk : N;
    const int d0 = blockIdx.y * DW_TILE;
    const int dn = D - d0 < DW_TILE ? D - d0 : DW_TILE;
    const int cells = (int)(n1 - n0) * dn;
    for (int i = threadIdx.x; i < cells; i += THREADS) {
        const int r = i / dn, d = d0 + (i - r * dn);
        const long long n = n0 + r;
        go[n * D + d] = out[n * ld_out + d] > 0.0f ? dout[n * ld_dout + d] : 0.0f;
    }
    const int per = dn * cpg, total = ctx * per;
    float *mine = part + (size_t)blockIdx.x * D * cpg * ctx;
    for (int e = threadIdx.x; e < total; e += THREADS) {          // c fastest: neighbours read neighbouring inputs
        const int j = e / per, rem = e - j * per;
        const int dl = rem / cpg, c = rem - dl * cpg;
        const int d = d0 + dl, gin = (d / cpg) * cpg + c;
        float acc = 0.0f;
        for (long long n = n0; n < n1; ++n) {
            const long long b = n / U;
            const int p = (int)(n - b * U) - (ctx - 1) + j;
            if (p < 0) continue;
            const int t = token_of(y[b * ldy + p], V);
            if (t < 0) continue;
            const float g = out[n * ld_out + d] > 0.0f ? dout[n * ld_dout + d] : 0.0f;
            acc = fmaf(g, E[(size_t)t * D + gin], acc);
        }
        mine[((size_t)d * cpg + c) * ctx + j] = acc;
    }
}

__global__ __launch_bounds__(THREADS) void stateless_dw_final_kernel(const float *__restrict__ part, int chunks, int count,
                                                                     float *__restrict__ d_w) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= count) return;
    float acc = part[i];
    for (int k = 1; k < chunks; ++k) acc += part[(size_t)k * count + i];      // ascending: a fixed order
    d_w[i] = acc;
}

__device__ __forceinline__ long long lower_bound(const long long *__restrict__ a, long long n, long long v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per token v: its positions are a run of the sorted tokens; each thread owns input channels i and sums
// the run in order.  A token that does not occur has an empty run and writes zeros.
__global__ __launch_bounds__(THREADS) void stateless_dE_kernel(
    const long long *__restrict__ sorted_tok, const long long *__restrict__ order, const float *__restrict__ w,
    const float *__restrict__ go, long long N, int U, int V, int D, int cpg, int ctx, float *__restrict__ d_E) {
    const long long v = blockIdx.x;
    const long long lo = lower_bound(sorted_tok, N, v);
    const long long hi = v == V - 1 ? N : lower_bound(sorted_tok, N, v + 1);      // (tokens >= V were clamped to V - 1)
    for (int i = threadIdx.x; i < D; i += blockDim.x) {
        const int g0 = (i / cpg) * cpg, ci = i - g0;
        float acc = 0.0f;
        for (long long s = lo; s < hi; ++s) {
            long long pos = order[s];
            pos = pos < 0 ? 0 : (pos > N - 1 ? N - 1 : pos);
            const long long b = pos / U;
            const int p = (int)(pos - b * U);
            for (int j = 0; j < ctx; ++j) {
                const int u = p + (ctx - 1) - j;
                if (u >= U) continue;
                const float *gr = go + (size_t)(b * U + u) * D + g0;
                for (int dd = 0; dd < cpg; ++dd) acc = fmaf(w[((size_t)(g0 + dd) * cpg + ci) * ctx + j], gr[dd], acc);
            }
        }
        d_E[(size_t)v * D + i] = acc;
    }
}

int check_net(int V, int D, int cpg, int ctx) {
    if (V < 1 || D < 1 || cpg < 1 || ctx < 1) return PIKA_EINVAL;
    if (ctx > MAX_CTX || cpg > PIKA_STATELESS_MAX_CPG || D > PIKA_STATELESS_MAX_DIM || D % cpg != 0) return PIKA_ETOOBIG;
    return PIKA_OK;
}

int check_rows(int B, int U) {
    if (B < 1 || U < 1) return PIKA_EINVAL;
    if (B > 65535 || (long long)B * U > MAX_ROWS) return PIKA_ETOOBIG;
    return PIKA_OK;
}

inline bool vec_ok(const float *E, int cpg) { return cpg % 4 == 0 && reinterpret_cast<uintptr_t>(E) % 16 == 0; }

inline int dw_rows_per_chunk(long long N) {
    const long long r = (N + DW_MAX_CHUNKS - 1) / DW_MAX_CHUNKS;
    return (int)(r < DW_ROWS ? DW_ROWS : r);
}

inline size_t go_bytes(long long N, int D) { return ((size_t)N * D * 4 + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int pika_stateless_forward(const long long *y, long long ldy, const float *E, const float *w, int B, int U, int V, int D,
                           int cpg, int ctx, float *out, long long ld, void *stream) {
    if (int rc = check_rows(B, U)) return rc;
    if (int rc = check_net(V, D, cpg, ctx)) return rc;
    if (!y || !E || !w || !out || ldy < U || ld < D) return PIKA_EINVAL;
    const long long N = (long long)B * U;
    const long long blocks = (N * D + THREADS - 1) / THREADS;
    const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec_ok(E, cpg))
        hipLaunchKernelGGL(stateless_forward_kernel<true>, grid, dim3(THREADS), 0, s, y, ldy, E, w, N, U, V, D, cpg, ctx,
                           out, ld);
    else
        hipLaunchKernelGGL(stateless_forward_kernel<false>, grid, dim3(THREADS), 0, s, y, ldy, E, w, N, U, V, D, cpg, ctx,
                           out, ld);
    return (int)hipGetLastError();
}

size_t pika_stateless_backward_workspace_bytes(int B, int U, int D, int cpg, int ctx) {
    if (check_rows(B, U) || check_net(1, D, cpg, ctx)) return 0;
    const long long N = (long long)B * U;
    const int R = dw_rows_per_chunk(N);
    const size_t chunks = (size_t)((N + R - 1) / R);
    return go_bytes(N, D) + chunks * D * cpg * ctx * 4;
}

int pika_stateless_backward(const long long *y, long long ldy, const long long *sorted_tok, const long long *order,
                            const float *E, const float *w, const float *out, long long ld_out, const float *dout,
                            long long ld_dout, int B, int U, int V, int D, int cpg, int ctx, float *d_E, float *d_w,
                            void *workspace, void *stream) {
    if (int rc = check_rows(B, U)) return rc;
    if (int rc = check_net(V, D, cpg, ctx)) return rc;
    if (!y || !sorted_tok || !order || !E || !w || !out || !dout || !d_E || !d_w || !workspace || ldy < U || ld_out < D
        || ld_dout < D)
        return PIKA_EINVAL;
    const long long N = (long long)B * U;
    const int R = dw_rows_per_chunk(N);
    const int chunks = (int)((N + R - 1) / R);
    const int count = D * cpg * ctx;
    float *go = static_cast<float *>(workspace);
    float *part = reinterpret_cast<float *>(static_cast<char *>(workspace) + go_bytes(N, D));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(stateless_dw_chunk_kernel, dim3((unsigned)chunks, (unsigned)((D + DW_TILE - 1) / DW_TILE)),
                       dim3(THREADS), 0, s, y, ldy, E, out, ld_out, dout, ld_dout, N, U, V, D, cpg, ctx, R, go, part);
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(stateless_dw_final_kernel, dim3((unsigned)((count + THREADS - 1) / THREADS)), dim3(THREADS), 0, s,
                       part, chunks, count, d_w);
    if (hipError_t e = hipGetLastError()) return (int)e;
    const int threads = D >= THREADS ? THREADS : ((D + 63) / 64) * 64;
    hipLaunchKernelGGL(stateless_dE_kernel, dim3((unsigned)V), dim3(threads), 0, s, sorted_tok, order, w, go, N, U, V, D,
                       cpg, ctx, d_E);
    return (int)hipGetLastError();
}

int pika_stateless_step(int *ctx_tok, const long long *parent, const long long *token, int B, int K, int ctx, int blank,
                        const float *E, const float *w, int V, int D, int cpg, float *rows, long long ld, void *stream) {
    if (B < 1 || K < 1) return PIKA_EINVAL;
    if (B > 65535 || K > MAX_BEAM) return PIKA_ETOOBIG;
    if (int rc = check_net(V, D, cpg, ctx)) return rc;
    if (!ctx_tok || !parent || !token || !E || !w || !rows || ld < D || blank < 0 || blank >= V) return PIKA_EINVAL;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec_ok(E, cpg))
        hipLaunchKernelGGL(stateless_step_kernel<true>, dim3((unsigned)B), dim3(THREADS), 0, s, ctx_tok, parent, token, K,
                           ctx, blank, E, w, V, D, cpg, rows, ld);
    else
        hipLaunchKernelGGL(stateless_step_kernel<false>, dim3((unsigned)B), dim3(THREADS), 0, s, ctx_tok, parent, token,
                           K, ctx, blank, E, w, V, D, cpg, rows, ld);
    return (int)hipGetLastError();
}

}  // extern "C"
