// pika_amd/csrc/rnnt_simple.hip -- the planes of the smoothed "simple" joiner am + lm of pruned RNN-T
// (include/pika_rnnt.h "Smoothed simple planes", DESIGN.md section 3 "Pruned lattice").
//
// Everything that touches (B, T, V), or contracts (B, T, U1) against V, is here; what is (B, U1, V)- or (V,)-sized (the
// lm row maxima, elm = exp(lm - lmax), the batch unigram q, Zl) is prepared by the caller.  With e = exp(am - amax):
//
//   forward   simple_rowmax_gather   amax[b,t] and gathered[b,t,u] = am[b,t,y_bu] (column U: am[b,t,blank]), one wave per
//                                    row: the gathers hit the row the wave has just read
//             simple_contract_fwd    sums[b,t,j] = sum_v e[b,t,v] * elm[b,j,v]: a 64 x 64 tile of (t, j) per workgroup,
//                                    V in chunks of 64 staged in LDS (the next chunk is in flight in registers meanwhile)
//             simple_planes          the two planes from sums, amax, gathered and the caller's per-(b,u) constants
//   backward  simple_bwd             a workgroup per (utterance, 64 columns of V) walks t in tiles of 64: it reads am once,
//                                    writes d_am once (the label / blank scatter terms are added in LDS, in ascending u,
//                                    by the one thread that owns the row) and owns m[b, :, chunk] = sum_t w[t,j] e[t,v]
//                                    outright, so nothing is accumulated across workgroups and there are no atomics.
//                                    NC > 64: workgroup (chunk, jy > 0) only accumulates columns [64 jy, 64 jy + 64) of m.
//
// All sums run in a fixed order: two calls are bit-identical.  Plain fp32 FMA on 4 x 4 register tiles.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "pika_rnnt.h"

namespace {

constexpr int TILE = 64;      // edge of every tile: t, j and the V chunk
constexpr int LDP = 68;       // LDS row pitch in floats: rows stay 16-byte aligned for the float4 reads
constexpr int NSIDE = 5;      // per-(b,u) constants of simple_planes (pika_rnnt.h)

__device__ __forceinline__ int label_at(const int *labels, int b, int u, int U, int V, int blank) {
    if (u >= U) return blank;
    const int y = labels[(size_t)b * U + u];
    return y < 0 ? 0 : (y >= V ? V - 1 : y);
}

__global__ __launch_bounds__(256) void simple_rowmax_gather(const float *__restrict__ am, const int *__restrict__ labels,
                                                            int T, int U1, int V, int blank, long long rows,
                                                            float *__restrict__ amax, float *__restrict__ gathered) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *a = am + (size_t)row * V;
    float m = -INFINITY;
    if ((V & 3) == 0 && (reinterpret_cast<uintptr_t>(am) & 15) == 0) {
        const float4 *a4 = reinterpret_cast<const float4 *>(a);
        for (int i = lane; i < (V >> 2); i += 64) {
            const float4 x = a4[i];
            m = fmaxf(fmaxf(m, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
        }
    } else {
        for (int v = lane; v < V; v += 64) m = fmaxf(m, a[v]);
    }
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) amax[row] = m;
    const int b = (int)(row / T);
    for (int u = lane; u < U1; u += 64) gathered[(size_t)row * U1 + u] = a[label_at(labels, b, u, U1 - 1, V, blank)];
}

// grid (ceil(T / 64), ceil(NC / 64), B)
__global__ __launch_bounds__(256) void simple_contract_fwd(const float *__restrict__ am, const float *__restrict__ amax,
                                                           const float *__restrict__ elm, int T, int NC, int V,
                                                           float *__restrict__ sums) {
    __shared__ __attribute__((aligned(16))) float sA[TILE][LDP];   // [v][t]
    __shared__ __attribute__((aligned(16))) float sE[TILE][LDP];   // [v][j]
    const int b = blockIdx.z, t0 = blockIdx.x * TILE, j0 = blockIdx.y * TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid & 15, ty = tid >> 4;                        // this thread's 4 j and 4 t
    const float *amb = am + (size_t)b * T * V;
    const float *eb = elm + (size_t)b * NC * V;

    float mx[16], ra[16], re[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + wave + 4 * i;
        mx[i] = t < T ? amax[(size_t)b * T + t] : 0.f;
    }
    auto fetch = [&](int v0) {       // wave w brings rows w, w + 4, ...; a lane is one column of the chunk
        const int v = v0 + lane;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int t = t0 + wave + 4 * i, j = j0 + wave + 4 * i;
            ra[i] = (t < T && v < V) ? amb[(size_t)t * V + v] : -INFINITY;
            re[i] = (j < NC && v < V) ? eb[(size_t)j * V + v] : 0.f;
        }
    };
    float acc[4][4] = {};
    fetch(0);
    for (int v0 = 0; v0 < V; v0 += TILE) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sA[lane][wave + 4 * i] = expf(ra[i] - mx[i]);        // exp(-inf) = 0 outside the tensor
            sE[lane][wave + 4 * i] = re[i];
        }
        __syncthreads();
        if (v0 + TILE < V) fetch(v0 + TILE);
#pragma unroll 8
        for (int k = 0; k < TILE; ++k) {
            const float4 a = *reinterpret_cast<const float4 *>(&sA[k][ty * 4]);
            const float4 e = *reinterpret_cast<const float4 *>(&sE[k][tx * 4]);
            const float av[4] = {a.x, a.y, a.z, a.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], ev[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int jj = j0 + tx * 4 + j;
            if (t < T && jj < NC) sums[((size_t)b * T + t) * NC + jj] = acc[i][j];
        }
    }
}

// One thread per (b, t, u).  side[b][u] = {lm_blank - lmax, lm_y - lmax, Zl - lmax, log q[blank], log q[y]}.
__global__ __launch_bounds__(256) void simple_planes(const float *__restrict__ sums, const float *__restrict__ amax,
                                                     const float *__restrict__ gathered, const float *__restrict__ side,
                                                     int T, int U1, int NC, long long n, float c, float ll, float la,
                                                     float *__restrict__ blank_lp, float *__restrict__ label_lp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long row = i / U1;
    const int u = (int)(i - row * U1), b = (int)(row / T);
    const float mx = amax[row];
    const float am_b = gathered[(size_t)row * U1 + U1 - 1] - mx, am_y = gathered[i] - mx;
    const float *sd = side + ((size_t)b * U1 + u) * NSIDE;
    const float log_s = logf(fmaxf(sums[(size_t)row * NC + u], FLT_MIN));
    float bl = c * ((am_b + sd[0]) - log_s), lb = c * ((am_y + sd[1]) - log_s);
    if (ll != 0.f) {
        bl += ll * (sd[0] - sd[2]);
        lb += ll * (sd[1] - sd[2]);
    }
    if (la != 0.f) {
        const float log_sq = logf(fmaxf(sums[(size_t)row * NC + U1], FLT_MIN));
        bl += la * ((am_b + sd[3]) - log_sq);
        lb += la * ((am_y + sd[4]) - log_sq);
    }
    blank_lp[i] = bl;
    label_lp[i] = u < U1 - 1 ? lb : -1.0e30f;
}

// grid (ceil(V / 64), ceil(NC / 64), B)
__global__ __launch_bounds__(256) void simple_bwd(const float *__restrict__ am, const float *__restrict__ amax,
                                                  const float *__restrict__ elm, const float *__restrict__ w,
                                                  const float *__restrict__ sg, const int *__restrict__ labels, int T,
                                                  int U1, int NC, int V, int blank, float *__restrict__ d_am,
                                                  float *__restrict__ m) {
    __shared__ __attribute__((aligned(16))) float sX[TILE][LDP];   // [t][v]: e, then the d_am tile
    __shared__ __attribute__((aligned(16))) float sW[TILE][LDP];   // [t][j]
    __shared__ __attribute__((aligned(16))) float sE[TILE][LDP];   // [j][v]
    __shared__ int sY[1024];
    const int b = blockIdx.z, v0 = blockIdx.x * TILE, jy = blockIdx.y, nj = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid & 15, ty = tid >> 4;
    const int v = v0 + lane;
    const float *amb = am + (size_t)b * T * V;
    const float *eb = elm + (size_t)b * NC * V;
    const float *wb = w + (size_t)b * T * NC;
    const bool lead = jy == 0;                 // the workgroup that also writes d_am for this chunk
    const int jt_lo = jy, jt_hi = lead ? nj : jy + 1;

    if (lead)
        for (int u = tid; u < U1; u += 256) sY[u] = label_at(labels, b, u, U1 - 1, V, blank) - v0;
    float acc_m[4][4] = {};
    for (int t0 = 0; t0 < T; t0 += TILE) {
        for (int r = wave; r < TILE; r += 4) {
            const int t = t0 + r;
            sX[r][lane] = (t < T && v < V) ? expf(amb[(size_t)t * V + v] - amax[(size_t)b * T + t]) : 0.f;
        }
        float acc_p[4][4] = {};
        for (int jt = jt_lo; jt < jt_hi; ++jt) {
            const int j = jt * TILE + lane;
            for (int r = wave; r < TILE; r += 4) {
                const int t = t0 + r;
                sW[r][lane] = (t < T && j < NC) ? wb[(size_t)t * NC + j] : 0.f;
            }
            if (lead && (nj > 1 || t0 == 0))   // one tile of elm serves every t when NC <= 64
                for (int r = wave; r < TILE; r += 4) {
                    const int jr = jt * TILE + r;
                    sE[r][lane] = (jr < NC && v < V) ? eb[(size_t)jr * V + v] : 0.f;
                }
            __syncthreads();
            if (lead) {                        // p[t][v] += sum_j w[t][j] elm[j][v]
#pragma unroll 8
                for (int k = 0; k < TILE; ++k) {
                    const float4 e = *reinterpret_cast<const float4 *>(&sE[k][tx * 4]);
                    const float ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float a = sW[ty * 4 + i][k];
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc_p[i][q] = fmaf(a, ev[q], acc_p[i][q]);
                    }
                }
            }
            if (jt == jy) {                    // m[j][v] += sum_t w[t][j] e[t][v]
#pragma unroll 8
                for (int k = 0; k < TILE; ++k) {
                    const float4 a = *reinterpret_cast<const float4 *>(&sW[k][ty * 4]);
                    const float4 e = *reinterpret_cast<const float4 *>(&sX[k][tx * 4]);
                    const float av[4] = {a.x, a.y, a.z, a.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc_m[i][q] = fmaf(av[i], ev[q], acc_m[i][q]);
                }
            }
            __syncthreads();
        }
        if (lead) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) sX[ty * 4 + i][tx * 4 + q] *= -acc_p[i][q];
            __syncthreads();
            if (tid < TILE && t0 + tid < T) {  // the scatter terms of row t0 + tid, in ascending u
                const float *sgr = sg + ((size_t)b * T + t0 + tid) * U1;
                for (int u = 0; u < U1; ++u) {
                    const int y = sY[u];
                    if (y >= 0 && y < TILE) sX[tid][y] += sgr[u];
                }
            }
            __syncthreads();
            for (int r = wave; r < TILE; r += 4) {
                const int t = t0 + r;
                if (t < T && v < V) d_am[((size_t)b * T + t) * V + v] = sX[r][lane];
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = jy * TILE + ty * 4 + i;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int vv = v0 + tx * 4 + q;
            if (j < NC && vv < V) m[((size_t)b * NC + j) * V + vv] = acc_m[i][q];
        }
    }
}

int check_common(int B, int T, int U1, int V, int blank, float ll, float la) {
    if (B <= 0 || T <= 0 || U1 <= 0 || V <= 0 || blank < 0 || blank >= V) return PIKA_EINVAL;
    if (!(ll >= 0.f && la >= 0.f && ll + la < 1.f)) return PIKA_EINVAL;
    if (U1 > 1024 || B > 65535) return PIKA_ETOOBIG;
    return 0;
}

}  // namespace

extern "C" {

int pika_prnnt_smoothed_fwd(const float *am, const float *elm, const float *side, const int *labels, int B, int T, int U1,
                            int V, int blank, float lm_only_scale, float am_only_scale, float *amax, float *gathered,
                            float *sums, float *blank_lp, float *label_lp, void *stream) {
    if (const int rc = check_common(B, T, U1, V, blank, lm_only_scale, am_only_scale)) return rc;
    if (!am || !elm || !side || !amax || !gathered || !sums || !blank_lp || !label_lp || (U1 > 1 && !labels))
        return PIKA_EINVAL;
    const int NC = U1 + (am_only_scale != 0.f ? 1 : 0);
    const long long rows = (long long)B * T, n = rows * U1;
    if ((rows + 3) / 4 > 0x7fffffffLL || (n + 255) / 256 > 0x7fffffffLL) return PIKA_ETOOBIG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float c = (float)(1.0 - (double)lm_only_scale - (double)am_only_scale);
    simple_rowmax_gather<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(am, labels, T, U1, V, blank, rows, amax,
                                                                                gathered);
    simple_contract_fwd<<<dim3((T + TILE - 1) / TILE, (NC + TILE - 1) / TILE, B), dim3(256), 0, s>>>(am, amax, elm, T, NC,
                                                                                                    V, sums);
    simple_planes<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(sums, amax, gathered, side, T, U1, NC, n, c,
                                                                          lm_only_scale, am_only_scale, blank_lp,
                                                                          label_lp);
    return (int)hipGetLastError();
}

int pika_prnnt_smoothed_bwd(const float *am, const float *amax, const float *elm, const float *w, const float *sg,
                            const int *labels, int B, int T, int U1, int V, int blank, float lm_only_scale,
                            float am_only_scale, float *d_am, float *m, void *stream) {
    if (const int rc = check_common(B, T, U1, V, blank, lm_only_scale, am_only_scale)) return rc;
    if (!am || !amax || !elm || !w || !sg || !d_am || !m || (U1 > 1 && !labels)) return PIKA_EINVAL;
    const int NC = U1 + (am_only_scale != 0.f ? 1 : 0);
    simple_bwd<<<dim3((V + TILE - 1) / TILE, (NC + TILE - 1) / TILE, B), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(
        am, amax, elm, w, sg, labels, T, U1, NC, V, blank, d_am, m);
    return (int)hipGetLastError();
}

}  // extern "C"
