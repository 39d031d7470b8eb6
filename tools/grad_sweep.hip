// tools/grad_sweep.hip -- hardware A/B harness for the HBM-bound dense-gradient writer.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -o tools/grad_sweep tools/grad_sweep.hip
// Run on the GPU box: ./tools/grad_sweep [B T U1 V [check]]   (check: the bit comparison only)
// Every variant writes the same (B,T,U1,V) fp32 tensor; timing = hipEvents around N launches,
// variants interleaved over several rounds (cdna guide 5.4 rule 24).
#include "../pika_amd/csrc/rnnt_loss.hip"

#include <stdio.h>
#include <vector>
#include <algorithm>
#include <string>
#include <functional>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1);} } while (0)

namespace {

template <bool NT, int PER_THREAD>
__global__ __launch_bounds__(256) void fill_chunk(v4f *p, size_t n4) {
    const size_t base = (size_t)blockIdx.x * (256 * PER_THREAD) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const size_t i = base + (size_t)k * 256;
        if (i < n4) {
            v4f v = {0.f, 0.f, 0.f, 0.f};
            if constexpr (NT) __builtin_nontemporal_store(v, p + i); else p[i] = v;
        }
    }
}

// per-lane meta lookup (the library form), PER_THREAD as a parameter
template <bool NT, int PER_THREAD>
__global__ __launch_bounds__(256) void grad_flat_lane(const RowMeta *__restrict__ meta, size_t n4, int V4,
                                                     int blank, v4f *__restrict__ grads) {
    const int qb = blank >> 2, cb = blank & 3;
    size_t i = (size_t)blockIdx.x * (256 * PER_THREAD) + threadIdx.x;
    size_t row = i / (unsigned)V4;
    int q = (int)(i - row * V4);
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        if (i < n4) {
            v4f v = {0.f, 0.f, 0.f, 0.f};
            const int ye = meta[row].ye;
            const int qe = ye >> 2;
            if (q == qb || q == qe) {
                const float gb = meta[row].gb, ge = meta[row].ge;
                if (q == qb) { v.x = cb == 0 ? gb : 0.f; v.y = cb == 1 ? gb : 0.f; v.z = cb == 2 ? gb : 0.f; v.w = cb == 3 ? gb : 0.f; }
                if (q == qe) { const int ce = ye & 3; v.x = ce == 0 ? ge : v.x; v.y = ce == 1 ? ge : v.y; v.z = ce == 2 ? ge : v.z; v.w = ce == 3 ? ge : v.w; }
            }
            if constexpr (NT) __builtin_nontemporal_store(v, grads + i); else grads[i] = v;
        }
        i += 256; q += 256;
        while (q >= V4) { q -= V4; ++row; }
    }
}

// wave-uniform meta: a wave instruction (64 groups) spans at most two rows when V4 >= 64;
// both rows' metadata come in through the scalar cache.
template <bool NT, int PER_THREAD>
__global__ __launch_bounds__(256) void grad_flat_scalar(const RowMeta *__restrict__ meta, size_t n4, size_t nrows,
                                                       int V4, int blank, v4f *__restrict__ grads) {
    const int qb = blank >> 2, cb = blank & 3;
    const int lane = threadIdx.x & 63;
    // first group of this wave's first instruction (wave-uniform)
    size_t i0 = (size_t)blockIdx.x * (256 * PER_THREAD) + (threadIdx.x & ~63);
    i0 = ((size_t)__builtin_amdgcn_readfirstlane((int)(i0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)i0);
    size_t row0 = i0 / (unsigned)V4;
    int q0 = (int)(i0 - row0 * V4);
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const size_t i = i0 + lane;
        const size_t r0 = row0 < nrows ? row0 : nrows - 1;  // a tail wave past the tensor still reads inside the table
        const size_t row1 = row0 + 1 < nrows ? row0 + 1 : nrows - 1;
        const RowMeta m0 = meta[r0], m1 = meta[row1];  // scalar loads
        int q = q0 + lane;
        const bool second = q >= V4;
        q = second ? q - V4 : q;
        const float gb = second ? m1.gb : m0.gb, ge = second ? m1.ge : m0.ge;
        const int ye = second ? m1.ye : m0.ye;
        const int qe = ye >> 2, ce = ye & 3;
        v4f v = {0.f, 0.f, 0.f, 0.f};
        if (q == qb) { v.x = cb == 0 ? gb : 0.f; v.y = cb == 1 ? gb : 0.f; v.z = cb == 2 ? gb : 0.f; v.w = cb == 3 ? gb : 0.f; }
        if (q == qe) { v.x = ce == 0 ? ge : v.x; v.y = ce == 1 ? ge : v.y; v.z = ce == 2 ? ge : v.z; v.w = ce == 3 ? ge : v.w; }
        if (i < n4) { if constexpr (NT) __builtin_nontemporal_store(v, grads + i); else grads[i] = v; }
        i0 += 256; q0 += 256;
        while (q0 >= V4) { q0 -= V4; ++row0; }
    }
}

// ---------------------------------------------------------------------------------------------
// launch-geometry sweep of the scalar-metadata writer.  One body, one axis per parameter:
//   WG      threads per workgroup (256 / 512 / 1024); a workgroup covers WG*PT consecutive groups
//   PT      16-byte groups per thread
//   CONTIG  false: a thread's stores are WG groups apart (the library form: a wave's stores are
//                  WG*16 bytes apart), metadata looked up per store
//           true:  a wave owns 64*PT consecutive groups and issues PT back-to-back 1 KiB stores;
//                  one division and one metadata lookup per wave.  Needs V4 >= 64*PT (the wave's
//                  span then touches at most two rows)
//   META    META_PLAIN  the library form (division per wave, plain scalar loads)
//           META_HOIST  one division per workgroup (from blockIdx alone); the waves step from it
//           META_NT     as PLAIN, metadata through __builtin_nontemporal_load
//   rshift  workgroup-to-chunk map: 0 = linear; r > 0: every aligned group of 8 << r workgroups is
//           permuted so that workgroups b, b+8, b+16, .. (one XCD under round-robin placement) take
//           1 << r consecutive chunks.  A bijection whatever the placement; the last, partial group
//           keeps the linear map
// ---------------------------------------------------------------------------------------------
enum { META_PLAIN = 0, META_HOIST = 1, META_NT = 2 };
typedef int v4i __attribute__((ext_vector_type(4)));

template <int META>
__device__ inline RowMeta sweep_meta(const RowMeta *meta, size_t r) {
    if constexpr (META == META_NT) {
        const v4i w = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(meta) + r);
        return RowMeta{__int_as_float(w.x), __int_as_float(w.y), w.z, w.w};
    } else {
        return meta[r];
    }
}

__device__ inline size_t remap_chunk(size_t b, size_t nblocks, int rshift) {
    if (rshift == 0) return b;
    if (rshift < 0) {  // "R = all": workgroups b, b+8, .. walk one eighth of the tensor; the last nblocks % 8 stay linear
        const size_t per = nblocks >> 3;
        return b < per * 8 ? (b & 7) * per + (b >> 3) : b;
    }
    const size_t gmask = ((size_t)8 << rshift) - 1;
    if ((b | gmask) >= nblocks) return b;  // last, partial group: linear
    const size_t j = b & gmask;
    return (b & ~gmask) | ((j & 7) << rshift) | (j >> 3);
}

template <int WG, int PT, bool CONTIG, int META>
__device__ inline void geo_chunk(size_t c, const RowMeta *__restrict__ meta, size_t n4, size_t nrows, int V4,
                                 int blank, v4f *__restrict__ grads) {
    const int qb = blank >> 2, cb = blank & 3;
    const int lane = threadIdx.x & 63;
    const int woff = CONTIG ? (int)(threadIdx.x >> 6) * (64 * PT) : (int)(threadIdx.x & ~63);
    size_t i0, row0;
    int q0;
    if constexpr (META == META_HOIST) {
        const size_t base = c * (size_t)(WG * PT);
        row0 = base / (unsigned)V4;
        q0 = (int)(base - row0 * V4) + __builtin_amdgcn_readfirstlane(woff);
        while (q0 >= V4) { q0 -= V4; ++row0; }
        i0 = base + (size_t)__builtin_amdgcn_readfirstlane(woff);
    } else {
        i0 = c * (size_t)(WG * PT) + woff;
        i0 = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(i0 >> 32)) << 32) |
             (unsigned)__builtin_amdgcn_readfirstlane((int)i0);
        row0 = i0 / (unsigned)V4;
        q0 = (int)(i0 - row0 * V4);
    }
    if constexpr (CONTIG) {
        const size_t r0 = row0 < nrows ? row0 : nrows - 1;
        const size_t r1 = row0 + 1 < nrows ? row0 + 1 : nrows - 1;
        const RowMeta m0 = sweep_meta<META>(meta, r0), m1 = sweep_meta<META>(meta, r1);
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const size_t i = i0 + k * 64 + lane;
            int q = q0 + k * 64 + lane;
            const bool second = q >= V4;
            q = second ? q - V4 : q;
            const v4f v = blend_row(q, qb, cb, second ? m1.gb : m0.gb, second ? m1.ge : m0.ge,
                                    second ? m1.ye : m0.ye);
            if (i < n4) grads[i] = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const size_t i = i0 + lane;
            const size_t r0 = row0 < nrows ? row0 : nrows - 1;
            const size_t r1 = row0 + 1 < nrows ? row0 + 1 : nrows - 1;
            const RowMeta m0 = sweep_meta<META>(meta, r0), m1 = sweep_meta<META>(meta, r1);
            int q = q0 + lane;
            const bool second = q >= V4;
            q = second ? q - V4 : q;
            const v4f v = blend_row(q, qb, cb, second ? m1.gb : m0.gb, second ? m1.ge : m0.ge,
                                    second ? m1.ye : m0.ye);
            if (i < n4) grads[i] = v;
            i0 += WG;
            q0 += WG;
            while (q0 >= V4) { q0 -= V4; ++row0; }
        }
    }
}

// one chunk per workgroup (grid = number of chunks)
template <int WG, int PT, bool CONTIG, int META>
__global__ __launch_bounds__(WG) void grad_geo(const RowMeta *__restrict__ meta, size_t n4, size_t nrows, int V4,
                                               int blank, v4f *__restrict__ grads, int rshift) {
    geo_chunk<WG, PT, CONTIG, META>(remap_chunk(blockIdx.x, gridDim.x, rshift), meta, n4, nrows, V4, blank, grads);
}

// bounded grid, grid-stride over the chunks: iteration it of workgroup b writes chunk it*grid + b
template <int WG, int PT, bool CONTIG, int META>
__global__ __launch_bounds__(WG) void grad_geo_stride(const RowMeta *__restrict__ meta, size_t n4, size_t nrows,
                                                      int V4, int blank, v4f *__restrict__ grads, size_t nchunks) {
    for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x)
        geo_chunk<WG, PT, CONTIG, META>(c, meta, n4, nrows, V4, blank, grads);
}

// bit-for-bit comparison of two tensors as 32-bit words (-0.0 and NaN payloads count)
__global__ __launch_bounds__(256) void diff_kernel(const unsigned *a, const unsigned *b, size_t n,
                                                   unsigned long long *out) {
    unsigned long long bad = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) bad += a[i] != b[i];
    if (bad) atomicAdd(out, bad);
}

__global__ __launch_bounds__(256) void checksum_kernel(const float *p, size_t n, double *out) {
    double acc = 0.0; unsigned long long nz = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float v = p[i];
        if (v != 0.f) { acc += (double)v * (double)(1 + (i % 8191)); ++nz; }
    }
    atomicAdd(out, acc);
    atomicAdd(out + 1, (double)nz);
}

struct Variant { std::string name; std::function<void(hipStream_t)> run; std::vector<float> ms; };

}  // namespace

int main(int argc, char **argv) {
    int B = 32, T = 1000, U1 = 51, V = 5000;
    if (argc >= 5) { B = atoi(argv[1]); T = atoi(argv[2]); U1 = atoi(argv[3]); V = atoi(argv[4]); }
    const bool check_only = argc >= 6 && std::string(argv[5]) == "check";  // bit comparison only, no timing
    const int blank = 0;
    const size_t nrows = (size_t)B * T * U1;
    const size_t n = nrows * V, n4 = n / 4;
    float *grads; CK(hipMalloc(&grads, (n + 64) * 4));  // 64 floats of guard for the bit comparison
    const size_t wsb = pika_rnnt_workspace_bytes(B, T, U1);
    void *ws; CK(hipMalloc(&ws, wsb)); CK(hipMemset(ws, 0, wsb));
    std::vector<int> hl((size_t)B * (U1 - 1)), hT(B, T), hU(B, U1 - 1);
    for (size_t i = 0; i < hl.size(); ++i) hl[i] = 1 + (int)((i * 2654435761u) % (V - 1));
    int *labels, *Tn, *Un;
    CK(hipMalloc(&labels, hl.size() * 4)); CK(hipMalloc(&Tn, B * 4)); CK(hipMalloc(&Un, B * 4));
    CK(hipMemcpy(labels, hl.data(), hl.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(Tn, hT.data(), B * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(Un, hU.data(), B * 4, hipMemcpyHostToDevice));
    const Lattice L = carve(ws, B, T, U1);
    hipStream_t s; CK(hipStreamCreate(&s));
    const RowMeta *meta = L.meta;
    v4f *g4 = (v4f *)grads;

    std::vector<Variant> vs;
    vs.push_back({"hipMemsetAsync", [&](hipStream_t st) { CK(hipMemsetAsync(grads, 0, n * 4, st)); }, {}});
    vs.push_back({"fill_chunk<nt,4>", [=](hipStream_t st) { hipLaunchKernelGGL((fill_chunk<true, 4>), dim3((unsigned)((n4 + 1023) / 1024)), dim3(256), 0, st, g4, n4); }, {}});
    vs.push_back({"fill_chunk<plain,4>", [=](hipStream_t st) { hipLaunchKernelGGL((fill_chunk<false, 4>), dim3((unsigned)((n4 + 1023) / 1024)), dim3(256), 0, st, g4, n4); }, {}});
    vs.push_back({"fill_chunk<plain,2>", [=](hipStream_t st) { hipLaunchKernelGGL((fill_chunk<false, 2>), dim3((unsigned)((n4 + 511) / 512)), dim3(256), 0, st, g4, n4); }, {}});
    vs.push_back({"fill_chunk<plain,8>", [=](hipStream_t st) { hipLaunchKernelGGL((fill_chunk<false, 8>), dim3((unsigned)((n4 + 2047) / 2048)), dim3(256), 0, st, g4, n4); }, {}});
    vs.push_back({"LIB backward (rowmeta + grad)", [=](hipStream_t st) {
        int rc = pika_rnnt_loss_backward(labels, Tn, Un, B, T, U1, V, blank, nullptr, ws, grads, st);
        if (rc) { printf("lib rc=%d\n", rc); exit(1); } }, {}});
#define LANE(NTV, PT) vs.push_back({std::string("flat_lane<") + (NTV ? "nt" : "plain") + "," #PT ">", [=](hipStream_t st) { \
        hipLaunchKernelGGL((grad_flat_lane<NTV, PT>), dim3((unsigned)((n4 + 256 * PT - 1) / (256 * PT))), dim3(256), 0, st, meta, n4, V / 4, blank, g4); }, {}})
#define SCAL(NTV, PT) vs.push_back({std::string("flat_scalar<") + (NTV ? "nt" : "plain") + "," #PT ">", [=](hipStream_t st) { \
        hipLaunchKernelGGL((grad_flat_scalar<NTV, PT>), dim3((unsigned)((n4 + 256 * PT - 1) / (256 * PT))), dim3(256), 0, st, meta, n4, nrows, V / 4, blank, g4); }, {}})
    LANE(false, 1); LANE(false, 2); LANE(false, 4); LANE(false, 8); LANE(true, 4); LANE(true, 2);
    SCAL(false, 1); SCAL(false, 2); SCAL(false, 4); SCAL(false, 8); SCAL(true, 4); SCAL(true, 2);
    // the shipped writer alone (the LIB line above also runs the 33 us rowmeta kernel)
    vs.push_back({"LIB dense_grads (writer alone)", [=](hipStream_t st) {
        int rc = pika_rnnt_loss_dense_grads(ws, B, T, U1, V, blank, grads, st);
        if (rc) { printf("lib rc=%d\n", rc); exit(1); } }, {}});

    // launch-geometry sweep: geo<WG,PT,layout,meta,R>; the base point geo<256,2,strided,plain,R0> is the library kernel
    const int V4 = V / 4;
    const char *meta_name[] = {"plain", "hoist", "ntload"};
#define GEO(WG, PT, CONTIG, META, RSH) do { if (!(CONTIG) || V4 >= 64 * (PT)) { \
        char nm_[96]; snprintf(nm_, sizeof nm_, "geo<%d,%d,%s,%s,R%d>", WG, PT, CONTIG ? "contig" : "strided", meta_name[META], (RSH) > 0 ? 1 << (RSH) : (RSH)); \
        vs.push_back({nm_, [=](hipStream_t st) { \
            hipLaunchKernelGGL((grad_geo<WG, PT, CONTIG, META>), dim3((unsigned)((n4 + (WG) * (PT) - 1) / ((WG) * (PT)))), dim3(WG), 0, st, \
                               meta, n4, nrows, V4, blank, g4, RSH); }, {}}); } } while (0)
#define GEOS(WG, PT, CONTIG, K) do { if (!(CONTIG) || V4 >= 64 * (PT)) { \
        char nm_[96]; snprintf(nm_, sizeof nm_, "stride<%d,%d,%s,plain> grid=%dxCU", WG, PT, CONTIG ? "contig" : "strided", K); \
        vs.push_back({nm_, [=](hipStream_t st) { \
            const size_t nchunks_ = (n4 + (WG) * (PT) - 1) / ((WG) * (PT)); \
            const size_t grid_ = std::min(nchunks_, (size_t)(K) * ncu); \
            hipLaunchKernelGGL((grad_geo_stride<WG, PT, CONTIG, META_PLAIN>), dim3((unsigned)grid_), dim3(WG), 0, st, \
                               meta, n4, nrows, V4, blank, g4, nchunks_); }, {}}); } } while (0)
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const size_t ncu = (size_t)prop.multiProcessorCount;
    if (V4 >= 64) {
        GEO(256, 2, false, META_PLAIN, 0);                                      // base point
        GEO(256, 2, true, META_PLAIN, 0); GEO(256, 4, true, META_PLAIN, 0);     // wave-contiguous 2 / 4 KiB
        GEO(256, 3, true, META_PLAIN, 0); GEO(256, 8, true, META_PLAIN, 0);
        GEO(512, 2, false, META_PLAIN, 0); GEO(1024, 2, false, META_PLAIN, 0);  // workgroup size
        GEO(256, 3, false, META_PLAIN, 0);                                      // PT = 3
        GEO(256, 4, false, META_PLAIN, 0);
        GEO(256, 2, false, META_PLAIN, 2); GEO(256, 2, false, META_PLAIN, 4); GEO(256, 2, false, META_PLAIN, 6);  // remap R = 4 / 16 / 64
        GEO(256, 2, false, META_HOIST, 0); GEO(256, 2, false, META_NT, 0);      // division hoisting, metadata route
        // combinations of the axes
        GEO(512, 2, true, META_PLAIN, 0); GEO(1024, 2, true, META_PLAIN, 0);
        GEO(512, 4, true, META_PLAIN, 0); GEO(1024, 4, true, META_PLAIN, 0);
        GEO(512, 4, false, META_PLAIN, 0); GEO(1024, 4, false, META_PLAIN, 0);
        GEO(256, 2, true, META_PLAIN, 4); GEO(256, 4, true, META_PLAIN, 4); GEO(512, 2, true, META_PLAIN, 4);
        GEO(512, 2, false, META_PLAIN, 4); GEO(512, 4, true, META_PLAIN, 4);
        GEO(256, 2, true, META_HOIST, 0); GEO(256, 4, true, META_HOIST, 0); GEO(512, 2, true, META_HOIST, 0);
        GEO(256, 2, true, META_NT, 0); GEO(256, 4, true, META_NT, 0);
        // the remap axis further out, and the other axes on top of the remap
        GEO(256, 2, false, META_PLAIN, 5); GEO(256, 2, false, META_PLAIN, 7); GEO(256, 2, false, META_PLAIN, 8);
        GEO(256, 2, false, META_PLAIN, 10); GEO(256, 2, false, META_PLAIN, 12); GEO(256, 2, false, META_PLAIN, 14);
        GEO(256, 2, false, META_PLAIN, -1);
        GEO(256, 2, true, META_PLAIN, 6); GEO(256, 2, true, META_NT, 6); GEO(256, 2, false, META_HOIST, 6);
        GEO(256, 2, false, META_NT, 6); GEO(512, 2, false, META_PLAIN, 6); GEO(256, 4, false, META_PLAIN, 6);
        GEO(256, 4, true, META_PLAIN, 6); GEO(256, 3, false, META_PLAIN, 6); GEO(256, 1, false, META_PLAIN, 6);
        GEO(256, 2, true, META_PLAIN, 8); GEO(512, 2, false, META_PLAIN, 8); GEO(256, 4, true, META_PLAIN, 8);
        // bounded grid, grid-stride (comparison only)
        GEOS(256, 2, false, 4); GEOS(256, 2, false, 8); GEOS(256, 2, false, 16);
        GEOS(256, 2, true, 4); GEOS(256, 2, true, 8); GEOS(256, 2, true, 16);
        GEOS(256, 4, true, 4); GEOS(256, 4, true, 8); GEOS(256, 4, true, 16);
        GEOS(512, 2, true, 8); GEOS(1024, 2, true, 8);
    }

    // correctness: every gradient variant must reproduce the library's tensor bit for bit; one that does not is
    // reported and left out of the timing
    {
        // make the lattice non-trivial: alpha/beta planes = small pseudo-random values
        std::vector<float> h(4 * plane_elems(B, T, U1, false));
        for (size_t i = 0; i < h.size(); ++i) h[i] = -0.001f * (float)((i * 2654435761u) % 4096);
        CK(hipMemcpy(ws, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        float *ref; CK(hipMalloc(&ref, (n + 64) * 4));
        unsigned long long *bad; CK(hipMalloc(&bad, 8));
        CK(hipMemsetAsync(ref, 0xff, (n + 64) * 4, s));
        int rc = pika_rnnt_loss_backward(labels, Tn, Un, B, T, U1, V, blank, nullptr, ws, ref, s);  // fills the metadata too
        if (rc) { printf("lib rc=%d\n", rc); exit(1); }
        std::vector<Variant> keep;
        for (auto &v : vs) {
            if (v.name.find("fill") != std::string::npos || v.name.find("Memset") != std::string::npos) { keep.push_back(v); continue; }
            CK(hipMemsetAsync(grads, 0xff, (n + 64) * 4, s));  // poison (NaN pattern): unwritten elements show up
            CK(hipMemsetAsync(bad, 0, 8, s));
            v.run(s);
            // the 64 floats past the end stay poison on both sides: a write past the end shows up as well
            hipLaunchKernelGGL(diff_kernel, dim3(8192), dim3(256), 0, s, (const unsigned *)grads, (const unsigned *)ref, n + 64, bad);
            unsigned long long hb; CK(hipMemcpy(&hb, bad, 8, hipMemcpyDeviceToHost));
            printf("check %-44s differing words %llu %s\n", v.name.c_str(), hb, hb ? "MISMATCH (not timed)" : "OK");
            if (!hb) keep.push_back(v);
        }
        vs.swap(keep);
        CK(hipFree(ref)); CK(hipFree(bad));
    }
    if (check_only) return 0;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int rounds = 10, reps = 3;
    for (int r = 0; r < rounds; ++r) {
        for (auto &v : vs) {
            v.run(s);  // warm
            CK(hipEventRecord(e0, s));
            for (int k = 0; k < reps; ++k) v.run(s);
            CK(hipEventRecord(e1, s));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            v.ms.push_back(ms / reps);
        }
    }
    printf("tensor %.2f GB (B=%d T=%d U1=%d V=%d)\n", n * 4 / 1e9, B, T, U1, V);
    for (auto &v : vs) {
        std::sort(v.ms.begin(), v.ms.end());
        const float med = v.ms[v.ms.size() / 2], mn = v.ms.front();
        printf("%-44s median %8.3f ms  min %8.3f ms  -> %7.1f GB/s (median)\n", v.name.c_str(), med, mn, n * 4 / (med * 1e-3) / 1e9);
    }
    return 0;
}
