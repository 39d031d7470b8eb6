// pika_amd/csrc/rnnt_loss.hip -- RNN-T loss for gfx950 (MI355X), hand-written HIP.
//
// Replaces the third-party `warp_rnnt` CUDA loss the reference calls at
//   /root/reference/trainer/train_transducer_bmuf_otfaug.py:58,97-99
// (SURVEY.md 8a row 10).  From-scratch CDNA4 design, not a hipify:
//
//   gather    : one wave per anti-diagonal row (lane = u) pulls the TWO log-probs each cell
//               needs (blank, next label) out of the (B,T,U1,V) tensor into two compact planes
//               stored SKEWED: cell (t,u) lives at [t+u][u], so every anti-diagonal is one
//               contiguous row and a wave writes it with one store per plane.
//   alpha/beta: one 64-lane wavefront per utterance and direction walks the anti-diagonals;
//               lane = u, the neighbour term moves one lane with a single DPP wave-shift (no
//               LDS, no barrier); log-probs are prefetched into registers ahead of use (the
//               recurrence is latency-bound).  With one wave, the band of diagonals where every
//               live lane is inside the lattice runs branch-free (see the kernel).
//               Every 16 diagonals the wave subtracts its running maximum and accumulates it
//               in fp64 ("offsets"), so the fp32 lattice values stay O(100) however long the
//               utterance is -- the absolute error of a plain fp32 log-space lattice grows
//               with |alpha| ~ T (ulp(9000) = 1e-3 at the benchmark shape).
//               U1 > 64: one workgroup of up to 16 waves, LDS hand-off at the wave edges.
//   rowmeta   : per lattice cell, the two non-zero gradient values (fp64 offset arithmetic,
//               scaled by autograd's grad_output) + the label index, 16 bytes per cell.
//   grad      : THE HBM-bound kernel -- one flat, address-ordered streaming pass that writes the
//               dense (B,T,U1,V) gradient exactly once with 16-byte stores in 1 KiB-aligned
//               wave transactions; each 16-byte group looks up its row's rowmeta and blends
//               the non-zeros in registers (no memset + scatter, log_probs is not re-read).
//               Measured on MI355X: row-structured writers (a wave or a workgroup per 20 kB
//               V-row) reach only 3.5-4.7 TB/s because rows start on non-128-byte boundaries;
//               the flat form runs at the hipMemsetAsync rate (5.7-5.9 TB/s).
//
//   pruned    : the loss on a banded lattice (B,T,S,V) is the BANDED layout of gather / rowmeta over the same planes and
//               the same alpha/beta, writer and d(logits) kernels; with it the loss of a lattice given by its two
//               planes, its occupation probabilities and the band search (the end of the kernel section).
//   modified  : k2's modified topology is the MOD instantiation of the same layout kernels over un-skewed planes, with
//               its own alpha/beta walker and row centres.
//
// Host side (the end of the file): the kernels first, then ONE host path for all of them.  A `Call` says how a call's
// (rows, V) tensor maps to lattice cells (layout PADDED / PACKED / BANDED, regular or modified topology); dispatch_layout
// turns it into the compile-time pair of the five instantiated combinations; one launcher per kernel family
// (launch_gather, launch_lse_gather, launch_rowmeta, finish_forward) and four bodies (loss_forward, loss_backward,
// fused_forward, fused_backward) serve every layout.  An extern "C" entry is its own argument checks, a Call and a body.
//
// Algorithmic HBM bytes per utterance (T=1000,U1=51,V=5000): 1.020 GB gradient write + ~1.2 MB
// lattice traffic; see DESIGN.md.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <initializer_list>
#include <type_traits>
#include <utility>

#include "pika_rnnt.h"
#include "pika_internal.h"

namespace {

constexpr float NEG = -1.0e30f;  // "log zero": finite, so NEG+NEG / NEG-NEG never make NaN
constexpr float NEG_HALF = -0.5e30f;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int UNR = 8;     // diagonals prefetched per register batch
constexpr int RENORM = 16; // diagonals between renormalisations (multiple of UNR)

typedef float v4f __attribute__((ext_vector_type(4)));

// The wave counts the per-utterance kernels (alpha/beta, alignment) are instantiated for: THE list -- lattice_width
// searches it, dispatch_nw turns a run-time count into the compile-time one.
using Waves = std::integer_sequence<int, 1, 2, 3, 4, 6, 8, 12, 16>;

// Width (in lanes) of one skewed lattice row = threads of the alpha/beta workgroup: the
// smallest instantiated wave count that covers U1 label columns.
template <int... NW>
inline int lattice_width(int U1, std::integer_sequence<int, NW...>) {
    for (int nw : {NW...})
        if (nw * 64 >= U1) return nw * 64;
    return 0;
}
inline int lattice_width(int U1) { return lattice_width(U1, Waves{}); }

// f(std::integral_constant<int, NW>{}) for the instantiated NW == nw; false when there is none
template <class F, int... NW>
inline bool dispatch_nw(int nw, F f, std::integer_sequence<int, NW...>) {
    return ((nw == NW && (f(std::integral_constant<int, NW>{}), true)) || ...);
}
template <class F>
inline bool dispatch_nw(int nw, F f) { return dispatch_nw(nw, f, Waves{}); }

struct RowMeta {  // 16 bytes per lattice cell
    float gb;     // gradient at [.., blank]
    float ge;     // gradient at [.., ye]
    int ye;       // next label, -1 if the cell emits none
    int pad;
};

// The workspace of every call.  mod (the modified topology, below): the planes are not skewed -- cell (t,u) at row t, col u,
// D = T + 1 rows -- and every row has a centre.
struct Lattice {
    float *lpb;    // [B][D][Wp] blank log-prob of cell (t,u) at row t+u, col u
    float *lpe;    // [B][D][Wp] log-prob of emitting y_{u+1} from cell (t,u)
    float *alpha;  // [B][D][Wp] alpha minus off_a[b][row]
    float *beta;   // [B][D][Wp] beta  minus off_b[b][row]
    double *off_a; // [B][D]
    double *off_b; // [B][D]
    double *ll;    // [B] log-likelihood, beta side
    double *ll_a;  // [B] log-likelihood, alpha side (diagnostic)
    RowMeta *meta; // [B*T*U1]
    float *rowc;   // [B][D] row centres; null unless mod
    int Wp, D;
};

inline int lattice_rows(int T, int U1, bool mod) { return mod ? T + 1 : T + U1 - 1; }

inline size_t plane_elems(int B, int T, int U1, bool mod) {
    return (size_t)B * (size_t)lattice_rows(T, U1, mod) * (size_t)lattice_width(U1);
}

inline Lattice carve(void *ws, int B, int T, int U1, bool mod = false) {
    Lattice L;
    const size_t n = plane_elems(B, T, U1, mod);
    L.Wp = lattice_width(U1);
    L.D = lattice_rows(T, U1, mod);
    float *p = static_cast<float *>(ws);
    L.lpb = p;
    L.lpe = p + n;
    L.alpha = p + 2 * n;
    L.beta = p + 3 * n;
    double *q = reinterpret_cast<double *>(p + 4 * n);  // n is a multiple of 64: 8-byte aligned
    L.off_a = q;
    L.off_b = q + (size_t)B * L.D;
    L.ll = q + 2 * (size_t)B * L.D;
    L.ll_a = L.ll + B;
    L.meta = reinterpret_cast<RowMeta *>(L.ll_a + B);  // 2BD+2B doubles: 16-byte aligned
    L.rowc = mod ? reinterpret_cast<float *>(L.meta + (size_t)B * T * U1) : nullptr;
    return L;
}

inline size_t workspace_bytes(int B, int T, int U1, bool mod) {
    const size_t D = (size_t)lattice_rows(T, U1, mod);
    return 4 * plane_elems(B, T, U1, mod) * sizeof(float) +
           (2 * (size_t)B * D + 2 * (size_t)B) * sizeof(double) +
           (size_t)B * T * U1 * sizeof(RowMeta) + (mod ? (size_t)B * D * sizeof(float) : 0);
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// How the (rows, V) tensor of a call maps to lattice cells: the padded (B,T,U1,V) batch, the packed (N, V) rows, or the
// banded (B,T,S,V) rows of a pruned lattice (pika_rnnt.h: row j of frame t is cell (t, s_t + j)).
enum Layout { PADDED = 0, PACKED = 1, BANDED = 2 };

// s_t of a banded call: the frame's entry of `ranges`, clamped so that the band stays inside the utterance's columns
__device__ inline int band_start(const int *__restrict__ ranges, int b, int T, int t, int Un, int S) {
    return clampi(ranges[(size_t)b * T + t], 0, max(0, Un + 1 - S));
}

// log(exp(x)+exp(y)) on the transcendental pipe (v_exp_f32 / v_log_f32).
__device__ inline float lae(float x, float y) {
    const float m = fmaxf(x, y);
    const float d = fminf(x, y) - m;  // <= 0
    return m + LN2 * __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(d * LOG2E));
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ inline float dpp(float v, float fill) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL,
                                                      ROW_MASK, 0xf, false));
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
// gather: (B,T,U1,V) -> two skewed planes.  A wave owns GATHER_ROWS consecutive rows d of one
// utterance and 64 columns u (lane = u), so each plane store is one contiguous 256-byte row piece;
// the lane's label is loaded once for all its rows, and every blank load is issued before the
// first wait.  Cells outside the (Tn, Un+1) sub-lattice (and columns >= U1) get NEG.
// PACKED: log_probs are the (N, V) rows of the packed layout -- cell (t, u) of utterance b is row
// roff[b] + t (Un+1) + u, its label labels[loff[b] + u] -- and the planes are the same as above.
// BANDED: log_probs are (B,T,S,V); cell (t, u) is row (b T + t) S + (u - s_t) when s_t <= u < s_t + S and dead (NEG in
// both planes) otherwise.
// grid = (ceil(D / (4 * GATHER_ROWS)), Wp / 64, B), block = 256.
// ---------------------------------------------------------------------------------------------
constexpr int GATHER_ROWS = 4;

// MOD (the modified topology, below): the planes are NOT skewed -- cell (t, u) lives at [t][u], D = T + 1 rows.
template <int LAYOUT = PADDED, bool MOD = false>
__global__ __launch_bounds__(256) void rnnt_gather_kernel(
    const float *__restrict__ lp, const int *__restrict__ labels, const int *__restrict__ Tn_,
    const int *__restrict__ Un_, int B, int T, int U1, int V, int blank, float *__restrict__ lpb,
    float *__restrict__ lpe, int Wp, int D, const int *__restrict__ roff = nullptr,
    const int *__restrict__ loff = nullptr, const int *__restrict__ ranges = nullptr, int S = 0) {
    constexpr bool PACKED = LAYOUT == Layout::PACKED, BANDED = LAYOUT == Layout::BANDED;
    const int b = blockIdx.z;
    const int d0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * GATHER_ROWS;
    const int u = blockIdx.y * 64 + (threadIdx.x & 63);
    if (d0 >= D) return;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    // row of cell (0, u) and the row step of t
    const size_t r0 = PACKED ? (size_t)roff[b] + u : BANDED ? (size_t)b * T * S : (size_t)b * T * U1 + u;
    const size_t rt = PACKED ? (size_t)(Un + 1) : BANDED ? (size_t)S : (size_t)U1;
    const int *lab = PACKED ? labels + loff[b] : labels + (size_t)b * (U1 - 1);
    const int y = u < Un ? lab[u] : -1;
    const bool emits = y >= 0 && y < V;
    float vb[GATHER_ROWS], ve[GATHER_ROWS];
    if constexpr (BANDED) {
        int j[GATHER_ROWS];  // the band row of cell (t, u); -1: outside the sub-lattice or the band
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) {
            const int t = d0 + r - (MOD ? 0 : u);
            j[r] = -1;
            if (u <= Un && t >= 0 && t < Tn) {
                const int k = u - band_start(ranges, b, T, t, Un, S);
                if (k >= 0 && k < S) j[r] = k;
            }
        }
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) {
            const int t = d0 + r - (MOD ? 0 : u);
            vb[r] = NEG;
            if (j[r] >= 0) vb[r] = fmaxf(lp[(r0 + (size_t)t * rt + j[r]) * V + blank], NEG);
        }
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) {
            const int t = d0 + r - (MOD ? 0 : u);
            ve[r] = NEG;
            if (emits && j[r] >= 0) ve[r] = fmaxf(lp[(r0 + (size_t)t * rt + j[r]) * V + y], NEG);
        }
    } else {
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) {
            const int t = d0 + r - (MOD ? 0 : u);
            vb[r] = NEG;
            if (u <= Un && t >= 0 && t < Tn)
                vb[r] = fmaxf(lp[(r0 + (size_t)t * rt) * V + blank], NEG);
        }
#pragma unroll
        for (int r = 0; r < GATHER_ROWS; ++r) {
            const int t = d0 + r - (MOD ? 0 : u);
            ve[r] = NEG;
            if (emits && t >= 0 && t < Tn)
                ve[r] = fmaxf(lp[(r0 + (size_t)t * rt) * V + y], NEG);
        }
    }
#pragma unroll
    for (int r = 0; r < GATHER_ROWS; ++r) {
        if (d0 + r < D) {
            const size_t o = ((size_t)b * D + d0 + r) * Wp + u;
            lpb[o] = vb[r];
            lpe[o] = ve[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// alpha / beta recurrences.  grid = (2, B): blockIdx.x 0 = alpha, 1 = beta.
// block = NW*64 threads = lattice_width(U1); thread u owns lattice column u.
// ---------------------------------------------------------------------------------------------
template <int NW>
struct Xchg {
    // NW == 1: pure DPP.  NW > 1: DPP inside a wave + LDS hand-off at wave edges.
    float *edge;  // [2][NW+1], edge[.][0] and edge[.][NW] stay NEG
    float *red;   // [2][NW]
    __device__ inline float up(float v, int step) const {  // thread u <- thread u-1
        if constexpr (NW == 1) {
            return wave_shr1(v, NEG);
        } else {
            const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
            float *e = edge + (step & 1) * (NW + 1);
            if (l == 63 && w + 1 < NW) e[w + 1] = v;
            __syncthreads();
            return wave_shr1(v, e[w]);
        }
    }
    __device__ inline float down(float v, int step) const {  // thread u <- thread u+1
        if constexpr (NW == 1) {
            return wave_shl1(v, NEG);
        } else {
            const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
            float *e = edge + (step & 1) * (NW + 1);
            if (l == 0 && w > 0) e[w] = v;
            __syncthreads();
            return wave_shl1(v, e[w + 1]);
        }
    }
    __device__ inline float max_all(float v, int step) const {  // workgroup-wide max
        float m = wave_max(v);
        if constexpr (NW > 1) {
            float *r = red + ((step / RENORM) & 1) * NW;
            if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = m;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NW; ++w) m = fmaxf(m, r[w]);
        }
        return m;
    }
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void rnnt_alpha_beta_kernel(
    const float *__restrict__ lpb_, const float *__restrict__ lpe_, float *__restrict__ alpha_,
    float *__restrict__ beta_, double *__restrict__ off_a_, double *__restrict__ off_b_,
    const int *__restrict__ Tn_, const int *__restrict__ Un_, double *__restrict__ ll_,
    double *__restrict__ ll_a_, float *__restrict__ costs, int T, int U1, int Wp, int D) {
    __shared__ float lds[2 * (NW + 1) + 2 * NW];
    Xchg<NW> xc{lds, lds + 2 * (NW + 1)};
    if constexpr (NW > 1) {
        if (threadIdx.x < 2 * (NW + 1) + 2 * NW) lds[threadIdx.x] = NEG;
        __syncthreads();
    }
    const int b = blockIdx.y;
    const int u = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    const int dend = Tn - 1 + Un;  // last diagonal of the (Tn, Un+1) sub-lattice
    const size_t base = (size_t)b * D * Wp + u;
    const float *lpb = lpb_ + base;
    const float *lpe = lpe_ + base;

    // cell (d-u, u) is inside the sub-lattice
    auto inside = [&](int d) __attribute__((always_inline)) { const int t = d - u; return t >= 0 && t < Tn && u <= Un; };

    float pbv[2][UNR], pev[2][UNR];
    double off = 0.0;  // sum of subtracted maxima (identical in every thread)

    // One wave (NW == 1): for d in [Un, Tn-1] the cell (d-u, u) of every lane u <= Un is inside
    // and lanes u > Un never are.  Whole renormalisation groups of 16 diagonals in that band run
    // a "bulk" loop with no per-step masks or guards: lanes > Un are held at NEG by one
    // loop-invariant select and load column Un (real plane data, never garbage), addresses are a
    // uniform row pointer plus a fixed lane offset, offs[] goes out once per group, and the next
    // group's rows are loaded one step at a time, 16 diagonals ahead.  The masked code below walks
    // the head and the tail; inside-cell arithmetic and renorm points are the same in both.
    // The masked walker is inlined three times per direction (head, tail, and the whole walk when
    // there is no bulk): each copy is straight-line code of ~1k instructions, so the kernel grows
    // by a few KB of instruction cache -- one resident wave per utterance and direction, and the
    // bulk loop it spends ~90 % of its diagonals in is a single ~5 KB body.
    constexpr int G = RENORM;
    constexpr int ROWB = NW * 64 * 4;  // bytes per plane row (Wp == NW * 64)
    const bool live = u <= Un;
    const int lcol = (live ? u : Un) * 4;  // byte offset of the column loaded
    const int scol = u * 4;                // byte offset of the column stored
    // buffer descriptors over this utterance's rows of each plane (uniform: kernargs + blockIdx)
    const size_t plane_b = (size_t)b * D * (NW * 64);
    auto rsrc = [&](const float *plane) __attribute__((always_inline)) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(plane + plane_b), 0, D * ROWB,
                                                 0x00020000);
    };
    auto ldb = [](__amdgpu_buffer_rsrc_t r, int voff, int soff) __attribute__((always_inline)) {
        return __uint_as_float(
            __builtin_amdgcn_raw_buffer_load_b32(r, voff, __builtin_amdgcn_readfirstlane(soff), 0));
    };
    auto stb = [](float v, __amdgpu_buffer_rsrc_t r, int voff, int soff) __attribute__((always_inline)) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff,
                                              __builtin_amdgcn_readfirstlane(soff), 0);
    };
    if (blockIdx.x == 0) {
        // ----- alpha: A_d[u] = lae(A_{d-1}[u] + lpb_{d-1}[u], A_{d-1}[u-1] + lpe_{d-1}[u-1]) -----
        float *alpha = alpha_ + base;
        double *offs = off_a_ + (size_t)b * D;
        float a = (u == 0) ? 0.0f : NEG;
        alpha[0] = a;
        if (u == 0) offs[0] = 0.0;
        auto load = [&](int buf, int d0) __attribute__((always_inline)) {  // rows d0-1 .. d0+UNR-2
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int r = min(d0 + i - 1, D - 1);
                const bool ok = inside(r);
                const float vb = lpb[(size_t)r * Wp], ve = lpe[(size_t)r * Wp];
                pbv[buf][i] = ok ? vb : 0.0f;  // masked: scratch outside the sub-lattice is garbage
                pev[buf][i] = ok ? ve : 0.0f;
            }
        };
        // diagonals d0 .. d0+UNR-1 (<= dlast); d0 = 1 (mod RENORM) at the first half of a group
        auto steps = [&](int buf, int d0, int dlast, auto second_half) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int d = d0 + i;
                if (d <= dlast) {  // workgroup-uniform
                    const float x = a + pbv[buf][i];
                    const float y = xc.up(a + pev[buf][i], d);
                    a = inside(d) ? lae(x, y) : NEG;
                    if (decltype(second_half)::value && i == UNR - 1) {  // d = 0 (mod RENORM)
                        const float m = xc.max_all(a, d);
                        a = a > NEG_HALF ? a - m : NEG;
                        off += (double)m;
                    }
                    alpha[(size_t)d * Wp] = a;
                    if (u == 0) offs[d] = off;
                }
            }
        };
        auto masked = [&](int dfirst, int dlast) __attribute__((always_inline)) {  // dfirst = 1 (mod RENORM)
            load(0, dfirst);
            for (int d0 = dfirst; d0 <= dlast; d0 += 2 * UNR) {
                load(1, d0 + UNR);
                steps(0, d0, dlast, std::false_type{});
                load(0, d0 + 2 * UNR);
                steps(1, d0 + UNR, dlast, std::true_type{});
            }
        };
        // bulk groups [G*g+1, G*g+G]: rows read G*g .. G*g+G-1 >= Un, last diagonal <= Tn-1
        const int g0 = (Un + G - 1) / G, g1 = NW == 1 ? (Tn - 1) / G : 0;
        if (NW == 1 && g1 > g0) {
            masked(1, G * g0);
            const auto rb = rsrc(lpb_), re = rsrc(lpe_), ra = rsrc(alpha_);
            float qb[2][G], qe[2][G];
            auto fetch = [&](int buf, int i, int g) __attribute__((always_inline)) {  // row G*g+i
                qb[buf][i] = ldb(rb, lcol + i * ROWB, G * g * ROWB);
                qe[buf][i] = ldb(re, lcol + i * ROWB, G * g * ROWB);
            };
            // diagonals G*g+1 .. G*g+G from qb/qe[buf]; step i also fetches row i of group g+1
            // (the last group fetches itself again) into 1-buf
            auto group = [&](int buf, int g) __attribute__((always_inline)) {
                const int gn = min(g + 1, g1 - 1);
                const double off0 = off;
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    const float x = a + qb[buf][i];
                    const float y = wave_shr1(a + qe[buf][i], NEG);
                    const float v = lae(x, y);
                    a = live ? v : NEG;
                    if (i == G - 1) {
                        const float m = wave_max(a);
                        a = a > NEG_HALF ? a - m : NEG;
                        off += (double)m;
                    }
                    stb(a, ra, scol + i * ROWB, (G * g + 1) * ROWB);
                    fetch(1 - buf, i, gn);
                    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch where it is
                }
                if (u < G) offs[G * g + 1 + u] = u == G - 1 ? off : off0;
            };
#pragma unroll
            for (int i = 0; i < G; ++i) fetch(0, i, g0);
            group(0, g0);  // peeled: the loop is entered in its steady state of pending loads
            int g = g0 + 1;
            for (; g + 1 < g1; g += 2) {
                group(1, g);
                group(0, g + 1);
            }
            if (g < g1) group(1, g);
            masked(G * g1 + 1, dend);
        } else {
            masked(1, dend);
        }
        if (u == Un) ll_a_[b] = (double)a + off + (double)fmaxf(lpb[(size_t)dend * Wp], NEG);
    } else {
        // ----- beta: B_d[u] = lae(B_{d+1}[u] + lpb_d[u], B_{d+1}[u+1] + lpe_d[u]) -----
        float *beta = beta_ + base;
        double *offs = off_b_ + (size_t)b * D;
        float bt = NEG;
        auto load = [&](int buf, int d0) __attribute__((always_inline)) {  // rows d0, d0-1, ..., d0-UNR+1
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int r = max(d0 - i, 0);
                const bool ok = inside(r);
                const float vb = lpb[(size_t)r * Wp], ve = lpe[(size_t)r * Wp];
                pbv[buf][i] = ok ? vb : 0.0f;
                pev[buf][i] = ok ? ve : 0.0f;
            }
        };
        // diagonals d0, d0-1, ..., d0-UNR+1 (>= dstop); renormalised after every RENORM steps
        // counted from dend (the last step of a second half)
        auto steps = [&](int buf, int d0, int dstop, auto second_half) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int d = d0 - i;
                if (d >= dstop) {
                    const int t = d - u;
                    const float dn = xc.down(bt, d);
                    const float x = bt + pbv[buf][i];
                    const float y = dn + pev[buf][i];
                    float nb = lae(x, y);
                    if (t == Tn - 1 && u == Un) nb = pbv[buf][i];  // terminal blank
                    bt = inside(d) ? nb : NEG;
                    if (decltype(second_half)::value && i == UNR - 1) {
                        const float m = xc.max_all(bt, d);
                        bt = bt > NEG_HALF ? bt - m : NEG;
                        off += (double)m;
                    }
                    beta[(size_t)d * Wp] = bt;
                    if (u == 0) offs[d] = off;
                }
            }
        };
        auto masked = [&](int dfirst, int dstop) __attribute__((always_inline)) {  // dend - dfirst = 0 (mod RENORM)
            load(0, dfirst);
            for (int d0 = dfirst; d0 >= dstop; d0 -= 2 * UNR) {
                load(1, d0 - UNR);
                steps(0, d0, dstop, std::false_type{});
                load(0, d0 - 2 * UNR);
                steps(1, d0 - UNR, dstop, std::true_type{});
            }
        };
        // bulk groups: steps j = dend-d in [G*n, G*n+G-1] with Un <= d <= Tn-1 and j >= 1 (the
        // terminal cell, j = 0, stays in the masked head)
        const int n0 = (max(Un, 1) + G - 1) / G, n1 = NW == 1 ? Tn / G : 0;
        if (NW == 1 && n1 > n0) {
            masked(dend, dend - G * n0 + 1);
            const auto rb = rsrc(lpb_), re = rsrc(lpe_), rbt = rsrc(beta_);
            float qb[2][G], qe[2][G];
            // group n's rows dend-G*n .. dend-G*n-G+1, addressed from its lowest one
            auto fetch = [&](int buf, int i, int n) __attribute__((always_inline)) {  // row dend-G*n-i
                const int r0 = (dend - G * n - (G - 1)) * ROWB;
                qb[buf][i] = ldb(rb, lcol + (G - 1 - i) * ROWB, r0);
                qe[buf][i] = ldb(re, lcol + (G - 1 - i) * ROWB, r0);
            };
            auto group = [&](int buf, int n) __attribute__((always_inline)) {
                const int nn = min(n + 1, n1 - 1);
                const int r0 = (dend - G * n - (G - 1)) * ROWB;
                const double off0 = off;
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    const float dn = wave_shl1(bt, NEG);
                    const float x = bt + qb[buf][i];
                    const float y = dn + qe[buf][i];
                    const float v = lae(x, y);
                    bt = live ? v : NEG;
                    if (i == G - 1) {
                        const float m = wave_max(bt);
                        bt = bt > NEG_HALF ? bt - m : NEG;
                        off += (double)m;
                    }
                    stb(bt, rbt, scol + (G - 1 - i) * ROWB, r0);
                    fetch(1 - buf, i, nn);
                    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch where it is
                }
                if (u < G) offs[dend - G * n - u] = u == G - 1 ? off : off0;
            };
#pragma unroll
            for (int i = 0; i < G; ++i) fetch(0, i, n0);
            group(0, n0);  // peeled: the loop is entered in its steady state of pending loads
            int n = n0 + 1;
            for (; n + 1 < n1; n += 2) {
                group(1, n);
                group(0, n + 1);
            }
            if (n < n1) group(1, n);
            masked(dend - G * n1, 0);
        } else {
            masked(dend, 0);
        }
        if (u == 0) {
            const double ll = (double)bt + off;
            ll_[b] = ll;
            costs[b] = (float)(-ll);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// rowmeta: the two non-zeros of every V-row of the gradient.  The label entry carries the FastEmit
// factor lscale = 1 + lambda (Yu et al. 2021: d/d lp of every emission scaled, costs unchanged);
// 1.0f leaves it exact.  PACKED: row r of the (N, V) packed layout, utterance found by a binary
// search over the row offsets roff (T_n >= 1: strictly increasing).  BANDED: row (b T + t) S + j of the banded layout is
// cell (t, s_t + j); a row past the utterance's last column is zero like a row past its last frame.
// ---------------------------------------------------------------------------------------------
__device__ inline int packed_utterance(const int *__restrict__ roff, int B, long r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (roff[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// What a row's metadata is computed from: the call's labels and lengths, the lattice planes and, per layout, the offsets
// (PACKED) or the band (BANDED).  An instantiation does not read what its layout does not have.
struct MetaArgs {
    const int *labels, *Tn, *Un;
    int B, T, U1, V;
    const float *grad_costs;  // null: ones
    long gc_stride;           // utterance b's factor is grad_costs[b * gc_stride] (0: one expanded scalar)
    const float *lpb, *lpe, *alpha, *beta;
    const double *off_a, *off_b, *ll;
    int Wp, D;
    float lscale;
    const int *roff, *loff;
    long npacked;
    const int *ranges;
    int S;
};

// The metadata of cell (t, u) of utterance b, whose labels are lab: THE definition, for rnnt_rowmeta_kernel (through
// row_meta, which finds the cell of a row) and for the in-place updates that compute it on the way
// (rnnt_grad_rowmeta_update_kernel through row_meta, rnnt_grad_rowmeta_update_frames_kernel from its own (b, t, u)).
// MOD (the modified topology, below): un-skewed planes, both edges of cell (t, u) end in row t + 1 -- the blank edge in
// (t+1, u), the label edge in (t+1, u+1) -- and row T_n is terminal, so the last frame has no special case.
template <bool MOD = false>
__device__ inline RowMeta cell_meta(const MetaArgs &in, int b, int t, int u, const int *__restrict__ lab) {
    const int T = in.T, U1 = in.U1, V = in.V, Wp = in.Wp, D = in.D;
    const float *lpb = in.lpb, *lpe = in.lpe, *alpha = in.alpha, *beta = in.beta, *grad_costs = in.grad_costs;
    const double *off_a = in.off_a, *off_b = in.off_b, *ll = in.ll;
    const float lscale = in.lscale;
    float gb = 0.f, ge = 0.f;
    int ye = -1;
    const int Tn = clampi(in.Tn[b], 1, T), Un = clampi(in.Un[b], 0, U1 - 1);
    if constexpr (MOD) {
        if (t < Tn && u <= Un) {
            const size_t o = ((size_t)b * D + t) * Wp + u;
            const float a = alpha[o];
            const float sc = grad_costs ? grad_costs[b * in.gc_stride] : 1.0f;
            // (ll = +inf where the utterance has no path: every exponent is -inf, every entry zero)
            const float k1 = (float)(off_a[(size_t)b * D + t] - ll[b] + off_b[(size_t)b * D + t + 1]);
            gb = -sc * __expf(k1 + (a + beta[o + Wp] + lpb[o]));
            if (u < Un) {
                const int y = lab[u];
                if (y >= 0 && y < V) {
                    ye = y;
                    ge = -sc * lscale * __expf(k1 + (a + beta[o + Wp + 1] + lpe[o]));
                }
            }
        }
    } else if (t < Tn && u <= Un) {
        const int d = t + u;
        const size_t o = ((size_t)b * D + d) * Wp + u;
        const float a = alpha[o];
        const float sc = grad_costs ? grad_costs[b * in.gc_stride] : 1.0f;
        const double base = off_a[(size_t)b * D + d] - ll[b];
        // exponent = alpha + beta' + lp - ll, with the large parts cancelled in fp64
        const float k1 = (d + 1 < D) ? (float)(base + off_b[(size_t)b * D + d + 1]) : 0.0f;
        if (t < Tn - 1)
            gb = -sc * __expf(k1 + (a + beta[o + Wp] + lpb[o]));
        else if (u == Un)
            gb = -sc * __expf((float)base + (a + lpb[o]));
        if (u < Un) {
            const int y = lab[u];
            if (y >= 0 && y < V) {
                ye = y;
                ge = -sc * lscale * __expf(k1 + (a + beta[o + Wp + 1] + lpe[o]));
            }
        }
    }
    return RowMeta{gb, ge, ye, 0};
}

// the padded layout's labels of utterance b
__device__ inline const int *padded_labels(const MetaArgs &in, int b) { return in.labels + (size_t)b * (in.U1 - 1); }

// The metadata of row `row` (< the layout's row count): the row's cell, then cell_meta.
template <int LAYOUT = PADDED, bool MOD = false>
__device__ inline RowMeta row_meta(const MetaArgs &in, long row) {
    constexpr bool PACKED = LAYOUT == Layout::PACKED, BANDED = LAYOUT == Layout::BANDED;
    const int B = in.B, T = in.T, U1 = in.U1, S = in.S;
    int u, t, b;
    const int *lab;
    if constexpr (PACKED) {
        b = packed_utterance(in.roff, B, row);
        const int w = clampi(in.Un[b], 0, U1 - 1) + 1;
        const int i = (int)(row - in.roff[b]);
        t = i / w;
        u = i - t * w;
        lab = in.labels + in.loff[b];
    } else if constexpr (BANDED) {
        t = (int)((row / S) % T);
        b = (int)(row / ((long)S * T));
        u = (int)(row % S) + band_start(in.ranges, b, T, t, clampi(in.Un[b], 0, U1 - 1), S);
        lab = padded_labels(in, b);
    } else {
        u = (int)(row % U1);
        t = (int)((row / U1) % T);
        b = (int)(row / ((long)U1 * T));
        lab = padded_labels(in, b);
    }
    return cell_meta<MOD>(in, b, t, u, lab);
}

template <int LAYOUT = PADDED, bool MOD = false>
__global__ __launch_bounds__(256) void rnnt_rowmeta_kernel(MetaArgs in, RowMeta *__restrict__ meta) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nrows = LAYOUT == Layout::PACKED ? in.npacked : LAYOUT == Layout::BANDED ? (long)in.B * in.T * in.S
                                                                                       : (long)in.B * in.T * in.U1;
    if (row >= nrows) return;
    meta[row] = row_meta<LAYOUT, MOD>(in, row);
}

// ---------------------------------------------------------------------------------------------
// grad: flat streaming writer.  Thread -> PT 16-byte groups, 256 groups apart, so each wave
// instruction stores one 1 KiB-aligned contiguous KiB and a workgroup one contiguous chunk
// (address order within groups of 512 workgroups, see grad_chunk).  A wave instruction (64 groups) spans at most two V-rows when V/4 >= 64, so both rows'
// metadata arrive through the scalar cache (s_load) and the per-lane work is two compares.
// Hardware A/B (tools/grad_sweep.hip, MI355X, 32.64 GB tensor): PT=2 + scalar metadata 4.65 ms
// (7.0 TB/s) vs per-lane metadata PT=4 5.3 ms, hipMemsetAsync 5.1-5.5 ms, row-structured
// writers 7-9 ms.
// The scalar-metadata writer does not take its 8 KiB chunk straight from blockIdx.x: workgroups
// are dealt to the 8 XCDs round-robin, so under the linear map every XCD writes every eighth chunk.
// grad_chunk permutes each aligned group of 8 * GRAD_RUN workgroups so that workgroups b, b+8,
// b+16, .. take GRAD_RUN consecutive chunks (512 KiB runs).  Same sweep, same tensor: linear 4.72-
// 4.75 ms, runs of 4 chunks 5.4-5.6 (worse), 16: 4.53-4.57, 64 to 16384: 4.50-4.55 (a plateau),
// one eighth of the tensor per residue 4.67.  The map is a bijection on the chunk indices whatever
// the placement is (only the speed rests on it); the last, partial group keeps the linear map, so
// every chunk, the tail's partial one included, is written exactly once.  Workgroup size, PT and
// wave-contiguous spans all lost to 256 threads x PT=2 (DESIGN.md has the table).
// ---------------------------------------------------------------------------------------------
constexpr int GRAD_RUN_SHIFT = 6;  // GRAD_RUN = 64 chunks

// the map itself, for runs of 1 << RUN_SHIFT chunks (shared with the frame runs of rnnt_grad_rowmeta_update_frames_kernel)
template <int RUN_SHIFT>
__device__ inline unsigned xcd_run_chunk(unsigned b, unsigned nblocks) {
    constexpr unsigned gmask = (8u << RUN_SHIFT) - 1;
    if ((b | gmask) >= nblocks) return b;  // the last group is partial: linear
    const unsigned j = b & gmask;
    return (b & ~gmask) | ((j & 7u) << RUN_SHIFT) | (j >> 3);
}

__device__ inline unsigned grad_chunk(unsigned b, unsigned nblocks) { return xcd_run_chunk<GRAD_RUN_SHIFT>(b, nblocks); }

__device__ inline v4f blend_row(int q, int qb, int cb, float gb, float ge, int ye) {
    const int qe = ye >> 2, ce = ye & 3;  // ye = -1 -> qe = -1: never matches
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (q == qb) {
        v.x = cb == 0 ? gb : 0.f; v.y = cb == 1 ? gb : 0.f;
        v.z = cb == 2 ? gb : 0.f; v.w = cb == 3 ? gb : 0.f;
    }
    if (q == qe) {  // label wins if it equals blank (oracle order)
        v.x = ce == 0 ? ge : v.x; v.y = ce == 1 ? ge : v.y;
        v.z = ce == 2 ? ge : v.z; v.w = ce == 3 ? ge : v.w;
    }
    return v;
}

template <bool SCALAR_META, int PT>
__global__ __launch_bounds__(256) void rnnt_grad_kernel(const RowMeta *__restrict__ meta,
                                                        size_t n4, size_t nrows, int V4, int blank,
                                                        v4f *__restrict__ grads) {
    const int qb = blank >> 2, cb = blank & 3;
    if constexpr (SCALAR_META) {  // requires V4 >= 64
        const int lane = threadIdx.x & 63;
        // first group of this wave's first store (wave-uniform, made provably so)
        size_t i0 = (size_t)grad_chunk(blockIdx.x, gridDim.x) * (256 * PT) + (threadIdx.x & ~63);
        i0 = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(i0 >> 32)) << 32) |
             (unsigned)__builtin_amdgcn_readfirstlane((int)i0);
        size_t row0 = i0 / (unsigned)V4;
        int q0 = (int)(i0 - row0 * V4);
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            const size_t i = i0 + lane;
            const size_t r0 = row0 < nrows ? row0 : nrows - 1;
            const size_t r1 = row0 + 1 < nrows ? row0 + 1 : nrows - 1;
            const RowMeta m0 = meta[r0], m1 = meta[r1];  // scalar loads
            int q = q0 + lane;
            const bool second = q >= V4;
            q = second ? q - V4 : q;
            const v4f v = blend_row(q, qb, cb, second ? m1.gb : m0.gb, second ? m1.ge : m0.ge,
                                    second ? m1.ye : m0.ye);
            if (i < n4) grads[i] = v;
            i0 += 256;
            q0 += 256;
            while (q0 >= V4) { q0 -= V4; ++row0; }
        }
    } else {
        size_t i = (size_t)blockIdx.x * (256 * PT) + threadIdx.x;
        size_t row = i / (unsigned)V4;
        int q = (int)(i - row * V4);
#pragma unroll
        for (int k = 0; k < PT; ++k) {
            if (i < n4) {
                const RowMeta m = meta[row];
                grads[i] = blend_row(q, qb, cb, m.gb, m.ge, m.ye);
            }
            i += 256;
            q += 256;
            while (q >= V4) { q -= V4; ++row; }
        }
    }
}

// generic path (V % 4 != 0 or unaligned base): one float per thread-iteration
__global__ __launch_bounds__(256) void rnnt_grad_scalar_kernel(const RowMeta *__restrict__ meta,
                                                               size_t n, int V, int blank,
                                                               float *__restrict__ grads) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t row = i / (unsigned)V;
        const int j = (int)(i - row * V);
        float v = 0.f;
        const RowMeta m = meta[row];
        if (j == blank) v = m.gb;
        if (j == m.ye) v = m.ge;
        grads[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// grad, in place: the tensor already holds a gradient this library wrote -- rows [0, prev_rows) with
// their non-zeros in column prev_blank and column prev_cols[r] (if >= 0), every other word +0.0f, rows
// beyond all +0.0f -- so the new gradient of rows [0, rows) takes the old non-zeros out and puts the
// new ones in: at most four dword stores per row instead of the V-row.  One thread per row over
// max(prev_rows, rows) does both, so no store of one thread depends on another's.  A word gets ONE
// store: the new value where a new entry lands on an old one, +0.0f where only the old one was, and
// none where the new value is +0.0f over a word that is +0.0f already; -0.0f (an underflowed
// -sc * exp(..)) is a value like any other, so the tensor is word for word what the streaming writer
// leaves.  The label wins over blank (blend_row).  cols_out may be prev_cols (read before written).
// ---------------------------------------------------------------------------------------------
// One V-row: its old entries sat in columns ob and oe (-1: none), its new ones are m's (live) or none.
__device__ inline void update_row(float *__restrict__ row, bool live, const RowMeta &m, int blank, int ob, int oe) {
    int cb = -1, ce = -1;   // the columns this row's new entries go to
    float gb = 0.f, ge = 0.f;
    if (live) {
        ce = m.ye;
        ge = m.ge;
        if (m.ye != blank) { cb = blank; gb = m.gb; }
    }
    if (ob >= 0 && ob != cb && ob != ce) row[ob] = 0.f;
    if (oe >= 0 && oe != ob && oe != cb && oe != ce) row[oe] = 0.f;
    if (cb >= 0 && (cb == ob || cb == oe || __float_as_uint(gb) != 0u)) row[cb] = gb;
    if (ce >= 0 && (ce == ob || ce == oe || __float_as_uint(ge) != 0u)) row[ce] = ge;
}

__global__ __launch_bounds__(256) void rnnt_grad_update_kernel(const RowMeta *__restrict__ meta, long rows, int V,
                                                               int blank, const int *prev_cols, long prev_rows,
                                                               int prev_blank, float *__restrict__ grads, int *cols_out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool had = r < prev_rows, live = r < rows;
    if (!had && !live) return;
    const int oe = had ? prev_cols[r] : -1;
    RowMeta m{0.f, 0.f, -1, 0};
    if (live) m = meta[r];
    update_row(grads + (size_t)r * V, live, m, blank, had ? prev_blank : -1, oe);
    if (live) cols_out[r] = m.ye;
}

// The same update with the row metadata computed on the way (padded layout, regular topology): a row of this call gets
// its RowMeta from row_meta, stores it -- the workspace stays complete for the readers of the compact gradient -- and
// updates its V-row from the registers.  The plane loads and the two exponentials of a wave run under the scattered
// stores of the others, so the backward over a reused tensor is this one launch.  Workgroups of 512: measured at the
// benchmark shape against 64 / 128 / 256 threads and 2 / 4 rows per thread (DESIGN.md has the table).  This is the
// linear map, row = workgroup * 512 + thread, with row_meta's divisions: what runs when more than 512 columns, or the
// tail of a far larger earlier gradient, keep a call off the frame map below.
constexpr int UPDATE_FUSED_THREADS = 512;

__global__ __launch_bounds__(UPDATE_FUSED_THREADS) void rnnt_grad_rowmeta_update_kernel(
    MetaArgs in, RowMeta *__restrict__ meta, long rows, int blank, const int *prev_cols, long prev_rows, int prev_blank,
    float *__restrict__ grads, int *cols_out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool had = r < prev_rows, live = r < rows;
    if (!had && !live) return;
    const int oe = had ? prev_cols[r] : -1;
    RowMeta m{0.f, 0.f, -1, 0};
    if (live) meta[r] = m = row_meta<>(in, r);
    update_row(grads + (size_t)r * in.V, live, m, blank, had ? prev_blank : -1, oe);
    if (live) cols_out[r] = m.ye;
}

// The same kernel with a thread-to-row map that needs no division by a run-time number: a workgroup with
// blockIdx.y < B owns F = UPDATE_FUSED_THREADS / U1 consecutive frames of utterance blockIdx.y (U1 <= the workgroup), thread
// i < F * U1 is cell (t0 + i / U1, i % U1), and i / U1 is a multiply by the host's recip = ceil(2^20 / U1) and a shift
// (exact for i < 512 and U1 <= 512: 512 * (recip * U1 - 2^20) < 512 * 512 < 2^20).  Threads past F * U1, and past frame T
// in an utterance's last workgroup, have no row.  Rows [rows, prev_rows) of a larger earlier gradient belong to no
// utterance of this call: the workgroups with blockIdx.y >= B take them, 512 consecutive rows each.  So every row below
// max(prev_rows, rows) has exactly one thread, as in the linear map, and no store of one thread depends on another's.
// The frame chunk of a workgroup is not blockIdx.x itself: a line of the lattice planes (32 columns of one diagonal) is
// read by 32 consecutive frames, that is by three or four consecutive chunks at the benchmark shape, and under the
// linear map those run on different XCDs, each of which pulls the line into its own L2.  xcd_run_chunk hands the
// workgroups blockIdx.x, blockIdx.x + 8, .. (one XCD, whatever the row's first one is) runs of 1 << FRAME_RUN_SHIFT
// consecutive chunks of the utterance; a bijection for any grid, the partial last group linear.
struct FrameMap {
    int F;           // frames per workgroup
    unsigned recip;  // ceil(2^20 / U1)
};

constexpr int FRAME_RUN_SHIFT = 2;  // runs of 4 frame chunks

__global__ __launch_bounds__(UPDATE_FUSED_THREADS) void rnnt_grad_rowmeta_update_frames_kernel(
    MetaArgs in, RowMeta *__restrict__ meta, FrameMap fm, long rows, int blank, const int *prev_cols, long prev_rows,
    int prev_blank, float *__restrict__ grads, int *cols_out) {
    const unsigned i = threadIdx.x;
    const bool live = blockIdx.y < (unsigned)in.B;
    long r;
    int t = 0, u = 0;
    if (live) {
        const unsigned f = (i * fm.recip) >> 20;
        t = (int)(xcd_run_chunk<FRAME_RUN_SHIFT>(blockIdx.x, gridDim.x) * (unsigned)fm.F + f);
        u = (int)(i - f * (unsigned)in.U1);
        if (f >= (unsigned)fm.F || t >= in.T) return;
        r = ((long)blockIdx.y * in.T + t) * in.U1 + u;
    } else {
        r = rows + ((long)(blockIdx.y - (unsigned)in.B) * gridDim.x + blockIdx.x) * UPDATE_FUSED_THREADS + i;
        if (r >= prev_rows) return;
    }
    const bool had = r < prev_rows;
    const int oe = had ? prev_cols[r] : -1;
    RowMeta m{0.f, 0.f, -1, 0};
    if (live) meta[r] = m = cell_meta<>(in, (int)blockIdx.y, t, u, padded_labels(in, (int)blockIdx.y));
    update_row(grads + (size_t)r * in.V, live, m, blank, had ? prev_blank : -1, oe);
    if (live) cols_out[r] = m.ye;
}

// the label column of every row (-1: none), beside a tensor the streaming writer has written
__global__ __launch_bounds__(256) void rnnt_grad_cols_kernel(const RowMeta *__restrict__ meta, long rows,
                                                             int *__restrict__ cols_out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) cols_out[r] = meta[r].ye;
}

__global__ __launch_bounds__(256) void rnnt_export_kernel(
    const float *__restrict__ alpha, const float *__restrict__ beta, const double *__restrict__ off_a,
    const double *__restrict__ off_b, const int *__restrict__ Tn_, const int *__restrict__ Un_,
    int B, int T, int U1, int Wp, int D, float *__restrict__ out_a, float *__restrict__ out_b) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * T * U1) return;
    const int u = (int)(idx % U1);
    const int t = (int)((idx / U1) % T);
    const int b = (int)(idx / ((size_t)U1 * T));
    const size_t o = ((size_t)b * D + (t + u)) * Wp + u;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    const bool ok = t < Tn && u <= Un;
    if (out_a) out_a[idx] = ok ? (float)((double)alpha[o] + off_a[(size_t)b * D + t + u]) : NEG;
    if (out_b) out_b[idx] = ok ? (float)((double)beta[o] + off_b[(size_t)b * D + t + u]) : NEG;
}

// the lattice alone (the calls that take no vocabulary) ...
int check_lattice_dims(int B, int T, int U1) {
    if (B <= 0 || T <= 0 || U1 <= 0) return PIKA_EINVAL;
    if (U1 > 1024) return PIKA_ETOOBIG;
    return PIKA_OK;
}

// ... and with V and blank: a bad V or blank is PIKA_EINVAL even where U1 > 1024 would be PIKA_ETOOBIG
int check_dims(int B, int T, int U1, int V, int blank) {
    if (V <= 0 || blank < 0 || blank >= V) return PIKA_EINVAL;
    return check_lattice_dims(B, T, U1);
}

// B*T*U1 rows (N packed) index the row kernels as an int
constexpr long long ROWS_MAX = 0x7fffffffLL;

// ---------------------------------------------------------------------------------------------
// forced alignment: the max-plus (Viterbi) recurrence over the same skewed planes,
//   delta_d[u] = max(delta_{d-1}[u] + lpb_{d-1}[u], delta_{d-1}[u-1] + lpe_{d-1}[u-1]),
// one workgroup per utterance, lane = u, the neighbour term by Xchg<NW>::up as in the alpha sweep.
// Plain fp32 accumulation: max picks one of its operands, so a cell's value is the fp32 running sum
// of ONE path's edges -- T_n + U_n rounded additions, no transcendental, nothing to renormalise.
// The decision of a cell (1 = came over the emission edge from (t, u-1); a tie is 0, the blank
// predecessor) is one __ballot bit: row d of the back-pointers is NW 64-bit words, written to the
// LDS buffer by lane 0 of every wave when the utterance's T_n+U_n-1 rows fit its ALIGN_WORDS / NW
// (the benchmark's 1049 do), to the caller's scratch otherwise.  Back-trace, same workgroup: thread 0
// walks the rows from (T_n-1, U_n) down; rows in scratch are staged through LDS a chunk at a time.  Every step lowers d = t + u by one, so the row read
// does not depend on the walk (for NW == 1 the loads of an unrolled batch all issue at once) and
// only the column u is carried.  u == 0 forces the blank edge and t == 0 the emission edge (the sweep
// writes both into the bits), so the walk stays inside the sub-lattice and ends in (0, 0) whatever
// the planes hold (a label outside [0, V) leaves NEG there).
// grid = B, block = NW * 64.  frames: (B, U1-1) padded with -1, or -- loff given -- utterance b's
// U_n entries at frames + loff[b].
// ---------------------------------------------------------------------------------------------
constexpr int ALIGN_WORDS = 1536;  // 12 KB of LDS; a multiple of every instantiated NW
constexpr int AUNR = 8;            // diagonals prefetched per register batch of the alignment sweep

template <int NW>
__global__ __launch_bounds__(NW * 64) void rnnt_align_kernel(
    const float *__restrict__ lpb_, const float *__restrict__ lpe_, const int *__restrict__ Tn_,
    const int *__restrict__ Un_, const int *__restrict__ loff, float *__restrict__ scores,
    int *__restrict__ frames, unsigned long long *__restrict__ bp_, int T, int U1, int Wp, int D) {
    __shared__ float lds[2 * (NW + 1) + 2 * NW];
    __shared__ unsigned long long bits[ALIGN_WORDS];
    __shared__ int fr[NW * 64 + 1];
    Xchg<NW> xc{lds, lds + 2 * (NW + 1)};
    if constexpr (NW > 1) {
        if (threadIdx.x < 2 * (NW + 1) + 2 * NW) lds[threadIdx.x] = NEG;
        __syncthreads();
    }
    const int b = blockIdx.x;
    const int u = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    const int dend = Tn - 1 + Un;
    const size_t base = (size_t)b * D * Wp + u;
    const float *lpb = lpb_ + base;
    unsigned long long *bp = bp_ + (size_t)b * D * NW;  // row d: bp[d * NW + wave]
    // an utterance whose dend rows fit the LDS buffer keeps them there (row d at bits[(d-1) * NW + wave]): no global
    // store shares the loads' counter in the sweep, and the walk needs no staging
    constexpr int ROWS = ALIGN_WORDS / NW;
    const bool fits = dend <= ROWS;  // workgroup-uniform

    // Rows come in by buffer loads at a uniform row offset plus the lane's fixed column (a row past the planes reads
    // 0), unmasked: the planes hold garbage outside the sub-lattice, but a cell inside it never consumes any -- its
    // value is selected by the decision bit, which the borders force, and both operands of an interior cell come
    // from cells inside.
    constexpr int ROWB = NW * 64 * 4;  // bytes per plane row (Wp == NW * 64)
    const size_t plane_b = (size_t)b * D * (NW * 64);
    const auto rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(lpb_ + plane_b), 0, D * ROWB, 0x00020000);
    const auto re = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(lpe_ + plane_b), 0, D * ROWB, 0x00020000);
    float pbv[2][AUNR], pev[2][AUNR];
    float v = (u == 0) ? 0.0f : NEG;
    auto load = [&](int buf, int d0) __attribute__((always_inline)) {  // rows d0-1 .. d0+AUNR-2
        const int soff = __builtin_amdgcn_readfirstlane((d0 - 1) * ROWB);
#pragma unroll
        for (int i = 0; i < AUNR; ++i) {
            pbv[buf][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, u * 4 + i * ROWB, soff, 0));
            pev[buf][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(re, u * 4 + i * ROWB, soff, 0));
        }
    };
    // (bitwise & and |: no exec-mask branches in the dependent chain; the compare that makes the bit also selects the
    //  maximum; the eight words of a batch go out under one lane-0 branch)
    const bool live = u <= Un;
    auto steps = [&](int buf, int d0) __attribute__((always_inline)) {  // diagonals d0 .. d0+AUNR-1 (<= dend)
        unsigned long long m[AUNR];
#pragma unroll
        for (int i = 0; i < AUNR; ++i) {
            const int d = d0 + i;
            if (d <= dend) {  // workgroup-uniform
                const float x = v + pbv[buf][i];
                const float y = xc.up(v + pev[buf][i], d);
                // a tie is the blank predecessor; u == 0 has no emission edge and t == 0 no blank one, whatever the
                // values say
                const bool emit = (u > 0) & ((y > x) | (d == u));
                m[i] = __ballot(emit);
                const bool in = ((unsigned)(d - u) < (unsigned)Tn) & live;
                v = in ? (emit ? y : x) : NEG;
            }
        }
        if ((u & 63) == 0) {
#pragma unroll
            for (int i = 0; i < AUNR; ++i)
                if (d0 + i <= dend) {
                    if (fits) bits[(d0 + i - 1) * NW + (u >> 6)] = m[i];
                    else bp[(size_t)(d0 + i) * NW + (u >> 6)] = m[i];
                }
        }
    };
    load(0, 1);
    for (int d0 = 1; d0 <= dend; d0 += 2 * AUNR) {
        load(1, d0 + AUNR);
        steps(0, d0);
        load(0, d0 + 2 * AUNR);
        steps(1, d0 + AUNR);
    }
    if (u == Un) scores[b] = v + fmaxf(lpb[(size_t)dend * Wp], NEG);

    // back-trace.  The sweep already forced the two borders into the bits, so a step is
    //   e = bit(d, cu);  fr[cu] = d - cu;  cu -= e
    // with no branch: the last value a column c >= 1 receives is the frame at which the walk leaves it over
    // the emission edge, which is emit_frames[c - 1]; the workgroup copies fr out at the end.
    int cu = Un;  // thread 0: the walk's column; its cell on diagonal d is (d - cu, cu)
    for (int dhi = dend; dhi >= 1; dhi -= ROWS) {  // workgroup-uniform
        const int dlo = max(dhi - ROWS + 1, 1);
        __syncthreads();  // the sweep's rows are written; the previous chunk is walked
        if (!fits) {
            for (int i = threadIdx.x; i < (dhi - dlo + 1) * NW; i += NW * 64) bits[i] = bp[(size_t)dlo * NW + i];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
#pragma unroll 8
            for (int d = dhi; d >= dlo; --d) {
                const unsigned long long w = bits[(d - dlo) * NW + (NW == 1 ? 0 : cu >> 6)];
                fr[cu] = d - cu;
                cu -= (int)((w >> (cu & 63)) & 1ull);
            }
        }
    }
    __syncthreads();
    int *out = loff ? frames + loff[b] : frames + (size_t)b * (U1 - 1);
    if (u < Un) out[u] = fr[u + 1];
    else if (!loff && u < U1 - 1) out[u] = -1;
}

// d(logits) of log_softmax(scale * logits) under the RNN-T gradient WITHOUT reading the dense gradient:
// row r of it has at most two non-zeros, kept in meta[r] by the backward call; with s = gb + ge
//   out[r, v] = scale * ((v == blank) * gb + (v == ye) * ge - exp(lp[r, v]) * s)      (bf16, zero-padded)
// One wavefront per row (V <= 64*4*CQ, V % 4 == 0), 16-byte loads, 8-byte stores.  CQ = 20 (V <= 5120: the 80 row
// registers the benchmarked V = 5000 needs) or 32 (V <= 8192: the shipped recipes' own vocabulary is 6268,
// egs/train_transducer_bmuf_otfaug.sh:37).
constexpr int CQ_MAX = 32, V_MAX = 64 * 4 * CQ_MAX;
#define PIKA_CQ(extent, CALL) do { if ((extent) <= 64 * 4 * 20) { constexpr int CQ = 20; CALL; } else { constexpr int CQ = 32; CALL; } } while (0)
// Rows a wave of the column-summing d(logits) kernels walks before its column sums go out (one atomicAdd per column and
// workgroup): as many as still leave two workgroups per CU.  (It was 64 from 2^18 rows on and 4 below: the recipes' own
// lattice -- 8 utterances, 97 920 rows -- issued 38 M atomics per pass and ran at 1.5 TB/s, 1.62 ms; now 0.5.)
inline int rows_per_wave(long long rows) {
    const long long r = rows / (4 * 2 * 256);
    return (int)(r < 4 ? 4 : (r > 64 ? 64 : r));
}
typedef __bf16 cbf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// COLSUM: every wave walks RPW consecutive rows and keeps the column sums of what it writes in registers
// (d(bias) of the layer that produced the logits); the four waves of a workgroup combine through LDS and issue one
// atomicAdd per column.
// The logits arrive as fp32 (TI = float) or as the fp16 matrix of pika_gemm_bf16_nt_lse_f16 (TI = _Float16, row pitch
// ld_in): half the bytes of the pass's input.
typedef _Float16 ch16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 ch16x8 __attribute__((ext_vector_type(8)));
__device__ inline f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ inline f32x4 ld4(const _Float16 *p) { return __builtin_convertvector(*reinterpret_cast<const ch16x4 *>(p), f32x4); }

template <bool COLSUM, typename TI, int CQ>
__global__ __launch_bounds__(256) void rnnt_dlogits_compact_kernel(const TI *__restrict__ lp,
                                                                   const RowMeta *__restrict__ meta,
                                                                   __bf16 *__restrict__ out, long long rows,
                                                                   int V, long long ld_out, int blank,
                                                                   float scale, int rpw,
                                                                   float *__restrict__ colsum,
                                                                   const float *__restrict__ lse,
                                                                   long long ld_in,
                                                                   const float *__restrict__ gathered,
                                                                   const int *__restrict__ g_labels,
                                                                   int g_blank, int T, int U1) {
    if (ld_in == 0) ld_in = V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c4 = V >> 2, o4 = (int)(ld_out >> 2);
    const long long r0 = ((long long)blockIdx.x * 4 + wave) * rpw;
    f32x4 cs[COLSUM ? CQ : 1];
    if constexpr (COLSUM) {
#pragma unroll
        for (int q = 0; q < CQ; ++q) cs[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (long long r = r0; r < r0 + rpw && r < rows; ++r) {
        const RowMeta m = meta[r];
        const float s = m.gb + m.ge;
        const float l = lse ? lse[r] : 0.f;   // `lp` holds raw logits: log-prob = logit - log-sum-exp of its row
        const TI *lrow = lp + r * ld_in;
        cbf16x4 *orow = reinterpret_cast<cbf16x4 *>(out + r * ld_out);
        // rows outside an utterance's sub-lattice carry no gradient and, when `lp` holds raw logits, no defined
        // log-sum-exp: their exp() must not reach the output (inf * 0).  The row is fetched regardless -- making
        // the loads wait for the metadata would serialise two memory latencies per row.
        const bool live = (m.gb != 0.f) || (m.ge != 0.f);
        // (the gathered pair of a row belongs to column g_blank and to the label the PRODUCT was given for it: used where they
        // are the loss' blank and label)
        const bool use_gb = gathered && g_blank == blank;
        bool use_ge = false;
        if (gathered && m.ye >= 0) {
            const int u = (int)(r % U1);
            const long long b_ = r / ((long long)T * U1);
            use_ge = u < U1 - 1 && g_labels[b_ * (U1 - 1) + u] == m.ye;
        }
        f32x4 v[CQ];
#pragma unroll
        for (int q = 0; q < CQ; ++q)
            if (lane + q * 64 < c4) v[q] = ld4(lrow + 4 * (lane + q * 64));
#pragma unroll
        for (int q = 0; q < CQ; ++q) {
            const int i = lane + q * 64;
            if (i < c4) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (live) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = 4 * i + e;
                        float g = col == blank ? m.gb : 0.f;
                        if (col == m.ye) g += m.ge;
                        float x = v[q][e];
                        // the two columns whose gradient carries the loss' own terms: their logits in fp32 (the forward
                        // product's epilogue kept them) instead of the fp16 copy -- 2^-11 of |logit| is percents of a softmax
                        if (use_gb && col == blank) x = gathered[2 * r];
                        if (use_ge && col == m.ye) x = gathered[2 * r + 1];
                        o[e] = scale * (g - __expf(x - l) * s);
                    }
                }
                orow[i] = __builtin_convertvector(o, cbf16x4);
                if constexpr (COLSUM) cs[q] += o;
            } else if (i < o4) {
                orow[i] = cbf16x4{(__bf16)0.f, (__bf16)0.f, (__bf16)0.f, (__bf16)0.f};
            }
        }
    }
    if constexpr (COLSUM) {
        __shared__ f32x4 red[4][64];
#pragma unroll
        for (int q = 0; q < CQ; ++q) {
            if (q * 64 >= c4) break;          // uniform
            __syncthreads();
            red[wave][lane] = cs[q];
            __syncthreads();
            const int i = lane + q * 64;
            if (wave == 0 && i < c4) {
                const f32x4 t = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
                atomicAdd(colsum + 4 * i + 0, t.x); atomicAdd(colsum + 4 * i + 1, t.y);
                atomicAdd(colsum + 4 * i + 2, t.z); atomicAdd(colsum + 4 * i + 3, t.w);
            }
        }
    }
}


// The same on 8-column granules (V % 8 == 0, ld_out % 8 == 0, V <= 512 * NIT): a lane loads two adjacent 16-byte
// groups and stores ONE 16-byte bf16 granule, nothing of the row is staged in registers (the row log-sum-exp is
// known: every element is one fma + exp2 + mul), and the two special columns of a row are patched under
// wave-uniform tests instead of two compares per element -- a third of the instructions of the kernel above, 120
// registers instead of 289 (one wave per SIMD before), so the loads of several rows are in flight per CU.
typedef __bf16 cbf16x8 __attribute__((ext_vector_type(8)));
template <int NIT, typename TI = float>
__global__ __launch_bounds__(256) void rnnt_dlogits_compact8_kernel(const TI *__restrict__ lp,
                                                                    const RowMeta *__restrict__ meta,
                                                                    __bf16 *__restrict__ out, long long rows,
                                                                    int V, long long ld_out, int blank,
                                                                    float scale, int rpw,
                                                                    float *__restrict__ colsum,
                                                                    const float *__restrict__ lse,
                                                                    long long ld_in,
                                                                    const float *__restrict__ gathered,
                                                                    const int *__restrict__ g_labels,
                                                                    int g_blank, int T, int U1) {
    if (ld_in == 0) ld_in = V;
    constexpr float LOG2E = 1.4426950408889634f;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long r0 = ((long long)blockIdx.x * 4 + wave) * rpw;
    float cs[NIT][8];
#pragma unroll
    for (int it = 0; it < NIT; ++it)
#pragma unroll
        for (int e = 0; e < 8; ++e) cs[it][e] = 0.f;
    const int gb_lane = (blank >> 3) & 63;                       // the lane that stores the granule of the blank column
    float cs_blank = 0.f;
    for (long long r = r0; r < r0 + rpw && r < rows; ++r) {
        const RowMeta m = meta[r];
        const float ssum = m.gb + m.ge;
        const bool live = (m.gb != 0.f) || (m.ge != 0.f);       // wave-uniform; dead rows are zeros (see above)
        const float nl2 = lse ? -lse[r] * LOG2E : 0.f;
        const float k = -scale * ssum;
        const TI *lrow = lp + r * ld_in;
        __bf16 *orow = out + r * ld_out;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int c = (lane + 64 * it) * 8;
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
            if (live) {
                const TI *src = lrow + (c < V ? c : 0);          // always a valid address; the store is guarded
                f32x4 a, b2;
                if constexpr (sizeof(TI) == 2) {                 // one 16-byte load carries the eight columns
                    const ch16x8 h = *reinterpret_cast<const ch16x8 *>(src);
                    a = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                    b2 = f32x4{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
                } else {
                    a = ld4(src);
                    b2 = ld4(src + 4);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = k * __builtin_amdgcn_exp2f(__builtin_fmaf(a[e], LOG2E, nl2));
                    o[4 + e] = k * __builtin_amdgcn_exp2f(__builtin_fmaf(b2[e], LOG2E, nl2));
                }
            }
            if (c < V) {
                if (c + 8 > V) {            // V % 8 == 4: the last granule holds four columns and four of the pitch's padding
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = c + e < V ? o[e] : 0.f;
                }
                cbf16x8 w;
#pragma unroll
                for (int e = 0; e < 8; ++e) w[e] = (__bf16)o[e];
                *reinterpret_cast<cbf16x8 *>(orow + c) = w;
#pragma unroll
                for (int e = 0; e < 8; ++e) cs[it][e] += o[e];
            } else if (c < ld_out) {
                cbf16x8 z;
#pragma unroll
                for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.f;
                *reinterpret_cast<cbf16x8 *>(orow + c) = z;
            }
        }
        // the (at most two) columns that carry an extra term: the lane that stored their granule stores the element
        // again (same thread, same address: program order), their share of the column sums goes in separately
        if (live) {
            // (their logits in fp32 where the forward product's epilogue kept them: `gathered`; the fp16 copy is 2^-11 of
            // |logit| off, percents of a softmax value at |logit| ~ 30 -- and these two entries carry the gradient's own terms.
            // The column sums took the bulk value above: they get the difference.  Patched in every live row, also where
            // the row's own term is zero -- gb on the last frame -- since the softmax part still takes the fp32 logit.)
            if (lane == gb_lane) {
                const float vb = k * __builtin_amdgcn_exp2f(__builtin_fmaf((float)lrow[blank], LOG2E, nl2));
                const float v = (gathered && g_blank == blank) ? k * __builtin_amdgcn_exp2f(__builtin_fmaf(gathered[2 * r], LOG2E, nl2)) : vb;
                orow[blank] = (__bf16)(v + scale * m.gb);
                cs_blank += scale * m.gb + (v - vb);
            }
            const int ye = m.ye;
            if (ye >= 0 && lane == ((ye >> 3) & 63)) {
                const float vb = k * __builtin_amdgcn_exp2f(__builtin_fmaf((float)lrow[ye], LOG2E, nl2));
                // (the gathered label logit belongs to the label the PRODUCT was given for this row: used where it is the loss')
                const int u = (int)(r % U1);
                const bool mine = gathered && u < U1 - 1 && g_labels[(r / ((long long)T * U1)) * (U1 - 1) + u] == ye;
                const float v = mine ? k * __builtin_amdgcn_exp2f(__builtin_fmaf(gathered[2 * r + 1], LOG2E, nl2)) : vb;
                float add = scale * m.ge;
                if (ye == blank && m.gb != 0.f) add += scale * m.gb;         // never in practice (labels > blank)
                orow[ye] = (__bf16)(v + add);
                atomicAdd(colsum + ye, scale * m.ge + (v - vb));
            }
        }
    }
    __shared__ float red[4][64][9];      // pitch 9: the 8 floats of a lane never share a bank with its neighbour's
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const bool any = it * 512 < V;    // uniform
        __syncthreads();
        if (any) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[wave][lane][e] = cs[it][e];
        }
        __syncthreads();
        const int c = (lane + 64 * it) * 8;
        if (any && wave == 0 && c < V) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c + e < V)
                    atomicAdd(colsum + c + e, (red[0][lane][e] + red[1][lane][e]) + (red[2][lane][e] + red[3][lane][e]));
        }
    }
    if (cs_blank != 0.f) atomicAdd(colsum + blank, cs_blank);
}

// The arguments of a padded forward: the dimensions; then own_ok -- the entry point's own tests of its pointers, V and
// pitches -- and the labels when some utterance can have one (PIKA_EINVAL); then, for the calls whose kernels index the
// B*T*U1 rows as an int (`rows` given), the row count (PIKA_ETOOBIG).
int forward_args_ok(int B, int T, int U1, int V, int blank, bool own_ok, const int *labels, long long *rows = nullptr) {
    if (int rc = check_dims(B, T, U1, V, blank)) return rc;
    if (!own_ok || (U1 > 1 && !labels)) return PIKA_EINVAL;
    if (rows && (*rows = (long long)B * T * U1) > ROWS_MAX) return PIKA_ETOOBIG;
    return PIKA_OK;
}

// fp32 logits as the one-wave-per-row kernels read them: 16-byte groups, the row in registers
bool logits_ok(const float *logits, int V) {
    return !(V & 3) && V <= V_MAX && !(reinterpret_cast<uintptr_t>(logits) & 15);
}

// The 8-column d(logits) kernel takes fp32 input in whole 8-column granules ...
bool compact8_ok_f32(int V, long long ld_out, const void *out) {
    return !(V & 7) && !(ld_out & 7) && V > 512 * 9 && !(reinterpret_cast<uintptr_t>(out) & 15);
}

// ... and fp16 input on a pitch of whole granules (V % 8 == 4 -- the shipped recipes' 6268 -- rides on it: the last
// granule is masked)
bool compact8_ok_f16(int V, long long ld_out, long long ld_in, const void *out, const void *logits16) {
    return !(ld_out & 7) && !(ld_in & 7) && ld_in >= ((V + 7) & ~7) && V > 512 * 9 &&
           !(reinterpret_cast<uintptr_t>(out) & 15) && !(reinterpret_cast<uintptr_t>(logits16) & 15);
}

// The compact d(logits) pass of both input types, after the entry point's own checks.  ld_in 0: the rows of `x` are V
// apart; wide: the 8-column kernel may take the column-summing form (compact8_ok_*).
template <typename TI>
int launch_dlogits_compact(const TI *x, long long ld_in, bool wide, const float *lse, const void *workspace, int B, int T,
                           int U1, int V, int blank, void *out, long long ld_out, float scale, float *colsum,
                           const float *gathered, const int *g_labels, int g_blank, void *stream) {
    const Lattice L = carve(const_cast<void *>(workspace), B, T, U1);
    const long long rows = (long long)B * T * U1;
    if (rows > ROWS_MAX) return PIKA_ETOOBIG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    __bf16 *o = static_cast<__bf16 *>(out);
    if (!colsum) {
        PIKA_CQ(ld_out, hipLaunchKernelGGL((rnnt_dlogits_compact_kernel<false, TI, CQ>), dim3((unsigned)((rows + 3) / 4)),
                                           dim3(256), 0, s, x, L.meta, o, rows, V, ld_out, blank, scale, 1, colsum, lse, ld_in,
                                           gathered, g_labels, g_blank, T, U1));
        return (int)hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(colsum, 0, (size_t)V * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    static const int rpw_env = [] { const char *e = pika_knob("PIKA_DLOGITS_RPW"); return e ? atoi(e) : 0; }();   // A/B
    // tools/dlogits_bench.py at the config-2 lattice: 16 rows per wave 2.43 ms, 32: 2.35, 64: 2.31, 128: 2.31, 256: 2.57;
    // the 4- and 8-column kernels tie (2.35 ms): the pass is the mixed read / write HBM stream at 5.0-5.1 TB/s
    const int rpw = rpw_env > 0 ? rpw_env : rows_per_wave(rows);
    const dim3 grid((unsigned)((rows + 4LL * rpw - 1) / (4LL * rpw)));
    static const bool wide_off = pika_knob("PIKA_DLOGITS_NARROW") != nullptr;     // A/B: the 4-column kernel
    if (wide && !wide_off) {
#define PIKA_C8(NIT) hipLaunchKernelGGL((rnnt_dlogits_compact8_kernel<NIT, TI>), grid, dim3(256), 0, s, x, L.meta, o, rows, V, \
                                        ld_out, blank, scale, rpw, colsum, lse, ld_in, gathered, g_labels, g_blank, T, U1)
        if (ld_out <= 512 * 10) PIKA_C8(10); else if (ld_out <= 512 * 13) PIKA_C8(13); else PIKA_C8(16);
#undef PIKA_C8
    } else
        PIKA_CQ(ld_out, hipLaunchKernelGGL((rnnt_dlogits_compact_kernel<true, TI, CQ>), grid, dim3(256), 0, s, x, L.meta, o, rows,
                                           V, ld_out, blank, scale, rpw, colsum, lse, ld_in, gathered, g_labels, g_blank, T, U1));
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Fused boundary logits -> (costs, d loss / d logits)  (SURVEY 8d M1'): the log-softmax of the joint output
// is never materialised.  Pass 1 reads every V-row of the logits once (one wavefront per row, row in
// registers): log-sum-exp -> lse[row], and the two log-probs the lattice needs go straight into the skewed
// planes.  After alpha/beta and the row metadata, pass 2 re-reads the logits and writes
//   grad[r, v] = (v == blank) * gb + (v == ye) * ge - exp(logits[r, v] - lse[r]) * (gb + ge).
// 3 x B*T*U1*V*4 bytes in total instead of 6 x for log_softmax + loss + log_softmax backward.
__device__ inline float fwave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ inline float fwave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// PACKED: `logits` are the (N, V) rows of the packed layout (rows = N, roff / loff the row and label offsets of the
// utterances, B of them): the wave's utterance comes from a binary search over roff, everything else is the same.
// BANDED: `logits` are (B,T,S,V), rows = B*T*S; row (b T + t) S + j is cell (t, s_t + j).  Only live cells are written:
// the caller fills both planes with NEG first (rnnt_fill_neg_kernel), which is what the dead cells keep.
template <int CQ, int LAYOUT = PADDED, bool MOD = false>
__global__ __launch_bounds__(256) void rnnt_lse_gather_kernel(
    const float *__restrict__ logits, const int *__restrict__ labels, const int *__restrict__ Tn_,
    const int *__restrict__ Un_, long long rows, int T, int U1, int V, int blank, float *__restrict__ lse,
    float *__restrict__ lpb, float *__restrict__ lpe, int Wp, int D, const int *__restrict__ roff = nullptr,
    const int *__restrict__ loff = nullptr, int B = 0, const int *__restrict__ ranges = nullptr, int S = 0) {
    constexpr bool PACKED = LAYOUT == Layout::PACKED, BANDED = LAYOUT == Layout::BANDED;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, c4 = V >> 2;
    int u, t, b;
    const int *lab;
    if constexpr (PACKED) {   // rows < 2^31 (host check); the search runs on wave-uniform values
        b = packed_utterance(roff, B, __builtin_amdgcn_readfirstlane((int)r));
        const int w = clampi(Un_[b], 0, U1 - 1) + 1;
        const int i = (int)r - roff[b];
        t = i / w;
        u = i - t * w;
        lab = labels + loff[b];
    } else if constexpr (BANDED) {
        t = (int)((r / S) % T);
        b = (int)(r / ((long long)S * T));
        u = (int)(r % S) + band_start(ranges, b, T, t, clampi(Un_[b], 0, U1 - 1), S);
        lab = labels + (size_t)b * (U1 - 1);
    } else {
        u = (int)(r % U1);
        t = (int)((r / U1) % T);
        b = (int)(r / ((long long)U1 * T));
        lab = labels + (size_t)b * (U1 - 1);
    }
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    if (t >= Tn || u > Un) {            // outside the sub-lattice: no gradient, nothing to gather
        if (lane == 0) lse[r] = 0.f;
        return;
    }
    const float *row = logits + r * V;
    const f32x4 *row4 = reinterpret_cast<const f32x4 *>(row);
    // The row's label is requested FIRST and its two gathered logits right behind the row's own loads: the tail of a row
    // (label -> row[label], row[blank] -> three stores on one lane) was a chain of dependent round trips as long as the
    // streaming part, with the whole wave's registers parked behind it (7.4 ms for one 32.6 GB read = 4.4 TB/s).
    int y = -1;
    if (u < Un) y = lab[u];
    f32x4 v[CQ];
#pragma unroll
    for (int q = 0; q < CQ; ++q)
        if (lane + q * 64 < c4) v[q] = row4[lane + q * 64];
    const bool y_ok = y >= 0 && y < V;
    const float xb = row[blank], xy = y_ok ? row[y] : 0.f;       // (wave-uniform addresses: one request each, L2 hits)
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < CQ; ++q)
        if (lane + q * 64 < c4) m = fmaxf(m, fmaxf(fmaxf(v[q].x, v[q].y), fmaxf(v[q].z, v[q].w)));
    m = fwave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < CQ; ++q)
        if (lane + q * 64 < c4)
            sum += (__expf(v[q].x - m) + __expf(v[q].y - m)) + (__expf(v[q].z - m) + __expf(v[q].w - m));
    const float l = m + __logf(fwave_sum(sum));
    if (lane == 0) {
        lse[r] = l;
        const size_t o = ((size_t)b * D + (MOD ? t : t + u)) * Wp + u;   // MOD: un-skewed planes (the modified topology)
        lpb[o] = fmaxf(xb - l, NEG);
        lpe[o] = y_ok ? fmaxf(xy - l, NEG) : NEG;
    }
}

// The same outputs from the per-row partial (max, sum exp) pairs the joint's output GEMM emitted in its epilogue
// (pika_gemm_bf16_nt_lse): 16 lanes per row merge n_part pairs, then the row's two needed logits are fetched (two
// 64-byte sectors per lattice cell instead of the whole 20 KB row).
// GATHERED: the logits are the fp16 matrix `logits16` (pitch ld16) of pika_gemm_bf16_nt_lse_f16, whose epilogue left
// the blank column g_blank and the column of g_labels[b][u] of every row in fp32 (gathered[2 r], gathered[2 r + 1]): a
// cell whose label / blank IS that one takes the fp32 value, any other one the fp16 logit.
template <bool GATHERED = false>
__global__ __launch_bounds__(256) void rnnt_lse_merge_gather_kernel(
    const float *__restrict__ logits, const float *__restrict__ pmax, const float *__restrict__ psum, int n_part,
    const int *__restrict__ labels, const int *__restrict__ Tn_, const int *__restrict__ Un_, long long rows, int T,
    int U1, int V, int blank, float *__restrict__ lse, float *__restrict__ lpb, float *__restrict__ lpe, int Wp, int D,
    const _Float16 *__restrict__ logits16 = nullptr, long long ld16 = 0, const float *__restrict__ gathered = nullptr,
    const int *__restrict__ g_labels = nullptr, int g_blank = 0) {
    const long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int l16 = threadIdx.x & 15;
    const bool in = r < rows;
    int u = 0, t = 0, b = 0, Tn = 1, Un = 0;
    if (in) {
        u = (int)(r % U1);
        t = (int)((r / U1) % T);
        b = (int)(r / ((long long)U1 * T));
        Tn = clampi(Tn_[b], 1, T);
        Un = clampi(Un_[b], 0, U1 - 1);
    }
    const bool live = in && t < Tn && u <= Un;
    float m = -INFINITY;
    if (live)
        for (int q = l16; q < n_part; q += 16) m = fmaxf(m, pmax[r * n_part + q]);
    for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f;
    if (live)
        for (int q = l16; q < n_part; q += 16) {
            const float pm = pmax[r * n_part + q];
            if (pm > -INFINITY) s += psum[r * n_part + q] * __expf(pm - m);
        }
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (!in || l16) return;
    if (!live) { lse[r] = 0.f; return; }
    const float l = m + __logf(s);
    lse[r] = l;
    float ve = NEG, vb;
    if constexpr (GATHERED) {
        const _Float16 *row = logits16 + r * ld16;
        if (u < Un) {
            const int y = labels[(size_t)b * (U1 - 1) + u];
            if (y >= 0 && y < V) {
                const float x = (g_labels && g_labels[(size_t)b * (U1 - 1) + u] == y) ? gathered[2 * r + 1] : (float)row[y];
                ve = fmaxf(x - l, NEG);
            }
        }
        vb = (blank == g_blank ? gathered[2 * r] : (float)row[blank]) - l;
    } else {
        const float *row = logits + r * V;
        if (u < Un) {
            const int y = labels[(size_t)b * (U1 - 1) + u];
            if (y >= 0 && y < V) ve = fmaxf(row[y] - l, NEG);
        }
        vb = row[blank] - l;
    }
    const size_t o = ((size_t)b * D + (t + u)) * Wp + u;
    lpb[o] = fmaxf(vb, NEG);
    lpe[o] = ve;
}

template <typename TO, int CQ>
__global__ __launch_bounds__(256) void rnnt_dlogits_fused_kernel(const float *__restrict__ logits,
                                                                 const float *__restrict__ lse,
                                                                 const RowMeta *__restrict__ meta,
                                                                 TO *__restrict__ out, long long rows, int V,
                                                                 long long ld_out, int blank) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63, c4 = V >> 2, o4 = (int)(ld_out >> 2);
    const RowMeta m = meta[r];
    const float s = m.gb + m.ge, l = lse[r];
    const bool live = (m.gb != 0.f) || (m.ge != 0.f);
    const f32x4 *lrow = reinterpret_cast<const f32x4 *>(logits + r * V);
    f32x4 v[CQ];
    if (live) {
#pragma unroll
        for (int q = 0; q < CQ; ++q)
            if (lane + q * 64 < c4) v[q] = lrow[lane + q * 64];
    }
#pragma unroll
    for (int q = 0; q < CQ; ++q) {
        const int i = lane + q * 64;
        if (i >= o4) continue;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (live && i < c4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = 4 * i + e;
                float g = col == blank ? m.gb : 0.f;
                if (col == m.ye) g += m.ge;
                o[e] = g - __expf(v[q][e] - l) * s;
            }
        }
        if constexpr (sizeof(TO) == 4) reinterpret_cast<f32x4 *>(out + r * ld_out)[i] = o;
        else reinterpret_cast<cbf16x4 *>(out + r * ld_out)[i] = __builtin_convertvector(o, cbf16x4);
    }
}


// ---------------------------------------------------------------------------------------------
// Pruned (banded) lattice, pika_rnnt.h "Pruned RNN-T".  The banded loss itself is the BANDED layout of the gather /
// log-sum-exp gather / row metadata kernels above; alpha/beta, the flat writer and the fused d(logits) kernel run
// unchanged over the B*T*S band rows.  Below: the NEG fill under the banded log-sum-exp gather, the loss that takes the
// two planes directly (the "simple" loss of an am + lm joiner) with its occupation probabilities, and the band search.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rnnt_fill_neg_kernel(v4f *__restrict__ p, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) p[i] = v4f{NEG, NEG, NEG, NEG};
}

// dense (B,T,U1) planes -> the skewed ones: NEG outside the sub-lattice, and in the label plane from column U_n on.
// grid = (ceil(D / 4), Wp / 64, B), block = 256: a wave per skewed row, lane = u.
// MOD (the modified topology): the same masking without the skew, row d is frame t.
template <bool MOD = false>
__global__ __launch_bounds__(256) void rnnt_skew_planes_kernel(
    const float *__restrict__ blank_lp, const float *__restrict__ label_lp, const int *__restrict__ Tn_,
    const int *__restrict__ Un_, int T, int U1, float *__restrict__ lpb, float *__restrict__ lpe, int Wp, int D) {
    const int b = blockIdx.z;
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int u = blockIdx.y * 64 + (threadIdx.x & 63);
    if (d >= D) return;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    const int t = MOD ? d : d - u;
    float vb = NEG, ve = NEG;
    if (u <= Un && t >= 0 && t < Tn) {
        const size_t i = ((size_t)b * T + t) * U1 + u;
        vb = fmaxf(blank_lp[i], NEG);
        if (u < Un) ve = fmaxf(label_lp[i], NEG);
    }
    const size_t o = ((size_t)b * D + d) * Wp + u;
    lpb[o] = vb;
    lpe[o] = ve;
}

// Occupation probabilities exp(alpha + lp + beta' - ll) of the blank and the label edge of every cell, un-skewed into
// dense (B,T,U1) planes: the values of rnnt_rowmeta_kernel with unit grad_costs, without the sign.  Zero outside the
// sub-lattice (and for the label edge of column U_n, the blank edge of the last frame below U_n).
// MOD (the modified topology): un-skewed planes, both edges end in row t + 1, no terminal blank.
template <bool MOD = false>
__global__ __launch_bounds__(256) void rnnt_occupancy_kernel(
    const int *__restrict__ Tn_, const int *__restrict__ Un_, int B, int T, int U1, const float *__restrict__ lpb,
    const float *__restrict__ lpe, const float *__restrict__ alpha, const float *__restrict__ beta,
    const double *__restrict__ off_a, const double *__restrict__ off_b, const double *__restrict__ ll, int Wp, int D,
    float *__restrict__ blank_occ, float *__restrict__ label_occ) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * T * U1) return;
    const int u = (int)(idx % U1);
    const int t = (int)((idx / U1) % T);
    const int b = (int)(idx / ((size_t)U1 * T));
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    float eb = 0.f, ee = 0.f;
    if constexpr (MOD) {
        if (t < Tn && u <= Un) {
            const size_t o = ((size_t)b * D + t) * Wp + u;
            const float a = alpha[o];
            const float k1 = (float)(off_a[(size_t)b * D + t] - ll[b] + off_b[(size_t)b * D + t + 1]);
            eb = __expf(k1 + (a + beta[o + Wp] + lpb[o]));
            if (u < Un) ee = __expf(k1 + (a + beta[o + Wp + 1] + lpe[o]));
        }
    } else if (t < Tn && u <= Un) {
        const int d = t + u;
        const size_t o = ((size_t)b * D + d) * Wp + u;
        const float a = alpha[o];
        const double base = off_a[(size_t)b * D + d] - ll[b];
        const float k1 = (d + 1 < D) ? (float)(base + off_b[(size_t)b * D + d + 1]) : 0.0f;
        if (t < Tn - 1)
            eb = __expf(k1 + (a + beta[o + Wp] + lpb[o]));
        else if (u == Un)
            eb = __expf((float)base + (a + lpb[o]));
        if (u < Un) ee = __expf(k1 + (a + beta[o + Wp + 1] + lpe[o]));
    }
    blank_occ[idx] = eb;
    label_occ[idx] = ee;
}

// Band search (pika_rnnt.h): one workgroup per utterance.  Phase 1, a wave per frame and a lane per band start s: the
// window sums of occ = blank_occ + label_occ and their arg-max (ties to the smallest s), into ranges[b][t].  Phases 2 and
// 3 run in place over that row in chunks of PRUNE_THREADS frames with a carried value: the suffix minimum m, then
//   f(t) = min(m(t), f(t-1) + S-1), f(0) = 0   ==   t (S-1) + prefix-min of g,  g(0) = 0, g(t) = m(t) - t (S-1),
// and the lower bound that still reaches s_max at the last frame.
constexpr int PRUNE_THREADS = 1024;

// inclusive prefix minimum over the workgroup's threads (sh: PRUNE_THREADS values; sh[PRUNE_THREADS - 1] is the total)
__device__ inline long long block_prefix_min(long long v, long long *sh) {
    const int i = threadIdx.x;
    sh[i] = v;
    __syncthreads();
    for (int o = 1; o < PRUNE_THREADS; o <<= 1) {
        const long long w = i >= o ? sh[i - o] : v;
        __syncthreads();
        v = w < v ? w : v;
        sh[i] = v;
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(PRUNE_THREADS) void rnnt_prune_ranges_kernel(
    const float *__restrict__ blank_occ, const float *__restrict__ label_occ, const int *__restrict__ Tn_,
    const int *__restrict__ Un_, int T, int U1, int S, int step_, int *ranges) {
    __shared__ long long sh[PRUNE_THREADS];
    constexpr long long BIG = 0x7fffffffffffffffLL;
    const int b = blockIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    const int smax = max(0, Un + 1 - S);
    int *out = ranges + (size_t)b * T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = wave; t < Tn; t += PRUNE_THREADS / 64) {  // wave-uniform
        const float *ob = blank_occ + ((size_t)b * T + t) * U1;
        const float *ol = label_occ + ((size_t)b * T + t) * U1;
        float bv = -INFINITY;
        int bs = 0;
        for (int s = lane; s <= smax; s += 64) {
            const int hi = min(s + S - 1, Un);
            float sum = 0.f;
            for (int u = s; u <= hi; ++u) sum += ob[u] + ol[u];
            if (sum > bv) { bv = sum; bs = s; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o);
            const int s2 = __shfl_xor(bs, o);
            if (v2 > bv || (v2 == bv && s2 < bs)) { bv = v2; bs = s2; }
        }
        if (lane == 0) out[t] = t == Tn - 1 ? smax : bs;
    }
    __syncthreads();
    // suffix minimum: thread i of a chunk takes its frames from the top, so the prefix scan over i is a suffix scan over t
    long long carry = BIG;
    for (int base = ((Tn - 1) / PRUNE_THREADS) * PRUNE_THREADS; base >= 0; base -= PRUNE_THREADS) {
        const int t = base + (PRUNE_THREADS - 1 - (int)threadIdx.x);
        long long v = t < Tn ? (long long)out[t] : BIG;
        v = block_prefix_min(v, sh);
        v = carry < v ? carry : v;
        if (t < Tn) out[t] = (int)v;
        const long long tot = sh[PRUNE_THREADS - 1];
        carry = tot < carry ? tot : carry;
        __syncthreads();
    }
    carry = BIG;
    const long long step = step_;  // S - 1; 1 in the modified topology (a label edge advances the frame)
    for (int base = 0; base < T; base += PRUNE_THREADS) {
        const int t = base + (int)threadIdx.x;
        long long g = BIG;
        if (t < Tn) g = t == 0 ? 0 : (long long)out[t] - t * step;
        g = block_prefix_min(g, sh);
        g = carry < g ? carry : g;
        if (t < Tn) {
            const long long f = g + t * step, lo = smax - (long long)(Tn - 1 - t) * step;
            out[t] = (int)(f > lo ? f : lo);
        } else if (t < T) {
            out[t] = smax;
        }
        const long long tot = sh[PRUNE_THREADS - 1];
        carry = tot < carry ? tot : carry;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Modified topology (k2's rnnt_loss(modified=True), pika_rnnt.h "Modified topology"): every frame emits exactly one
// symbol, so the label edge runs (t, u) -> (t+1, u+1) and the recurrence is the regular line with d read as t,
//   A_{t+1}[u] = lae(A_t[u] + lpb_t[u], A_t[u-1] + lpe_t[u-1]),     ll = A_{T_n}[U_n],
// over UN-skewed planes [B][T+1][Wp] (row = frame; row T_n is terminal, both edge kinds out of frame T_n - 1 reach it).
// One workgroup per (direction, utterance), lane = u, Xchg<NW> at the wave edges, and the regular kernel's
// renormalisation: every RENORM rows the running maximum leaves the fp32 values and is summed in fp64.
// A cell is LIVE iff a path through it exists at all: u <= min(t, U_n) (reachable from (0, 0)) and U_n - u <= T_n - t
// (can still reach (T_n, U_n)); every other cell is held at NEG in both sweeps, so the maximum that is subtracted is
// one of cells that carry probability.  No cell is live when U_n > T_n, and a band may leave none in some row: a row
// whose maximum is log-zero subtracts nothing, and an utterance whose ll is log-zero costs +inf; its ll is stored as
// +inf, which zeroes every occupancy and gradient entry of it (exp(-inf)) without touching its neighbours.
// The plane loads need no mask: a live cell reads its own row's lpb / lpe (beta) or those of (t-1, u), (t-1, u-1)
// (alpha), cells of the sub-lattice, which every gather writes (NEG outside the band); what else a lane loads only
// reaches values the live-select discards.
// Row centres: a whole frame's log-probs may sit far from zero (unnormalised planes), and every path crosses every
// frame exactly once, so the largest live log-prob c_t of frame t (rnnt_mod_rowcentre_kernel; 0 for a frame with none) is
// taken out of both planes' values before they meet the running fp32 values and summed into the fp64 offsets instead.
// grid = (2, B): blockIdx.x 0 = alpha, 1 = beta; block = NW * 64 = lattice_width(U1).
// ---------------------------------------------------------------------------------------------
// a wave per plane row (b, t): rowc[b][t] = max over the sub-lattice's columns of max(lpb, lpe); 0 when that is log zero
// or t >= T_n.  grid = ceil(B * D / 4), block = 256.
__global__ __launch_bounds__(256) void rnnt_mod_rowcentre_kernel(
    const float *__restrict__ lpb, const float *__restrict__ lpe, const int *__restrict__ Tn_,
    const int *__restrict__ Un_, int B, int T, int U1, int Wp, int D, float *__restrict__ rowc) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B * D) return;
    const int b = row / D, t = row - b * D;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    float m = NEG;
    if (t < Tn)
        for (int u = lane; u <= Un; u += 64) {
            const size_t o = (size_t)row * Wp + u;
            m = fmaxf(m, fmaxf(lpb[o], lpe[o]));
        }
    m = wave_max(m);
    if (lane == 0) rowc[row] = m > NEG_HALF ? m : 0.0f;
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void rnnt_mod_alpha_beta_kernel(
    const float *__restrict__ lpb_, const float *__restrict__ lpe_, float *__restrict__ alpha_,
    float *__restrict__ beta_, double *__restrict__ off_a_, double *__restrict__ off_b_,
    const int *__restrict__ Tn_, const int *__restrict__ Un_, double *__restrict__ ll_,
    double *__restrict__ ll_a_, float *__restrict__ costs, const float *__restrict__ rowc_, int T, int U1, int Wp,
    int D) {
    __shared__ float lds[2 * (NW + 1) + 2 * NW];
    Xchg<NW> xc{lds, lds + 2 * (NW + 1)};
    if constexpr (NW > 1) {
        if (threadIdx.x < 2 * (NW + 1) + 2 * NW) lds[threadIdx.x] = NEG;
        __syncthreads();
    }
    const int b = blockIdx.y;
    const int u = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    const size_t base = (size_t)b * D * Wp + u;
    const float *lpb = lpb_ + base;
    const float *lpe = lpe_ + base;
    const float *rowc = rowc_ + (size_t)b * D;
    // cell (t, u) is live for tlo <= t <= thi (never, when u > U_n or U_n > T_n)
    const int tlo = u <= Un ? u : T + 2, thi = Tn - Un + u;
    auto live = [&](int t) __attribute__((always_inline)) { return t >= tlo && t <= thi; };

    float pbv[2][UNR], pev[2][UNR], cv[2][UNR];
    double off = 0.0;  // sum of subtracted maxima and row centres (identical in every thread)
    // subtract the row maximum m (workgroup-uniform) unless the whole row is log-zero
    auto renorm = [&](float &v, float m) __attribute__((always_inline)) {
        m = m > NEG_HALF ? m : 0.0f;
        v = v > NEG_HALF ? v - m : NEG;
        off += (double)m;
    };
    if (blockIdx.x == 0) {
        float *alpha = alpha_ + base;
        double *offs = off_a_ + (size_t)b * D;
        float a = live(0) ? 0.0f : NEG;  // (0, 0), when the utterance has a path at all
        alpha[0] = a;
        if (u == 0) offs[0] = 0.0;
        auto load = [&](int buf, int t0) __attribute__((always_inline)) {  // rows t0-1 .. t0+UNR-2
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int r = min(t0 + i - 1, T - 1);
                pbv[buf][i] = lpb[(size_t)r * Wp];
                pev[buf][i] = lpe[(size_t)r * Wp];
                cv[buf][i] = rowc[r];
            }
        };
        // rows t0 .. t0+UNR-1 (<= Tn); t0 = 1 (mod RENORM) at the first half of a group
        auto steps = [&](int buf, int t0, auto second_half) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int t = t0 + i;
                if (t <= Tn) {  // workgroup-uniform
                    const float c = cv[buf][i];  // the centre of row t - 1, uniform: off the dependent chain
                    const float x = a + (pbv[buf][i] - c);
                    const float y = xc.up(a + (pev[buf][i] - c), t);
                    a = live(t) ? lae(x, y) : NEG;
                    off += (double)c;
                    if (decltype(second_half)::value && i == UNR - 1) renorm(a, xc.max_all(a, t));  // t = 0 (mod RENORM)
                    alpha[(size_t)t * Wp] = a;
                    if (u == 0) offs[t] = off;
                }
            }
        };
        load(0, 1);
        for (int t0 = 1; t0 <= Tn; t0 += 2 * UNR) {
            load(1, t0 + UNR);
            steps(0, t0, std::false_type{});
            load(0, t0 + 2 * UNR);
            steps(1, t0 + UNR, std::true_type{});
        }
        if (u == Un) ll_a_[b] = a > NEG_HALF ? (double)a + off : -(double)INFINITY;
    } else {
        float *beta = beta_ + base;
        double *offs = off_b_ + (size_t)b * D;
        float bt = (u == Un && live(Tn)) ? 0.0f : NEG;  // the terminal row: (T_n, U_n)
        beta[(size_t)Tn * Wp] = bt;
        if (u == 0) offs[Tn] = 0.0;
        auto load = [&](int buf, int t0) __attribute__((always_inline)) {  // rows t0, t0-1, ..., t0-UNR+1
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int r = max(t0 - i, 0);
                pbv[buf][i] = lpb[(size_t)r * Wp];
                pev[buf][i] = lpe[(size_t)r * Wp];
                cv[buf][i] = rowc[r];
            }
        };
        // rows t0, t0-1, ..., t0-UNR+1 (>= 0); step j = Tn - t, renormalised where j = 0 (mod RENORM)
        auto steps = [&](int buf, int t0, auto second_half) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < UNR; ++i) {
                const int t = t0 - i;
                if (t >= 0) {  // workgroup-uniform
                    const int j = Tn - t;
                    const float dn = xc.down(bt, j);
                    const float c = cv[buf][i];  // the centre of row t
                    const float x = bt + (pbv[buf][i] - c);
                    const float y = dn + (pev[buf][i] - c);
                    bt = live(t) ? lae(x, y) : NEG;
                    off += (double)c;
                    if (decltype(second_half)::value && i == UNR - 1) renorm(bt, xc.max_all(bt, j));
                    beta[(size_t)t * Wp] = bt;
                    if (u == 0) offs[t] = off;
                }
            }
        };
        load(0, Tn - 1);
        for (int t0 = Tn - 1; t0 >= 0; t0 -= 2 * UNR) {
            load(1, t0 - UNR);
            steps(0, t0, std::false_type{});
            load(0, t0 - 2 * UNR);
            steps(1, t0 - UNR, std::true_type{});
        }
        if (u == 0) {
            const bool path = bt > NEG_HALF;
            ll_[b] = path ? (double)bt + off : (double)INFINITY;
            costs[b] = path ? (float)(-((double)bt + off)) : INFINITY;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// forced alignment in the modified topology: rnnt_align_kernel's max-plus sweep over the UN-skewed planes,
//   delta_{t+1}[u] = max(delta_t[u] + lpb_t[u], delta_t[u-1] + lpe_t[u-1]),     score = delta_{T_n}[U_n],
// T_n dependent steps, one workgroup per utterance, lane = u, the neighbour term by Xchg<NW>::up, plain fp32 (a cell's
// value is the running sum of ONE path's T_n edges).  Liveness is rnnt_mod_alpha_beta_kernel's, from the indices alone;
// dead cells are held at NEG, and both operands of a live cell come from live cells -- except on the two borders, where
// the decision is forced: u == 0 has no label edge into it and cell (t, t) no blank one.  So the planes are read unmasked
// (garbage outside the sub-lattice never reaches a live value), and the walk from (T_n, U_n), which loses at most one
// column per row, stays inside the live cells and ends in (0, 0) whatever the planes hold.
// Back-pointers: bit u of row t (1 <= t <= T_n) = cell (t, u) was reached over the label edge from (t-1, u-1); a tie
// is 0, the blank predecessor, i.e. the earliest emission.  One __ballot word per wave and row, in LDS when the T_n rows
// fit (ALIGN_WORDS / NW), in the caller's scratch ([B][T+1][NW] words) otherwise and then staged through LDS a chunk at
// a time.  Thread 0 walks rows T_n .. 1 carrying only the column (the row a step reads does not depend on the walk):
//   e = bit(t, cu);  fr[cu] = t - 1;  cu -= e
// so the last value a column c >= 1 receives is the frame of the label edge that enters it, emit_frames[c - 1].
// An utterance without a path (U_n > T_n, a band that holds none, a dead label: delta(T_n, U_n) is log zero) gets score
// -inf and frames -1; the walk still runs, inside its own LDS.  grid = B, block = NW * 64.
// ---------------------------------------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(NW * 64) void rnnt_mod_align_kernel(
    const float *__restrict__ lpb_, const float *__restrict__ lpe_, const int *__restrict__ Tn_,
    const int *__restrict__ Un_, float *__restrict__ scores, int *__restrict__ frames,
    unsigned long long *__restrict__ bp_, int T, int U1, int D) {
    __shared__ float lds[2 * (NW + 1) + 2 * NW];
    __shared__ unsigned long long bits[ALIGN_WORDS];
    __shared__ int fr[NW * 64 + 1];
    __shared__ int has_path;
    Xchg<NW> xc{lds, lds + 2 * (NW + 1)};
    if constexpr (NW > 1) {
        if (threadIdx.x < 2 * (NW + 1) + 2 * NW) lds[threadIdx.x] = NEG;
        __syncthreads();
    }
    const int b = blockIdx.x;
    const int u = threadIdx.x;
    const int Tn = clampi(Tn_[b], 1, T), Un = clampi(Un_[b], 0, U1 - 1);
    unsigned long long *bp = bp_ + (size_t)b * D * NW;  // row t: bp[t * NW + wave]
    constexpr int ROWS = ALIGN_WORDS / NW;
    const bool fits = Tn <= ROWS;  // workgroup-uniform; row t at bits[(t-1) * NW + wave]
    // cell (t, u) is live for tlo <= t <= thi (never, when u > U_n or U_n > T_n)
    const int tlo = u <= Un ? u : T + 2, thi = Tn - Un + u;

    // buffer loads at a uniform row offset plus the lane's fixed column; a row past the planes reads 0
    constexpr int ROWB = NW * 64 * 4;  // bytes per plane row (Wp == NW * 64)
    const size_t plane_b = (size_t)b * D * (NW * 64);
    const auto rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(lpb_ + plane_b), 0, D * ROWB, 0x00020000);
    const auto re = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(lpe_ + plane_b), 0, D * ROWB, 0x00020000);
    float pbv[2][AUNR], pev[2][AUNR];
    float v = (u == 0 && Un <= Tn) ? 0.0f : NEG;  // (0, 0), when the utterance has a path at all
    auto load = [&](int buf, int t0) __attribute__((always_inline)) {  // rows t0-1 .. t0+AUNR-2
        const int soff = __builtin_amdgcn_readfirstlane((t0 - 1) * ROWB);
#pragma unroll
        for (int i = 0; i < AUNR; ++i) {
            pbv[buf][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rb, u * 4 + i * ROWB, soff, 0));
            pev[buf][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(re, u * 4 + i * ROWB, soff, 0));
        }
    };
    auto steps = [&](int buf, int t0) __attribute__((always_inline)) {  // rows t0 .. t0+AUNR-1 (<= Tn)
        unsigned long long m[AUNR];
#pragma unroll
        for (int i = 0; i < AUNR; ++i) {
            const int t = t0 + i;
            if (t <= Tn) {  // workgroup-uniform
                const float x = v + pbv[buf][i];
                const float y = xc.up(v + pev[buf][i], t);
                // a tie is the blank predecessor; the borders decide whatever the values say
                const bool emit = (u > 0) & ((y > x) | (t == u));
                m[i] = __ballot(emit);
                const bool in = (t >= tlo) & (t <= thi);
                v = in ? (emit ? y : x) : NEG;
            }
        }
        if ((u & 63) == 0) {
#pragma unroll
            for (int i = 0; i < AUNR; ++i)
                if (t0 + i <= Tn) {
                    if (fits) bits[(t0 + i - 1) * NW + (u >> 6)] = m[i];
                    else bp[(size_t)(t0 + i) * NW + (u >> 6)] = m[i];
                }
        }
    };
    load(0, 1);
    for (int t0 = 1; t0 <= Tn; t0 += 2 * AUNR) {
        load(1, t0 + AUNR);
        steps(0, t0);
        load(0, t0 + 2 * AUNR);
        steps(1, t0 + AUNR);
    }
    if (u == Un) {
        const bool path = v > NEG_HALF;
        scores[b] = path ? v : -INFINITY;
        has_path = path;
    }

    int cu = Un;  // thread 0: the walk's column; its cell in row t is (t, cu)
    for (int hi = Tn; hi >= 1; hi -= ROWS) {  // workgroup-uniform, T_n steps in all
        const int lo = max(hi - ROWS + 1, 1);
        __syncthreads();  // the sweep's rows are written; the previous chunk is walked
        if (!fits) {
            for (int i = threadIdx.x; i < (hi - lo + 1) * NW; i += NW * 64) bits[i] = bp[(size_t)lo * NW + i];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
#pragma unroll 8
            for (int t = hi; t >= lo; --t) {
                const unsigned long long w = bits[(t - lo) * NW + (NW == 1 ? 0 : cu >> 6)];
                fr[cu] = t - 1;
                cu -= (int)((w >> (cu & 63)) & 1ull);
            }
        }
    }
    __syncthreads();
    if (u < U1 - 1) frames[(size_t)b * (U1 - 1) + u] = (has_path && u < Un) ? fr[u + 1] : -1;
}

// ---------------------------------------------------------------------------------------------
// Host side.  Every loss entry point is its own argument checks, a Call -- how the call's (rows, V) tensor maps to lattice
// cells -- and one of four bodies (loss_forward, loss_backward, fused_forward, fused_backward) over one launcher per
// kernel family.  A further layout or topology is a Call maker and a line of dispatch_layout.
// ---------------------------------------------------------------------------------------------
struct Call {
    Layout layout;
    bool mod;                // the modified topology
    int B, T, U1, V, blank;  // (T, U1: T_max, U1_max of a packed batch)
    long long rows;          // of the (rows, V) tensor: B*T*U1 padded, N packed, B*T*S banded
    const int *labels, *frames_lengths, *labels_lengths;
    const int *roff, *loff;  // packed: the utterances' row and label offsets
    const int *ranges;       // banded: the band starts (B, T) ...
    int S;                   // ... and the band's width
    hipStream_t s;
};

Call padded_call(const int *labels, const int *frames_lengths, const int *labels_lengths, int B, int T, int U1, int V,
                 int blank, void *stream, bool mod = false) {
    return Call{PADDED, mod, B, T, U1, V, blank, (long long)B * T * U1, labels, frames_lengths, labels_lengths,
                nullptr, nullptr, nullptr, 0, static_cast<hipStream_t>(stream)};
}

Call packed_call(const int *labels, const int *frames_lengths, const int *labels_lengths, const int *roff, const int *loff,
                 int B, int T_max, int U1_max, long long N, int V, int blank, void *stream) {
    return Call{PACKED, false, B, T_max, U1_max, V, blank, N, labels, frames_lengths, labels_lengths,
                roff, loff, nullptr, 0, static_cast<hipStream_t>(stream)};
}

// ranges null (the modified topology only, where S == U1): the padded layout
Call banded_call(bool mod, const int *labels, const int *ranges, const int *frames_lengths, const int *labels_lengths, int B,
                 int T, int U1, int S, int V, int blank, void *stream) {
    return Call{ranges ? BANDED : PADDED, mod, B, T, U1, V, blank, (long long)B * T * S, labels, frames_lengths,
                labels_lengths, nullptr, nullptr, ranges, ranges ? S : 0, static_cast<hipStream_t>(stream)};
}

// The (layout, topology) pairs the layout kernels are instantiated for: THE list.  f(LayoutOf<LAYOUT, MOD>{}) for the
// call's pair; false when there is none.  (LayoutOf<PADDED, false> is the kernels' default template arguments: the
// instantiations otherwise spelt rnnt_gather_kernel<>, rnnt_lse_gather_kernel<CQ> and rnnt_rowmeta_kernel<>.)
template <int LAYOUT, bool MOD>
struct LayoutOf {
    static constexpr int layout = LAYOUT;
    static constexpr bool mod = MOD;
};
template <class F, class... P>
inline bool dispatch_layout(const Call &c, F f, P... pair) {
    return ((c.layout == pair.layout && c.mod == pair.mod && (f(pair), true)) || ...);
}
template <class F>
inline bool dispatch_layout(const Call &c, F f) {
    return dispatch_layout(c, f, LayoutOf<PADDED, false>{}, LayoutOf<PACKED, false>{}, LayoutOf<BANDED, false>{},
                           LayoutOf<PADDED, true>{}, LayoutOf<BANDED, true>{});
}

// One launcher per kernel family.  Each passes the full argument list: an instantiation does not read what its layout
// does not have (null offsets, null ranges, S = 0).
int launch_gather(const Call &c, const Lattice &L, const float *log_probs) {
    const dim3 grid((unsigned)((L.D + 4 * GATHER_ROWS - 1) / (4 * GATHER_ROWS)), (unsigned)(L.Wp / 64), (unsigned)c.B);
    const bool ok = dispatch_layout(c, [&](auto pair) {
        using P = decltype(pair);
        hipLaunchKernelGGL((rnnt_gather_kernel<P::layout, P::mod>), grid, dim3(256), 0, c.s, log_probs, c.labels,
                           c.frames_lengths, c.labels_lengths, c.B, c.T, c.U1, c.V, c.blank, L.lpb, L.lpe, L.Wp, L.D, c.roff,
                           c.loff, c.ranges, c.S);
    });
    return ok ? PIKA_OK : PIKA_EINVAL;
}

int launch_lse_gather(const Call &c, const Lattice &L, const float *logits, float *lse) {
    if (c.layout == BANDED) {  // the banded kernel writes the live cells only: NEG under it
        const size_t n4 = 2 * ((size_t)c.B * L.D * L.Wp) / 4;  // lpb and lpe are adjacent; a plane is a multiple of 64 floats
        hipLaunchKernelGGL(rnnt_fill_neg_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, c.s,
                           reinterpret_cast<v4f *>(L.lpb), n4);
    }
    const dim3 grid((unsigned)((c.rows + 3) / 4));
    const bool ok = dispatch_layout(c, [&](auto pair) {
        using P = decltype(pair);
        PIKA_CQ(c.V, hipLaunchKernelGGL((rnnt_lse_gather_kernel<CQ, P::layout, P::mod>), grid, dim3(256), 0, c.s, logits,
                                        c.labels, c.frames_lengths, c.labels_lengths, c.rows, c.T, c.U1, c.V, c.blank, lse,
                                        L.lpb, L.lpe, L.Wp, L.D, c.roff, c.loff, c.B, c.ranges, c.S));
    });
    return ok ? PIKA_OK : PIKA_EINVAL;
}

MetaArgs meta_args(const Call &c, const Lattice &L, const float *grad_costs, float lscale, long gc_stride = 1) {
    return MetaArgs{c.labels, c.frames_lengths, c.labels_lengths, c.B, c.T, c.U1, c.V, grad_costs, gc_stride, L.lpb, L.lpe, L.alpha,
                    L.beta, L.off_a, L.off_b, L.ll, L.Wp, L.D, lscale, c.roff, c.loff, (long)c.rows, c.ranges, c.S};
}

// row metadata of the call's rows
int launch_rowmeta(const Call &c, const Lattice &L, const float *grad_costs, float lscale, long gc_stride = 1) {
    const bool ok = dispatch_layout(c, [&](auto pair) {
        using P = decltype(pair);
        hipLaunchKernelGGL((rnnt_rowmeta_kernel<P::layout, P::mod>), dim3((unsigned)((c.rows + 255) / 256)), dim3(256), 0, c.s,
                           meta_args(c, L, grad_costs, lscale, gc_stride), L.meta);
    });
    return ok ? PIKA_OK : PIKA_EINVAL;
}

// What every forward does once its one launch has filled the lpb / lpe planes: alpha, beta and the costs (the modified
// topology: over the row centres).
int finish_forward(const Call &c, const Lattice &L, float *costs) {
    bool ok;
    if (c.mod) {
        hipLaunchKernelGGL(rnnt_mod_rowcentre_kernel, dim3((unsigned)(((size_t)c.B * L.D + 3) / 4)), dim3(256), 0, c.s, L.lpb,
                           L.lpe, c.frames_lengths, c.labels_lengths, c.B, c.T, c.U1, L.Wp, L.D, L.rowc);
        ok = dispatch_nw(L.Wp / 64, [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            hipLaunchKernelGGL((rnnt_mod_alpha_beta_kernel<NW>), dim3(2, c.B), dim3(NW * 64), 0, c.s, L.lpb, L.lpe, L.alpha,
                               L.beta, L.off_a, L.off_b, c.frames_lengths, c.labels_lengths, L.ll, L.ll_a, costs, L.rowc, c.T,
                               c.U1, L.Wp, L.D);
        });
    } else {
        ok = dispatch_nw(L.Wp / 64, [&](auto nw) {
            constexpr int NW = decltype(nw)::value;
            hipLaunchKernelGGL((rnnt_alpha_beta_kernel<NW>), dim3(2, c.B), dim3(NW * 64), 0, c.s, L.lpb, L.lpe, L.alpha,
                               L.beta, L.off_a, L.off_b, c.frames_lengths, c.labels_lengths, L.ll, L.ll_a, costs, c.T, c.U1,
                               L.Wp, L.D);
        });
    }
    return ok ? (int)hipGetLastError() : PIKA_ETOOBIG;
}

// the streaming pass: dense (nrows, V) gradient from the row metadata in the workspace
int write_dense_grads(const Lattice &L, size_t nrows, int V, int blank, float *grads, hipStream_t s) {
    const size_t n = nrows * (size_t)V;
    const bool vec4 = (V % 4 == 0) && ((reinterpret_cast<uintptr_t>(grads) & 15) == 0);
    if (vec4) {
        const size_t n4 = n / 4;
        const int V4 = V / 4;
        if (V4 >= 64) {
            const size_t blocks = (n4 + 511) / 512;
            if (blocks > 0x7fffffffu) return PIKA_ETOOBIG;
            hipLaunchKernelGGL((rnnt_grad_kernel<true, 2>), dim3((unsigned)blocks), dim3(256), 0, s,
                               L.meta, n4, nrows, V4, blank, reinterpret_cast<v4f *>(grads));
        } else {
            const size_t blocks = (n4 + 1023) / 1024;
            if (blocks > 0x7fffffffu) return PIKA_ETOOBIG;
            hipLaunchKernelGGL((rnnt_grad_kernel<false, 4>), dim3((unsigned)blocks), dim3(256), 0, s,
                               L.meta, n4, nrows, V4, blank, reinterpret_cast<v4f *>(grads));
        }
    } else {
        const size_t want = (n + 255) / 256;
        hipLaunchKernelGGL(rnnt_grad_scalar_kernel, dim3((unsigned)(want < 65536 ? want : 65536)),
                           dim3(256), 0, s, L.meta, n, V, blank, grads);
    }
    return (int)hipGetLastError();
}

// What the tensor `grads` points into held before this call (pika_rnnt.h, pika_rgrad_*), and where the label columns of
// what it holds afterwards go.  prev_cols null: nothing known, the streaming pass writes every word.
struct PrevGrad {
    const int *cols;
    long long rows;
    int blank;
    int *cols_out;
};

int check_prev_grad(const PrevGrad &p, int V) {
    if (!p.cols_out) return PIKA_EINVAL;
    if (p.cols && (p.rows < 0 || p.blank < 0 || p.blank >= V)) return PIKA_EINVAL;
    return (p.cols && p.rows > ROWS_MAX) ? PIKA_ETOOBIG : PIKA_OK;
}

// the dense (nrows, V) gradient and its label columns: streamed, or -- over a tensor that holds an earlier one -- updated
int write_or_update_dense_grads(const Lattice &L, long long nrows, int V, int blank, float *grads, const PrevGrad &p,
                                hipStream_t s) {
    if (nrows > ROWS_MAX) return PIKA_ETOOBIG;
    if (!p.cols) {
        if (int rc = write_dense_grads(L, (size_t)nrows, V, blank, grads, s)) return rc;
        hipLaunchKernelGGL(rnnt_grad_cols_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s, L.meta, (long)nrows,
                           p.cols_out);
        return (int)hipGetLastError();
    }
    const long long n = nrows > p.rows ? nrows : p.rows;
    hipLaunchKernelGGL(rnnt_grad_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, L.meta, (long)nrows, V,
                       blank, p.cols, (long)p.rows, p.blank, grads, p.cols_out);
    return (int)hipGetLastError();
}

// d(logits) of the fused route over `rows` rows, from the row metadata in L
int launch_dlogits_fused(const Lattice &L, const float *logits, const float *lse, long long rows, int V, int blank,
                         void *grad_logits, int out_dtype, long long ld_out, hipStream_t s) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (out_dtype == 0)
        PIKA_CQ(ld_out, hipLaunchKernelGGL((rnnt_dlogits_fused_kernel<float, CQ>), grid, dim3(256), 0, s, logits, lse, L.meta,
                                           static_cast<float *>(grad_logits), rows, V, ld_out, blank));
    else
        PIKA_CQ(ld_out, hipLaunchKernelGGL((rnnt_dlogits_fused_kernel<__bf16, CQ>), grid, dim3(256), 0, s, logits, lse, L.meta,
                                           static_cast<__bf16 *>(grad_logits), rows, V, ld_out, blank));
    return (int)hipGetLastError();
}

// FastEmit lambda -> the factor of the label entries of the row metadata (finite, >= 0; NaN fails the compare)
int label_scale(float fastemit_lambda, float *lscale) {
    if (!(fastemit_lambda >= 0.0f && fastemit_lambda <= 3.4e38f)) return PIKA_EINVAL;
    *lscale = 1.0f + fastemit_lambda;
    return PIKA_OK;
}

// The padded call's row metadata and, in the same launch, the update of a tensor that holds an earlier gradient (p.cols
// set, the row counts checked): what launch_rowmeta and then write_or_update_dense_grads do, word for word.
int rowmeta_and_update_dense_grads(const Call &c, const Lattice &L, const float *grad_costs, long long gc_stride,
                                   float fastemit_lambda, float *grads, const PrevGrad &p) {
    float lscale;
    if (int rc = label_scale(fastemit_lambda, &lscale)) return rc;
    constexpr int NT = UPDATE_FUSED_THREADS;
    const MetaArgs in = meta_args(c, L, grad_costs, lscale, (long)gc_stride);
    // the frame map: whole frames in a workgroup, and the tail of a larger earlier gradient within the grid's y range
    // (ny > 65535 needs an earlier gradient of more than 33 million rows behind a call of one workgroup per utterance:
    // no test builds one; that call takes the linear kernel, which the tests reach through U1 = 513 and 1024)
    const int F = c.U1 <= NT ? NT / c.U1 : 0;
    const long long nx = F ? (c.T + F - 1) / F : 0, tail = p.rows > c.rows ? p.rows - c.rows : 0;
    const long long ny = F ? c.B + (tail + nx * NT - 1) / (nx * NT) : 0;
    if (F && ny <= 65535) {
        const FrameMap fm{F, (unsigned)(((1u << 20) + c.U1 - 1) / c.U1)};
        hipLaunchKernelGGL(rnnt_grad_rowmeta_update_frames_kernel, dim3((unsigned)nx, (unsigned)ny), dim3(NT), 0, c.s, in, L.meta,
                           fm, (long)c.rows, c.blank, p.cols, (long)p.rows, p.blank, grads, p.cols_out);
        return (int)hipGetLastError();
    }
    const long long n = c.rows > p.rows ? c.rows : p.rows;   // the linear map: one thread per row, divisions in row_meta
    hipLaunchKernelGGL(rnnt_grad_rowmeta_update_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, c.s, in, L.meta,
                       (long)c.rows, c.blank, p.cols, (long)p.rows, p.blank, grads, p.cols_out);
    return (int)hipGetLastError();
}

// the d(logits) arguments of the fused backward calls
int check_dlogits_out(const float *logits, int V, const void *grad_logits, int out_dtype, long long ld_out) {
    if (!logits_ok(logits, V) || ld_out < V || (ld_out & 3) || ld_out > V_MAX) return PIKA_EINVAL;
    if (out_dtype != 0 && out_dtype != 1) return PIKA_EINVAL;   // PIKA_F32 / PIKA_BF16 (pika_gemm.h)
    if (reinterpret_cast<uintptr_t>(grad_logits) & (out_dtype == 0 ? 15 : 7)) return PIKA_EINVAL;
    return PIKA_OK;
}

// The four bodies, after the entry point's own checks of its dimensions and pointers.
int loss_forward(const Call &c, const float *log_probs, float *costs, void *workspace) {
    const Lattice L = carve(workspace, c.B, c.T, c.U1, c.mod);
    if (int rc = launch_gather(c, L, log_probs)) return rc;
    return finish_forward(c, L, costs);
}

// grads null: row metadata only (pika_rnnt.h)
int loss_backward(const Call &c, const float *grad_costs, float fastemit_lambda, const void *workspace, float *grads,
                  long gc_stride = 1) {
    float lscale;
    if (int rc = label_scale(fastemit_lambda, &lscale)) return rc;
    const Lattice L = carve(const_cast<void *>(workspace), c.B, c.T, c.U1, c.mod);
    if (int rc = launch_rowmeta(c, L, grad_costs, lscale, gc_stride)) return rc;
    if (!grads) return (int)hipGetLastError();
    return write_dense_grads(L, (size_t)c.rows, c.V, c.blank, grads, c.s);
}

int fused_forward(const Call &c, const float *logits, float *costs, float *lse, void *workspace) {
    const Lattice L = carve(workspace, c.B, c.T, c.U1, c.mod);
    if (int rc = launch_lse_gather(c, L, logits, lse)) return rc;
    return finish_forward(c, L, costs);
}

int fused_backward(const Call &c, const float *logits, const float *lse, const float *grad_costs, float fastemit_lambda,
                   const void *workspace, void *grad_logits, int out_dtype, long long ld_out) {
    if (int rc = check_dlogits_out(logits, c.V, grad_logits, out_dtype, ld_out)) return rc;
    float lscale;
    if (int rc = label_scale(fastemit_lambda, &lscale)) return rc;
    if (c.rows > ROWS_MAX) return PIKA_ETOOBIG;  // (the padded call's test of its row count; the others have made theirs)
    const Lattice L = carve(const_cast<void *>(workspace), c.B, c.T, c.U1, c.mod);
    if (int rc = launch_rowmeta(c, L, grad_costs, lscale)) return rc;
    return launch_dlogits_fused(L, logits, lse, c.rows, c.V, c.blank, grad_logits, out_dtype, ld_out, c.s);
}

// The loss of a lattice given by its two dense planes, and its occupation probabilities.
template <bool MOD>
int planes_forward(const float *blank_lp, const float *label_lp, const int *frames_lengths, const int *labels_lengths, int B,
                   int T, int U1, float *costs, float *blank_occ, float *label_occ, void *workspace, void *stream) {
    if (int rc = check_lattice_dims(B, T, U1)) return rc;
    if (!blank_lp || !label_lp || !frames_lengths || !labels_lengths || !costs || !blank_occ || !label_occ || !workspace)
        return PIKA_EINVAL;
    const Call c = padded_call(nullptr, frames_lengths, labels_lengths, B, T, U1, 0, 0, stream, MOD);
    const Lattice L = carve(workspace, B, T, U1, MOD);
    hipLaunchKernelGGL(rnnt_skew_planes_kernel<MOD>, dim3((unsigned)((L.D + 3) / 4), (unsigned)(L.Wp / 64), (unsigned)B),
                       dim3(256), 0, c.s, blank_lp, label_lp, frames_lengths, labels_lengths, T, U1, L.lpb, L.lpe, L.Wp, L.D);
    if (int rc = finish_forward(c, L, costs)) return rc;
    hipLaunchKernelGGL(rnnt_occupancy_kernel<MOD>, dim3((unsigned)((c.rows + 255) / 256)), dim3(256), 0, c.s, frames_lengths,
                       labels_lengths, B, T, U1, L.lpb, L.lpe, L.alpha, L.beta, L.off_a, L.off_b, L.ll, L.Wp, L.D, blank_occ,
                       label_occ);
    return (int)hipGetLastError();
}

// The band search; step: how far the band may move per frame (S - 1; 1 in the modified topology).
int prune_ranges(int step, const float *blank_occ, const float *label_occ, const int *frames_lengths,
                 const int *labels_lengths, int B, int T, int U1, int S, int *ranges, void *stream) {
    if (B <= 0 || T <= 0 || U1 <= 0 || S < 1 || S > U1) return PIKA_EINVAL;
    if (U1 > 1024) return PIKA_ETOOBIG;
    if (!blank_occ || !label_occ || !frames_lengths || !labels_lengths || !ranges) return PIKA_EINVAL;
    hipLaunchKernelGGL(rnnt_prune_ranges_kernel, dim3((unsigned)B), dim3(PRUNE_THREADS), 0, static_cast<hipStream_t>(stream),
                       blank_occ, label_occ, frames_lengths, labels_lengths, T, U1, S, step, ranges);
    return (int)hipGetLastError();
}

// the packed calls' shared checks: (B, T_max, U1_max) as check_dims, 0 < N <= B*T_max*U1_max (the metadata region) and
// N < 2^31; the offsets are required, the labels and their offsets when some utterance has a label (U1_max > 1)
int check_packed(int B, int T, int U1, long long N, int V, int blank, const int *labels, const int *frames_lengths,
                 const int *labels_lengths, const int *roff, const int *loff) {
    if (int rc = check_dims(B, T, U1, V, blank)) return rc;
    if (!frames_lengths || !labels_lengths || !roff || N <= 0) return PIKA_EINVAL;
    if (U1 > 1 && (!labels || !loff)) return PIKA_EINVAL;
    if (N > ROWS_MAX) return PIKA_ETOOBIG;
    if (N > (long long)B * T * U1) return PIKA_EINVAL;
    return PIKA_OK;
}

// the banded calls' shared checks: (B, T, U1, V, blank) as check_dims, 1 <= S <= U1, the lengths, the band starts and --
// when some utterance can have a label -- the labels; B*T*S rows index the row kernels as an int.  mod (the modified
// topology): the band starts may be null, which is the padded layout and needs S == U1.
int check_banded(bool mod, int B, int T, int U1, int S, int V, int blank, const int *labels, const int *ranges,
                 const int *frames_lengths, const int *labels_lengths) {
    if (V <= 0 || blank < 0 || blank >= V || B <= 0 || T <= 0 || U1 <= 0) return PIKA_EINVAL;
    if (S < 1 || S > U1) return PIKA_EINVAL;
    if (U1 > 1024) return PIKA_ETOOBIG;
    if (!frames_lengths || !labels_lengths || (!ranges && !mod) || (U1 > 1 && !labels)) return PIKA_EINVAL;
    if ((long long)B * T * S > ROWS_MAX) return PIKA_ETOOBIG;
    return (!ranges && S != U1) ? PIKA_EINVAL : PIKA_OK;
}

// The four loss entries of the banded (B,T,S,V) tensor, pika_prnnt_* and pika_prnnt_mod_*: they differ in `mod` alone.
int banded_forward(bool mod, const float *log_probs, const int *frames_lengths, const int *labels_lengths, const int *labels,
                   const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs, void *workspace,
                   void *stream) {
    if (int rc = check_banded(mod, B, T, U1, S, V, blank, labels, ranges, frames_lengths, labels_lengths)) return rc;
    if (!log_probs || !costs || !workspace) return PIKA_EINVAL;
    return loss_forward(banded_call(mod, labels, ranges, frames_lengths, labels_lengths, B, T, U1, S, V, blank, stream),
                        log_probs, costs, workspace);
}

int banded_backward(bool mod, const int *frames_lengths, const int *labels_lengths, const int *labels, const int *ranges,
                    int B, int T, int U1, int S, int V, int blank, const float *grad_costs, const void *workspace,
                    float *grads, float fastemit_lambda, void *stream) {
    if (int rc = check_banded(mod, B, T, U1, S, V, blank, labels, ranges, frames_lengths, labels_lengths)) return rc;
    if (!workspace) return PIKA_EINVAL;
    return loss_backward(banded_call(mod, labels, ranges, frames_lengths, labels_lengths, B, T, U1, S, V, blank, stream),
                         grad_costs, fastemit_lambda, workspace, grads);
}

int banded_fused_forward(bool mod, const float *logits, const int *frames_lengths, const int *labels_lengths,
                         const int *labels, const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs,
                         float *lse, void *workspace, void *stream) {
    if (int rc = check_banded(mod, B, T, U1, S, V, blank, labels, ranges, frames_lengths, labels_lengths)) return rc;
    if (!logits || !costs || !lse || !workspace || !logits_ok(logits, V)) return PIKA_EINVAL;
    return fused_forward(banded_call(mod, labels, ranges, frames_lengths, labels_lengths, B, T, U1, S, V, blank, stream),
                         logits, costs, lse, workspace);
}

int banded_fused_backward(bool mod, const float *logits, const float *lse, const int *frames_lengths,
                          const int *labels_lengths, const int *labels, const int *ranges, int B, int T, int U1, int S, int V,
                          int blank, const float *grad_costs, const void *workspace, void *grad_logits, int out_dtype,
                          long long ld_out, float fastemit_lambda, void *stream) {
    if (int rc = check_banded(mod, B, T, U1, S, V, blank, labels, ranges, frames_lengths, labels_lengths)) return rc;
    if (!logits || !lse || !workspace || !grad_logits) return PIKA_EINVAL;
    return fused_backward(banded_call(mod, labels, ranges, frames_lengths, labels_lengths, B, T, U1, S, V, blank, stream),
                          logits, lse, grad_costs, fastemit_lambda, workspace, grad_logits, out_dtype, ld_out);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// The C ABI (pika_rnnt.h): each entry is its checks, in the order and with the codes it has always had
// (tests/golden/rnnt_abi_rejections.json), a Call and a body.
// ---------------------------------------------------------------------------------------------
extern "C" {

int pika_amd_abi_version(void) { return 25; }

// padded layout (B,T,U1,V)
size_t pika_rnnt_workspace_bytes(int B, int T, int U1) {
    if (check_lattice_dims(B, T, U1)) return 0;
    return workspace_bytes(B, T, U1, false);
}

int pika_rnnt_loss_forward(const float *log_probs, const int *labels, const int *frames_lengths,
                           const int *labels_lengths, int B, int T, int U1, int V, int blank,
                           float *costs, void *workspace, void *stream) {
    if (int rc = forward_args_ok(B, T, U1, V, blank, log_probs && frames_lengths && labels_lengths && costs && workspace, labels))
        return rc;
    return loss_forward(padded_call(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, stream), log_probs, costs,
                        workspace);
}

int pika_rnnt_loss_backward_fe(const int *labels, const int *frames_lengths, const int *labels_lengths,
                               int B, int T, int U1, int V, int blank, const float *grad_costs,
                               const void *workspace, float *grads, float fastemit_lambda, void *stream) {
    if (int rc = check_dims(B, T, U1, V, blank)) return rc;
    if (!frames_lengths || !labels_lengths || !workspace) return PIKA_EINVAL;
    if (U1 > 1 && !labels) return PIKA_EINVAL;
    return loss_backward(padded_call(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, stream), grad_costs,
                         fastemit_lambda, workspace, grads);
}

int pika_rnnt_loss_backward(const int *labels, const int *frames_lengths, const int *labels_lengths,
                            int B, int T, int U1, int V, int blank, const float *grad_costs,
                            const void *workspace, float *grads, void *stream) {
    return pika_rnnt_loss_backward_fe(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, grad_costs, workspace,
                                      grads, 0.0f, stream);
}

int pika_rnnt_loss_dense_grads(const void *workspace, int B, int T, int U1, int V, int blank, float *grads,
                               void *stream) {
    if (int rc = check_dims(B, T, U1, V, blank)) return rc;
    if (!workspace || !grads) return PIKA_EINVAL;
    const Lattice L = carve(const_cast<void *>(workspace), B, T, U1);
    return write_dense_grads(L, (size_t)B * T * U1, V, blank, grads, static_cast<hipStream_t>(stream));
}

int pika_rgrad_dense_grads_update(const void *workspace, int B, int T, int U1, int V, int blank, float *grads,
                                  const int *prev_cols, long long prev_rows, int prev_blank, int *cols_out, void *stream) {
    if (int rc = check_dims(B, T, U1, V, blank)) return rc;
    if (!workspace || !grads) return PIKA_EINVAL;
    const PrevGrad p{prev_cols, prev_rows, prev_blank, cols_out};
    if (int rc = check_prev_grad(p, V)) return rc;
    const Lattice L = carve(const_cast<void *>(workspace), B, T, U1);
    return write_or_update_dense_grads(L, (long long)B * T * U1, V, blank, grads, p, static_cast<hipStream_t>(stream));
}

int pika_rgrad_backward_fe(const int *labels, const int *frames_lengths, const int *labels_lengths, int B, int T, int U1,
                           int V, int blank, const float *grad_costs, const void *workspace, float *grads,
                           float fastemit_lambda, const int *prev_cols, long long prev_rows, int prev_blank, int *cols_out,
                           void *stream) {
    return pika_rgrad_backward_fe_s(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, grad_costs, 1, workspace,
                                    grads, fastemit_lambda, prev_cols, prev_rows, prev_blank, cols_out, stream);
}

int pika_rgrad_backward_fe_s(const int *labels, const int *frames_lengths, const int *labels_lengths, int B, int T, int U1,
                             int V, int blank, const float *grad_costs, long long gc_stride, const void *workspace,
                             float *grads, float fastemit_lambda, const int *prev_cols, long long prev_rows, int prev_blank,
                             int *cols_out, void *stream) {
    if (int rc = check_dims(B, T, U1, V, blank)) return rc;
    if (!frames_lengths || !labels_lengths || !workspace || !grads) return PIKA_EINVAL;
    if (U1 > 1 && !labels) return PIKA_EINVAL;
    const PrevGrad p{prev_cols, prev_rows, prev_blank, cols_out};
    if (int rc = check_prev_grad(p, V)) return rc;
    const Call c = padded_call(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, stream);
    if (c.rows > ROWS_MAX) return PIKA_ETOOBIG;
    if (gc_stride < 0) return PIKA_EINVAL;
    const Lattice L = carve(const_cast<void *>(workspace), B, T, U1);
    if (p.cols) return rowmeta_and_update_dense_grads(c, L, grad_costs, gc_stride, fastemit_lambda, grads, p);   // one launch
    if (int rc = loss_backward(c, grad_costs, fastemit_lambda, workspace, nullptr, (long)gc_stride)) return rc;   // the row metadata
    return write_or_update_dense_grads(L, c.rows, V, blank, grads, p, c.s);
}

int pika_rnnt_loss_fwd_bwd(const float *log_probs, const int *labels, const int *frames_lengths,
                           const int *labels_lengths, int B, int T, int U1, int V, int blank,
                           float *costs, float *grads, void *workspace, void *stream) {
    if (int rc = pika_rnnt_loss_forward(log_probs, labels, frames_lengths, labels_lengths, B, T, U1,
                                        V, blank, costs, workspace, stream))
        return rc;
    return pika_rnnt_loss_backward(labels, frames_lengths, labels_lengths, B, T, U1, V, blank,
                                   nullptr, workspace, grads, stream);
}

int pika_rnnt_export_lattice(const void *workspace, const int *frames_lengths,
                             const int *labels_lengths, int B, int T, int U1, float *alphas,
                             float *betas, void *stream) {
    // (U1 > 1024 is PIKA_EINVAL here, PIKA_ETOOBIG in the calls that fill the workspace: kept)
    if (check_lattice_dims(B, T, U1) || !workspace || !frames_lengths || !labels_lengths) return PIKA_EINVAL;
    const Lattice L = carve(const_cast<void *>(workspace), B, T, U1);
    const size_t cells = (size_t)B * T * U1;
    hipLaunchKernelGGL(rnnt_export_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), L.alpha, L.beta, L.off_a, L.off_b,
                       frames_lengths, labels_lengths, B, T, U1, L.Wp, L.D, alphas, betas);
    return (int)hipGetLastError();
}

int pika_rnnt_dlogits_compact_bf16(const float *log_probs, const float *lse, const void *workspace, int B, int T,
                                   int U1, int V, int blank, void *out, long long ld_out, float scale,
                                   float *colsum, void *stream) {
    // (both compact calls: U1 > 1024 is PIKA_EINVAL, where the calls that fill the workspace answer PIKA_ETOOBIG: kept)
    if (check_dims(B, T, U1, V, blank) || !log_probs || !workspace || !out) return PIKA_EINVAL;
    if ((V & 3) || V > V_MAX || ld_out < V || (ld_out & 3) || ld_out > V_MAX ||
        (reinterpret_cast<uintptr_t>(log_probs) & 15) || (reinterpret_cast<uintptr_t>(out) & 7))
        return PIKA_EINVAL;
    return launch_dlogits_compact<float>(log_probs, 0, compact8_ok_f32(V, ld_out, out), lse, workspace, B, T, U1, V, blank, out,
                                         ld_out, scale, colsum, nullptr, nullptr, 0, stream);
}

int pika_rnnt_dlogits_compact_bf16_f16in(const void *logits16, long long ld_in, const float *lse, const void *workspace,
                                         int B, int T, int U1, int V, int blank, void *out, long long ld_out, float scale,
                                         float *colsum, const float *gathered, const int *g_labels, int g_blank,
                                         void *stream) {
    if (gathered && !g_labels) return PIKA_EINVAL;
    if (check_dims(B, T, U1, V, blank) || !logits16 || !lse || !workspace || !out) return PIKA_EINVAL;
    if ((V & 3) || V > V_MAX || ld_out < V || (ld_out & 3) || ld_out > V_MAX || ld_in < V || (ld_in & 3) ||
        (reinterpret_cast<uintptr_t>(logits16) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
        return PIKA_EINVAL;
    return launch_dlogits_compact<_Float16>(static_cast<const _Float16 *>(logits16), ld_in,
                                            compact8_ok_f16(V, ld_out, ld_in, out, logits16), lse, workspace, B, T, U1, V,
                                            blank, out, ld_out, scale, colsum, gathered, g_labels, g_blank, stream);
}

int pika_rnnt_fused_forward(const float *logits, const int *labels, const int *frames_lengths,
                            const int *labels_lengths, int B, int T, int U1, int V, int blank, float *costs,
                            float *lse, void *workspace, void *stream) {
    long long rows;
    if (int rc = forward_args_ok(B, T, U1, V, blank, logits && frames_lengths && labels_lengths && costs && lse && workspace &&
                                 logits_ok(logits, V), labels, &rows))
        return rc;
    return fused_forward(padded_call(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, stream), logits, costs, lse,
                         workspace);
}

// (the partials and gathered forwards: their own fill launch, the padded layout only)
int pika_rnnt_fused_forward_partials(const float *logits, const float *pmax, const float *psum, int n_part,
                                     const int *labels, const int *frames_lengths, const int *labels_lengths, int B,
                                     int T, int U1, int V, int blank, float *costs, float *lse, void *workspace,
                                     void *stream) {
    long long rows;
    if (int rc = forward_args_ok(B, T, U1, V, blank, logits && pmax && psum && n_part > 0 && frames_lengths && labels_lengths &&
                                 costs && lse && workspace, labels, &rows))
        return rc;
    const Call c = padded_call(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, stream);
    const Lattice L = carve(workspace, B, T, U1);
    hipLaunchKernelGGL(rnnt_lse_merge_gather_kernel<false>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, c.s, logits,
                       pmax, psum, n_part, labels, frames_lengths, labels_lengths, rows, T, U1, V, blank, lse, L.lpb, L.lpe,
                       L.Wp, L.D, static_cast<const _Float16 *>(nullptr), 0LL, static_cast<const float *>(nullptr),
                       static_cast<const int *>(nullptr), 0);
    return finish_forward(c, L, costs);
}

int pika_rnnt_fused_forward_gathered(const void *logits16, long long ld16, const float *gathered, const int *g_labels,
                                     int g_blank, const float *pmax, const float *psum, int n_part, const int *labels,
                                     const int *frames_lengths, const int *labels_lengths, int B, int T, int U1, int V,
                                     int blank, float *costs, float *lse, void *workspace, void *stream) {
    long long rows;
    if (int rc = forward_args_ok(B, T, U1, V, blank, logits16 && ld16 >= V && gathered && pmax && psum && n_part > 0 &&
                                 frames_lengths && labels_lengths && costs && lse && workspace, labels, &rows))
        return rc;
    const Call c = padded_call(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, stream);
    const Lattice L = carve(workspace, B, T, U1);
    hipLaunchKernelGGL(rnnt_lse_merge_gather_kernel<true>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, c.s,
                       static_cast<const float *>(nullptr), pmax, psum, n_part, labels, frames_lengths, labels_lengths, rows,
                       T, U1, V, blank, lse, L.lpb, L.lpe, L.Wp, L.D, static_cast<const _Float16 *>(logits16), ld16, gathered,
                       g_labels, g_blank);
    return finish_forward(c, L, costs);
}

int pika_rnnt_fused_backward_fe(const float *logits, const float *lse, const int *labels,
                                const int *frames_lengths, const int *labels_lengths, int B, int T, int U1, int V,
                                int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                                int out_dtype, long long ld_out, float fastemit_lambda, void *stream) {
    if (int rc = check_dims(B, T, U1, V, blank)) return rc;
    if (!logits || !lse || !frames_lengths || !labels_lengths || !workspace || !grad_logits) return PIKA_EINVAL;
    if (U1 > 1 && !labels) return PIKA_EINVAL;
    return fused_backward(padded_call(labels, frames_lengths, labels_lengths, B, T, U1, V, blank, stream), logits, lse,
                          grad_costs, fastemit_lambda, workspace, grad_logits, out_dtype, ld_out);
}

int pika_rnnt_fused_backward(const float *logits, const float *lse, const int *labels,
                             const int *frames_lengths, const int *labels_lengths, int B, int T, int U1, int V,
                             int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                             int out_dtype, long long ld_out, void *stream) {
    return pika_rnnt_fused_backward_fe(logits, lse, labels, frames_lengths, labels_lengths, B, T, U1, V, blank, grad_costs,
                                       workspace, grad_logits, out_dtype, ld_out, 0.0f, stream);
}

// packed layout (N, V): the lattice planes, alpha/beta and the workspace of a padded (B, T_max, U1_max) batch
int pika_rnnt_packed_forward(const float *log_probs, const int *labels, const int *frames_lengths,
                             const int *labels_lengths, const int *row_offsets, const int *label_offsets, int B,
                             int T_max, int U1_max, long long N, int V, int blank, float *costs, void *workspace,
                             void *stream) {
    if (int rc = check_packed(B, T_max, U1_max, N, V, blank, labels, frames_lengths, labels_lengths, row_offsets,
                              label_offsets))
        return rc;
    if (!log_probs || !costs || !workspace) return PIKA_EINVAL;
    return loss_forward(packed_call(labels, frames_lengths, labels_lengths, row_offsets, label_offsets, B, T_max, U1_max, N, V,
                                    blank, stream), log_probs, costs, workspace);
}

int pika_rnnt_packed_backward(const int *labels, const int *frames_lengths, const int *labels_lengths,
                              const int *row_offsets, const int *label_offsets, int B, int T_max, int U1_max,
                              long long N, int V, int blank, const float *grad_costs, const void *workspace,
                              float *grads, float fastemit_lambda, void *stream) {
    if (int rc = check_packed(B, T_max, U1_max, N, V, blank, labels, frames_lengths, labels_lengths, row_offsets,
                              label_offsets))
        return rc;
    if (!workspace) return PIKA_EINVAL;
    return loss_backward(packed_call(labels, frames_lengths, labels_lengths, row_offsets, label_offsets, B, T_max, U1_max, N, V,
                                     blank, stream), grad_costs, fastemit_lambda, workspace, grads);
}

int pika_rnnt_packed_fused_forward(const float *logits, const int *labels, const int *frames_lengths,
                                   const int *labels_lengths, const int *row_offsets, const int *label_offsets, int B,
                                   int T_max, int U1_max, long long N, int V, int blank, float *costs, float *lse,
                                   void *workspace, void *stream) {
    if (int rc = check_packed(B, T_max, U1_max, N, V, blank, labels, frames_lengths, labels_lengths, row_offsets,
                              label_offsets))
        return rc;
    if (!logits || !costs || !lse || !workspace || !logits_ok(logits, V)) return PIKA_EINVAL;
    return fused_forward(packed_call(labels, frames_lengths, labels_lengths, row_offsets, label_offsets, B, T_max, U1_max, N, V,
                                     blank, stream), logits, costs, lse, workspace);
}

int pika_rnnt_packed_fused_backward(const float *logits, const float *lse, const int *labels,
                                    const int *frames_lengths, const int *labels_lengths, const int *row_offsets,
                                    const int *label_offsets, int B, int T_max, int U1_max, long long N, int V,
                                    int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                                    int out_dtype, long long ld_out, float fastemit_lambda, void *stream) {
    if (int rc = check_packed(B, T_max, U1_max, N, V, blank, labels, frames_lengths, labels_lengths, row_offsets,
                              label_offsets))
        return rc;
    if (!logits || !lse || !workspace || !grad_logits) return PIKA_EINVAL;
    return fused_backward(packed_call(labels, frames_lengths, labels_lengths, row_offsets, label_offsets, B, T_max, U1_max, N,
                                      V, blank, stream), logits, lse, grad_costs, fastemit_lambda, workspace, grad_logits,
                          out_dtype, ld_out);
}

// forced alignment: Viterbi over the lpb / lpe planes any forward call of the regular topology left
size_t pika_rnnt_align_scratch_bytes(int B, int T, int U1) {
    if (check_lattice_dims(B, T, U1)) return 0;
    return (size_t)B * (size_t)(T + U1 - 1) * (size_t)(lattice_width(U1) / 64) * sizeof(unsigned long long);
}

int pika_rnnt_align(const void *workspace, const int *frames_lengths, const int *labels_lengths,
                    const int *label_offsets, int B, int T, int U1, float *scores, int *emit_frames, void *scratch,
                    void *stream) {
    if (int rc = check_lattice_dims(B, T, U1)) return rc;
    if (!workspace || !frames_lengths || !labels_lengths || !scores || !scratch) return PIKA_EINVAL;
    if (U1 > 1 && !emit_frames) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Lattice L = carve(const_cast<void *>(workspace), B, T, U1);
    const bool ok = dispatch_nw(L.Wp / 64, [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        hipLaunchKernelGGL((rnnt_align_kernel<NW>), dim3(B), dim3(NW * 64), 0, s, L.lpb, L.lpe, frames_lengths, labels_lengths,
                           label_offsets, scores, emit_frames, static_cast<unsigned long long *>(scratch), T, U1, L.Wp, L.D);
    });
    return ok ? (int)hipGetLastError() : PIKA_ETOOBIG;
}

// pruned (banded) lattice (B,T,S,V): the planes, alpha/beta and the workspace of the padded (B, T, U1) batch
int pika_prnnt_forward(const float *log_probs, const int *frames_lengths, const int *labels_lengths, const int *labels,
                       const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs, void *workspace,
                       void *stream) {
    return banded_forward(false, log_probs, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank, costs,
                          workspace, stream);
}

int pika_prnnt_backward(const int *frames_lengths, const int *labels_lengths, const int *labels, const int *ranges, int B,
                        int T, int U1, int S, int V, int blank, const float *grad_costs, const void *workspace,
                        float *grads, float fastemit_lambda, void *stream) {
    return banded_backward(false, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank, grad_costs, workspace,
                           grads, fastemit_lambda, stream);
}

int pika_prnnt_fused_forward(const float *logits, const int *frames_lengths, const int *labels_lengths, const int *labels,
                             const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs, float *lse,
                             void *workspace, void *stream) {
    return banded_fused_forward(false, logits, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank, costs,
                                lse, workspace, stream);
}

int pika_prnnt_fused_backward(const float *logits, const float *lse, const int *frames_lengths, const int *labels_lengths,
                              const int *labels, const int *ranges, int B, int T, int U1, int S, int V, int blank,
                              const float *grad_costs, const void *workspace, void *grad_logits, int out_dtype,
                              long long ld_out, float fastemit_lambda, void *stream) {
    return banded_fused_backward(false, logits, lse, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank,
                                 grad_costs, workspace, grad_logits, out_dtype, ld_out, fastemit_lambda, stream);
}

int pika_prnnt_planes_forward(const float *blank_lp, const float *label_lp, const int *frames_lengths,
                              const int *labels_lengths, int B, int T, int U1, float *costs, float *blank_occ,
                              float *label_occ, void *workspace, void *stream) {
    return planes_forward<false>(blank_lp, label_lp, frames_lengths, labels_lengths, B, T, U1, costs, blank_occ, label_occ,
                                 workspace, stream);
}

int pika_prnnt_prune_ranges(const float *blank_occ, const float *label_occ, const int *frames_lengths,
                            const int *labels_lengths, int B, int T, int U1, int S, int *ranges, void *stream) {
    return prune_ranges(S - 1, blank_occ, label_occ, frames_lengths, labels_lengths, B, T, U1, S, ranges, stream);
}

// modified topology: un-skewed planes and their own alpha/beta over a workspace of pika_prnnt_mod_workspace_bytes; the row
// metadata is the regular RowMeta, so the flat writer and the fused d(logits) kernel run unchanged.  ranges == NULL: the
// padded (B, T, U1, V) layout (S must be U1); else the banded (B, T, S, V) one.
size_t pika_prnnt_mod_workspace_bytes(int B, int T, int U1) {
    if (check_lattice_dims(B, T, U1)) return 0;
    return workspace_bytes(B, T, U1, true);
}

int pika_prnnt_mod_forward(const float *log_probs, const int *frames_lengths, const int *labels_lengths, const int *labels,
                           const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs, void *workspace,
                           void *stream) {
    return banded_forward(true, log_probs, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank, costs,
                          workspace, stream);
}

int pika_prnnt_mod_backward(const int *frames_lengths, const int *labels_lengths, const int *labels, const int *ranges, int B,
                            int T, int U1, int S, int V, int blank, const float *grad_costs, const void *workspace,
                            float *grads, float fastemit_lambda, void *stream) {
    return banded_backward(true, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank, grad_costs, workspace,
                           grads, fastemit_lambda, stream);
}

int pika_prnnt_mod_fused_forward(const float *logits, const int *frames_lengths, const int *labels_lengths,
                                 const int *labels, const int *ranges, int B, int T, int U1, int S, int V, int blank,
                                 float *costs, float *lse, void *workspace, void *stream) {
    return banded_fused_forward(true, logits, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank, costs, lse,
                                workspace, stream);
}

int pika_prnnt_mod_fused_backward(const float *logits, const float *lse, const int *frames_lengths,
                                  const int *labels_lengths, const int *labels, const int *ranges, int B, int T, int U1, int S,
                                  int V, int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                                  int out_dtype, long long ld_out, float fastemit_lambda, void *stream) {
    return banded_fused_backward(true, logits, lse, frames_lengths, labels_lengths, labels, ranges, B, T, U1, S, V, blank,
                                 grad_costs, workspace, grad_logits, out_dtype, ld_out, fastemit_lambda, stream);
}

int pika_prnnt_mod_planes_forward(const float *blank_lp, const float *label_lp, const int *frames_lengths,
                                  const int *labels_lengths, int B, int T, int U1, float *costs, float *blank_occ,
                                  float *label_occ, void *workspace, void *stream) {
    return planes_forward<true>(blank_lp, label_lp, frames_lengths, labels_lengths, B, T, U1, costs, blank_occ, label_occ,
                                workspace, stream);
}

int pika_prnnt_mod_prune_ranges(const float *blank_occ, const float *label_occ, const int *frames_lengths,
                                const int *labels_lengths, int B, int T, int U1, int S, int *ranges, void *stream) {
    return prune_ranges(1, blank_occ, label_occ, frames_lengths, labels_lengths, B, T, U1, S, ranges, stream);
}

// forced alignment in the modified topology: Viterbi over the un-skewed lpb / lpe planes any pika_prnnt_mod_*forward left
size_t pika_mrnnt_align_scratch_bytes(int B, int T, int U1) {
    if (check_lattice_dims(B, T, U1)) return 0;
    return (size_t)B * (size_t)(T + 1) * (size_t)(lattice_width(U1) / 64) * sizeof(unsigned long long);
}

int pika_mrnnt_align(const void *workspace, const int *frames_lengths, const int *labels_lengths, int B, int T, int U1,
                     float *scores, int *emit_frames, void *scratch, void *stream) {
    if (int rc = check_lattice_dims(B, T, U1)) return rc;
    if (!workspace || !frames_lengths || !labels_lengths || !scores || !scratch) return PIKA_EINVAL;
    if (U1 > 1 && !emit_frames) return PIKA_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Lattice L = carve(const_cast<void *>(workspace), B, T, U1, /*mod=*/true);
    const bool ok = dispatch_nw(L.Wp / 64, [&](auto nw) {
        constexpr int NW = decltype(nw)::value;
        hipLaunchKernelGGL((rnnt_mod_align_kernel<NW>), dim3(B), dim3(NW * 64), 0, s, L.lpb, L.lpe, frames_lengths,
                           labels_lengths, scores, emit_frames, static_cast<unsigned long long *>(scratch), T, U1, L.D);
    });
    return ok ? (int)hipGetLastError() : PIKA_ETOOBIG;
}

}  // extern "C"
