// pika_amd/csrc/ctc_edit.hip -- token edit (Levenshtein) distances between the entries of two lists per utterance, on the
// device (include/pika_ctc.h: pika_ctc_edit_distance, pika_ctc_edit_distance_host).  What MWER training needs between a
// search's n-best list and the reference transcript, and MBR decoding between the entries of the list itself.
//
// One wave64 per (b, i, j) pair; the recurrence is ctc_edit_core.h's bit-vector step with the wave's 64-bit ballot as the
// machine word.  The reference side r is the pattern: lane l holds r[64 w + l] of the current block, and the match vector
// of a hypothesis token c is __ballot(r_lane == c), masked to the positions below S -- there is no per-class table, so the
// vocabulary costs nothing and any int32 is a token.  The state (pv, mv) of block w rests in lane w (64 lanes: 4096
// positions); while a block is worked on, its state and all carries are wave-uniform values.
//
// Order of the work, the same on the host: the hypothesis in chunks of 64 tokens (lane l holds token j0 + l); inside a
// chunk block after block; inside a block token after token.  The horizontal differences that block w hands to block w+1
// for the chunk's 64 columns are two 64-bit words (one bit per column: +1, -1), so nothing per column is ever stored.
// The differences that leave the LAST block -- read at bit (S-1) % 64 -- are the changes of D[S][j] along the chunk: the
// score moves by popcount(plus) - popcount(minus).  Work per pair: n * ceil(S / 64) steps against the DP's n * S cells.
#include <hip/hip_runtime.h>

#include <limits.h>

#include "ctc_edit_core.h"
#include "pika_ctc.h"

namespace {

__device__ inline edit_word lane_get(edit_word v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((edit_word)hi << 32) | lo;
}

// grid: any number of 64-thread workgroups, striding over the pairs; p = (b Na + i) Nr + j
__global__ __launch_bounds__(64) void ctc_edit_kernel(const int *__restrict__ a_tokens, const int *__restrict__ a_lengths,
                                                      int Na, int La, const int *__restrict__ r_tokens,
                                                      const int *__restrict__ r_lengths, int Nr, int Lr, long long pairs,
                                                      int *__restrict__ out) {
    const int lane = (int)threadIdx.x;
    for (long long p = blockIdx.x; p < pairs; p += gridDim.x) {
        const long long ai = p / Nr;                            // b Na + i
        const long long ri = ai / Na * Nr + (p - ai * Nr);      // b Nr + j
        const int n = ctc_edit_length(a_lengths[ai], La), S = ctc_edit_length(r_lengths[ri], Lr);
        int score = n < 0 || S < 0 ? -1 : S;                    // D[S][0] = S; S == 0: no block, one insertion per token
        if (n > 0 && S == 0) score = n;
        if (n > 0 && S > 0) {
            const int *a = a_tokens + (size_t)ai * La, *r = r_tokens + (size_t)ri * Lr;
            const int W = ctc_edit_blocks(S);
            edit_word pv_l = ~0ull, mv_l = 0ull;                // lane w: block w at column 0
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int nj = n - j0 < 64 ? n - j0 : 64;
                const int a_l = lane < nj ? a[j0 + lane] : 0;
                edit_word cp = ~0ull, cm = 0ull;                // into block 0: the boundary row, +1 per column
                for (int w = 0; w < W; ++w) {
                    const int pos = 64 * w + lane;
                    const int r_l = pos < S ? r[pos] : 0;       // one 256-byte load per 64 steps
                    const edit_word valid = ctc_edit_valid(S, w);
                    const int top = ctc_edit_top(S, w);
                    edit_word pv = lane_get(pv_l, w), mv = lane_get(mv_l, w), np = 0ull, nm = 0ull;
                    for (int j = 0; j < nj; ++j) {
                        const int c = __builtin_amdgcn_readlane(a_l, j);
                        const edit_word eq = __ballot(r_l == c) & valid;
                        edit_word hp, hm;
                        ctc_edit_step(eq, pv, mv, (cp >> j) & 1ull, (cm >> j) & 1ull, top, hp, hm);
                        np |= hp << j;
                        nm |= hm << j;
                    }
                    pv_l = lane == w ? pv : pv_l;
                    mv_l = lane == w ? mv : mv_l;
                    cp = np;
                    cm = nm;
                }
                score += __popcll(cp) - __popcll(cm);
            }
        }
        if (lane == 0) out[p] = score;
    }
}

// the same pair on the host: eq from a loop over the block's positions, everything else as above
int edit_pair_host(const int *a, int n, const int *r, int S) {
    if (n < 0 || S < 0) return -1;
    if (S == 0) return n;
    const int W = ctc_edit_blocks(S);
    edit_word pvs[PIKA_EDIT_MAX_REF / 64], mvs[PIKA_EDIT_MAX_REF / 64];
    for (int w = 0; w < W; ++w) {
        pvs[w] = ~0ull;
        mvs[w] = 0ull;
    }
    int score = S;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int nj = n - j0 < 64 ? n - j0 : 64;
        edit_word cp = ~0ull, cm = 0ull;
        for (int w = 0; w < W; ++w) {
            const int top = ctc_edit_top(S, w), rows = S - 64 * w < 64 ? S - 64 * w : 64;
            edit_word pv = pvs[w], mv = mvs[w], np = 0ull, nm = 0ull;
            for (int j = 0; j < nj; ++j) {
                edit_word eq = 0ull, hp, hm;
                for (int i = 0; i < rows; ++i) eq |= (edit_word)(r[64 * w + i] == a[j0 + j]) << i;
                ctc_edit_step(eq, pv, mv, (cp >> j) & 1ull, (cm >> j) & 1ull, top, hp, hm);
                np |= hp << j;
                nm |= hm << j;
            }
            pvs[w] = pv;
            mvs[w] = mv;
            cp = np;
            cm = nm;
        }
        score += __builtin_popcountll(cp) - __builtin_popcountll(cm);
    }
    return score;
}

// the refusals both entries share; *pairs receives B Na Nr.  1: nothing to do
int check_edit(const int *a_tokens, const int *a_lengths, int Na, int La, const int *r_tokens, const int *r_lengths,
               int Nr, int Lr, int B, const int *out, long long *pairs) {
    if (Na < 0 || La < 0 || Nr < 0 || Lr < 0 || B < 0) return PIKA_EINVAL;
    if (Lr > PIKA_EDIT_MAX_REF) return PIKA_ETOOBIG;
    if (Nr > 0 && (long long)B * Na > INT_MAX / Nr) return PIKA_ETOOBIG;
    *pairs = (long long)B * Na * Nr;
    if (*pairs == 0) return 1;
    if (!a_lengths || !r_lengths || !out || (La > 0 && !a_tokens) || (Lr > 0 && !r_tokens)) return PIKA_EINVAL;
    return PIKA_OK;
}

}  // namespace

extern "C" {

int pika_ctc_edit_distance(const int *a_tokens, const int *a_lengths, int Na, int La, const int *r_tokens,
                           const int *r_lengths, int Nr, int Lr, int B, int *out, void *stream) {
    long long pairs = 0;
    if (int rc = check_edit(a_tokens, a_lengths, Na, La, r_tokens, r_lengths, Nr, Lr, B, out, &pairs))
        return rc < 0 ? rc : PIKA_OK;
    const long long cap = 1 << 20;      // beyond that many workgroups each strides over several pairs
    hipLaunchKernelGGL(ctc_edit_kernel, dim3((unsigned)(pairs < cap ? pairs : cap)), dim3(64), 0,
                       static_cast<hipStream_t>(stream), a_tokens, a_lengths, Na, La, r_tokens, r_lengths, Nr, Lr, pairs,
                       out);
    return (int)hipGetLastError();
}

int pika_ctc_edit_distance_host(const int *a_tokens, const int *a_lengths, int Na, int La, const int *r_tokens,
                                const int *r_lengths, int Nr, int Lr, int B, int *out) {
    long long pairs = 0;
    if (int rc = check_edit(a_tokens, a_lengths, Na, La, r_tokens, r_lengths, Nr, Lr, B, out, &pairs))
        return rc < 0 ? rc : PIKA_OK;
    for (long long p = 0; p < pairs; ++p) {
        const long long ai = p / Nr, ri = ai / Na * Nr + (p - ai * Nr);
        out[p] = edit_pair_host(a_tokens + (size_t)ai * La, ctc_edit_length(a_lengths[ai], La),
                                r_tokens + (size_t)ri * Lr, ctc_edit_length(r_lengths[ri], Lr));
    }
    return PIKA_OK;
}

}  // extern "C"
