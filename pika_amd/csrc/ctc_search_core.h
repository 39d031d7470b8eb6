// pika_amd/csrc/ctc_search_core.h -- what the CTC prefix beam searches share (ctc_decode.hip: ctc_beam_kernel,
// ctc_lm.hip: ctc_lm_kernel, and the streaming kernels of both; not part of the C ABI): the beam, the trie of prefixes in
// an open-addressing table, the per-frame slot work, the total order of the arg-max, node assignment, the
// renormalisation, the n-best tail, the state a stream carries between launches and the host-side limits.  What differs
// -- which candidates a slot offers and how they are scored -- stays with each kernel.
#ifndef PIKA_CTC_SEARCH_CORE_H
#define PIKA_CTC_SEARCH_CORE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctc_numerics.h"
#include "pika_ctc_decode.h"  // PIKA_OK / PIKA_EINVAL / PIKA_ETOOBIG

namespace {

constexpr int MAX_BEAM = 64;
constexpr int MAX_CLASSES = 128;  // the frame's class list: the row pass's K
constexpr int RENORM = 8;         // frames between renormalisations
constexpr int ROOT = 0x7ffffffe;  // node of the empty prefix
constexpr int NONE = 0x7ffffffd;  // its parent
constexpr int PENDING = -1;
constexpr unsigned long long EMPTY = ~0ull;

struct Beam {
    int node[MAX_BEAM];   // the prefix: slot of its (parent, token) key in the utterance's table, ROOT for the empty one
    int last[MAX_BEAM];   // its last label, -1 for the empty prefix
    int pnode[MAX_BEAM];  // its parent's node
    int len[MAX_BEAM];
    float pb[MAX_BEAM], pnb[MAX_BEAM], tot[MAX_BEAM];
};

// the beam a search starts from: the empty prefix in slot 0
__device__ __forceinline__ void root_slot(Beam &A) {
    A.node[0] = ROOT; A.last[0] = -1; A.pnode[0] = NONE; A.len[0] = 0;
    A.pb[0] = 0.0f; A.pnb[0] = NEG; A.tot[0] = 0.0f;
}

// slot r from one beam to another (LDS <-> a stream's record)
__device__ __forceinline__ void copy_slot(Beam &D, const Beam &G, int r) {
    D.node[r] = G.node[r]; D.last[r] = G.last[r]; D.pnode[r] = G.pnode[r]; D.len[r] = G.len[r];
    D.pb[r] = G.pb[r]; D.pnb[r] = G.pnb[r]; D.tot[r] = G.tot[r];
}

// slot r of G into slot j of D (the commit closes the gaps that dropped slots leave)
__device__ __forceinline__ void move_slot(Beam &D, int j, const Beam &G, int r) {
    D.node[j] = G.node[r]; D.last[j] = G.last[r]; D.pnode[j] = G.pnode[r]; D.len[j] = G.len[r];
    D.pb[j] = G.pb[r]; D.pnb[j] = G.pnb[r]; D.tot[j] = G.tot[r];
}

__device__ inline unsigned long long trie_key(int parent, int token) {
    return ((unsigned long long)(unsigned)parent << 32) | (unsigned)token;
}

// insert-or-find: every probe is an atomic, so a slot is never seen through a stale cache line; only this workgroup
// touches the table
__device__ inline int trie_node(unsigned long long *table, unsigned mask, int parent, int token) {
    const unsigned long long key = trie_key(parent, token);
    unsigned h = ((unsigned)parent * 0x9E3779B1u) ^ ((unsigned)token * 0x85EBCA6Bu);
    h = (h ^ (h >> 15)) & mask;
    for (unsigned probes = 0; probes <= mask; ++probes) {  // at most T * beam <= (mask + 1) / 2 keys: it ends early
        const unsigned long long old = atomicCAS(&table[h], EMPTY, key);
        if (old == EMPTY || old == key) break;
        h = (h + 1) & mask;
    }
    return (int)h;
}

// the key of a node, read as it was inserted
__device__ inline unsigned long long trie_load(const unsigned long long *table, unsigned mask, int node) {
    return __hip_atomic_load(&table[(unsigned)node & mask], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a beam slot in its owner's registers
struct Slot {
    int node, last, pnode, len;
    float pb, pnb, tot;
};

// slot r of A if `act`, otherwise the values that stand for "no such slot".  A kernel reads its slot once per frame,
// before the gather of the slot's last label from the full row, so the LDS reads overlap that load.
__device__ __forceinline__ Slot load_slot(const Beam &A, int r, bool act) {
    return {act ? A.node[r] : NONE, act ? A.last[r] : -1, act ? A.pnode[r] : NONE, act ? A.len[r] : 0,
            act ? A.pb[r] : NEG, act ? A.pnb[r] : NEG, act ? A.tot[r] : NEG};
}

// (F, hi, lo) before (G, ghi, glo) in the total order: higher score, then the lower key
__device__ inline bool before(float F, unsigned hi, unsigned lo, float G, unsigned ghi, unsigned glo) {
    return F > G || (F == G && (hi < ghi || (hi == ghi && lo < glo)));
}

// The slot work of one frame, between two barriers that EVERY thread of the workgroup reaches.  A `slot` thread owns
// beam slot r; `me` is load_slot(A, r, slot && r < n), g the frame's value of the slot's last label.  Slot r < n finds
// its parent's slot (node identity) and the position of its own last label in the frame's class list ci[0..K), and
// strikes that position from its own list (the repeat is a candidate of its own, scored with p_b) and from its
// parent's (that child is in the beam: the contribution is added to it).  Out: the slot's (p_b, p_nb) and tot after
// the frame if it stays, and excl / hasrep complete.
__device__ __forceinline__ void slot_work(const Beam &A, int n, int r, bool slot, const Slot &me, const int *ci, int K,
                                          float lpb, float g, unsigned (*excl)[MAX_CLASSES / 32], int *hasrep,
                                          float &npb, float &npnb, float &s_stay) {
    if (slot) {
        for (int q = 0; q < MAX_CLASSES / 32; ++q) excl[r][q] = 0;
        hasrep[r] = 0;
    }
    __syncthreads();
    npb = NEG; npnb = NEG; s_stay = NEG;
    if (slot && r < n) {
        int ps = -1;  // the parent's slot, if the parent is in the beam
        if (me.pnode != NONE)
            for (int q = 0; q < n; ++q)
                if (A.node[q] == me.pnode) ps = q;
        int pos = -1;  // where the slot's last label stands in the frame's class list
        if (me.last >= 0)
            for (int j = 0; j < K; ++j)
                if (ci[j] == me.last) pos = j;
        if (pos >= 0) {
            atomicOr(&excl[r][pos >> 5], 1u << (pos & 31));               // the repeat
            if (ps >= 0) atomicOr(&excl[ps][pos >> 5], 1u << (pos & 31));  // the parent's child that is in the beam
        }
        const bool rep_child = ps >= 0 && A.last[ps] == me.last;
        if (rep_child) hasrep[ps] = 1;
        npb = addn(lpb, me.tot);
        if (me.last >= 0) npnb = addn(g, me.pnb);
        if (ps >= 0) npnb = lse2(npnb, addn(g, rep_child ? A.pb[ps] : A.tot[ps]));
        s_stay = lse2(npb, npnb);
    }
    __syncthreads();  // excl and hasrep are complete
}

// a fresh winner gets its node: the table slot of its (parent node, token) key
__device__ __forceinline__ void assign_node(Beam &N, int r, bool mine, unsigned long long *table, unsigned mask) {
    if (mine && N.node[r] == PENDING) N.node[r] = trie_node(table, mask, N.pnode[r], N.last[r]);
}

// frame t (counted from the utterance's first frame) ends with k > 0 slots and is the last of RENORM
// (workgroup-uniform)
__device__ inline bool renorm_due(int t, int k) { return t % RENORM == RENORM - 1 && k > 0; }

// subtracts the best tot from the slots (`mine`: this thread owns slot r < k) and returns it for the caller's fp64
// offset.  Every thread of the workgroup reaches the barrier.
__device__ __forceinline__ float renorm(Beam &N, int r, bool mine) {
    const float m = N.tot[0];  // slot 0 is the best: finite
    __syncthreads();
    if (mine) {
        N.pb[r] = N.pb[r] > NEG_HALF ? N.pb[r] - m : NEG;
        N.pnb[r] = N.pnb[r] > NEG_HALF ? N.pnb[r] - m : NEG;
        N.tot[r] = N.tot[r] - m;
    }
    return m;
}

// the n-best of utterance b by THREADS threads: entry k is slot perm(k) for k < n; lengths, -1 beyond each length (and
// for entries that do not exist), then the back-trace through the table.  Scores stay with the caller.  CLIP: a prefix
// may be longer than the T tokens the caller allocated (the streaming results); its labels beyond T are not written.
template <int THREADS, bool CLIP = false, class Perm>
__device__ __forceinline__ void write_nbest(const Beam &A, int n, Perm perm, int tid, int b, int T, int nbest,
                                            int *tokens, int *lengths, const unsigned long long *table,
                                            unsigned mask) {
    if (tid < nbest) lengths[(size_t)b * nbest + tid] = tid < n ? A.len[perm(tid)] : -1;
    for (int e = tid; e < nbest * T; e += THREADS) {
        const int kk = e / T, p = e - kk * T;
        if (kk >= n || p >= A.len[perm(kk)]) tokens[((size_t)b * nbest + kk) * T + p] = -1;
    }
    if (tid < nbest && tid < n) {
        const int src = perm(tid);
        int node = A.node[src];
        int *out = tokens + ((size_t)b * nbest + tid) * T;
        for (int p = A.len[src] - 1; p >= 0 && node != ROOT; --p) {  // len <= T_n <= T: one label per frame at most
            const unsigned long long key = trie_load(table, mask, node);
            if (!CLIP || p < T) out[p] = (int)(unsigned)(key & 0xffffffffull);
            node = (int)(unsigned)(key >> 32);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// streaming: the search is a function of (state, frame), so the state can rest in device memory between launches.
// A batch's blob is its B tables (sized for max_frames frames) followed by one record per stream.
// ---------------------------------------------------------------------------------------------
struct StreamHdr {
    int n;         // slots of the beam
    int frames;    // frames consumed: the phase of the renormalisation, and the table's fill
    int overflow;  // frames were dropped because max_frames was reached
    int retired;   // frames a commit has given back: frames + retired is what the stream consumed
    double off, boff;  // what was moved out of tot (and, with an LM, out of bonus)
};

static_assert(offsetof(StreamHdr, retired) == PIKA_CTC_STREAM_RETIRED_OFFSET && sizeof(StreamHdr) == 32,
              "the header the C ABI documents");

template <class BeamT>
struct StreamRec {
    StreamHdr h;
    BeamT beam;  // slots [0, n)
};

// what a launch may take from a record, read as it stands: a blob that was never reset holds anything, and n, frames and
// every len bound loops and stores
__device__ __forceinline__ StreamHdr load_hdr(const StreamHdr &G, int beam, int max_frames) {
    StreamHdr h = G;
    h.n = clampi(h.n, 0, beam);
    h.frames = clampi(h.frames, 0, max_frames);
    return h;
}

// Reset, one kernel for every record type.  grid = (B, y), block = 256: the workgroups (b, *) clear stream b's table,
// (b, 0) writes its record; streams with which[b] == 0 are not touched.  `start...` is what the search's root_slot takes
// after the beam: nothing, the LM's start state, or that and the second automaton's.
template <class BeamT, class... START>
__global__ __launch_bounds__(256) void ctc_stream_reset_kernel(unsigned long long *tables, size_t slots,
                                                               StreamRec<BeamT> *recs, const int *__restrict__ which,
                                                               START... start) {
    const int b = blockIdx.x;
    if (which && which[b] == 0) return;  // workgroup-uniform
    unsigned long long *table = tables + (size_t)b * slots;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < slots; i += (size_t)gridDim.y * 256) table[i] = EMPTY;
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        StreamRec<BeamT> &R = recs[b];
        R.h.n = 1; R.h.frames = 0; R.h.overflow = 0; R.h.retired = 0;
        R.h.off = 0.0; R.h.boff = 0.0;
        root_slot(R.beam, start...);
    }
}

// Commit, one kernel for every record type.  grid = B, block = 256; streams with which[b] == 0 keep their state and get
// length 0.  The prefix that every slot of the beam shares -- the path from the root to the slots' common ancestor -- can
// never change again: it goes to tokens[b], the trie is re-rooted at the ancestor, and the table is rebuilt with the
// nodes on the paths from the new root to the slots and nothing else.  max_tail >= 0: when slot 0 would keep more than
// max_tail labels, the new root is slot 0's ancestor max_tail labels up, and the slots that do not descend from it are
// dropped (the others keep their order).  A node's identity is the table slot of its (parent, token) key, so a rebuilt
// table needs the parents first: wave 0's lane r walks slot r up to the new root and leaves the labels it meets in
// paths[b][r][0, tail), root side first; the table is cleared; the lane replays its labels through trie_node from ROOT.
// Lanes that share a prefix find each other's keys.  Then `frames` is lowered to what the live keys and the longest
// tail need, in the same phase of the renormalisation, and the difference goes to `retired`.  Everything read from the
// record bounds loops and stores through load_hdr and the clamp of len, and every walk by a step count: a blob that was
// never reset ends with some beam, inside its own memory.
template <class BeamT>
__global__ __launch_bounds__(256) void ctc_stream_commit_kernel(unsigned long long *tables, unsigned mask,
                                                                StreamRec<BeamT> *recs, const int *__restrict__ which,
                                                                int beam, int max_frames, int max_tail, int L,
                                                                int *__restrict__ tokens, int *__restrict__ lengths,
                                                                int *__restrict__ paths) {
    __shared__ BeamT S;
    __shared__ int s_depth, s_live, s_tail, s_n;
    const int b = blockIdx.x, tid = threadIdx.x, r = tid;
    int *out = tokens + (size_t)b * L;
    if (which && which[b] == 0) {  // workgroup-uniform
        for (int p = tid; p < L; p += 256) out[p] = -1;
        if (tid == 0) lengths[b] = 0;
        return;
    }
    unsigned long long *table = tables + (size_t)b * ((size_t)mask + 1);
    StreamRec<BeamT> &R = recs[b];
    const StreamHdr h = load_hdr(R.h, beam, max_frames);
    const int n = h.n;
    // one step towards the root; whatever a node holds, the load stays inside the table
    auto up = [&](int node) __attribute__((always_inline)) {
        return node == ROOT ? ROOT : (int)(unsigned)(trie_load(table, mask, node) >> 32);
    };
    int tail = -1, j = 0;  // wave 0, lane r: the labels slot r keeps (-1: the slot is dropped), its slot afterwards
    if (tid < 64) {        // wave 0: lane r owns beam slot r
        const bool act = r < n;
        if (act) copy_slot(S, R.beam, r);
        const int node = act ? R.beam.node[r] : ROOT;
        const int len = act ? clampi(R.beam.len[r], 0, h.frames) : 0;
        // the common ancestor: every slot up to the depth of the shallowest, then all of them in step until they meet
        int lmin = act ? len : 0x7fffffff;
        for (int o = 32; o > 0; o >>= 1) lmin = min(lmin, __shfl_xor(lmin, o));
        if (n == 0) lmin = 0;
        int cur = node;
        for (int k = len - lmin; k > 0; --k) cur = up(cur);  // (no slot: len = 0, no step)
        int steps = 0, first;
        bool same;
        for (;; ++steps) {  // wave-uniform
            first = __shfl(cur, 0);
            same = __all(!act || cur == first);
            if (same || steps >= lmin) break;
            cur = up(cur);
        }
        int depth = same ? lmin - steps : 0;  // labels from the root to the new root
        int root = same ? first : ROOT;       // (no meeting point within lmin steps: not a trie; nothing is shared)
        const int len0 = __shfl(len, 0);
        if (max_tail >= 0 && n > 0 && len0 - depth > max_tail) {  // wave-uniform: forced
            int c = node;
            if (r == 0)
                for (int k = 0; k < max_tail; ++k) c = up(c);  // max_tail < len0 <= frames
            root = __shfl(c, 0);
            depth = len0 - max_tail;
        }
        if (r == 0) {  // the committed labels, back from the new root; L may be narrower than the prefix
            int c = root;
            for (int p = depth - 1; p >= 0; --p) {
                int tok = -1;
                if (c != ROOT) {
                    const unsigned long long key = trie_load(table, mask, c);
                    tok = (int)(unsigned)(key & 0xffffffffull);
                    c = (int)(unsigned)(key >> 32);
                }
                if (p < L) out[p] = tok;
            }
            lengths[b] = depth;
            s_depth = depth;
            s_live = 0;
        }
        // the labels between the new root and the slot; a slot stays if that walk ends at the new root
        if (act && len >= depth) {
            const int tl = len - depth;  // <= frames <= max_frames
            int *path = paths + ((size_t)b * beam + r) * max_frames;
            int c = node;
            for (int k = 0; k < tl; ++k) {
                const unsigned long long key = trie_load(table, mask, c);
                path[tl - 1 - k] = (int)(unsigned)(key & 0xffffffffull);
                c = c == ROOT ? ROOT : (int)(unsigned)(key >> 32);
            }
            if (c == root) tail = tl;
        }
        const unsigned long long kept = __ballot(tail >= 0);
        j = __popcll(kept & ((1ull << r) - 1ull));
        int tmax = tail;
        for (int o = 32; o > 0; o >>= 1) tmax = max(tmax, __shfl_xor(tmax, o));
        if (r == 0) { s_n = __popcll(kept); s_tail = max(tmax, 0); }
    }
    __syncthreads();  // every walk through the old table is over; S holds the beam
    for (int p = s_depth + tid; p < L; p += 256) out[p] = -1;
    for (size_t i = tid; i <= (size_t)mask; i += 256) table[i] = EMPTY;
    __syncthreads();  // the table is empty
    if (tail >= 0) {  // (wave 0's lanes of the slots that stay)
        const int *path = paths + ((size_t)b * beam + r) * max_frames;
        int node = ROOT, pnode = NONE;
        for (int k = 0; k < tail; ++k) {
            pnode = node;
            node = trie_node(table, mask, node, path[k]);
        }
        move_slot(R.beam, j, S, r);
        R.beam.node[j] = node; R.beam.pnode[j] = pnode; R.beam.len[j] = tail;
    }
    __syncthreads();  // the table holds the live keys
    int live = 0;
    for (size_t i = tid; i <= (size_t)mask; i += 256) live += trie_load(table, mask, (int)i) != EMPTY;
    if (live) atomicAdd(&s_live, live);
    __syncthreads();
    if (tid == 0) {
        // the fewest frames that account for the live keys (beam per frame) and for the longest prefix, in the phase
        // of the renormalisation that `frames` had; never more than before
        const int need = max((s_live + beam - 1) / beam, s_tail);
        int fnew = need + (((h.frames - need) % RENORM) + RENORM) % RENORM;
        if (fnew > h.frames) fnew = h.frames;
        R.h.n = s_n; R.h.frames = fnew; R.h.retired += h.frames - fnew;
    }
}

// the frames of a chunk that stream b takes: its length clamped to [0, Tc], cut where max_frames would be passed
// (`cut`: frames were dropped)
__device__ __forceinline__ int stream_frames(const int *len, int b, int Tc, int frames, int max_frames, bool &cut) {
    const int L = clampi(len[b], 0, Tc);
    cut = L > max_frames - frames;
    return cut ? max_frames - frames : L;
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static inline size_t table_slots(int T, int beam) {
    size_t n = 64;
    while (n < 2 * (size_t)T * beam) n <<= 1;
    return n;
}

// `classes`: the length of the frame's class list
static inline int check_search_dims(int B, int T, int beam, int classes) {
    if (B <= 0 || T <= 0 || beam <= 0 || classes <= 0) return PIKA_EINVAL;
    if (beam > MAX_BEAM || classes > MAX_CLASSES || B > 65535 || 2ll * T * beam > (1ll << 28)) return PIKA_ETOOBIG;
    return PIKA_OK;
}

static inline size_t table_bytes(int B, int T, int beam) { return 8 * (size_t)B * table_slots(T, beam); }

// every key of the B tables EMPTY
static inline hipError_t clear_tables(void *scratch, int B, int T, int beam, hipStream_t s) {
    return hipMemsetAsync(scratch, 0xff, table_bytes(B, T, beam), s);
}

// the streaming calls: where the blob's parts lie
template <class Rec>
static inline Rec *stream_recs(const void *state, int B, int max_frames, int beam) {
    return reinterpret_cast<Rec *>(static_cast<char *>(const_cast<void *>(state)) + table_bytes(B, max_frames, beam));
}

// the whole of a reset entry point behind its own arguments' checks (`classes` as check_search_dims)
template <class BeamT, class... START>
static int reset_streams(void *state, int B, int max_frames, int beam, int classes, const int *which, void *stream,
                         START... start) {
    if (int rc = check_search_dims(B, max_frames, beam, classes)) return rc;
    if (!state) return PIKA_EINVAL;
    const size_t slots = table_slots(max_frames, beam), y = slots / 4096;  // 16 keys per thread
    hipLaunchKernelGGL((ctc_stream_reset_kernel<BeamT, START...>),
                       dim3((unsigned)B, (unsigned)(y < 1 ? 1 : (y > 256 ? 256 : y))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<unsigned long long *>(state), slots,
                       stream_recs<StreamRec<BeamT>>(state, B, max_frames, beam), which, start...);
    return (int)hipGetLastError();
}

// what a commit needs beside the state: per stream and slot, the labels of a prefix of max_frames frames (a quarter of
// the tables at most)
static inline size_t commit_scratch_bytes(int B, int max_frames, int beam) {
    return sizeof(int) * (size_t)B * beam * max_frames;
}

// the whole of a commit entry point behind its own arguments' checks (`classes` as check_search_dims)
template <class BeamT>
static int commit_streams(void *state, int B, int max_frames, int beam, int classes, const int *which, int max_tail, int L,
                          int *tokens, int *lengths, void *scratch, void *stream) {
    if (L <= 0) return PIKA_EINVAL;
    if (int rc = check_search_dims(B, max_frames, beam, classes)) return rc;
    if (!state || !tokens || !lengths || !scratch) return PIKA_EINVAL;
    hipLaunchKernelGGL((ctc_stream_commit_kernel<BeamT>), dim3((unsigned)B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<unsigned long long *>(state),
                       (unsigned)(table_slots(max_frames, beam) - 1),
                       stream_recs<StreamRec<BeamT>>(state, B, max_frames, beam), which, beam, max_frames, max_tail, L,
                       tokens, lengths, static_cast<int *>(scratch));
    return (int)hipGetLastError();
}

// the n-best outputs of a results call: nbest entries of L tokens
static inline int check_results_dims(int B, int max_frames, int beam, int classes, int nbest, int L) {
    if (nbest <= 0 || L <= 0) return PIKA_EINVAL;
    if (int rc = check_search_dims(B, max_frames, beam, classes)) return rc;
    if (nbest > beam || (long long)nbest * L > 0x7fffffffll) return PIKA_ETOOBIG;
    return PIKA_OK;
}

}  // namespace

#endif
