/*
 * include/pika_msearch.h -- C ABI of the one-symbol-per-frame ("modified") transducer beam search (libpika_amd.so): the
 * search that belongs to the modified topology of pika_rnnt.h, in which every frame emits exactly one symbol, blank or a
 * label.  Every hypothesis consumes one frame per step, so an utterance of T_n frames takes exactly T_n calls of
 * pika_msearch_advance and a batch max(T_n) calls, known on the host before the first launch: nothing is read back.
 *
 * Conventions are those of pika_rnnt.h: plain pointers + sizes, every pointer DEVICE memory owned by the caller, no
 * allocation, work enqueued on `stream` (a hipStream_t as void*, NULL = default stream) and stream-ordered with no host
 * synchronisation; return 0 on success, PIKA_EINVAL / PIKA_ETOOBIG for bad arguments (before any launch), a positive
 * hipError_t if a launch failed.  Every call can be captured in a hipGraph.
 *
 * State: one blob of pika_msearch_state_bytes(B, K, max_frames) bytes per search, B utterances of K slots:
 *   offset 0            f32 score[B][K]     -inf marks an empty slot
 *   4 B K               i32 node[B][K]      the trie node that stands for the slot's token sequence
 *   8 B K               i32 len[B][K]       its number of labels
 *   12 B K              i32 frames[B]       frames consumed so far
 *   12 B K + 4 B        i32 overflowed[B]   frames were offered beyond max_frames
 *   the above rounded up to 16 bytes: B open-addressing tables of N 8-byte (parent node, token) keys, N the smallest
 *   power of two >= max(64, 2 K max_frames).  A node's identity is the slot its key occupies; the empty sequence is the
 *   node PIKA_MSEARCH_ROOT.  A step makes at most K nodes, so a table never fills within max_frames.
 * Live slots sit at the front, best first.  After a reset slot 0 has score 0, node ROOT, len 0; the others are empty.
 *
 * The step, for an utterance with frames[b] < min(num_frames[b], max_frames) (an ACTIVE one), on the K rows
 * logits[b K + k] -- the joint network's output for slot k at frame frames[b]:
 *   x[k,v]    = sm_scale * logits[k,v] - (v == blank ? blank_penalty : 0)       (product and difference rounded apart)
 *   lp[k,v]   = x[k,v] - logsumexp_v x[k,.]     evaluated as (x - max) - log(sum exp(x - max))
 *   cand[k,v] = score[k] + lp[k,v]              for live k
 *   the K best candidates > -inf are taken (fewer may exist) in the total order: larger value, then lower k, then lower
 *   v; the position in that order is the candidate's RANK.  A candidate's key is node[k] for blank and
 *   child(node[k], v) otherwise (created when absent, len + 1).  Candidates with equal keys merge into
 *   m + log(sum_i exp(c_i - m)), m the group's largest value, the sum in rank order, fp32 with accurate expf / logf
 *   (a group of one keeps its value bit for bit); the group's REPRESENTATIVE is its best-ranked member.  The new beam is
 *   the groups by merged score descending, ties by the representative's rank; parent_out[b,j] is the representative's
 *   old slot and token_out[b,j] its v.  Empty slots get score -inf, parent 0, token blank.  frames[b] += 1.
 * An inactive utterance keeps its state and gets parent_out[b,j] = j, token_out[b,j] = blank.  overflowed[b] is set by
 * any call that leaves frames[b] == max_frames while num_frames[b] > max_frames; the further frames are ignored.
 * A -inf logit is never selected; a row of -inf only kills its slot; a constant added to a row changes nothing beyond
 * the rounding of x.  NaN and +inf are outside the contract (every loop is bounded by K, V or the table size whatever
 * the input).  No floating-point atomics: two runs give the same bits.  K = 1 is the modified greedy search.
 *
 * Limits: 1 <= K <= 64 (the selection's LDS), B <= 65535, 2 K max_frames <= 2^28 (PIKA_ETOOBIG beyond); V >= 2,
 * 0 <= blank < V, ld >= V, max_frames >= 1, finite sm_scale and blank_penalty.
 */
#ifndef PIKA_MSEARCH_H
#define PIKA_MSEARCH_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

#define PIKA_MSEARCH_ROOT 0x7ffffffe
#define PIKA_MSEARCH_MAX_BEAM 64

/* Bytes of the state blob; 0 for dimensions the calls refuse. */
size_t pika_msearch_state_bytes(int B, int K, int max_frames);

/* Every utterance (which == NULL) or those with which[b] != 0 (i32 (B,)) back to the empty sequence; the others' state,
 * tables included, is not touched. */
int pika_msearch_reset(void *state, int B, int K, int max_frames, const int *which, void *stream);

/* One frame step.  logits f32 (B K, V) with row stride ld >= V elements (16-byte loads where ld % 4 == 0 and the
 * base is 16-byte aligned, scalar loads otherwise; the result does not depend on it); num_frames i64 (B,), clamped on
 * the device to [0, max_frames]; parent_out, token_out i64 (B, K). */
int pika_msearch_advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K,
                         int max_frames, int V, int blank, float sm_scale, float blank_penalty, long long *parent_out,
                         long long *token_out, void *stream);

/* The nbest <= K best entries of the beams as they stand, in the beam's order.  tokens i64 (B, nbest, L), -1 beyond
 * the length; lengths i64 (B, nbest), -1 for a missing entry; scores f32 (B, nbest), -inf for a missing entry.  An
 * entry longer than L reports its true length and its first L tokens.  The state is only read. */
int pika_msearch_results(const void *state, int B, int K, int max_frames, int nbest, int L, long long *tokens,
                         long long *lengths, float *scores, void *stream);

/* The same walk for the K current slots: tokens i64 (B, K, L), lengths i64 (B, K) (-1: empty slot).  For prediction
 * networks that are re-run on the prefix. */
int pika_msearch_hyps(const void *state, int B, int K, int max_frames, int L, long long *tokens, long long *lengths,
                      void *stream);

#ifdef __cplusplus
}
#endif

#endif
