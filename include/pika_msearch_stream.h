/*
 * include/pika_msearch_stream.h -- C ABI of the streaming form of the one-symbol-per-frame ("modified") transducer beam
 * searches (libpika_amd.so): what lets a state of pika_msearch.h or pika_msearch_lm.h outlive its max_frames.  Those
 * headers, their symbols and the layouts of their blobs are as they were; a stream is such a blob, advanced by its own
 * pika_msearch_advance / pika_msearch_lm_advance, plus a SIDE RECORD that the caller owns and a COMMIT that emits the
 * labels every hypothesis shares, re-roots and compacts the trie and gives the capacity back.
 * Conventions are those of pika_msearch.h: device pointers, work enqueued on `stream` and stream-ordered with no host
 * synchronisation, capturable in a hipGraph; every check comes before any launch; PIKA_EINVAL / PIKA_ETOOBIG with the
 * limits of the matching reset (K <= C <= 64 -- C = K for the plain blob --, B <= 65535, 2 C max_frames <= 2^28).
 *
 * Side record: pika_msearch_stream_side_bytes(B) bytes for B streams, three arrays, each rounded up to 16 bytes:
 *   PIKA_MSEARCH_STREAM_RETIRED_OFFSET(B)        i32 retired[B]       frames the commits have given back: a stream has
 *                                                                     consumed frames[b] + retired[b] frames
 *   PIKA_MSEARCH_STREAM_OFFSET_OFFSET(B)         f64 offset[B]        what the rebases moved out of score (plain) / am
 *   PIKA_MSEARCH_STREAM_BONUS_OFFSET_OFFSET(B)   f64 bonus_offset[B]  what they moved out of bonus (the LM blob)
 * pika_msearch_stream_reset zeros the records of the selected streams; the blob is reset by its own reset.
 * The step's time index is frames[b], which a commit lowers: a caller that counts in absolute frames passes
 * num_frames[b] - retired[b] to the advance call and reads row consumed[b] = frames[b] + retired[b] of its logits.
 *
 * Commit, per stream with which == NULL or which[b] != 0:
 *   1  The LIVE slots are the front slots with score > -inf (F for the LM blob).  The new root is the deepest common
 *      ancestor of their nodes; d is its depth.
 *   2  FORCED: with max_tail = m >= 0, if slot 0 keeps more than m labels beyond the common ancestor, the new root is
 *      slot 0's ancestor m labels up.  Slots that do not descend from it are DROPPED; the survivors close ranks in their
 *      old order; the vacated slots become empty: score (F, am) -inf, node PIKA_MSEARCH_ROOT, len 0, bonus 0,
 *      lmst = lmst2 = 0 (as the step leaves an empty slot; the automata's states of an empty slot are never read).
 *      max_tail < 0 is the exact commit: nothing is dropped.
 *   3  tokens[b, 0:d] are the labels from the old root to the new root, in order, -1 beyond d; labels at or beyond L are
 *      not written.  lengths[b] = d.  slot_map[b, j] is the old slot that new slot j came from -- a caller re-orders
 *      its prediction-network state by it exactly as by advance's parent_out --, the identity for an exact commit, for
 *      empty slots and for unselected streams.
 *   4  The table is cleared and rebuilt, parents first, with the keys between the new root and the surviving slots and
 *      nothing else: node ids change, len drops by d.  score, am, bonus, lmst and lmst2 move with their slot and are
 *      otherwise untouched.
 *   5  CAPACITY: frames[b] becomes min(frames[b], max(ceil(live keys / NSEL), longest remaining tail)), NSEL = K for the
 *      plain blob and C for the LM blob; the difference is added to retired[b].  A step adds at most NSEL keys and the
 *      table has N >= 2 NSEL max_frames slots, so keys <= NSEL frames[b] holds before and after every call and a table
 *      never fills, however long the stream runs.
 *   6  REBASE (rebase != 0, after the above, only when slot 0 is live).  Plain blob: c = score[b][0]; every live score
 *      becomes score - c (fp32, rounded once); offset[b] += (double)c.  LM blob: c = am[b][0], e = bonus[b][0]; every
 *      live am becomes am - c, every live bonus bonus - e (fp64), F = fp32((double)am + bonus) as the step forms it;
 *      offset[b] += (double)c, bonus_offset[b] += e.  Absolute scores are score + offset (plain) and am + offset,
 *      F + offset + bonus_offset (LM).  A rebase changes the rounding of every sum that follows: WITHOUT rebase a
 *      stream's scores, tokens and order equal the one-shot search's bit for bit; WITH it they agree to the precision
 *      of the format only, which is what it is for -- near frame 90 000 one ulp of a running fp32 sum is 0.008.
 *   An unselected stream gets lengths[b] = 0, tokens -1, the identity slot_map, and is not touched.
 * scratch: pika_msearch_commit_scratch_bytes(B, K, max_frames) = 4 B K max_frames bytes, the paths of the slots.
 * One workgroup per stream; every loop is bounded by K, max_frames or the table size and every index read from the blob
 * is clamped, so a blob that was never reset ends with some beam, inside its own memory and the call's outputs.  No
 * floating-point atomics: two runs give the same outputs, scores, tokens and order, bit for bit.  (Not the same blob
 * bytes: a node's id is the table slot its key came to rest in, and where two lanes' insertions contend for a slot the
 * hardware decides; nothing that is read out depends on node ids.  The step of pika_msearch.h behaves the same way.)
 */
#ifndef PIKA_MSEARCH_STREAM_H
#define PIKA_MSEARCH_STREAM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

#define PIKA_MSEARCH_STREAM_ROUND16(n) (((size_t)(n) + 15) & ~(size_t)15)
#define PIKA_MSEARCH_STREAM_RETIRED_OFFSET(B) ((size_t)0)
#define PIKA_MSEARCH_STREAM_OFFSET_OFFSET(B) PIKA_MSEARCH_STREAM_ROUND16(4 * (size_t)(B))
#define PIKA_MSEARCH_STREAM_BONUS_OFFSET_OFFSET(B) \
    (PIKA_MSEARCH_STREAM_OFFSET_OFFSET(B) + PIKA_MSEARCH_STREAM_ROUND16(8 * (size_t)(B)))

/* Bytes of the side record of B streams; 0 for a B the calls refuse. */
size_t pika_msearch_stream_side_bytes(int B);

/* Zeros the records of every stream (which == NULL) or of those with which[b] != 0 (i32 (B,)). */
int pika_msearch_stream_reset(void *side, int B, const int *which, void *stream);

/* Bytes of a commit's scratch, 4 B K max_frames; 0 for dimensions pika_msearch_commit refuses.  (It does not know C:
 * pika_msearch_lm_commit checks its own limit, 2 C max_frames <= 2^28, and may refuse dimensions this sizes.) */
size_t pika_msearch_commit_scratch_bytes(int B, int K, int max_frames);

/* The commit of a pika_msearch.h blob.  tokens i64 (B, L), lengths i64 (B,), slot_map i64 (B, K). */
int pika_msearch_commit(void *state, void *side, int B, int K, int max_frames, const int *which, int max_tail,
                        int rebase, int L, long long *tokens, long long *lengths, long long *slot_map, void *scratch,
                        void *stream);

/* The commit of a pika_msearch_lm.h blob (C = candidates sizes its tables). */
int pika_msearch_lm_commit(void *state, void *side, int B, int K, int C, int max_frames, const int *which, int max_tail,
                           int rebase, int L, long long *tokens, long long *lengths, long long *slot_map, void *scratch,
                           void *stream);

#ifdef __cplusplus
}
#endif

#endif
