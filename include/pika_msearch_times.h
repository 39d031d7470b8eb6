/*
 * include/pika_msearch_times.h -- C ABI of the token time stamps of the one-symbol-per-frame ("modified") transducer
 * beam searches (libpika_amd.so): a TIME RECORD that the caller owns and keeps next to a search of pika_msearch.h or
 * pika_msearch_lm.h -- a stream of pika_msearch_stream.h included --, stepped after every advance from the (parent,
 * token) pairs the advance returned.  Those headers, their symbols and the layouts of their blobs are as they were.
 * Conventions are those of pika_msearch_stream.h: device pointers, work enqueued on `stream` and stream-ordered with no
 * host synchronisation, capturable in a hipGraph; every check comes before any launch; PIKA_EINVAL / PIKA_ETOOBIG with the
 * limits of the matching reset (1 <= K <= 64, B <= 65535, 2 max(K, C) max_frames <= 2^28).
 * C names the blob: C = 0 is the blob of pika_msearch.h, K <= C <= 64 the blob of pika_msearch_lm.h with C candidates
 * (as pika_msearch_lm_commit takes K, C); C < 0 and 0 < C < K are PIKA_EINVAL.
 *
 * Definition.  For every slot the record holds one i32 per label of the slot's current token sequence: the ABSOLUTE
 * index of the frame at which the slot's lineage emitted that label, len[b][k] entries, relative to the last commit's
 * root as the sequence is.  A slot's lineage is that of its REPRESENTATIVE: the step of pika_msearch.h reports, for every
 * merged group, the old slot and the token of its best-ranked member in parent_out / token_out, and the record follows
 * exactly those.  It is an integer function of the (parent, token) pairs: no floating point, no atomics, two runs give
 * the same bytes of the current planes.
 *
 * Record: pika_msearch_times_bytes(B, K, max_frames) = ROUND16(12 B) + 8 B K max_frames bytes:
 *   PIKA_MSEARCH_TIMES_SEEN_OFFSET(B)     i32 seen[B]   consumed[b] as the last step (or the reset: 0) left it
 *   PIKA_MSEARCH_TIMES_LOST_OFFSET(B)     i32 lost[B]   != 0: the record of b missed a step; read-outs give -1
 *   PIKA_MSEARCH_TIMES_CUR_OFFSET(B)      i32 cur[B]    which plane is current (its lowest bit)
 *   PIKA_MSEARCH_TIMES_PLANES_OFFSET(B)   two planes of i32 [B][K][max_frames], plane p at + 4 p B K max_frames
 * Step and commit read the current plane of an utterance, write its other plane and flip cur[b]; an utterance that was
 * not stepped does not flip.  consumed[b] = frames[b] of the blob, + retired[b] of the side record for a stream.
 *
 * Reset, for every utterance (which == NULL) or those with which[b] != 0: seen = lost = cur = 0, both planes -1.  It
 * belongs with the reset of the search (and of the side record), which leaves consumed[b] = 0.
 *
 * Step, after every advance, with that call's parent_out / token_out and the state as the advance left it:
 *   lost[b] != 0                 nothing happens.
 *   consumed[b] == seen[b]       the utterance was inactive (or overflowed): nothing happens.
 *   consumed[b] == seen[b] + 1   new slot j takes the first n entries of old slot parent[b,j], n = len[b][j] - 1 when
 *                                token[b,j] != blank and len[b][j] otherwise; a label's entry len[b][j] - 1 is the
 *                                step's frame index consumed[b] - 1.  seen[b] = consumed[b].  Empty slots (parent 0,
 *                                token blank, len 0) need no special case.
 *   anything else                a step was skipped, or the state was reset without the record: lost[b] = 1.
 *
 * Read-out per slot (hyps): out i64 (B, K, L), the entries of slot k in [0, len), -1 beyond, -1 everywhere for an empty
 * slot (score -inf) and for a lost record.
 * Read-out per n-best entry (results): tokens i64 (B, N, L) and lengths i64 (B, N) as any results call of the search
 * returned them; out i64 (B, N, L).  The entry's slot is the live slot whose trie path spells the entry's tokens (live
 * slots hold distinct sequences), found on the device by walking the trie; a missing entry (length < 0), an entry with
 * length > L and an entry with no such slot get -1 everywhere.
 *
 * Commit, right after pika_msearch_commit / pika_msearch_lm_commit with that call's lengths and slot_map and the state
 * as the commit left it; for a selected stream (which as in the commit) with d = lengths[b]:
 *   out[b, i], i < d, is the EARLIEST value, over the slots j that are live after the commit, of
 *   record_old[slot_map[b,j]][i]; -1 beyond d; positions at or beyond L are not written.
 *   record_new[j] = record_old[slot_map[b,j]][d : d + len[b][j]].
 * The live slots share the committed labels, not necessarily their lineages; the minimum is the rule under which a
 * stream's committed times followed by ANY live tail's times are strictly increasing, whatever the schedule (every
 * survivor s has min_i <= t_s[i] < t_s[i+1], so min_i < min_{i+1} and min_{d-1} < every tail's first entry), and it is
 * the tie rule of the project: the earliest emission.  With one live slot it is that slot's lineage.
 * An unselected stream and a lost record get -1 everywhere and are not touched.
 *
 * One workgroup per utterance in step, hyps and commit, one wave per (b, entry) in results; rows move with coalesced
 * loads and stores, 16 bytes per lane where max_frames % 4 == 0 and the record is 16-byte aligned (the result does not
 * depend on it), and only len entries per slot move.  Every len, parent, slot_map, lengths and node id read from memory
 * is clamped before it indexes, every loop is bounded by K, max_frames, L or the table size: a record or a blob that
 * was never reset ends inside its own memory and the call's outputs.
 */
#ifndef PIKA_MSEARCH_TIMES_H
#define PIKA_MSEARCH_TIMES_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

#define PIKA_MSEARCH_TIMES_ROUND16(n) (((size_t)(n) + 15) & ~(size_t)15)
#define PIKA_MSEARCH_TIMES_SEEN_OFFSET(B) ((size_t)0)
#define PIKA_MSEARCH_TIMES_LOST_OFFSET(B) (4 * (size_t)(B))
#define PIKA_MSEARCH_TIMES_CUR_OFFSET(B) (8 * (size_t)(B))
#define PIKA_MSEARCH_TIMES_PLANES_OFFSET(B) PIKA_MSEARCH_TIMES_ROUND16(12 * (size_t)(B))

/* Bytes of the record; 0 for dimensions the calls refuse. */
size_t pika_msearch_times_bytes(int B, int K, int max_frames);

/* The records of every utterance (which == NULL) or of those with which[b] != 0 (i32 (B,)) back to the start. */
int pika_msearch_times_reset(void *times, int B, int K, int max_frames, const int *which, void *stream);

/* The step.  side: the side record of a stream, NULL for a bare state; parent, token i64 (B, K) as the advance wrote
 * them; blank >= 0. */
int pika_msearch_times_step(void *times, const void *state, const void *side, int B, int K, int C, int max_frames,
                            const long long *parent, const long long *token, int blank, void *stream);

/* The times of the K current slots: out i64 (B, K, L). */
int pika_msearch_times_hyps(const void *times, const void *state, int B, int K, int C, int max_frames, int L,
                            long long *out, void *stream);

/* The times of N <= K entries that a results call returned: tokens i64 (B, N, L), lengths i64 (B, N), out i64 (B, N, L). */
int pika_msearch_times_results(const void *times, const void *state, int B, int K, int C, int max_frames, int N, int L,
                               const long long *tokens, const long long *lengths, long long *out, void *stream);

/* The commit.  lengths i64 (B,), slot_map i64 (B, K) as the search's commit wrote them; out i64 (B, L). */
int pika_msearch_times_commit(void *times, const void *state, int B, int K, int C, int max_frames, const int *which,
                              const long long *lengths, const long long *slot_map, int L, long long *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
