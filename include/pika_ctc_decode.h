/*
 * include/pika_ctc_decode.h -- C ABI of the MI355X-native CTC decoders (libpika_amd.so): best path (greedy) and exact
 * prefix beam search over the full vocabulary.
 *
 * Conventions are those of pika_ctc.h: plain pointers + sizes, every pointer DEVICE memory owned by the caller, work
 * enqueued on `stream` (a hipStream_t as void*, NULL = default stream) and stream-ordered with no host synchronisation;
 * return 0 on success, a negative PIKA_E* code for bad arguments (before any launch), a positive hipError_t if a launch
 * failed.
 *
 * Three steps.  pika_ctc_decode_rows is the only one that reads the (T,B,C) input, once: per row t < T_n it leaves the
 * blank's log-prob and the K best NON-BLANK classes.  pika_ctc_greedy (K = 1) and pika_ctc_beam_search (K = 2 beam) work
 * on those compact arrays; the search also gathers at most `beam` single values per frame from the input.
 *
 * Tensor contract:
 *   x              f32, row (t,b) at x + t * stride_t + b * stride_b (strides in ELEMENTS), C contiguous classes; log-probs,
 *                  or raw logits with logits != 0 (the row's log-sum-exp is then taken in the same pass and subtracted:
 *                  every value below is logit - lse rounded once).  Rows t >= T_n are never read.  16-byte loads where
 *                  C % 4 == 0 and the row is 16-byte aligned, scalar loads otherwise; the result does not depend on it.
 *   input_lengths  i32 (B,) T_n, clamped on the device to [1,T]
 *   blank_lp       f32 (T,B)    the blank's value           } rows t >= T_n are not written
 *   top_val        f32 (T,B,K)  the K best non-blank values, descending; equal values: lower class first; -1e30 padding
 *   top_idx        i32 (T,B,K)  their classes; -1 where fewer than K non-blank classes exist
 *   lse            f32 (T,B)    the row's log-sum-exp (logits != 0 only; NULL otherwise)
 * Values below -1e30 (-inf, and NaN) are read as -1e30, "log zero".
 * Limits: 1 <= K <= 128, 1 <= nbest <= beam <= 64, B <= 65535 (PIKA_ETOOBIG beyond); any C >= 1, blank in [0,C).
 *
 * Beam search: every prefix l of the beam carries (p_b, p_nb), tot = p_b (+) p_nb.  At each frame blank adds
 * lp[blank] + tot to p_b(l); a class c == last(l) adds lp[c] + p_nb to p_nb(l) and lp[c] + p_b to p_nb(l+c); any other
 * class adds lp[c] + tot to p_nb(l+c); contributions to one label sequence are summed whichever parent they come from;
 * the `beam` best by tot survive.  Nothing is pruned by class: K = 2 beam is exact.
 * Tie order (total, so the output is a function of the input alone): higher tot first (the fp32 value the search
 * carries); then prefixes already in the beam, by their previous rank; then fresh ones by their parent's rank; fresh
 * children of one parent in the order of the row pass (higher value, then lower class), the child that repeats the
 * parent's last label after a differently labelled child of equal tot only if its class is higher.
 * Numerics: fp32 (p_b, p_nb) with the running maximum moved into an fp64 offset every 8 frames; a score is
 * offset + tot, rounded to fp32 once.
 */
#ifndef PIKA_CTC_DECODE_H
#define PIKA_CTC_DECODE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

/* Row pass: one workgroup per (t,b) row. */
int pika_ctc_decode_rows(const float *x, long long stride_t, long long stride_b, const int *input_lengths, int B, int T,
                         int C, int blank, int K, int logits, float *blank_lp, float *top_val, int *top_idx, float *lse,
                         void *stream);

/* Best path from the K = 1 arrays of the row pass: the per-frame arg-max over ALL classes (the blank wins against
 * top_idx where its value is higher, or equal with blank < top_idx), repeats merged, blanks dropped.
 *   tokens  i32 (B,T)  the transcript, -1 beyond lengths[n]
 *   lengths i32 (B,)
 *   scores  f32 (B,)   sum of the chosen values over t < T_n (accumulated in fp64, rounded once)
 *   frames  i32 (B,T)  frames[n,k] = first frame of the run that emits tokens[n,k]; -1 beyond lengths[n] */
int pika_ctc_greedy(const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths, int B,
                    int T, int C, int blank, int *tokens, int *lengths, float *scores, int *frames, void *stream);

/* Bytes of device scratch of pika_ctc_beam_search; 0 for dimensions the call refuses (B, T, beam < 1, beam > 64,
 * B > 65535, 2 T beam > 2^28).  With N = the smallest power of two >= max(64, 2 T beam):
 *   one open-addressing table of N 8-byte (parent node, token) keys per utterance          8 B N
 * A prefix is a node of a trie; the node's identity is the slot its (parent, token) key occupies, so it is unique for
 * the whole utterance however often the prefix leaves and re-enters the beam.  At most T beam nodes are ever made. */
size_t pika_ctc_beam_scratch_bytes(int B, int T, int beam);

/* Prefix beam search on the K = 2 * beam arrays of the row pass (same B, T, C, blank, lengths, and the same x / strides
 * / lse: the search gathers the values of the beam's own last labels from x).  lse NULL: x holds log-probs.
 *   tokens  i32 (B,nbest,T)  the nbest best prefixes of the final beam, best first; -1 beyond the length
 *   lengths i32 (B,nbest)    -1 for a missing entry (fewer distinct prefixes exist than nbest)
 *   scores  f32 (B,nbest)    log of the summed probability of the paths the beam kept; -inf for a missing entry */
int pika_ctc_beam_search(const float *x, long long stride_t, long long stride_b, const float *lse,
                         const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths,
                         int B, int T, int C, int blank, int beam, int nbest, int *tokens, int *lengths, float *scores,
                         void *scratch, void *stream);

/* ---- Streaming: the beam search with its state carried across calls -------------------------------------------------
 * The search is a function of (state, frame), so the state can rest in device memory between launches: feed the frames
 * of an utterance in chunks of any sizes and the n-best is BIT FOR BIT what pika_ctc_beam_search gives on the whole
 * tensor.  One opaque blob serves a batch of B independent streams with room for max_frames frames each; the limits are
 * the one-shot's with T := max_frames.  Layout, with N = the smallest power of two >= max(64, 2 max_frames beam):
 *   [0, 8 B N)                 the B tables of pika_ctc_beam_scratch_bytes(B, max_frames, beam)
 *   then B records of PIKA_CTC_STREAM_RECORD_BYTES, record b of stream b:
 *     i32 n (slots in the beam) | i32 frames (held: consumed, less what a commit gave back) | i32 overflow |
 *     i32 retired (frames given back by commits; 0 without one) | f64 off | f64 (unused here) |
 *     the beam, seven arrays of 64 (slots [0,n) hold values): i32 node, last, parent node, len; f32 p_b, p_nb, tot
 * `frames`, `overflow` and `retired` of stream b may be read at PIKA_CTC_STREAM_FRAMES_OFFSET / _OVERFLOW_OFFSET /
 * _RETIRED_OFFSET of its record; everything else is the library's.  frames + retired is the number of frames the stream
 * has consumed, max_frames - frames the number it can still take.  A blob must be reset before its first advance. */
#define PIKA_CTC_STREAM_RECORD_BYTES 1824
#define PIKA_CTC_STREAM_FRAMES_OFFSET 4
#define PIKA_CTC_STREAM_OVERFLOW_OFFSET 8
#define PIKA_CTC_STREAM_RETIRED_OFFSET 12

/* Bytes of the blob: pika_ctc_beam_scratch_bytes(B, max_frames, beam) + B * PIKA_CTC_STREAM_RECORD_BYTES; 0 for
 * dimensions the calls refuse. */
size_t pika_ctc_stream_state_bytes(int B, int max_frames, int beam);

/* The empty-prefix beam, frames = 0, offsets 0, overflow 0 and an empty table -- for every stream (which NULL), or for
 * the streams b with which[b] != 0 (i32 (B,), device): the others' records and tables are not touched. */
int pika_ctc_stream_reset(void *state, int B, int max_frames, int beam, const int *which, void *stream);

/* The frames t < L_b of a chunk (Tc,B,C) through the search.  x / strides / lse / blank_lp / top_val / top_idx as in
 * pika_ctc_beam_search, from pika_ctc_decode_rows on the chunk with K = 2 * beam and the same chunk_lengths.
 *   chunk_lengths  i32 (B,)  L_b, clamped on the device to [0,Tc]; 0: the stream is left exactly as it was.  (The row
 *                  pass clamps to [1,Tc] and may look at row 0 of such a stream; the advance does not use it.)
 * A stream never takes more than max_frames frames: L_b is cut there, the extra frames are ignored and `overflow` is
 * set (until the next reset), so a table is never more than half full. */
int pika_ctc_stream_advance(const float *x, long long stride_t, long long stride_b, const float *lse,
                            const float *blank_lp, const float *top_val, const int *top_idx, const int *chunk_lengths,
                            int B, int Tc, int C, int blank, int beam, void *state, int max_frames, void *stream);

/* The n-best of the current beams, as pika_ctc_beam_search writes them; the state is only read, so partial hypotheses
 * can be taken after any chunk.  tokens i32 (B,nbest,L): L >= 1 is the width the caller allocated -- an entry longer
 * than L (possible only for L < frames) keeps its length and its first L labels.  lengths, scores (B,nbest). */
int pika_ctc_stream_results(const void *state, int B, int max_frames, int beam, int nbest, int L, int *tokens,
                            int *lengths, float *scores, void *stream);

/* ---- Commit: emit the stable prefix, give capacity back --------------------------------------------------------------
 * The labels on the path from the root to the common ancestor of the beam's slots are shared by every hypothesis the
 * stream can still produce: they are final.  A commit writes them out, makes that ancestor the root (every slot's length
 * drops by their number d) and rebuilds the table with the nodes between the new root and the slots only.  `frames` is
 * then lowered to the smallest value >= max(ceil(live keys / beam), longest remaining prefix) that is congruent to the
 * old one modulo 8 (the renormalisation keeps its phase), and the difference is added to `retired`.  The beam's order,
 * scores, offsets and automaton states are untouched: the frames that follow give bit for bit what they would have
 * given without the commit, pika_ctc_stream_results returns the uncommitted tails (lengths relative to the commit,
 * scores absolute), and the stream may consume more than max_frames frames as long as commits keep `frames` below it.
 *   which     i32 (B,) or NULL, as in the reset: a stream with which[b] == 0 is not touched and gets lengths[b] = 0
 *   max_tail  < 0: the exact commit above.  m >= 0: FORCED -- if the best slot (slot 0 of the stored beam) would keep
 *             more than m uncommitted labels, the new root is its ancestor m labels up, and the slots that do not descend
 *             from it are dropped; the others keep their order.  This changes the search (finalisation by best path).
 *   tokens    i32 (B,L)  the labels that became final in this call, -1 beyond lengths[b]; L >= 1 is the width the caller
 *             allocated: labels at or beyond L are not written (d <= frames <= max_frames)
 *   lengths   i32 (B,)   d
 *   scratch   pika_ctc_stream_commit_scratch_bytes(B, max_frames, beam) bytes (4 B max_frames beam: per slot the labels
 *             of its path, from which the table is rebuilt parents first); 0 for dimensions the calls refuse
 * PIKA_EINVAL for a NULL state / tokens / lengths / scratch and for L <= 0; the dimension limits of the reset. */
size_t pika_ctc_stream_commit_scratch_bytes(int B, int max_frames, int beam);

int pika_ctc_stream_commit(void *state, int B, int max_frames, int beam, const int *which, int max_tail, int L,
                           int *tokens, int *lengths, void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKA_CTC_DECODE_H */
