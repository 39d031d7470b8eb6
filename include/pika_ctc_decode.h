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

#ifdef __cplusplus
}
#endif
#endif /* PIKA_CTC_DECODE_H */
