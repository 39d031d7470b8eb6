/*
 * include/pika_ctc_lm.h -- C ABI of the MI355X-native CTC prefix beam search with n-gram LM shallow fusion
 * (libpika_amd.so).  Conventions, the tensor contract of x / input_lengths / blank_lp / top_val / top_idx / lse and
 * the acoustic recursion (p_b, p_nb) are those of pika_ctc_decode.h; the row pass pika_ctc_decode_rows is used as it
 * is, with K = candidates.
 *
 * The LM is an ilabel-sorted CSR back-off FST in DEVICE memory, the layout of pika_decode.h:
 *   fst_offsets   i64 (S+1)  arcs of state s: [offsets[s], offsets[s+1])
 *   fst_ilabel    i32 (A)    ascending inside a state; class c is label c + label_offset; back-off arcs carry backoff_id
 *   fst_weight    f32 (A)    costs (-log, natural)
 *   fst_nextstate i32 (A)
 *   fst_final     f32 (S)    final cost, +inf = not final
 * step(s, c): look for the arc c + label_offset out of s (lower bound over the state's arcs); found: the increment is
 * -(back-off cost so far + weight), the new state its nextstate.  Otherwise take s's back-off arc, add its weight, move
 * to its nextstate and repeat; a state with neither arc, or more than 8 back-off hops: the child does not exist (LM
 * probability zero; it is excluded whatever lm_weight is).  The first match along the chain wins; no disambiguation
 * labels, no state sets.  final(s): the same walk to the first state with a finite final cost.
 * The device code ends on ANY table: the hop count, every bisection and every probe loop have fixed trip limits, arc
 * ranges are clamped to [0, A] and a state outside [0, S) ends the walk ("does not exist").
 *
 * Fused score of a prefix l: F(l) = tot(l) + bonus(l), bonus(l) = lm_weight * LM(l) + length_bonus * |l|, LM(l) the sum
 * of the step increments along l from `start` -- a function of the label sequence alone.  Only the ranking uses F;
 * contributions to one label sequence are summed whichever parent they come from, as in pika_ctc_decode.h.
 * Candidates of a parent l at frame t: the `candidates` best non-blank classes of the row (the row pass's order), plus
 * last(l), plus every class whose child is in the beam (these two take their value from the full row).  This is a
 * pruning: it is exact only when candidates >= C - 1.  (An LM term makes a fresh child's score non-monotone in lp[c],
 * so the K = 2 beam argument of the plain search does not apply.)
 * Tie order (total): higher F (the fp32 value carried); then prefixes already in the beam, by previous rank; then
 * fresh ones by parent rank; then class ascending.
 * End: with use_final every surviving prefix adds lm_weight * final(state); those whose walk finds no final state drop
 * out; the beam is re-sorted by the resulting fp32 score, ties by the rank before.
 * Numerics: fp32 (p_b, p_nb) with the head's tot moved into an fp64 offset every 8 frames; bonus in fp64 per slot (each
 * increment rounded to fp32 once), renormalised the same way; F = fp32(tot + bonus) of the renormalised values.
 * Limits: 1 <= nbest <= beam <= 64, 1 <= candidates <= 128, B <= 65535, 2 T beam <= 2^28, S >= 1, A >= 0,
 * start in [0,S) (PIKA_EINVAL / PIKA_ETOOBIG as in pika_ctc_decode.h, before any launch).
 */
#ifndef PIKA_CTC_LM_H
#define PIKA_CTC_LM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

/* Bytes of device scratch of pika_ctc_lm_beam_search; 0 for dimensions the call refuses (B, T, beam, candidates < 1,
 * beam > 64, candidates > 128, B > 65535, 2 T beam > 2^28).  With N = the smallest power of two >= max(64, 2 T beam):
 * one open-addressing table of N 8-byte (parent node, token) keys per utterance, 8 B N bytes (the trie of
 * pika_ctc_beam_search; the LM state and bonus of a prefix are recomputed from its parent, so a node has no payload). */
size_t pika_ctc_lm_scratch_bytes(int B, int T, int beam, int candidates);

/* Fused search on the K = candidates arrays of the row pass (same x / strides / lse / B, T, C, blank, lengths).
 *   tokens    i32 (B,nbest,T)  best first; -1 beyond the length
 *   lengths   i32 (B,nbest)    -1 for a missing entry
 *   scores    f32 (B,nbest)    the fused score F the ranking used (+ the final term with use_final); -inf when missing
 *   am_scores f32 (B,nbest)    tot alone: log of the summed probability of the paths the beam kept; -inf when missing */
int pika_ctc_lm_beam_search(const float *x, long long stride_t, long long stride_b, const float *lse,
                            const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths,
                            int B, int T, int C, int blank, int beam, int nbest, const long long *fst_offsets,
                            const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                            const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                            int label_offset, int candidates, float lm_weight, float length_bonus, int use_final,
                            int *tokens, int *lengths, float *scores, float *am_scores, void *scratch, void *stream);

/* ---- Streaming: the fused search with its state carried across calls (pika_ctc_decode.h, "Streaming") ----------------
 * Any chunking of the frames gives BIT FOR BIT what pika_ctc_lm_beam_search gives on the whole tensor.  The blob of a
 * batch of B streams with room for max_frames frames each: the B tables of pika_ctc_lm_scratch_bytes(B, max_frames,
 * beam, candidates), then B records of PIKA_CTC_LM_STREAM_RECORD_BYTES:
 *   i32 n | i32 frames | i32 overflow | i32 pad | f64 off (moved out of tot) | f64 boff (moved out of bonus) |
 *   the beam, arrays of 64 (slots [0,n) hold values): i32 node, last, parent node, len; f32 p_b, p_nb, tot; f64 bonus;
 *   i32 LM state
 * `frames` and `overflow` of stream b lie at PIKA_CTC_STREAM_FRAMES_OFFSET / _OVERFLOW_OFFSET of its record, as in
 * pika_ctc_decode.h.  The FST arrays, lm_weight, length_bonus, beam and candidates must be the same in every call on a
 * blob between two resets; nothing checks that. */
#define PIKA_CTC_LM_STREAM_RECORD_BYTES 2592
#ifndef PIKA_CTC_STREAM_FRAMES_OFFSET
#define PIKA_CTC_STREAM_FRAMES_OFFSET 4
#define PIKA_CTC_STREAM_OVERFLOW_OFFSET 8
#endif

/* pika_ctc_lm_scratch_bytes(B, max_frames, beam, candidates) + B * PIKA_CTC_LM_STREAM_RECORD_BYTES; 0 for dimensions the
 * calls refuse. */
size_t pika_ctc_lm_stream_state_bytes(int B, int max_frames, int beam, int candidates);

/* As pika_ctc_stream_reset; the empty prefix starts in LM state `start` in [0, num_states) with bonus 0. */
int pika_ctc_lm_stream_reset(void *state, int B, int max_frames, int beam, int candidates, int num_states, int start,
                             const int *which, void *stream);

/* As pika_ctc_stream_advance, on the K = candidates arrays of the row pass on the chunk. */
int pika_ctc_lm_stream_advance(const float *x, long long stride_t, long long stride_b, const float *lse,
                               const float *blank_lp, const float *top_val, const int *top_idx,
                               const int *chunk_lengths, int B, int Tc, int C, int blank, int beam,
                               const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                               const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                               int backoff_id, int label_offset, int candidates, float lm_weight, float length_bonus,
                               void *state, int max_frames, void *stream);

/* The n-best of the current beams with the outputs of pika_ctc_lm_beam_search and the token width L of
 * pika_ctc_stream_results.  use_final: the final term and the re-sort happen on the side; the state is only read, so
 * decoding can go on after it and a later call with the other setting gives that setting's answer. */
int pika_ctc_lm_stream_results(const void *state, int B, int max_frames, int beam, int candidates,
                               const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                               const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                               int backoff_id, int label_offset, float lm_weight, int use_final, int nbest, int L,
                               int *tokens, int *lengths, float *scores, float *am_scores, void *stream);

/* pika_ctc_stream_commit (pika_ctc_decode.h) on the LM record: the LM state and the bonus of a slot travel with it, and
 * the length bonus lives in `bonus`, not in the length, so no score moves.  Scratch as the plain commit's. */
size_t pika_ctc_lm_stream_commit_scratch_bytes(int B, int max_frames, int beam, int candidates);

int pika_ctc_lm_stream_commit(void *state, int B, int max_frames, int beam, int candidates, const int *which,
                              int max_tail, int L, int *tokens, int *lengths, void *scratch, void *stream);

/* ---- A second automaton beside the LM: contextual biasing (hotwords), or a second, domain LM ---------------------------
 * The pika_ctc_lm2_* calls are their pika_ctc_lm_* counterparts with a second FST of the same layout (fst2_*, its own
 * backoff_id2 / label_offset2) and its weight:
 *   F(l) = tot(l) + lm_weight * LM(l) + bias_weight * BIAS(l) + length_bonus * |l|
 * LM(l) and BIAS(l) each the sum of step increments of its own automaton from its own start state (start / start2), by
 * the step() above.  A child that EITHER automaton cannot reach does not exist.  With use_final a prefix adds
 * lm_weight * final(state) + bias_weight * final2(state2) and drops out when either walk finds no final state.
 * Candidates, the acoustic recursion, the tie order, am_scores, the limits and the renormalisation are unchanged.
 * Numerics: each automaton's increment is rounded to fp32 once; the products with the weights and the sums into the
 * slot's bonus are fp64; a slot carries ONE bonus for both terms and the length bonus; F = fp32(tot + bonus).
 * The second FST's arguments follow the first's (after label_offset), bias_weight follows lm_weight; a call without
 * `start` has no `start2`.  PIKA_EINVAL for num_states2 <= 0, num_arcs2 < 0, start2 outside [0, num_states2) or a
 * missing array of the second FST (the arc arrays may be NULL when num_arcs2 == 0), before any launch.  The device code
 * ends on any pair of tables, as it does for one.
 * A stream's record is the LM record followed by the second states, i32 x 64: PIKA_CTC_LM2_STREAM_RECORD_BYTES;
 * `frames` and `overflow` lie at the same offsets.  Both FSTs and both weights must be the same in every call on a
 * blob between two resets. */
#define PIKA_CTC_LM2_STREAM_RECORD_BYTES (PIKA_CTC_LM_STREAM_RECORD_BYTES + 256)

/* == pika_ctc_lm_scratch_bytes: the second automaton needs no scratch. */
size_t pika_ctc_lm2_scratch_bytes(int B, int T, int beam, int candidates);

int pika_ctc_lm2_beam_search(const float *x, long long stride_t, long long stride_b, const float *lse,
                             const float *blank_lp, const float *top_val, const int *top_idx, const int *input_lengths,
                             int B, int T, int C, int blank, int beam, int nbest, const long long *fst_offsets,
                             const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                             const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                             int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                             const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                             int num_states2, int num_arcs2, int start2, int backoff_id2, int label_offset2,
                             int candidates, float lm_weight, float bias_weight, float length_bonus, int use_final,
                             int *tokens, int *lengths, float *scores, float *am_scores, void *scratch, void *stream);

/* pika_ctc_lm2_scratch_bytes(B, max_frames, beam, candidates) + B * PIKA_CTC_LM2_STREAM_RECORD_BYTES; 0 for dimensions
 * the calls refuse. */
size_t pika_ctc_lm2_stream_state_bytes(int B, int max_frames, int beam, int candidates);

/* The empty prefix starts in state `start` of the first and `start2` of the second automaton with bonus 0. */
int pika_ctc_lm2_stream_reset(void *state, int B, int max_frames, int beam, int candidates, int num_states, int start,
                              int num_states2, int start2, const int *which, void *stream);

int pika_ctc_lm2_stream_advance(const float *x, long long stride_t, long long stride_b, const float *lse,
                                const float *blank_lp, const float *top_val, const int *top_idx,
                                const int *chunk_lengths, int B, int Tc, int C, int blank, int beam,
                                const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                                const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                                int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                                const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                                int num_states2, int num_arcs2, int backoff_id2, int label_offset2, int candidates,
                                float lm_weight, float bias_weight, float length_bonus, void *state, int max_frames,
                                void *stream);

int pika_ctc_lm2_stream_results(const void *state, int B, int max_frames, int beam, int candidates,
                                const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                                const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                                int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                                const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                                int num_states2, int num_arcs2, int backoff_id2, int label_offset2, float lm_weight,
                                float bias_weight, int use_final, int nbest, int L, int *tokens, int *lengths,
                                float *scores, float *am_scores, void *stream);

size_t pika_ctc_lm2_stream_commit_scratch_bytes(int B, int max_frames, int beam, int candidates);

int pika_ctc_lm2_stream_commit(void *state, int B, int max_frames, int beam, int candidates, const int *which,
                               int max_tail, int L, int *tokens, int *lengths, void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKA_CTC_LM_H */
