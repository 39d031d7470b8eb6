/*
 * include/pika_msearch_lm.h -- C ABI of the one-symbol-per-frame ("modified") transducer beam search with n-gram LM and
 * hotword shallow fusion (libpika_amd.so): the search of pika_msearch.h with up to two back-off FSTs fused into the
 * ranking (icefall's modified_beam_search_lm_shallow_fusion / _LODR and the context graph of modified_beam_search).
 * Conventions, the logits contract, ACTIVE utterances, frames and overflowed are those of pika_msearch.h; an automaton is
 * passed as in pika_ctc_lm.h -- offsets, ilabel, weight, nextstate, final, num_states, num_arcs, [start,] backoff_id,
 * label_offset, DEVICE memory -- and walked by that header's step(s, c) / final(s), 8 back-off hops at most.  The second
 * automaton is optional: num_states2 == 0 with NULL arrays (and num_arcs2 == 0) means "none"; with num_states2 > 0 it is
 * checked exactly as the first.
 *
 * State: one blob of pika_msearch_lm_state_bytes(B, K, C, max_frames) bytes per search, B utterances of K = beam slots,
 * C = candidates, K <= C <= 64:
 *   offset 0            f64 bonus[B][K]     lm_weight * LM + bias_weight * BIAS + length_bonus * len of the slot's tokens
 *   8 B K               f32 F[B][K]         the fused score fp32((double)am + bonus); -inf marks an empty slot
 *   12 B K              f32 am[B][K]        the log-sum of the paths kept; -inf in an empty slot
 *   16 B K              i32 node[B][K]      the trie node that stands for the slot's token sequence
 *   20 B K              i32 len[B][K]       its number of labels
 *   24 B K              i32 lmst[B][K]      its state in the first automaton
 *   28 B K              i32 lmst2[B][K]     its state in the second (0 when there is none)
 *   32 B K              i32 frames[B]       frames consumed so far
 *   32 B K + 4 B        i32 overflowed[B]   frames were offered beyond max_frames
 *   the above rounded up to 16 bytes: B open-addressing tables of N 8-byte (parent node, token) keys, N the smallest
 *   power of two >= max(64, 2 C max_frames).  A step makes at most C nodes, so a table never fills within max_frames.
 * Live slots sit at the front, best F first.  After a reset slot 0 has am = 0, bonus = 0, F = 0, node
 * PIKA_MSEARCH_ROOT, len 0, lmst = start, lmst2 = start2; the others are empty, F = am = -inf.
 *
 * The step, for an ACTIVE utterance, on the K rows logits[b K + k]:
 *   1  x[k,v], lp[k,v] and the row statistics are exactly those of pika_msearch.h; cand[k,v] = F[k] + lp[k,v], live k.
 *   2  PRE-SELECTION.  The C best candidates > -inf are taken (fewer may exist) in the total order of pika_msearch.h:
 *      larger value, then lower k, then lower v; the position in that order is the candidate's RANK.  This is a PRUNING:
 *      the LM sees only what the cut by F[k] + lp leaves, so the step is the exact K best by fused score only when
 *      C >= the number of finite candidates.  C = K is icefall's rule (cut, then add the LM); C > K lets the LM rescue
 *      a candidate the acoustic cut would have dropped.
 *   3  EXTENSION of a pre-selected (k, v), a' = am[k] + lp[k,v]:
 *      blank: key node[k], bonus' = bonus[k], states unchanged.
 *      label: step(lmst[k], v) and, with a second automaton, step2(lmst2[k], v).  If either walk finds no child or
 *      returns a non-finite increment the candidate DOES NOT EXIST: it is dropped whatever the weights are and creates
 *      no trie node.  Otherwise bonus' = bonus[k] + (double)lm_weight * inc + (double)bias_weight * inc2 +
 *      (double)length_bonus -- each inc rounded to fp32 once by the walk, the products and sums fp64, rounded one by one
 *      in that order -- the states are the walks' next states and the key is child(node[k], v), created when absent.
 *      bonus' and the states are functions of the token sequence alone, evaluated by one formula: the members of a
 *      group agree on them bit for bit and the group takes its representative's.
 *   4  MERGE.  Candidates with equal keys merge their a' into a_rep + log(sum_i exp(a_i - a_rep)), the REPRESENTATIVE
 *      the group's best-ranked member, the sum in rank order, fp32 with accurate expf / logf; a group of one keeps its
 *      bits.
 *   5  NEW BEAM.  The groups by G = fp32((double)a_merged + bonus') descending, ties by the representative's rank; the
 *      K best stay: F = G, am = a_merged, bonus = bonus'.  parent_out[b,j] is the representative's old slot and
 *      token_out[b,j] its v.  Empty slots get F = am = -inf, parent 0, token blank.  frames[b] += 1.
 * Inactive utterances, frames and overflowed behave as in pika_msearch.h.  With lm_weight = bias_weight =
 * length_bonus = 0, C = K and automata that reach every class, the step is pika_msearch_advance bit for bit.
 * The device code ends on ANY table (pika_ctc_lm.h); every state read from the blob is clamped into its table before it
 * indexes anything.  No floating-point atomics: two runs give the same bits.  am is not renormalised.
 *
 * Results: with use_final a live slot's score is fp32(((double)am + bonus) + (double)lm_weight * final(lmst) +
 * (double)bias_weight * final2(lmst2)); a slot whose walk finds no final state drops out; the list is re-sorted by that
 * fp32 score, ties by the rank before.  Without use_final the scores are F in the beam's order.  The state is only read.
 *
 * Limits: 1 <= K <= C <= 64, B <= 65535, 2 C max_frames <= 2^28 (PIKA_ETOOBIG beyond; K > C is PIKA_EINVAL); V >= 2,
 * 0 <= blank < V, ld >= V, max_frames >= 1, finite sm_scale, blank_penalty, lm_weight, bias_weight and length_bonus;
 * num_states >= 1, num_arcs >= 0, start in [0, num_states), offsets and final present, the arc arrays present when
 * num_arcs > 0 (PIKA_EINVAL) -- all before any launch.
 */
#ifndef PIKA_MSEARCH_LM_H
#define PIKA_MSEARCH_LM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

/* Bytes of the state blob; 0 for dimensions the calls refuse. */
size_t pika_msearch_lm_state_bytes(int B, int K, int C, int max_frames);

/* Every utterance (which == NULL) or those with which[b] != 0 (i32 (B,)) back to the empty sequence in the automata's
 * start states; the others' state, tables included, is not touched.  num_states2 == 0: no second automaton. */
int pika_msearch_lm_reset(void *state, int B, int K, int C, int max_frames, int num_states, int start, int num_states2,
                          int start2, const int *which, void *stream);

/* One fused frame step; logits, ld, num_frames, parent_out and token_out as in pika_msearch_advance. */
int pika_msearch_lm_advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K,
                            int C, int max_frames, int V, int blank, float sm_scale, float blank_penalty,
                            const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                            const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                            int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int backoff_id2, int label_offset2, float lm_weight,
                            float bias_weight, float length_bonus, long long *parent_out, long long *token_out,
                            void *stream);

/* The nbest <= K best entries: tokens i64 (B, nbest, L), -1 beyond the length; lengths i64 (B, nbest), -1 for a missing
 * entry; scores f32 (B, nbest), the fused score (+ the final terms with use_final), -inf for a missing entry; am_scores
 * f32 (B, nbest), am alone.  An entry longer than L reports its true length and its first L tokens. */
int pika_msearch_lm_results(const void *state, int B, int K, int C, int max_frames, const long long *fst_offsets,
                            const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                            const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                            int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int start2, int backoff_id2, int label_offset2,
                            float lm_weight, float bias_weight, int use_final, int nbest, int L, long long *tokens,
                            long long *lengths, float *scores, float *am_scores, void *stream);

/* The token sequences of the K current slots, as pika_msearch_hyps. */
int pika_msearch_lm_hyps(const void *state, int B, int K, int C, int max_frames, int L, long long *tokens,
                         long long *lengths, void *stream);

#ifdef __cplusplus
}
#endif

#endif
