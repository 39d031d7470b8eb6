/*
 * include/pika_msearch_nn.h -- C ABI of the one-symbol-per-frame ("modified") transducer beam search with a NEURAL LM
 * fused into the ranking (libpika_amd.so): the search of pika_msearch_lm.h with a dense row of LM logits per live
 * hypothesis, new every frame, beside up to two back-off FSTs (icefall's modified_beam_search_lm_shallow_fusion; with a
 * low-order n-gram on a negative weight beside it, modified_beam_search_LODR).  A neural LM cannot be compiled into an
 * automaton: its state lives with the caller, as the prediction network's does, and the caller hands the step the LM's
 * output for every slot.  Conventions, the logits contract, ACTIVE utterances, frames, overflowed, the automata and the
 * STATE BLOB are those of pika_msearch_lm.h: pika_msearch_lm_state_bytes sizes the blob and pika_msearch_lm_hyps reads
 * the slots.  Here EITHER automaton may be "none" (num_states == 0, num_arcs == 0, NULL arrays); a second without a
 * first is PIKA_EINVAL.  lmst / lmst2 of an automaton that does not exist are 0.
 *
 * The step extends the step of pika_msearch_lm.h; everything not said here is that header's.
 *   Inputs beside the fused step's: lm_logits f32 (B K, V_lm), row stride lm_ld >= V_lm elements, row b K + k the LM's
 *   output for OLD slot k of utterance b (16-byte loads where lm_ld % 4 == 0 and the base is 16-byte aligned, scalar
 *   loads otherwise); V_lm >= 1; nn_label_offset; finite nn_scale and nn_weight.
 *   ROW STATISTICS, for every live old slot k: y[c] = nn_scale * lm_logits[k,c], the product rounded on its own;
 *   M[k] = max_c y[c], S[k] = log(sum_c exp(y[c] - M[k])) over all V_lm columns; a column whose y is -inf or NaN takes
 *   no part in either (a +inf makes M +inf).  fp32 with accurate expf / logf, summed as the acoustic row pass sums:
 *     a lane owns the columns 4 i .. 4 i + 3 for i = lane, lane + 64, ... < V_lm / 4 and then the columns
 *     4 (V_lm / 4) + lane, + 64, ... (16-byte loads), or the columns lane, lane + 64, ... (scalar loads), and folds them in
 *     that order into (m, s), from (-inf, 0):  y > m: s = s * exp(m - y) + 1, m = y (product and sum rounded apart);
 *     otherwise, y > -inf: s = s + exp(y - m).  The 64 lanes' pairs are combined in 6 rounds o = 32, 16, .. 1, lane l
 *     with lane l ^ o:  M = max(m, m'), s = s * exp(m - M) + s' * exp(m' - M) (a side with m = -inf counts 0), m = M;
 *     lane 0's pair is the row's, S = log(s).
 *   The load width therefore changes the ORDER of the sum (S in its last bits), nothing else; on given pointers two runs
 *   give the same bits.
 *   PRE-SELECTION: unchanged -- the C best of F[k] + lp[k,v] in the plain step's total order; the dense term does not
 *   enter the cut.  The same pruning contract; C = K is icefall's rule.
 *   EXTENSION of a pre-selected label (k, v): c = v + nn_label_offset.  The candidate DOES NOT EXIST if c is outside
 *   [0, V_lm), if M[k] is not finite, or if inc_nn = (y[c] - M[k]) - S[k] (fp32, the differences rounded apart) is not
 *   finite (inc_nn - inc_nn == 0 fails) -- as when an automaton does not reach v: it is dropped whatever the weights are
 *   and creates no trie node.  Otherwise
 *     bonus' = bonus[k] + (double)lm_weight * inc + (double)bias_weight * inc2 + (double)nn_weight * inc_nn
 *              + (double)length_bonus,
 *   the automaton terms present only for the automata that exist, inc_nn rounded to fp32 once, the products and sums
 *   fp64, rounded one by one in that order.  Blank is untouched by the dense term.
 *   MERGE and NEW BEAM as in the fused step: a group takes its REPRESENTATIVE's bonus' and states.  With automata alone
 *   the members of a group agree on them bit for bit, the bonus being a function of the tokens under one formula; with a
 *   neural LM they agree only if the caller's LM gives equal rows for equal token sequences.  The kernel does not check
 *   this.
 * c and the row index are clamped before they index; a dead slot's LM row is never read.  No floating-point atomics.
 * With nn_weight = 0, finite LM rows and every class in range the step is pika_msearch_lm_advance with the same automata,
 * bit for bit; with no automaton, nn_weight = length_bonus = 0 and C = K, F, node, len, parent_out and token_out are
 * pika_msearch_advance's.
 *
 * Results: as pika_msearch_lm_results; use_final adds the final terms of the automata that exist.  The neural LM has no
 * final term (no end-of-sentence class is scored): with no automaton the scores are F in the beam's order.
 *
 * Limits: those of pika_msearch_lm.h, and V_lm >= 1, lm_ld >= V_lm, finite nn_scale and nn_weight (PIKA_EINVAL) -- all
 * before any launch.
 */
#ifndef PIKA_MSEARCH_NN_H
#define PIKA_MSEARCH_NN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

/* As pika_msearch_lm_reset; num_states == 0: no first automaton (then no second either), lmst = 0. */
int pika_msearch_nn_reset(void *state, int B, int K, int C, int max_frames, int num_states, int start, int num_states2,
                          int start2, const int *which, void *stream);

/* One frame step with the LM's rows; the other arguments as in pika_msearch_lm_advance, either automaton "none". */
int pika_msearch_nn_advance(void *state, const float *logits, long long ld, const long long *num_frames, int B, int K,
                            int C, int max_frames, int V, int blank, float sm_scale, float blank_penalty,
                            const long long *fst_offsets, const int *fst_ilabel, const float *fst_weight,
                            const int *fst_nextstate, const float *fst_final, int num_states, int num_arcs,
                            int backoff_id, int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int backoff_id2, int label_offset2, float lm_weight,
                            float bias_weight, float length_bonus, const float *lm_logits, long long lm_ld, int V_lm,
                            int nn_label_offset, float nn_scale, float nn_weight, long long *parent_out,
                            long long *token_out, void *stream);

/* As pika_msearch_lm_results, either automaton "none". */
int pika_msearch_nn_results(const void *state, int B, int K, int C, int max_frames, const long long *fst_offsets,
                            const int *fst_ilabel, const float *fst_weight, const int *fst_nextstate,
                            const float *fst_final, int num_states, int num_arcs, int start, int backoff_id,
                            int label_offset, const long long *fst2_offsets, const int *fst2_ilabel,
                            const float *fst2_weight, const int *fst2_nextstate, const float *fst2_final,
                            int num_states2, int num_arcs2, int start2, int backoff_id2, int label_offset2,
                            float lm_weight, float bias_weight, int use_final, int nbest, int L, long long *tokens,
                            long long *lengths, float *scores, float *am_scores, void *stream);

#ifdef __cplusplus
}
#endif

#endif
