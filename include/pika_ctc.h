/*
 * include/pika_ctc.h -- C ABI of the MI355X-native CTC loss, its gradient and forced alignment (libpika_amd.so).
 *
 * The loss the reference's LAS trainer builds as `nn.CTCLoss()` for joint encoder training
 * (trainer/train_las_bmuf_otfaug.py:58-81).  Conventions are those of pika_rnnt.h: plain pointers + sizes, every pointer
 * DEVICE memory owned by the caller, work enqueued on `stream` (a hipStream_t as void*, NULL = default stream) and
 * stream-ordered with no host synchronisation, thread-safe per stream; return 0 on success, a negative PIKA_E* code for
 * bad arguments (before any launch), a positive hipError_t if a launch failed.
 *
 * The lattice: utterance n with U_n labels has S_n = 2 U_n + 1 states l' = (blank, y_1, blank, ..., y_U, blank) over T_n
 * frames,
 *   alpha_t(s) = lp_t(l'_s) + logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if l'_s != blank, != l'_{s-2}])
 *   cost_n     = -logsumexp(alpha_{T_n-1}(S_n-1), alpha_{T_n-1}(S_n-2)).
 *
 * Tensor contract:
 *   log_probs / logits f32 (T,B,C) contiguous (time-major, as torch.nn.functional.ctc_loss); frames t >= T_n are never read
 *   targets        i32; target_offsets == NULL: (B,U_max) padded, entries >= target_lengths[n] never read;
 *                  otherwise the 1-D concatenation, utterance n's labels at targets + target_offsets[n]
 *   target_offsets i32 (B,) exclusive prefix sum of the target lengths, or NULL
 *   input_lengths  i32 (B,) T_n, clamped on the device to [1,T]
 *   target_lengths i32 (B,) U_n, clamped on the device to [0,U_max]
 *   costs          f32 (B,) -log P(y_n | x_n); +inf for an infeasible utterance
 *   grads          f32 (T,B,C) DENSE: every element is written (zeros included), the caller may pass uninitialised memory
 * Limits: 2 U_max + 1 <= 1024 (one workgroup spans the state axis; PIKA_ETOOBIG beyond), any C >= 1, blank anywhere in
 * [0,C).  U_max == 0 is allowed (targets may then be NULL).
 * A label outside [0,C) makes its states impossible (-1e30 in the plane): an infeasible transcript, not a fault.
 * Infeasible utterances (T_n < U_n + number of adjacent repeats, or a label outside [0,C)): the cost is +inf and EVERY
 * gradient row of that utterance is zero.  (torch.nn.functional.ctc_loss gives NaN gradients there unless
 * zero_infinity=True; zero_infinity itself only turns the cost into 0 and is left to the caller.)
 * The gradient is the TRUE derivative with respect to the input: for log_probs, t < T_n,
 *   grads[t,n,c] = -grad_costs[n] * sum_{s : l'_s = c} exp(alpha_t(s) + beta_t(s) - lp_t(c) - ll_n)
 * (torch's native kernel returns exp(lp) minus that sum, which is the derivative only after a log_softmax backward);
 * for logits, grad_costs[n] * (softmax_t(c) - occ_t(c)).  Both are exactly zero for t >= T_n.  The states of one class are
 * summed in increasing state order, with no atomics: two runs give bit-identical gradients.
 */
#ifndef PIKA_CTC_H
#define PIKA_CTC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* state axis wider than one workgroup */
#endif

/* Bytes of device scratch `workspace` for a (B,T,U_max) batch; 0 for dimensions the calls refuse (B, T < 1, U_max < 0,
 * 2 U_max + 1 > 1024).  With Wp = 2 U_max + 1 rounded up to a multiple of 64:
 *   3 f32 planes [B][T][Wp]  (state log-probs lp_t(l'_s), -1e30 in invalid cells; alpha; beta)      12 B T Wp
 *   2 f64 offset rows [B][T] (alpha_t(s) = plane + off_a[t], likewise beta) + ll [B] f64            16 B T + 8 B
 *   3 i32 state rows [B][Wp] (class of a state, -1 beyond S_n; skip transition allowed;
 *                              next state of the same class, -1 at the last)                        12 B Wp
 * alpha and beta both INCLUDE the frame's own emission lp_t(l'_s). */
size_t pika_ctc_workspace_bytes(int B, int T, int U_max);

/* Bytes of back-pointer scratch of pika_ctc_align: one byte per plane cell, B T Wp; 0 for refused dimensions. */
size_t pika_ctc_align_scratch_bytes(int B, int T, int U_max);

/* Forward: gathers the state plane, runs the alpha and beta recurrences concurrently (one workgroup per utterance and
 * direction), writes costs[B] and leaves the lattice in `workspace` for the backward and alignment calls. */
int pika_ctc_loss_forward(const float *log_probs, const int *targets, const int *target_offsets,
                          const int *input_lengths, const int *target_lengths, int B, int T, int U_max, int C,
                          int blank, float *costs, void *workspace, void *stream);

/* Backward: one pass that writes the dense (T,B,C) gradient.  grad_costs (B,) f32 scales utterance n's gradient
 * (autograd's grad_output); NULL means all ones.  `workspace` is the buffer the matching forward call filled. */
int pika_ctc_loss_backward(const int *input_lengths, const int *target_lengths, int B, int T, int U_max, int C,
                           int blank, const float *grad_costs, const void *workspace, float *grads, void *stream);

/* Fused boundary logits -> (costs, d loss / d logits): log-softmax + loss + log-softmax backward.  `logits` (T,B,C) are
 * RAW; lse (T*B) f32 receives the log-sum-exp of every row t < T_n (0 beyond) in the same pass that fills the state plane
 * with logit - lse, and must be handed to the backward with the same logits and workspace.  The log-probabilities never
 * exist. */
int pika_ctc_fused_forward(const float *logits, const int *targets, const int *target_offsets,
                           const int *input_lengths, const int *target_lengths, int B, int T, int U_max, int C,
                           int blank, float *costs, float *lse, void *workspace, void *stream);
int pika_ctc_fused_backward(const float *logits, const float *lse, const int *input_lengths,
                            const int *target_lengths, int B, int T, int U_max, int C, int blank,
                            const float *grad_costs, const void *workspace, float *grad_logits, void *stream);

/* Forced alignment: the single best path of every utterance (Viterbi, max-plus over the same state plane, fp32).  Reads
 * ONLY the state plane and state rows a forward call above left in `workspace` (same B, T, U_max and lengths) and leaves
 * the workspace untouched: forward -> align -> backward gives the gradients of forward -> backward.
 *   scores       f32 (B,)   log-probability of the best path (<= -costs[n]); <= -1e30 for an infeasible transcript
 *   frame_labels i32 (B,T)  the class the best path emits at frame t (blank included; a label outside [0,C) is reported
 *                           as it stands in `targets`), -1 for t >= T_n
 *   scratch      pika_ctc_align_scratch_bytes(B,T,U_max) bytes of back-pointers
 * Tie rule: at the end state S_n-1 is preferred over S_n-2; in the back-trace the stay (s) is preferred, then s-1, then
 * s-2.  A move that would leave the state axis or that the skip rule forbids is never taken, so the path always consists
 * of valid state indices, whatever the plane holds. */
int pika_ctc_align(const void *workspace, const int *input_lengths, const int *target_lengths, int B, int T, int U_max,
                   float *scores, int *frame_labels, void *scratch, void *stream);

/* n-best alignment: for every hypothesis of an n-best list -- what pika_ctc_beam_search, pika_ctc_lm_beam_search and the
 * stream results calls return -- its full-sum score, its best path's score, and per token the frames of that path's run
 * and the run's summed log-probability.  One workgroup per hypothesis over the utterance's own rows of x: the input is
 * not replicated and no plane is written.
 *   x, stride_t, stride_b   f32, row (t,b) at x + t * stride_t + b * stride_b (strides in ELEMENTS), C contiguous classes,
 *                  as in pika_ctc_decode.h; rows t >= T_b are never read; values below -1e30 (-inf, NaN) read as -1e30
 *   lse            f32 (T,B) the rows' log-sum-exps as pika_ctc_decode_rows writes them: x holds raw logits and every value
 *                  is logit - lse rounded once; NULL: x holds log-probs
 *   input_lengths  i32 (B,)     T_b, clamped on the device to [1,T]
 *   tokens         i32 (B,N,L)  hypothesis (b,k) at tokens + (b N + k) L; entries at or beyond its length are never read
 *   lengths        i32 (B,N)    U; below 0: a missing entry
 *   full_scores    f32 (B,N)    log of the sum over ALL alignments of the hypothesis: -cost of pika_ctc_loss_forward for
 *                               that transcript, with its numerics (fp32 states, the running maximum moved into an fp64
 *                               offset every 8 frames)
 *   best_scores    f32 (B,N)    log-probability of the best (Viterbi) path: fp32 max-plus and the tie rule of pika_ctc_align
 *                               (at the end state S-1 over S-2; in the back-trace stay, then s-1, then s-2)
 *   starts, ends   i32 (B,N,L)  first and last frame (inclusive) of the run in which that path emits token j
 *   token_scores   f32 (B,N,L)  sum over t = starts[j] .. ends[j] of the value of token j's class at frame t, in fp32 in
 *                               increasing t; exp(token_scores / (ends - starts + 1)) is the geometric mean of the
 *                               token's frame posteriors
 * Beyond an entry's length starts / ends are -1 and token_scores -inf.  A missing entry, and an INFEASIBLE one
 * (T_b < U + adjacent repeats, a token outside [0,C), a token equal to blank), has both scores -inf, times -1 and token
 * scores -inf: not a fault, and nothing is read through such a token.  An entry LONGER than min(U_max, L) has both scores
 * NaN and the per-token outputs of a missing entry.  An empty hypothesis (U = 0) has full = best = the sum of the blank's
 * values.  Every output element is written.  Everything read from input_lengths, lengths and tokens bounds loops and
 * stores through clamps.  No atomics: two runs give bit-identical outputs.
 * Limits: 2 U_max + 1 <= 1024 (the limit is on U_max, the state axis one workgroup spans, not on the row width L of
 * `tokens`); B, N <= 65535 (the grid's extents); PIKA_ETOOBIG beyond, and for a scratch size beyond size_t.
 * PIKA_EINVAL for a null pointer (lse excepted), B, N, L, T, C < 1, U_max < 0, blank outside [0,C).
 *
 * Scratch: back-pointers at TWO BITS per cell -- four frames of one state to a byte -- in rows of Wp bytes (Wp = 2 U_max
 * + 1 rounded up to a multiple of 64): B N ceil(T / 4) Wp bytes; 0 for refused dimensions. */
size_t pika_ctc_nbest_align_scratch_bytes(int B, int N, int T, int U_max);
int pika_ctc_nbest_align(const float *x, long long stride_t, long long stride_b, const float *lse,
                         const int *input_lengths, const int *tokens, const int *lengths, int B, int N, int L, int T,
                         int C, int blank, int U_max, float *full_scores, float *best_scores, int *starts, int *ends,
                         float *token_scores, void *scratch, void *stream);

/* n-best loss: the full-sum scores of an n-best list and the gradient of sum_k grad_scores[b,k] * full_scores[b,k] with
 * respect to the UN-replicated (T,B,C) input -- the primitive under MWER / MBR training over the list.  x, stride_t,
 * stride_b, lse, input_lengths, tokens, lengths, B, N, L, T, C, blank, U_max: as pika_ctc_nbest_align, with its
 * classification of an entry, made before anything is read through a token: a missing entry (length < 0) and an
 * infeasible one (a token outside [0,C), a token equal to blank, no path to the end) score -inf, an entry longer than
 * min(U_max, L) scores NaN.  Every such entry is DEAD: it contributes nothing to the gradient and its grad_scores entry
 * is never brought into arithmetic -- NaN and +-inf there (what a softmax over -inf scores leaves) do not reach `grads`.
 *   full_scores  f32 (B,N)    as pika_ctc_nbest_align's, with the same numerics
 *   grad_scores  f32 (B,N)    g[b,k], the weight of hypothesis k (autograd's grad_output)
 *   grads        f32 (T,B,C)  contiguous, DENSE: every element is written.  Rows t >= T_b are exactly zero; for t < T_b
 *       log-probs (lse NULL):  grads[t,b,c] = sum_k g[b,k] occ_k(t,c)
 *       logits:                grads[t,b,c] = sum_k g[b,k] occ_k(t,c) - (sum_{k live} g[b,k]) softmax_t(c)
 *       occ_k(t,c) = sum_{s : l'_s = c} exp(alpha_t(s) + beta_t(s) - value_t(c) - ll_k), the exponent assembled in fp64
 *     (the sign is that of full = -cost).  The sum runs over k in increasing order and, inside a hypothesis, over the
 *     states of a class in increasing order; no atomics: two runs give bit-identical gradients.
 * The forward runs one workgroup per hypothesis and direction; the backward one per (t,b) row, which writes the row once
 * and then adds hypothesis after hypothesis into it: there are never N dense gradients.  Frames t >= T_b of x and tokens
 * at or beyond an entry's length are never read.  `workspace` is filled by the forward and read by the backward, which
 * takes the same x, strides, lse and input_lengths.
 * Limits and codes as pika_ctc_nbest_align: PIKA_EINVAL for a null pointer (lse excepted), B, N, L, T, C < 1, U_max < 0,
 * blank outside [0,C); PIKA_ETOOBIG for U_max > 511, B or N > 65535, a size beyond size_t; all before any launch.
 *
 * Workspace, with Wp = 2 U_max + 1 rounded up to a multiple of 64; 0 for refused dimensions:
 *   2 f32 planes [B][N][T][Wp]   (alpha, beta, each minus its offset and INCLUDING the frame's own value)   8 B N T Wp
 *   2 f64 offset rows [B][N][T] + ll [B][N] f64 (-1e30: a dead entry)                                16 B N T + 8 B N
 *   3 i32 state rows [B][N][Wp]  (class, -1 beyond S; bit 0 skip allowed, bit 1 first of its class;
 *                                 next state of the same class, -1 at the last)                             12 B N Wp */
size_t pika_ctc_nbest_loss_workspace_bytes(int B, int N, int T, int U_max);
int pika_ctc_nbest_loss_forward(const float *x, long long stride_t, long long stride_b, const float *lse,
                                const int *input_lengths, const int *tokens, const int *lengths, int B, int N, int L,
                                int T, int C, int blank, int U_max, float *full_scores, void *workspace, void *stream);
int pika_ctc_nbest_loss_backward(const float *x, long long stride_t, long long stride_b, const float *lse,
                                 const int *input_lengths, int B, int N, int T, int C, int blank, int U_max,
                                 const float *grad_scores, const void *workspace, float *grads, void *stream);

/* n-best edit distances: the token edit (Levenshtein, unit costs) distance between every entry of a list `a` and every
 * entry of a list `r` of the same utterance -- `a` an n-best list and `r` the reference transcript (Nr = 1) for the
 * `errors` of MWER training; `a` = `r` = the list for the pairwise distances of MBR decoding.
 *   a_tokens   i32 (B,Na,La)  entry (b,i) at a_tokens + (b Na + i) La
 *   a_lengths  i32 (B,Na)     below 0: a missing entry; beyond La: La tokens
 *   r_tokens   i32 (B,Nr,Lr), r_lengths i32 (B,Nr): likewise, beyond Lr: Lr tokens
 *   out        i32 (B,Na,Nr)  out[b,i,j] = distance(a[b,i], r[b,j]); -1 where either entry is missing
 * All contiguous.  Tokens are compared as plain int32, any value; what lies at or beyond an entry's length is never
 * read.  An empty entry (length 0; La = 0 or Lr = 0, the token pointer may then be NULL) is at the other side's length
 * from everything.  Every element of `out` is written; integer arithmetic, no atomics: two runs are identical.
 * One wave per pair over a flat grid (no extent is bound by 65535): Myers' bit-vector recurrence in blocks of 64
 * reference positions, the wave's ballot as the machine word -- La ceil(S / 64) steps for a pair instead of La S cells.
 * PIKA_EINVAL for a negative size and, with B Na Nr > 0, a null pointer; PIKA_ETOOBIG for Lr > 4096 (64 blocks, one per
 * lane) and for B Na Nr > 2^31 - 1; both before any launch.  B Na Nr = 0 succeeds and does nothing.
 * pika_ctc_edit_distance_host: the same on HOST pointers, on the calling thread -- the same recurrence in the same block
 * order with the match vector built by a loop; the CPU path of the Python functions and the reference of the tests. */
int pika_ctc_edit_distance(const int *a_tokens, const int *a_lengths, int Na, int La, const int *r_tokens,
                           const int *r_lengths, int Nr, int Lr, int B, int *out, void *stream);
int pika_ctc_edit_distance_host(const int *a_tokens, const int *a_lengths, int Na, int La, const int *r_tokens,
                                const int *r_lengths, int Nr, int Lr, int B, int *out);

/* Long-form alignment: the best (Viterbi) path of ONE transcript per recording, with the state axis cut into tiles -- no
 * limit of 511 labels and no fp32 plane: an hour of audio against its whole transcript.  The outputs per token are those
 * of pika_ctc_nbest_align; the path is that of pika_ctc_align (same tie rule) wherever both can run.
 *   x, stride_t, stride_b, lse, input_lengths   as pika_ctc_nbest_align: value_t(c) is x (lse NULL: log-probs) or
 *                  logit - lse rounded once; anything below -1e30 (-inf, NaN) reads as -1e30; rows t >= T_b are never read
 *   targets        i32 (B,U_max) padded; entries at or beyond target_lengths[b] are never read
 *   target_lengths i32 (B,) U_b, clamped on the device to [0,U_max]
 *   scores         f32 (B,)  the log-probability of the best path, fl32(fp64(v_end) + sum_{t<T_b} fp64(m_t))
 *   starts, ends   i32 (B,U_max)  first and last frame (inclusive) of the run in which the path emits token j
 *   token_scores   f32 (B,U_max)  sum over the run of value_t(y_j), in fp32 in increasing t
 * Beyond a length starts / ends are -1 and token_scores -inf.  An INFEASIBLE transcript (a token outside [0,C), a token
 * equal to blank, v_end <= -1e29: no path, e.g. T_b < U_b + adjacent repeats) has score -inf, times -1 and token scores
 * -inf; nothing is read through a bad token.  Every output element is written; everything read from the length and token
 * arrays bounds loops and stores through clamps; no atomics: two runs give bit-identical outputs.
 *
 * The recurrence, in fp32 over the states s of l' = (blank, y_1, blank, ..., y_U, blank), S = 2U + 1:
 *   m_t    = max_c value_t(c)                       (logits: also maxlogit_t, the maximum of the clamped logits)
 *   e_t(s) = fl32(value_t(l'_s) - m_t)              (logits: fl32(logit_t(l'_s) - maxlogit_t), independent of lse); <= 0
 *   v_0(0) = e_0(0), v_0(1) = e_0(1), v_0(s) = -1e30 otherwise
 *   v_t(s) = fl32(e_t(s) + max(v_{t-1}(s), v_{t-1}(s-1) [s >= 1], v_{t-1}(s-2) [s odd, >= 3, l'_s != l'_{s-2}]))
 * the back-pointer being the first maximal predecessor in the order stay, s-1, s-2; at the end S-1 is preferred over S-2
 * (U = 0: state 0 alone).  Subtracting the row maximum moves every path by the same amount -- the arg-max is unchanged --
 * and keeps a well-aligned path near 0 over 1e5 frames.  For logits m_t = fl32(maxlogit_t - lse_t).
 *
 * Launches: one row pass (reads x once), ceil(T / 64) recurrence launches (a frame block each; grid = tiles of 896 owned
 * states x B; a tile recomputes the 128 states below it from the state column at the block's first frame, which is kept
 * ping-pong in scratch), one back-trace (a wave per recording), one launch for the per-token outputs.  Tiles depend on
 * one another through stream order only: no workgroup waits on another.  The launch sequence depends on (T, U_max) alone;
 * no host synchronisation; capturable.
 * Limits: U_max <= 2^28 (state indices and the padded state axis fit an int), B <= 65535 (a grid extent), a scratch size
 * within size_t; PIKA_ETOOBIG beyond.  PIKA_EINVAL for a null pointer (lse excepted; targets may be NULL when U_max == 0),
 * B, T, C < 1, U_max < 0, blank outside [0,C).  All refusals come before any launch: a negative size first, then a size
 * that is too big, then pointers.
 *
 * Scratch, with Sp = ceil((2 U_max + 1) / 896) * 896 and Tp = T rounded up to a multiple of 4; 0 for refused dimensions:
 *   back-pointers, two bits per cell, four frames of one state to a byte, rows of Sp bytes      B ceil(T / 4) Sp
 *   2 f32 state columns [B][Sp] (ping-pong)                                                      8 B Sp
 *   the per-frame state of the path, i32 [B][Tp]                                                 4 B Tp
 *   the rows' maxima (m_t for log-probs, maxlogit_t for logits), f32 [B][Tp]                     4 B Tp
 *   per recording: feasible, end state (4 i32)                                                   16 B */
size_t pika_ctc_long_align_scratch_bytes(int B, int T, int U_max);
int pika_ctc_long_align(const float *x, long long stride_t, long long stride_b, const float *lse,
                        const int *input_lengths, const int *targets, const int *target_lengths, int B, int T, int C,
                        int blank, int U_max, float *scores, int *starts, int *ends, float *token_scores,
                        void *scratch, void *stream);

/* Long-form loss: cost and gradient of pika_ctc_loss_forward / _backward (log-probs) and pika_ctc_fused_* (logits) with
 * the state axis cut into tiles -- no limit of 511 labels.  Sum-product over the tiling of pika_ctc_long_align: the same
 * dependency cone (alpha at (t,s) needs s, s-1, s-2 at t-1; beta is its mirror image), both planes kept for the backward.
 *   x, stride_t, stride_b, lse, input_lengths, targets, target_lengths   as pika_ctc_long_align: strides in ELEMENTS, C
 *                  contiguous classes; lse (T,B) as pika_ctc_decode_rows writes it and x raw logits, or NULL and x
 *                  log-probs; anything below -1e30 (-inf, NaN) reads as -1e30; rows t >= T_b are never read; targets
 *                  (B,U_max) padded, entries at or beyond target_lengths[b] never read; lengths clamped on the device
 *   costs          f32 (B,) -log P(y_b | x_b); +inf for an infeasible utterance
 *   grad_costs     f32 (B,) the weight of utterance b's cost (autograd's grad_output); NULL: all ones
 *   grads          f32 (T,B,C) contiguous, DENSE: every element is written.  For t < T_b
 *       log-probs:  grads[t,b,c] = -grad_costs[b] occ_t(c)            (the true derivative, as pika_ctc_loss_backward)
 *       logits:     grads[t,b,c] = grad_costs[b] (softmax_t(c) - occ_t(c))
 *       occ_t(c) = sum_{s : l'_s = c} exp(alpha_t(s) + beta_t(s) - value_t(c) - ll_b), the exponent assembled in fp64 from
 *     planes and offsets and rounded once; rows t >= T_b are exactly zero.
 * A label is classified as pika_ctc_loss_forward classifies it: one outside [0,C) makes its state impossible and nothing is
 * read through it; one equal to blank is a state of the blank class that no transition skips into.  An INFEASIBLE
 * utterance (T_b < U_b + adjacent repeats, a label outside [0,C)) costs +inf and EVERY row of its gradient is zero; its
 * neighbours in the batch are not affected.
 *
 * Numerics: log-space fp32, -1e30 for "impossible", the usual guarded log-sum-exp.  Every frame's values are taken relative
 * to the row maximum r_t: e_t(s) = fl32(x_t(l'_s) - r_t) <= 0; and at the start of every block of 64 frames every tile takes
 * the same amount R out of all its states: the largest value of the state column the launch before left, which it reads
 * as one maximum per tile (max is exact and order-free, so every tile gets the same bits).  R and M_t = r_t (- lse_t for
 * logits) are summed in fp64 into one offset per frame and direction: alpha_t(s) = plane_a[t][s] + off_a[t], beta alike.
 * Both include the frame's own emission.  ll_b = off_a[T_b-1] + logsumexp(plane_a[T_b-1][S-1], plane_a[T_b-1][S-2]) in fp64
 * (state 0 alone at U_b = 0).
 *
 * Launches of the forward: one row pass (reads x once); one launch that sorts every transcript's labels by (class,
 * position), by counting ranks (U_max > 0); ceil(T / 64) recurrence launches, grid = tiles of 896 owned states x B x 2
 * directions: launch k advances alpha over frame block k and beta over frame block ceil(T / 64) - 1 - k.  A tile recomputes
 * 128 states beside its own (below for alpha, above for beta) from the state column at the block's edge, which is kept
 * ping-pong; beta of utterance b starts at T_b - 1 inside whichever block holds it.  Then a launch with a thread per
 * utterance for ll and the cost.  The backward is ONE launch, a workgroup per (t,b) row: it writes the row once (zeros, or
 * grad_costs softmax; 16-byte stores where C % 4 == 0 and the row is aligned) and then the class entries -- blank from the
 * even states, thread-strided partial sums joined in a fixed tree; the labels in sorted order, a contiguous chunk per
 * thread, a class that spans chunks joined in chunk order.  No float atomics; the order of every sum depends on
 * (t, T_b, U_b) alone: two runs give bit-identical outputs.  Tiles depend on one another through stream order only: no
 * workgroup waits on another.  The launch sequence depends on (T, U_max) alone; no host synchronisation; capturable.
 * `workspace` is filled by the forward and read by the backward, which takes the same x, strides, lse and lengths.
 * Limits: U_max <= 2^28, B <= 65535 (a grid extent), a workspace size within size_t; PIKA_ETOOBIG beyond.  PIKA_EINVAL for
 * a null pointer (lse and grad_costs excepted; targets may be NULL when U_max == 0), B, T, C < 1, U_max < 0, blank outside
 * [0,C).  All refusals come before any launch: a negative size first, then a size that is too big, then pointers.
 *
 * Workspace, with Sp = ceil((2 U_max + 1) / 896) * 896; 0 for refused dimensions:
 *   2 f32 planes [B][T][Sp] (alpha, beta, each minus its offset)                                  8 B T Sp
 *   2 f64 offset rows [B][T] + ll [B] f64 (-1e30: infeasible)                                     16 B T + 8 B
 *   4 f32 state columns [B][Sp] (direction x ping-pong)                                           16 B Sp
 *   their per-tile maxima, 4 f32 [B][Sp / 896]                                                    16 B Sp / 896
 *   the rows' maxima r_t, f32 [B][T]                                                              4 B T
 *   the sorted labels: position and class, 2 i32 [B][U_max]                                       8 B U_max
 * The planes are kept, not recomputed: about 8 B T Sp bytes, 29 GB for an hour (T = 90 000) against 20 000 labels. */
size_t pika_ctc_long_loss_workspace_bytes(int B, int T, int U_max);
int pika_ctc_long_loss_forward(const float *x, long long stride_t, long long stride_b, const float *lse,
                               const int *input_lengths, const int *targets, const int *target_lengths, int B, int T,
                               int C, int blank, int U_max, float *costs, void *workspace, void *stream);
int pika_ctc_long_loss_backward(const float *x, long long stride_t, long long stride_b, const float *lse,
                                const int *input_lengths, const int *target_lengths, int B, int T, int C, int blank,
                                int U_max, const float *grad_costs, const void *workspace, float *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKA_CTC_H */
