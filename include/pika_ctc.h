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

#ifdef __cplusplus
}
#endif
#endif /* PIKA_CTC_H */
