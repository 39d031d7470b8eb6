/*
 * include/pika_rnnt.h -- C ABI of the MI355X-native RNN-T loss (libpika_amd.so).
 *
 * Replaces, for PIKA's RNN-T training path, the third-party `warp_rnnt` CUDA
 * extension that the reference binds at
 *   /root/reference/trainer/train_transducer_bmuf_otfaug.py:25,58,97-99
 *   /root/reference/trainer/train_transducer_mbr_bmuf_otfaug.py:23,64,157-159
 * (`RNNTLoss(blank=0, reduction='sum').apply(log_probs, labels, frames_lengths,
 *   labels_lengths)` -> per-utterance costs, differentiable w.r.t. log_probs).
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory
 *     owned by the caller; the library never allocates or frees device memory;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and is stream-ordered: nothing synchronises the host;
 *   - thread-safe per stream (no global mutable state);
 *   - return value: 0 on success, a negative PIKA_E* code for bad arguments,
 *     a positive hipError_t value if a launch failed.
 *
 * Tensor contract:
 *   log_probs      f32 (B,T,U1,V) contiguous, already log-softmaxed
 *   labels         i32 (B,U1-1)   entries >= labels_lengths[n] are padding and never read
 *   frames_lengths i32 (B,)       T_n, clamped on device to [1,T]
 *   labels_lengths i32 (B,)       U_n, clamped on device to [0,U1-1]
 *   costs          f32 (B,)       -log P(y_n | x_n)
 *   grads          f32 (B,T,U1,V) d(sum_n grad_costs[n]*cost_n)/d log_probs, DENSE:
 *                                 every element is written (zeros included), so the
 *                                 caller may hand over uninitialised memory.
 */
#ifndef PIKA_RNNT_H
#define PIKA_RNNT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* U1 > 1024 (one workgroup spans the label axis) */

/* Library/ABI version, bumped on any signature change.  Adding symbols is not one: pika_ctc.h came in under 25. */
int pika_amd_abi_version(void);

/* Bytes of device scratch `workspace` needed by the calls below for a (B,T,U1)
 * lattice batch.  Layout (DESIGN.md "RNNT loss / HBM layout"): four skewed
 * f32 planes [B][T+U1-1][W] (W = workgroup width covering U1, a multiple of 64) (blank log-prob, emit log-prob, alpha,
 * beta) + per-utterance log-likelihoods. */
size_t pika_rnnt_workspace_bytes(int B, int T, int U1);

/* Forward: gathers the two log-probs each lattice cell needs, runs the alpha and
 * beta anti-diagonal recurrences (one wavefront per direction per utterance),
 * writes costs[B] and leaves the lattice in `workspace` for the backward call. */
int pika_rnnt_loss_forward(const float *log_probs, const int *labels,
                           const int *frames_lengths, const int *labels_lengths,
                           int B, int T, int U1, int V, int blank,
                           float *costs, void *workspace, void *stream);

/* Backward: one streaming pass that writes the dense gradient tensor.
 * `grad_costs` (B,) f32 scales utterance n's gradient (autograd's grad_output);
 * NULL means all ones.  `workspace` must be the buffer filled by the matching
 * forward call (same B,T,U1 and lengths).
 * grads == NULL: only the per-row metadata (the at most two non-zeros of every V-row, already scaled by
 * grad_costs) is left in `workspace`; pika_rnnt_loss_dense_grads writes the dense tensor from it later, and
 * pika_rnnt_dlogits_compact_bf16 needs nothing else. */
int pika_rnnt_loss_backward(const int *labels, const int *frames_lengths,
                            const int *labels_lengths,
                            int B, int T, int U1, int V, int blank,
                            const float *grad_costs, const void *workspace,
                            float *grads, void *stream);

/* pika_rnnt_loss_backward with FastEmit (Yu et al. 2021, arXiv:2010.11148): every label-emission entry
 * (n, t, u, y_{u+1}), u < U_n, of the gradient is multiplied by 1 + fastemit_lambda; blank entries, the costs
 * and the zeros outside the sub-lattice are unchanged.  fastemit_lambda must be finite and >= 0 (PIKA_EINVAL
 * otherwise); 0 gives exactly pika_rnnt_loss_backward.  The factor is part of the row metadata left in
 * `workspace`, so with grads == NULL every reader of it -- pika_rnnt_loss_dense_grads and the d(logits) calls
 * below -- gets the FastEmit gradient. */
int pika_rnnt_loss_backward_fe(const int *labels, const int *frames_lengths, const int *labels_lengths,
                               int B, int T, int U1, int V, int blank, const float *grad_costs,
                               const void *workspace, float *grads, float fastemit_lambda, void *stream);

/* The streaming pass of pika_rnnt_loss_backward on its own: dense (B,T,U1,V) gradient from the row metadata a
 * pika_rnnt_loss_backward call (with or without `grads`) left in `workspace`. */
int pika_rnnt_loss_dense_grads(const void *workspace, int B, int T, int U1, int V, int blank,
                               float *grads, void *stream);

/* pika_rnnt_loss_dense_grads into a tensor that may already hold a gradient this library wrote.  Every V-row of the
 * gradient has at most two non-zeros, in column `blank` and in the row's label column; the call leaves the label
 * column of every row (-1: none) in cols_out (B*T*U1 ints).
 * prev_cols == NULL: nothing is known about `grads`; the streaming pass of pika_rnnt_loss_dense_grads writes every
 * word, then a small pass writes cols_out.
 * prev_cols != NULL: the caller guarantees that `grads` holds, unmodified, what an earlier call of this entry wrote
 * with the same V: rows [0, prev_rows) with non-zeros in column prev_blank and column prev_cols[r] only, and +0.0f in
 * every other word of its first max(prev_rows, B*T*U1) rows.  One small kernel then stores +0.0f over the old
 * non-zeros and the new values where they belong: about four dword stores per row, not the V-row.  Rows from B*T*U1
 * up to prev_rows are left all zero.  The words are bit for bit those of the streaming pass.  cols_out may be
 * prev_cols.  prev_rows < 0 or prev_blank outside [0, V): PIKA_EINVAL; prev_rows >= 2^31: PIKA_ETOOBIG. */
int pika_rgrad_dense_grads_update(const void *workspace, int B, int T, int U1, int V, int blank, float *grads,
                                  const int *prev_cols, long long prev_rows, int prev_blank, int *cols_out,
                                  void *stream);

/* pika_rnnt_loss_backward_fe (grads required) with pika_rgrad_dense_grads_update as its writer: one host call per
 * backward. */
int pika_rgrad_backward_fe(const int *labels, const int *frames_lengths, const int *labels_lengths,
                           int B, int T, int U1, int V, int blank, const float *grad_costs,
                           const void *workspace, float *grads, float fastemit_lambda, const int *prev_cols,
                           long long prev_rows, int prev_blank, int *cols_out, void *stream);

/* pika_rgrad_backward_fe with an element stride for grad_costs: utterance b's factor is grad_costs[b * gc_stride]
 * (0: one expanded scalar, as `costs.sum().backward()` hands it over).  gc_stride < 0: PIKA_EINVAL, after the checks
 * of pika_rgrad_backward_fe, which is this entry with gc_stride = 1. */
int pika_rgrad_backward_fe_s(const int *labels, const int *frames_lengths, const int *labels_lengths,
                             int B, int T, int U1, int V, int blank, const float *grad_costs, long long gc_stride,
                             const void *workspace, float *grads, float fastemit_lambda, const int *prev_cols,
                             long long prev_rows, int prev_blank, int *cols_out, void *stream);

/* warp_rnnt-shaped one-shot: forward + backward with unit grad_costs. */
int pika_rnnt_loss_fwd_bwd(const float *log_probs, const int *labels,
                           const int *frames_lengths, const int *labels_lengths,
                           int B, int T, int U1, int V, int blank,
                           float *costs, float *grads, void *workspace, void *stream);

/* Test/diagnostic hook: un-skews the lattice held in `workspace` into dense
 * (B,T,U1) f32 planes (invalid cells = -1e30).  Either output may be NULL. */
int pika_rnnt_export_lattice(const void *workspace, const int *frames_lengths,
                             const int *labels_lengths, int B, int T, int U1,
                             float *alphas, float *betas, void *stream);

/* For a producer that computed log_probs = log_softmax(scale * logits) itself (the joint network,
 * trainer/model/transducer.py:108-111): d(loss)/d(logits) as a bf16 matrix (rows = B*T*U1, pitch ld_out,
 * columns [V, ld_out) zero) straight from the two non-zeros per row that the matching
 * pika_rnnt_loss_backward call left in `workspace` -- the dense gradient (B,T,U1,V) need not be read back,
 * nor even written (grads == NULL above):
 *   out[r, v] = scale * (grad[r, v] - exp(log_probs[r, v]) * sum_v' grad[r, v']).
 * colsum (V floats, may be NULL) receives sum_r out[r, :] before the bf16 rounding: the bias gradient of the
 * layer that produced the logits, without another pass over `out`.
 * lse (rows floats) non-NULL: `log_probs` holds the RAW logits and lse their per-row log-sum-exp (as written by
 * pika_rnnt_fused_forward) -- the log-probabilities never have to exist (scale must then be 1).
 * V % 4 == 0, V <= 8192, ld_out % 4 == 0 (a wave covers a row in 64 x 4 x 20 columns up to 5120, x 32 beyond). */
int pika_rnnt_dlogits_compact_bf16(const float *log_probs, const float *lse, const void *workspace, int B, int T,
                                   int U1, int V, int blank, void *out, long long ld_out, float scale,
                                   float *colsum, void *stream);

/* pika_rnnt_fused_forward with the row log-sum-exp taken from partial statistics instead of a pass over the logits:
 * pmax / psum (rows, n_part) as written by pika_gemm_bf16_nt_lse (pika_gemm.h) for the SAME logits.  Reads
 * 8*n_part bytes + two 64-byte sectors per lattice cell instead of 4*V bytes. */
int pika_rnnt_fused_forward_partials(const float *logits, const float *pmax, const float *psum, int n_part,
                                     const int *labels, const int *frames_lengths, const int *labels_lengths, int B,
                                     int T, int U1, int V, int blank, float *costs, float *lse, void *workspace,
                                     void *stream);

/* pika_rnnt_fused_forward_partials for the 16-bit logits of pika_gemm_bf16_nt_lse_f16 (pika_gemm.h): logits16 is the
 * fp16 matrix (row pitch ld16 halves), gathered / g_labels / g_blank what that product's epilogue left in fp32 -- per
 * lattice row the logits of column g_blank and of the row's label g_labels[b][u].  A lattice cell whose label (blank) is
 * the gathered one takes the fp32 value, so costs and log-sum-exp are those of the fp32 logits; any other label reads the
 * fp16 logit.  g_labels may be NULL (nothing gathered for labels). */
int pika_rnnt_fused_forward_gathered(const void *logits16, long long ld16, const float *gathered, const int *g_labels,
                                     int g_blank, const float *pmax, const float *psum, int n_part, const int *labels,
                                     const int *frames_lengths, const int *labels_lengths, int B, int T, int U1, int V,
                                     int blank, float *costs, float *lse, void *workspace, void *stream);

/* pika_rnnt_dlogits_compact_bf16 reading the RAW logits as fp16 (row pitch ld_in halves; lse = their row log-sum-exp from
 * the forward call above, required): d(logits) = scale * (g - softmax * sum(g)) as one bf16 matrix + column sums.
 * gathered (optional; with g_labels / g_blank as in pika_rnnt_fused_forward_gathered: the (rows, 2) f32 blank and label
 * logits of every row): the softmax of those two columns -- the only entries that also carry the loss' own gradient terms -- is then taken from
 * the fp32 values instead of the fp16 copy. */
int pika_rnnt_dlogits_compact_bf16_f16in(const void *logits16, long long ld_in, const float *lse, const void *workspace,
                                         int B, int T, int U1, int V, int blank, void *out, long long ld_out, float scale,
                                         float *colsum, const float *gathered, const int *g_labels, int g_blank,
                                         void *stream);

/* Fused boundary logits -> (costs, d loss / d logits)  (SURVEY.md 8d M1'): replaces
 * F.log_softmax (trainer/model/transducer.py:111) + the loss + the log-softmax backward for a caller that owns
 * the joint output.  `logits` (B,T,U1,V) f32 are the RAW fc2 outputs, V % 4 == 0, V <= 8192; lse (B*T*U1) f32
 * receives the per-row log-sum-exp and must be handed to the backward together with the same logits and
 * workspace.  grad_logits: f32 (out_dtype 0, ld_out >= V) or bf16 (out_dtype 1; columns [V, ld_out) zeroed).
 * Traffic 3 x B*T*U1*V*4 bytes (one read for lse + gather, one read + one write for the gradient) against
 * 6 x for the three separate passes. */
int pika_rnnt_fused_forward(const float *logits, const int *labels, const int *frames_lengths,
                            const int *labels_lengths, int B, int T, int U1, int V, int blank, float *costs,
                            float *lse, void *workspace, void *stream);
int pika_rnnt_fused_backward(const float *logits, const float *lse, const int *labels,
                             const int *frames_lengths, const int *labels_lengths, int B, int T, int U1, int V,
                             int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                             int out_dtype, long long ld_out, void *stream);

/* pika_rnnt_fused_backward with FastEmit (as pika_rnnt_loss_backward_fe): the label entry of g is scaled before
 * the softmax backward, out = g~ - p * sum g~. */
int pika_rnnt_fused_backward_fe(const float *logits, const float *lse, const int *labels,
                                const int *frames_lengths, const int *labels_lengths, int B, int T, int U1, int V,
                                int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                                int out_dtype, long long ld_out, float fastemit_lambda, void *stream);

/* Packed (compact) layout: a ragged batch without padding.
 *   log_probs / logits f32 (N, V), N = sum_n T_n (U_n + 1); row off_n + t (U_n + 1) + u holds cell (n, t, u)
 *   labels         i32 (sum_n U_n,)  the utterances' labels concatenated
 *   frames_lengths i32 (B,)          T_n >= 1
 *   labels_lengths i32 (B,)          U_n >= 0, U_n + 1 <= U1_max
 *   row_offsets    i32 (B,)          off_n: exclusive prefix sum of T_n (U_n + 1)
 *   label_offsets  i32 (B,)          exclusive prefix sum of U_n (may be NULL, with labels, when U1_max == 1)
 *   T_max, U1_max  the largest T_n and U_n + 1 (host values; the lattice planes and the workspace are those of a
 *                  padded (B, T_max, U1_max) batch: pika_rnnt_workspace_bytes(B, T_max, U1_max), whose metadata
 *                  region of B*T_max*U1_max rows covers N)
 *   costs          f32 (B,);  grads / grad_logits (N, V) (pitch ld_out for the fused call), every element written.
 * The lengths, offsets and N must agree: the calls read only what they describe, and cannot check that on the host
 * (stream-ordered, no synchronisation).  N <= 0, N > B*T_max*U1_max: PIKA_EINVAL; N > 0x7fffffff: PIKA_ETOOBIG.
 * The fused pair takes RAW logits (V % 4 == 0, V <= 8192, as pika_rnnt_fused_forward) and lse (N,). */
int pika_rnnt_packed_forward(const float *log_probs, const int *labels, const int *frames_lengths,
                             const int *labels_lengths, const int *row_offsets, const int *label_offsets, int B,
                             int T_max, int U1_max, long long N, int V, int blank, float *costs, void *workspace,
                             void *stream);
/* grads == NULL: row metadata only, as pika_rnnt_loss_backward. */
int pika_rnnt_packed_backward(const int *labels, const int *frames_lengths, const int *labels_lengths,
                              const int *row_offsets, const int *label_offsets, int B, int T_max, int U1_max,
                              long long N, int V, int blank, const float *grad_costs, const void *workspace,
                              float *grads, float fastemit_lambda, void *stream);
int pika_rnnt_packed_fused_forward(const float *logits, const int *labels, const int *frames_lengths,
                                   const int *labels_lengths, const int *row_offsets, const int *label_offsets, int B,
                                   int T_max, int U1_max, long long N, int V, int blank, float *costs, float *lse,
                                   void *workspace, void *stream);
int pika_rnnt_packed_fused_backward(const float *logits, const float *lse, const int *labels,
                                    const int *frames_lengths, const int *labels_lengths, const int *row_offsets,
                                    const int *label_offsets, int B, int T_max, int U1_max, long long N, int V,
                                    int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                                    int out_dtype, long long ld_out, float fastemit_lambda, void *stream);

/* Forced alignment: the single best path of every utterance's lattice (Viterbi, max-plus),
 *   delta(0,0) = 0,  delta(t,u) = max(delta(t-1,u) + lpb(t-1,u), delta(t,u-1) + lpe(t,u-1)),
 *   scores[n] = delta(T_n-1, U_n) + lpb(T_n-1, U_n)            (<= -costs[n])
 * with lpb / lpe the blank and label log-probs of a cell.  Reads ONLY those two planes of a `workspace` left by any
 * forward call above -- pika_rnnt_loss_forward, pika_rnnt_fused_forward (and its _partials / _gathered forms),
 * pika_rnnt_packed_forward, pika_rnnt_packed_fused_forward -- with the same (B, T, U1) (packed: T_max, U1_max) and
 * lengths, and leaves it untouched: forward -> align -> backward gives the gradients of forward -> backward.
 *   scores        f32 (B,)
 *   emit_frames   i32; label_offsets == NULL: (B, U1-1), entry [n][u], u < U_n, the frame t at which the best path
 *                 emits label u (takes the emission edge out of cell (t, u)), entries u >= U_n set to -1;
 *                 label_offsets (the packed layout's exclusive prefix sum of U_n) given: (sum_n U_n,), utterance
 *                 n's U_n frames at label_offsets[n], nothing else written.  May be NULL when U1 == 1.
 *                 Non-decreasing in u, in [0, T_n-1].  Ties go to the blank predecessor (t-1, u) in the back-trace
 *                 from (T_n-1, U_n), i.e. to the earliest emission.  A label outside [0, V) (an infeasible
 *                 transcript, -1e30 in the plane) still yields a valid monotone path; its score is <= -1e30.
 *   scratch       pika_rnnt_align_scratch_bytes(B, T, U1) bytes (one back-pointer bit per cell of the skewed
 *                 lattice); 0 is returned for dimensions the call refuses.
 * One launch, values accumulated in fp32.  PIKA_EINVAL / PIKA_ETOOBIG as above, before any launch. */
size_t pika_rnnt_align_scratch_bytes(int B, int T, int U1);
int pika_rnnt_align(const void *workspace, const int *frames_lengths, const int *labels_lengths,
                    const int *label_offsets, int B, int T, int U1, float *scores, int *emit_frames,
                    void *scratch, void *stream);

/* Pruned RNN-T: the loss on a banded lattice (k2 / icefall rnnt_loss_pruned; Kuang et al. 2022, arXiv:2206.13236).
 * Every frame keeps S consecutive label positions, so the joint output, the vocabulary product and the dense
 * gradient are (B, T, S, V) instead of (B, T, U1, V).
 *   ranges         i32 (B, T)      s_t = ranges[n][t], the first label position of frame t's band; every entry is
 *                                  clamped on the device to [0, max(0, U_n + 1 - S)]
 *   log_probs / logits f32 (B, T, S, V); row j of frame t is the distribution of lattice cell (t, s_t + j)
 *   labels         i32 (B, U1-1), lengths and costs as above
 * A cell (t, u) of the (T_n, U_n + 1) lattice is live iff s_t <= u < s_t + S; both outgoing log-probabilities of any
 * other cell are log zero, so the cost is -log of the sum over the paths from (0, 0) to the final blank out of
 * (T_n-1, U_n) that visit live cells only: the full loss on a (B, T, U1, V) tensor holding the band's rows at their
 * cells and -1e30 everywhere else.  The gradient is dense (B, T, S, V), every element written; rows with t >= T_n or
 * s_t + j > U_n are zero.  FastEmit as in pika_rnnt_loss_backward_fe.
 * A band connects the lattice's corners when, for t < T_n, s_0 = 0, s_{T_n-1} = max(0, U_n + 1 - S) and
 * 0 <= s_{t+1} - s_t <= S - 1 (pika_prnnt_prune_ranges returns such ranges).  On any other ranges the calls still read
 * and write inside their buffers and the other utterances of the batch are unaffected; the cost of that utterance is
 * unspecified.
 * `workspace` is that of the padded (B, T, U1) batch, pika_rnnt_workspace_bytes(B, T, U1); pika_rnnt_align works on
 * the planes these forwards leave (with the same B, T, U1 and lengths): the best path through live cells.
 * The fused pair takes RAW logits (V % 4 == 0, V <= 8192) and lse (B*T*S), out_dtype / ld_out as
 * pika_rnnt_fused_backward.  S < 1 or S > U1: PIKA_EINVAL; U1 > 1024, B*T*S > 0x7fffffff: PIKA_ETOOBIG.
 * (The family is pika_prnnt_*, not pika_rnnt_*: tests/test_rnnt_abi_rejections.py pins the set of pika_rnnt_* entry
 * points to the table recorded for them.) */
int pika_prnnt_forward(const float *log_probs, const int *frames_lengths, const int *labels_lengths, const int *labels,
                       const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs, void *workspace,
                       void *stream);
/* grads == NULL: row metadata (of the B*T*S band rows) only, as pika_rnnt_loss_backward. */
int pika_prnnt_backward(const int *frames_lengths, const int *labels_lengths, const int *labels, const int *ranges, int B,
                        int T, int U1, int S, int V, int blank, const float *grad_costs, const void *workspace,
                        float *grads, float fastemit_lambda, void *stream);
int pika_prnnt_fused_forward(const float *logits, const int *frames_lengths, const int *labels_lengths, const int *labels,
                             const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs, float *lse,
                             void *workspace, void *stream);
int pika_prnnt_fused_backward(const float *logits, const float *lse, const int *frames_lengths, const int *labels_lengths,
                              const int *labels, const int *ranges, int B, int T, int U1, int S, int V, int blank,
                              const float *grad_costs, const void *workspace, void *grad_logits, int out_dtype,
                              long long ld_out, float fastemit_lambda, void *stream);

/* The loss of a lattice given directly by its two planes (the "simple" loss of a joiner that is am + lm):
 *   blank_lp, label_lp  f32 (B, T, U1): log-probability of the blank edge (t, u) -> (t+1, u) and of the label edge
 *                       (t, u) -> (t, u+1); label_lp[.., u] is not read for u >= U_n; they need not be normalised
 *   blank_occ, label_occ f32 (B, T, U1), written: the occupation probabilities exp(alpha + lp + beta' - ll) of the two
 *                       edges of every cell (zero outside the sub-lattice); d cost / d lp = -occ.
 * The planes are skewed into `workspace` (pika_rnnt_workspace_bytes(B, T, U1)), so pika_rnnt_align works on it. */
int pika_prnnt_planes_forward(const float *blank_lp, const float *label_lp, const int *frames_lengths,
                              const int *labels_lengths, int B, int T, int U1, float *costs, float *blank_occ,
                              float *label_occ, void *workspace, void *stream);

/* Band search.  occ(t, u) = blank_occ + label_occ, s_max = max(0, U_n + 1 - S); for every utterance
 *   1. raw(t) = argmax over 0 <= s <= s_max of sum_{u = s}^{min(s + S - 1, U_n)} occ(t, u), ties to the smallest s,
 *      for t < T_n; then raw(T_n - 1) = s_max;
 *   2. m(t) = min_{t' >= t} raw(t');
 *   3. f(0) = 0, f(t) = min(m(t), f(t-1) + S - 1);
 *   4. ranges[n][t] = max(f(t), s_max - (T_n - 1 - t)(S - 1)); s_max for t >= T_n.
 * The result connects the corners (above) whenever (T_n - 1)(S - 1) >= s_max; otherwise no band of that width does,
 * and ranges[n][0] > 0 says so.  One workgroup per utterance, any T.  S < 1 or S > U1: PIKA_EINVAL; U1 > 1024:
 * PIKA_ETOOBIG. */
int pika_prnnt_prune_ranges(const float *blank_occ, const float *label_occ, const int *frames_lengths,
                            const int *labels_lengths, int B, int T, int U1, int S, int *ranges, void *stream);

/* Smoothed simple planes: the planes pika_prnnt_planes_forward takes, of the joiner am + lm interpolated with an lm-only
 * and an am-times-batch-unigram distribution (k2's get_rnnt_logprobs_smoothed, regular topology).
 * These two calls do everything that touches (B, T, V); the caller prepares what is (B, U1, V)- or (V,)-sized.
 * With c = 1 - lm_only_scale - am_only_scale, y_bu = labels[b][u] clamped into [0, V) (y_bU = blank) and
 * NC = U1 + (am_only_scale != 0):
 *   am        f32 (B, T, V) encoder logits
 *   elm       f32 (B, NC, V): rows u < U1 are exp(lm[b][u] - lmax[b][u]), lmax the row maximum; row U1 (when present)
 *             is the batch unigram q
 *   side      f32 (B, U1, 5): {lm[b][u][blank] - lmax, lm[b][u][y_bu] - lmax, Zl[b][u] - lmax, log q[blank], log q[y_bu]}
 *   labels    i32 (B, U1 - 1); may be NULL when U1 == 1
 * forward writes
 *   amax      f32 (B, T)      row maxima of am
 *   gathered  f32 (B, T, U1)  am[b][t][y_bu]
 *   sums      f32 (B, T, NC)  sum_v exp(am[b][t][v] - amax[b][t]) * elm[b][j][v]
 *   blank_lp, label_lp f32 (B, T, U1): lp(b, t, u, blank) and lp(b, t, u, y_bu), label_lp[..][U1 - 1] = -1e30, where
 *             lp(k) = c (am_k + lm_k - Z) + lm_only_scale (lm_k - Zl) + am_only_scale (am_k + log q_k - Za).
 * backward takes amax and elm again and
 *   w         f32 (B, T, NC): c (gB + gL)[b][t][u] / sums[b][t][u]; column U1: am_only_scale * sum_u (gB + gL) / sums
 *   sg        f32 (B, T, U1): (c + am_only_scale) gL[b][t][u]; column U1 - 1: (c + am_only_scale) sum_u gB[b][t][u]
 * (gB, gL the gradients of the planes, gL[..][U1 - 1] = 0) and writes, every element,
 *   d_am      f32 (B, T, V) = sum_u sg[b][t][u] [v == y_bu]  -  exp(am - amax) * sum_j w[b][t][j] elm[b][j][v]
 *   m         f32 (B, NC, V) = sum_t w[b][t][j] exp(am[b][t][v] - amax[b][t]),
 * from which the caller forms d lm = -elm * m + ... and d q = -sum_b m[b][U1] + ...  No atomics: every sum runs in a
 * fixed order.  Any T, any V >= 1.  Null pointers, non-positive sizes, blank outside [0, V), scales that are negative,
 * not finite or sum to >= 1: PIKA_EINVAL; U1 > 1024, B > 65535: PIKA_ETOOBIG; all before any launch. */
int pika_prnnt_smoothed_fwd(const float *am, const float *elm, const float *side, const int *labels, int B, int T, int U1,
                            int V, int blank, float lm_only_scale, float am_only_scale, float *amax, float *gathered,
                            float *sums, float *blank_lp, float *label_lp, void *stream);
int pika_prnnt_smoothed_bwd(const float *am, const float *amax, const float *elm, const float *w, const float *sg,
                            const int *labels, int B, int T, int U1, int V, int blank, float lm_only_scale,
                            float am_only_scale, float *d_am, float *m, void *stream);

/* Modified topology (k2's rnnt_loss / rnnt_loss_pruned with modified=True): every frame emits exactly one symbol, a
 * blank or one label, so the label edge runs (t, u) -> (t+1, u+1) instead of (t, u) -> (t, u+1).  Per utterance, with
 * blank_lp(t, u) and label_lp(t, u) for 0 <= t < T_n, 0 <= u <= U_n (label_lp(t, U_n) is dead):
 *   alpha(0, 0) = 0, every other alpha(0, u) log zero;
 *   alpha(t+1, u) = logaddexp(alpha(t, u) + blank_lp(t, u), alpha(t, u-1) + label_lp(t, u-1)),  0 <= t < T_n;
 *   ll = alpha(T_n, U_n): row T_n is terminal and both edge kinds out of frame T_n - 1 reach it, so a label may be
 *   emitted on the last frame; cost = -ll; beta is the mirror image with beta(T_n, U_n) = 0;
 *   occ_blank(t, u) = exp(alpha(t, u) + blank_lp(t, u) + beta(t+1, u) - ll),
 *   occ_label(t, u) = exp(alpha(t, u) + label_lp(t, u) + beta(t+1, u+1) - ll),   d cost / d lp = -occ.
 * Feasible iff U_n <= T_n.  An infeasible utterance, or a band that holds no path, costs +inf and has an all-zero
 * gradient and all-zero occupancies; the other utterances of the batch are not disturbed.  Lengths are clamped on the
 * device as everywhere above.  FastEmit as in pika_rnnt_loss_backward_fe.  No float atomics: two runs give the same bits.
 *
 * The calls mirror the pika_prnnt_* ones above, argument for argument, over a workspace of
 * pika_prnnt_mod_workspace_bytes(B, T, U1) bytes (the regular members over T + 1 un-skewed plane rows; NOT a workspace
 * pika_rnnt_align or pika_rnnt_export_lattice can read; pika_mrnnt_align, below, aligns on it).  forward / backward / fused_forward / fused_backward take the
 * banded layout (B, T, S, V) with `ranges`, or -- ranges == NULL, which requires S == U1 -- the padded (B, T, U1, V)
 * one; with S == U1 and all-zero ranges the banded calls give the padded calls' bits.  The row metadata they leave is
 * that of the regular calls (16 bytes per row of the B*T*S), and the dense and d(logits) writers are the regular ones.
 * Error codes as for the pika_prnnt_* calls. */
size_t pika_prnnt_mod_workspace_bytes(int B, int T, int U1);
int pika_prnnt_mod_forward(const float *log_probs, const int *frames_lengths, const int *labels_lengths, const int *labels,
                           const int *ranges, int B, int T, int U1, int S, int V, int blank, float *costs, void *workspace,
                           void *stream);
int pika_prnnt_mod_backward(const int *frames_lengths, const int *labels_lengths, const int *labels, const int *ranges, int B,
                            int T, int U1, int S, int V, int blank, const float *grad_costs, const void *workspace,
                            float *grads, float fastemit_lambda, void *stream);
int pika_prnnt_mod_fused_forward(const float *logits, const int *frames_lengths, const int *labels_lengths,
                                 const int *labels, const int *ranges, int B, int T, int U1, int S, int V, int blank,
                                 float *costs, float *lse, void *workspace, void *stream);
int pika_prnnt_mod_fused_backward(const float *logits, const float *lse, const int *frames_lengths,
                                  const int *labels_lengths, const int *labels, const int *ranges, int B, int T, int U1, int S,
                                  int V, int blank, const float *grad_costs, const void *workspace, void *grad_logits,
                                  int out_dtype, long long ld_out, float fastemit_lambda, void *stream);
/* pika_prnnt_planes_forward in the modified topology: blank_lp is the edge (t, u) -> (t+1, u), label_lp the edge
 * (t, u) -> (t+1, u+1); the occupancies are those defined above. */
int pika_prnnt_mod_planes_forward(const float *blank_lp, const float *label_lp, const int *frames_lengths,
                                  const int *labels_lengths, int B, int T, int U1, float *costs, float *blank_occ,
                                  float *label_occ, void *workspace, void *stream);
/* Band search with step bound 1: steps 1 and 2 of pika_prnnt_prune_ranges, then
 *   3. f(0) = 0, f(t) = min(m(t), f(t-1) + 1);
 *   4. ranges[n][t] = max(f(t), s_max - (T_n - 1 - t)); s_max for t >= T_n.
 * The result has s_0 = 0, 0 <= s_{t+1} - s_t <= 1 and s_{T_n-1} = s_max whenever T_n - 1 >= s_max (otherwise s_0 > 0
 * says so), and such a band holds a path whenever U_n <= T_n: u_t = min(t, s_t + S - 1) stays inside it, moves by 0 or
 * 1 per frame and reaches U_n at row T_n.  (A band of pika_prnnt_prune_ranges may move S - 1 columns per frame, which
 * no path of this topology can follow.) */
int pika_prnnt_mod_prune_ranges(const float *blank_occ, const float *label_occ, const int *frames_lengths,
                                const int *labels_lengths, int B, int T, int U1, int S, int *ranges, void *stream);

/* Forced alignment in the modified topology: the single best path (Viterbi, the max-plus image of the alpha line above),
 *   delta(0, 0) = 0, every other delta(0, u) log zero;
 *   delta(t+1, u) = max(delta(t, u) + blank_lp(t, u), delta(t, u-1) + label_lp(t, u-1)),  0 <= t < T_n;
 *   scores[n] = delta(T_n, U_n)                                  (<= -costs[n]).
 * Reads ONLY the lpb / lpe planes of a `workspace` (pika_prnnt_mod_workspace_bytes(B, T, U1)) that any of
 * pika_prnnt_mod_forward, pika_prnnt_mod_fused_forward (padded or banded) or pika_prnnt_mod_planes_forward has filled
 * with the same (B, T, U1) and lengths, and leaves it untouched: forward -> align -> backward gives the gradients of
 * forward -> backward.  On a band the path runs through live cells only.
 *   scores        f32 (B,)
 *   emit_frames   i32 (B, U1-1): entry [n][u], u < U_n, the frame t at which the best path takes the label edge out of
 *                 cell (t, u); strictly increasing in u, in [0, T_n-1]; entries u >= U_n are -1.  May be NULL when
 *                 U1 == 1.  Ties go to the blank predecessor (t, u) in the back-trace from (T_n, U_n), i.e. to the
 *                 earliest emission (pika_rnnt_align's rule).
 *   scratch       pika_mrnnt_align_scratch_bytes(B, T, U1) bytes (one back-pointer bit per cell: B (T+1) NW 64-bit
 *                 words, NW the waves that cover U1 columns); 0 is returned for dimensions the call refuses.
 * An utterance for which the modified loss is +inf -- U_n > T_n, a band that holds no path, a label outside [0, V) --
 * gets scores[n] = -inf and all its emit_frames -1; the other utterances of the batch are not disturbed.
 * One launch, T_n dependent steps, values accumulated in fp32.  PIKA_EINVAL / PIKA_ETOOBIG as for pika_rnnt_align,
 * before any launch.  (The prefix is its own: the pika_rnnt_* and pika_prnnt_* sets are closed.) */
size_t pika_mrnnt_align_scratch_bytes(int B, int T, int U1);
int pika_mrnnt_align(const void *workspace, const int *frames_lengths, const int *labels_lengths, int B, int T, int U1,
                     float *scores, int *emit_frames, void *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKA_RNNT_H */
