/*
 * include/pika_joint.h -- C ABI of the joint-network kernels around the fc2 GEMM.
 *
 * Reference: /root/reference/trainer/model/transducer.py:98-111
 *   out = fc2(tanh(fc1(z)) * sigmoid(fc_gate(z))),  z = cat(enc[b,t], pred[b,u]);  log_softmax
 * and its decode-time twin /root/reference/decoder/transducer_decoder.py:173-177.
 * With fc1/fc_gate split into encoder/prediction halves:
 *   h[b,t,u,:] = tanh(e1[b,t,:] + p1[b,u,:]) * sigmoid(eg[b,t,:] + pg[b,u,:])
 * Conventions as in pika_rnnt.h.  Every argument check below is made on the host and returns BEFORE any launch: a call
 * that returns PIKA_EINVAL / PIKA_ETOOBIG has touched no buffer.
 */
#ifndef PIKA_JOINT_H
#define PIKA_JOINT_H

#ifdef __cplusplus
extern "C" {
#endif

/* h (B,T,U,H) = tanh(e1+p1)*sigmoid(eg+pg); e* (B,T,H), p* (B,U,H) f32 contiguous; H % 4 == 0.
 * out_dtype PIKA_F32 | PIKA_BF16 (pika_gemm.h); the bf16 output is the fp32 result rounded to nearest even.
 * Non-finite inputs behave as in the formula: a NaN in e1+p1 or eg+pg (a NaN operand, or +inf meeting -inf) gives a NaN h
 * at exactly the (b,t,u,c) that read it; a lone +-inf gives the limit (tanh -> +-1, sigmoid -> 1 or 0).  Finite
 * pre-activations are clamped to z1 in [-15, 15] (tanh is +-1 in fp32 beyond) and zg >= -50 (sigmoid(-50) = 2e-22).
 * PIKA_EINVAL: a null pointer, B, T, U or H <= 0, H % 4 != 0, an unknown out_dtype.  PIKA_ETOOBIG: B > 65535. */
int pika_joint_gate_fwd(const float *e1, const float *p1, const float *eg, const float *pg,
                        void *h, int out_dtype, int B, int T, int U, int H, void *stream);

/* Backward of the gate given dh (B,T,U,H), dh_dtype PIKA_F32 | PIKA_BF16: de1/deg (B,T,H) = sum over u, dp1/dpg (B,U,H) =
 * sum over t of  dz1 = dh*sig(zg)*(1-tanh(z1)^2),  dzg = dh*tanh(z1)*sig(zg)*(1-sig(zg)).
 * tanh/sigmoid are recomputed from e*,p* (nothing of size B*T*U*H is kept from the forward).  A bf16 dh is widened
 * exactly: the result equals that of the same values passed as fp32, bit for bit.  A lattice position whose e1+p1 or eg+pg
 * is NaN makes every output element NaN whose sum includes it (all four outputs), and no other.
 * PIKA_EINVAL: a null pointer, B, T, U or H <= 0, H % 4 != 0, an unknown dh_dtype.  PIKA_ETOOBIG: B > 65535. */
int pika_joint_gate_bwd(const void *dh, int dh_dtype, const float *e1, const float *p1, const float *eg,
                        const float *pg, float *de1, float *dp1, float *deg, float *dpg,
                        int B, int T, int U, int H, void *stream);

/* The gate on a pruned (banded) lattice (pika_rnnt.h "Pruned RNN-T"): frame t keeps S of the U prediction rows, those
 * from s_t = clamp(ranges[b,t], 0, U - S); ranges (B,T) i32.  (U counts prediction rows: the loss's U + 1.)
 *   h[b,t,j,:] = gate(e1[b,t,:] + p1[b,s_t+j,:], eg[b,t,:] + pg[b,s_t+j,:]),  j = 0 .. S-1,  h (B,T,S,H)
 * which is pika_joint_gate_fwd on the rows rnnt_prune_lm gathers, without gathering them: clamps, NaN rule, bf16 rounding
 * and refusals are those of pika_joint_gate_fwd, and S == U with all-zero ranges gives its output bit for bit.  Lengths
 * are no argument: every (b,t,j) is computed.  Also PIKA_EINVAL: null ranges, S <= 0, S > U. */
int pika_joint_gate_banded_fwd(const float *e1, const float *p1, const float *eg, const float *pg,
                               const int *ranges, void *h, int out_dtype, int B, int T, int U, int S, int H,
                               void *stream);

/* Backward of the banded gate given dh (B,T,S,H), dh_dtype PIKA_F32 | PIKA_BF16, dz1 / dzg as for pika_joint_gate_bwd:
 *   de1/deg[b,t,:] = sum over j = 0 .. S-1 (in that order) of dz[b,t,j,:]
 *   dp1/dpg[b,u,:] = sum over the frames t with s_t <= u < s_t + S (in increasing t) of dz[b,t,u-s_t,:]
 * One accumulator per output element and no atomics: two runs give the same bits.  Every element of the four outputs is
 * written; a row u that no frame's band covers gets +0.  The ranges need not be monotone (a valid band's covering frames
 * are an interval; nothing relies on it).  Rows the loss treats as dead are expected to arrive with dh = 0.  S == U with
 * all-zero ranges gives pika_joint_gate_bwd's four outputs bit for bit.  Refusals as for pika_joint_gate_banded_fwd. */
int pika_joint_gate_banded_bwd(const void *dh, int dh_dtype, const float *e1, const float *p1, const float *eg,
                               const float *pg, const int *ranges, float *de1, float *dp1, float *deg, float *dpg,
                               int B, int T, int U, int S, int H, void *stream);

/* In place on x (rows, cols) f32 with pitch ld >= cols: x = log_softmax(scale * x) per row.  Columns [cols, ld) and rows
 * beyond `rows` are neither read into a result nor written.  Any cols, ld and alignment of x are accepted (cols % 4 == 0,
 * ld % 4 == 0, x 16-byte aligned and cols <= 8192 take the wave-per-row kernels, everything else the block kernel).
 * -inf entries stay -inf; a row that is all -inf or holds a NaN comes out all NaN (as torch.log_softmax), other rows
 * are unaffected.  PIKA_EINVAL: null x, rows <= 0, cols <= 0, ld < cols.  PIKA_ETOOBIG: rows > 2^31 - 1. */
int pika_log_softmax_rows(float *x, long long rows, int cols, long long ld, float scale,
                          void *stream);

/* In place on g: g = scale * (g - exp(lp) * rowsum(g))  (log-softmax backward; lp = the
 * forward output, same shape/pitch).  lp is only read; padding, routes and refusals as for pika_log_softmax_rows (the
 * wave kernels need lp AND g 16-byte aligned). */
int pika_log_softmax_bwd_rows(const float *lp, float *g, long long rows, int cols, long long ld,
                              float scale, void *stream);

/* Same, written as bf16 into `out` (rows, ld_out) instead of in place; columns [cols, ld_out) are
 * zero-filled (+0) so `out` can feed pika_gemm_bf16_nt with K = ld_out (a multiple of 64); lp and g are only read.
 * [0, cols) equals the in-place fp32 result rounded to bf16 (nearest even), bit for bit.  Wave-per-row kernels only:
 * PIKA_EINVAL for a null pointer, rows <= 0, cols <= 0, ld < cols, ld_out < cols, cols % 4 != 0, ld % 4 != 0,
 * ld_out % 4 != 0, ld_out > 8192, lp or g not 16-byte aligned, out not 8-byte aligned.  PIKA_ETOOBIG: rows > 2^31 - 1. */
int pika_log_softmax_bwd_rows_bf16(const float *lp, const float *g, void *out, long long rows,
                                   int cols, long long ld, long long ld_out, float scale,
                                   void *stream);

/* MBR risk gradient (reference: trainer/train_transducer_mbr_bmuf_otfaug.py:225-235, where a
 * dense (rows, V) tensor holding ONE non-zero per row is pushed through log_softmax backward).
 * In place on lp (rows, V) = log_softmax(scale * logits):
 *   lp[r, v] <- scale * val[r] * ((v == sym[r]) - exp(lp[r, v]))      (rows with val == 0 -> zeros)
 * i.e. d/dlogits of sum_r val[r] * lp[r, sym[r]].  sym i32, val f32.  A row with val == 0 becomes exact +0 whatever lp
 * holds (-inf, NaN); lp = -inf away from sym gives 0.  Columns [cols, ld) are untouched.
 * PIKA_EINVAL: a null pointer, rows <= 0, cols <= 0, ld < cols.  PIKA_ETOOBIG: rows > 2^31 - 1. */
int pika_mbr_risk_grad_rows(float *lp, const int *sym, const float *val, long long rows, int cols,
                            long long ld, float scale, void *stream);

/* Levenshtein distances of the N-best against their references (reference: editdistance.eval(hyp, ref) once per
 * hypothesis, trainer/train_transducer_mbr_bmuf_otfaug.py:186-190 -- editdistance==0.5.2, requirements.txt:1).
 * HOST function (no device work, no stream): pair i compares the int32 sequences seqs[a_off[i] .. a_off[i] + a_len[i])
 * and seqs[b_off[i] .. b_off[i] + b_len[i]); out[i] = minimum number of insertions, deletions and substitutions.
 * Empty sequences are allowed (distance = the other length); n_pairs == 0 writes nothing.  PIKA_EINVAL, with nothing
 * written: a null pointer, n_pairs < 0, a negative length in any pair. */
int pika_edit_distances(const int *seqs, const long long *a_off, const int *a_len, const long long *b_off,
                        const int *b_len, int n_pairs, int *out);

#ifdef __cplusplus
}
#endif
#endif /* PIKA_JOINT_H */
