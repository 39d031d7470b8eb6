/*
 * include/pika_frame_skip.h -- C ABI of CTC-guided frame skipping for the transducer (libpika_amd.so): a CTC head marks
 * the frames whose blank posterior is at or above a threshold, and those frames are removed from the encoder output
 * before the joint network sees them (Wang et al., arXiv:2210.16481; Yang et al., arXiv:2305.11558).
 *
 * Conventions are those of pika_ctc.h: plain pointers + sizes, every pointer DEVICE memory owned by the caller, work
 * enqueued on `stream` (a hipStream_t as void*, NULL = default stream) and stream-ordered with no host synchronisation
 * and no allocation; return 0 on success, a negative PIKA_E* code for bad arguments (before any launch), a positive
 * hipError_t if a launch failed.  Every output cell is written by every call: the shapes do not depend on the data.
 *
 * Three steps: rows (the only pass over the (B,T,C) class tensor, once) -> plan (integers) -> apply (bytes).
 *
 * Definition, per utterance b with L = clamp(lengths[b], 0, T):
 *   blank_lp[b,t]  t < L: the blank's log-prob of frame t -- the value itself (logits == 0), or logit[blank] - lse(row)
 *                  in fp32 from one online max / sum pass and a fixed reduction tree (logits != 0: the log-probs never
 *                  exist).  t >= L: 0, and the row is never read.
 *   frame t < L is DROPPED iff blank_lp[b,t] >= log_thr (a NaN compares false: a NaN frame is kept).
 *   m = 0 if L == 0, else clamp(min_frames ? min_frames[b] : 1, 1, L).  If fewer than m frames are kept, dropped frames
 *   are put back in the total order (blank_lp ascending, t ascending; -0.0 == +0.0) until m are kept.  Kept frames keep
 *   their time order.  The result is a function of the input alone (exact integer counting: no dependence on the
 *   workgroup size or on the order in which threads run).
 *
 * Limits: 1 <= T <= PIKA_FSKIP_MAX_T, B >= 1, B * T <= 2^31 - 1, C >= 1, blank in [0,C), 1 <= row_bytes <= 2^31 - 1
 * (PIKA_ETOOBIG beyond the upper ones, PIKA_EINVAL otherwise).
 */
#ifndef PIKA_FRAME_SKIP_H
#define PIKA_FRAME_SKIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

#define PIKA_FSKIP_MAX_T 8192

/* Row pass: blank_lp f32 (B,T) as defined above.
 *   x        f32, row (b,t) at x + b * stride_b + t * stride_t (strides in ELEMENTS, any sign of layout: (B,T,C) and
 *            (T,B,C) are the same entry), C contiguous classes.  logits != 0: one workgroup per row, 16-byte loads where
 *            C % 4 == 0 and the row is 16-byte aligned, scalar loads otherwise; the value does not depend on which.
 *            logits == 0: a strided gather of the blank's column.
 *   lengths  i32 (B,) */
int pika_fskip_rows(const float *x, long long stride_b, long long stride_t, const int *lengths, int B, int T, int C,
                    int blank, int logits, float *blank_lp, void *stream);

/* Plan: one workgroup per utterance.
 *   blank_lp     f32 (B,T) from the row pass (cells t >= L are not read)
 *   min_frames   i32 (B,) or NULL
 *   log_thr      float32(log(threshold)); +inf drops nothing, -inf drops every non-NaN frame
 *   kept_lengths i32 (B,)    frames kept, in [m, L]
 *   frame_index  i32 (B,T)   the original frame of output row j; -1 for j >= kept_lengths[b]
 *   position     i32 (B,T)   the output row of original frame t; -1 if it was dropped or t >= L */
int pika_fskip_plan(const float *blank_lp, const int *lengths, const int *min_frames, int B, int T, float log_thr,
                    int *kept_lengths, int *frame_index, int *position, void *stream);

/* Apply: out[b,j,:] = x[b, index[b,j], :] where 0 <= index[b,j] < T, zeros elsewhere; every row of out is written exactly
 * once, no atomics, so two runs agree bit for bit.  With index = frame_index it is the forward; with index = position and
 * x = d(out) it is the backward, dx[b,t,:] = dout[b, position[b,t], :] (the map is injective).
 *   x           rows of row_bytes bytes, row (b,t) at x + b * stride_b + t * stride_t (strides in BYTES, multiples of
 *               elem_bytes), copied bit for bit whatever the element type
 *   elem_bytes  2 or 4 (PIKA_EINVAL otherwise, and where it does not divide row_bytes or a stride, or a base is not
 *               aligned to it)
 *   out         (B,T,row_bytes) contiguous
 * 16-byte accesses where row_bytes, both strides and both bases are multiples of 16, elem_bytes accesses otherwise; the
 * bytes do not depend on which. */
int pika_fskip_apply(const void *x, long long stride_b, long long stride_t, const int *index, int B, int T,
                     long long row_bytes, int elem_bytes, void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PIKA_FRAME_SKIP_H */
