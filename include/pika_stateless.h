/*
 * include/pika_stateless.h -- C ABI of the STATELESS prediction network (libpika_amd.so): an embedding followed by a
 * grouped causal Conv1d over the last `ctx` labels and a ReLU (icefall's `Decoder`; ctx = 2 in its recipes).  A
 * hypothesis' row is a function of its last ctx tokens and of nothing else, which is why hypotheses that spell the same
 * sequence may be merged by the searches of pika_msearch*.h without any condition on the caller's network.
 *
 * Conventions are those of pika_msearch.h: plain pointers + sizes, every pointer DEVICE memory owned by the caller, no
 * allocation, work enqueued on `stream` (a hipStream_t as void*, NULL = default stream) and stream-ordered with no host
 * synchronisation; return 0 on success, PIKA_EINVAL / PIKA_ETOOBIG for bad arguments (before any launch), a positive
 * hipError_t if a launch failed.  Every call can be captured in a hipGraph.
 *
 * Definition.  E f32 (V, D), w f32 (D, cpg, ctx) -- the weight of a Conv1d(D, D, kernel_size = ctx, groups = D / cpg,
 * bias = False) --, both contiguous; a label row y[b, 0:U] that already starts with SOS:
 *   e[b,p,:]   = E[y[b,p]]  if p >= 0 and y[b,p] >= 0, else 0     (a negative token is padding: zero vector, no gradient)
 *   g(d)       = d / cpg                                          (channel d reads input channels g cpg .. g cpg + cpg-1)
 *   z[b,u,d]   = sum_{j=0}^{ctx-1} sum_{c=0}^{cpg-1} w[d,c,j] * e[b, u-(ctx-1)+j, g(d) cpg + c]
 *   out[b,u,d] = max(z, 0)
 * The sum runs j ascending outside and c ascending inside, fp32 from 0.0f, every product fused into the running sum
 * (fmaf); a padded position contributes nothing.  The forward and the search step call ONE device function for it, so
 * they agree bit for bit, and the result does not depend on the width of the loads: E rows are read with 16-byte loads
 * where cpg % 4 == 0 (hence D % 4 == 0) and E is 16-byte aligned, with scalar loads otherwise.  A token >= V is clamped
 * to V - 1 before it indexes and is otherwise outside the contract.
 *
 * Backward, with go = dout * (out > 0):
 *   d_w[d,c,j] = sum_{b,u} go[b,u,d] * e[b, u-(ctx-1)+j, g(d) cpg + c]
 *   d_E[v,i]   = sum_{(b,p): y[b,p] = v} sum_j sum_{d: g(d) = i/cpg} w[d, i - g(d) cpg, j] * go[b, p+(ctx-1)-j, d]
 *                                                                                (terms with p+(ctx-1)-j >= U absent)
 * Both are written in full, not accumulated; a token that does not occur gets an exactly zero row.  No floating-point
 * atomics: d_E sums each token's positions in the order of `order` (below), positions outside, j, then d inside; d_w is
 * summed over chunks of 32 or more consecutive (b,u) into the workspace and the chunks are added in ascending order.
 * Two runs on the same inputs give the same bits.
 *
 * The search context: a caller-owned record ctx_tok i32 (B, K, ctx), slot (b, j) holding the last ctx tokens of the
 * slot's hypothesis, [-1, ..., -1, blank] for the empty one.  pika_stateless_step takes what an `advance` returned.
 *
 * Limits: 1 <= ctx <= 8, 1 <= cpg <= 16, D % cpg == 0, D <= 8192, 1 <= K <= 64, B <= 65535, B U <= 2^30 (PIKA_ETOOBIG
 * beyond); null pointers, non-positive sizes, row strides below the row's width: PIKA_EINVAL.
 */
#ifndef PIKA_STATELESS_H
#define PIKA_STATELESS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PIKA_OK
#define PIKA_OK 0
#define PIKA_EINVAL (-1)   /* null pointer / non-positive dimension / blank out of range */
#define PIKA_ETOOBIG (-2)  /* beyond a stated limit */
#endif

#define PIKA_STATELESS_MAX_CTX 8
#define PIKA_STATELESS_MAX_CPG 16
#define PIKA_STATELESS_MAX_DIM 8192

/* out[b,u,:] for every position.  y i64 (B, U) with row stride ldy >= U elements; out f32 (B U, D) with row stride
 * ld >= D elements (row b U + u). */
int pika_stateless_forward(const long long *y, long long ldy, const float *E, const float *w, int B, int U, int V, int D,
                           int cpg, int ctx, float *out, long long ld, void *stream);

/* Bytes of the backward's workspace (go, then the chunk sums of d_w); 0 for dimensions the calls refuse. */
size_t pika_stateless_backward_workspace_bytes(int B, int U, int D, int cpg, int ctx);

/* d_E f32 (V, D) and d_w f32 (D, cpg, ctx), contiguous.  out is what the forward wrote (row stride ld_out), dout the
 * gradient with respect to it (row stride ld_dout).  sorted_tok, order i64 (B U,): the tokens y[b,p] in ascending order
 * and, for each, its position b U + p -- a STABLE sort of the flattened y, so that equal tokens come in position order
 * (any other order of equal tokens is accepted and sets the order of their sum).  workspace: the bytes above, 16-byte
 * aligned, no initialisation needed. */
int pika_stateless_backward(const long long *y, long long ldy, const long long *sorted_tok, const long long *order,
                            const float *E, const float *w, const float *out, long long ld_out, const float *dout,
                            long long ld_dout, int B, int U, int V, int D, int cpg, int ctx, float *d_E, float *d_w,
                            void *workspace, void *stream);

/* The search's per-frame step, in place from the caller's view: slot j of utterance b takes the OLD context of slot
 * clamp(parent[b,j], 0, K-1); if token[b,j] != blank the context is shifted left by one and token[b,j] appended;
 * rows[b K + j, :] = out of the new context at its last position.  parent, token i64 (B, K); rows f32 (B K, D) with row
 * stride ld >= D.  One workgroup per utterance stages all K old contexts in LDS before any store, so parent may repeat
 * a slot and may point anywhere.  With parent = a commit's slot_map and every token blank it re-orders the record. */
int pika_stateless_step(int *ctx_tok, const long long *parent, const long long *token, int B, int K, int ctx, int blank,
                        const float *E, const float *w, int V, int D, int cpg, float *rows, long long ld, void *stream);

#ifdef __cplusplus
}
#endif

#endif
