/*
 * notorch_amd_train.h — training-side additions to the C ABI of notorch_amd.h.
 *
 * Additive: the entry points below live in the same library and follow the conventions of
 * notorch_amd.h (plain C types, caller-owned device memory and workspace, stream-ordered calls,
 * int status with the message in nt_last_error()).  NT_ABI_VERSION and the export set of
 * notorch_amd.h do not change.
 */
#ifndef NOTORCH_AMD_TRAIN_H
#define NOTORCH_AMD_TRAIN_H

#include "notorch_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Backward of a sum-mode nn.EmbeddingBag (notorch/nn/gnn/embed.py:20-24,29) with respect to its
 * table:
 *   dT[t, :] = sum_{i < n, j < k : idx[i * k + j] == t} R[i, :]        (fp32, rounded once to out_dtype)
 *   R[i, :]  = dX[i, :]                                                 (seg_ptr == NULL; n_dx == n)
 *   R[i, :]  = sum_{p in seg_ptr[i] .. seg_ptr[i+1]} dX[perm[p], :]     (CSR of nt_csr_build over the
 *                                                                        n_dx rows of dX, ascending p)
 * dX: n_dx rows of h elements (dx_dtype) whose rows sit ld_dx >= h elements apart; idx: n x k int64;
 * out: num_types x h (out_dtype), contiguous; every row is written, a type no index names gets zeros
 * (n == 0 writes all zeros).  An index outside [0, num_types) contributes nothing; a perm entry
 * outside [0, n_dx) is clamped (never read out of bounds).
 *
 * Deterministic: the rows are cut into contiguous ranges (at most 1024); one
 * workgroup per range accumulates a private fp32 partial table in LDS, every (type, column) address
 * by one lane in ascending (i, j); a second kernel adds the partials in a fixed order.  No float
 * atomics: two calls on the same inputs return the same bits.  Tables larger than the LDS partial
 * (96 KiB) are taken in chunks of whole type rows, each chunk by its own workgroups over the same
 * row ranges (h * 4 bytes must fit: h <= 24576, else NT_EUNSUPPORTED).
 *
 * workspace: nt_embed_bag_backward_workspace(n, num_types, h) bytes of caller-owned device memory,
 * 16-byte aligned (the partial tables); its contents before the call do not matter.
 */
/* bytes of workspace for these sizes; -1 for bad sizes */
NT_API int64_t nt_embed_bag_backward_workspace(int64_t n, int64_t num_types, int64_t h);
NT_API int nt_embed_bag_backward(const void* dX, int64_t ld_dx, int64_t n_dx, const int64_t* idx, int64_t n,
                                 int64_t k, int64_t num_types, int64_t h, const int32_t* seg_ptr,
                                 const int32_t* perm, int dx_dtype, int out_dtype, void* out, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/*
 * Mixed precision (an fp32 ChempropBlock under torch.autocast(dtype=bfloat16)): the boundary between
 * fp32 leaves and the bf16 storage kernels, with the conversion inside the kernel that consumes the
 * data.  Every rounding is round-to-nearest-even, once per stored element.  The three entry points
 * accept the hidden sizes of the bf16 layer kernel (h <= 512, or h % 8 == 0 and h <= 8192; else
 * NT_EUNSUPPORTED with the rule in the message) and validate on the host before any device call.
 */

/*
 * The bf16 weight images of nlayers (1..16) separate h x h weights in ONE launch: W, Wp, WpT, b and
 * b16 are HOST arrays of nlayers device pointers.  W[l]: row-major h x h in src_dtype (NT_F32 or
 * NT_BF16; else NT_EUNSUPPORTED).  Wp[l] (16-byte aligned, nt_dmpnn_packed_weight_bytes(h, NT_BF16)
 * bytes) receives the image nt_dmpnn_pack_weight(NT_BF16) writes for W[l] rounded to bf16.  WpT may be
 * NULL; else WpT[l] receives the image of W[l]^T (the backward's dA = G W), read from W[l] directly.
 * b and b16 may both be NULL; else b[l] is NULL (a layer without a bias) or h elements in src_dtype
 * whose bf16 copy goes to b16[l].  Same bytes as nt_dmpnn_pack_weight of the bf16 copy of W[l] and of
 * W[l]^T.
 */
NT_API int nt_dmpnn_pack_weights_mixed(const void* const* W, int64_t nlayers, int64_t h, int src_dtype,
                                       void* const* Wp, void* const* WpT, const void* const* b,
                                       void* const* b16, void* stream);

/*
 * nt_dmpnn_init for fp32 Xv (V x h) / Xe (E x h) and bf16 outputs: H0[e] = bf16(Xv[src e] + Xe[e]),
 * added in fp32 and rounded once (not bf16(bf16(xv) + bf16(xe)), what a cast followed by the bf16 init
 * gives); S (may be NULL: H0 only) = reduce over dst of act(H0) with the arithmetic of the bf16 init,
 * i.e. the bits of nt_segment_reduce over that H0.  seg_ptr / perm: the dst CSR (needed with S).
 * Rows of whole 16-byte pieces (h % 8 == 0, 16-byte aligned pointers) move as vectors, others by element.
 */
NT_API int nt_dmpnn_init_mixed(const void* Xv, const void* Xe, const int64_t* src, const int32_t* seg_ptr,
                               const int32_t* perm, int64_t V, int64_t E, int64_t h, int act,
                               float act_alpha, int reduce, void* H0, void* S, void* stream);

/*
 * nt_dmpnn_init_embed for fp32 tables and bf16 outputs: both bags summed in fp32 in ascending j, added
 * in fp32, rounded once.  Bit-identical to nt_embed_bag (NT_F32) twice followed by nt_dmpnn_init_mixed,
 * with Xv / Xe never written.  An index outside its table contributes nothing.
 */
NT_API int nt_dmpnn_init_embed_mixed(const void* node_table, int64_t num_node_types,
                                     const int64_t* node_types, int64_t kv, const void* edge_table,
                                     int64_t num_edge_types, const int64_t* edge_types, int64_t ke,
                                     const int64_t* src, const int32_t* seg_ptr, const int32_t* perm,
                                     int64_t V, int64_t E, int64_t h, int act, float act_alpha,
                                     int reduce, void* H0, void* S, void* stream);

/*
 * nt_dmpnn_update_fused for a layer whose update passes training-mode dropout (notorch/nn/gnn/
 * chemprop.py:26 `update = Sequential(Linear, Dropout(p))` under residual.py:28), in the same ONE
 * persistent launch per layer:
 *   U[e]        = W (S[src[e]] - act(H[rev[e]])) + b
 *   H_out[e, j] = (residual ? H[e, j] : 0) + keep(seed, offset + e * h + j) * U[e, j] / (1 - p)
 *   S_out[v]    = reduce_{dst[e] = v} agg_act(H_out[e])                       (as nt_dmpnn_update_fused)
 * keep() is bit for bit the decision of nt_dropout_residual(p, seed, offset) on the dense E x h
 * element index e * h + j (whatever the row pitch), so the backward regenerates the mask with that
 * entry point; p = 1 drops everything (H_out = the residual term).  The mask is applied in the layer
 * kernel's epilogue: fp32 in update_fk_kernel (every walk of the fused plan: 128-row tiles, 64-row
 * tiles of one or two workgroups per CU, column chunks above h = 512, hub sub-run partials S_part),
 * where amax_out receives max|H_out| and max|S_out| of the values after dropout; bf16 in the 64-row
 * layer kernel and its h > 512 variant, keep * (acc + b) / (1 - p) + H in fp32 with one rounding (the
 * unfused sequence rounds U and H_out), the aggregation reading the rounded value.
 *
 * Arguments, shape, alignment and dtype rules: those of nt_dmpnn_update_fused, plus
 * 0 <= p <= 1 (else NT_EINVAL, checked on the host before anything else).  A tile plan is required
 * (tile_ptr != NULL, with S_out; NT_EUNSUPPORTED without one: callers without a plan run
 * nt_dmpnn_update + nt_dropout_residual); bf16 takes plans of at most 64 rows with perm and
 * dst_sorted.  nt_last_kernel() names the variant ("..., dropout in the epilogue").
 */
NT_API int nt_dmpnn_update_fused_dropout(const void* H, const void* S, const int64_t* src, const int64_t* rev,
                                         const void* Wp, const void* b, int64_t V, int64_t E, int64_t h,
                                         int residual, int act, float act_alpha, const int32_t* tile_ptr,
                                         int64_t ntiles, int tile_rows, int max_in_degree, const int32_t* perm,
                                         const int32_t* dst_sorted, const void* row_table, int reduce,
                                         int agg_act, float agg_alpha, int dtype, const float* amax_in,
                                         float* amax_out, void* H_out, void* S_out, void* S_part,
                                         int64_t ld_in, int64_t ld_out, float p, uint64_t seed, uint64_t offset,
                                         void* stream);

/*
 * The attention readouts (Gated, SDPAttention) under torch.autocast(dtype=bfloat16): bf16 node rows X
 * with fp32 keys (Gated's a / a_bias, SDPAttention's Q).  Every key element is rounded to bf16, to
 * nearest even, where the kernel loads it; from there the arithmetic is that of the NT_BF16 kernels of
 * nt_node_scores / nt_softmax_pool_backward, so the results are the bits those entry points return for
 * the bf16 copy of the key, and no bf16 copy of a key is written.  nt_softmax_pool reads no key and
 * serves both.  dtype is the dtype of X (and of out / dout / dX): NT_BF16, else NT_EUNSUPPORTED.
 * Arguments, shapes and validation order: those of nt_node_scores / nt_softmax_pool_backward, on the
 * host before any device call (NT_EINVAL for bad sizes, for both or neither of a and Q, and for a NULL
 * pointer).  Rows of whole 16-byte pieces (h % 8 == 0, 16-byte aligned X and key; the backward also
 * out, dout and dX) move as vectors, a key piece as two 16-byte loads per lane; others by element.
 * One wave per node row.  ds and P are fp32 and are not rounded: the caller forms the fp32 key
 * gradients from them (Gated da = sum_g P[g], db = sum_v ds[v]; SDPA dQ = P / sqrt_key).
 */
NT_API int nt_node_scores_mixed(const void* X, int64_t n, int64_t h, const void* a, const void* a_bias,
                                const void* Q, const int64_t* node_seg, float sqrt_key, int dtype,
                                float* scores, void* stream);
NT_API int nt_softmax_pool_backward_mixed(const void* X, const float* scores, const int32_t* seg_ptr,
                                          const int32_t* perm, const int64_t* node_seg, int64_t nseg,
                                          int64_t n, int64_t h, const void* out, const void* dout,
                                          const void* a, const void* Q, float sqrt_key, int dtype,
                                          float* stats, void* dX, float* ds, float* P, void* stream);

/*
 * The ranking part of the Rank-N-Contrast loss (notorch/nn/loss/rnc.py:39-79) for sim and dist, both
 * n x n fp32, contiguous: with s_ik = exp(sim[i,k] / temp) and
 *   denom_ij = eps + sum_{k : dist[i,k] >= dist[i,j]} s_ik             (k over all of 0..n-1: k = j always,
 *                                                                       k = i when dist[i,j] <= dist[i,i])
 *   row_nll[i] = sum_{j != i} ( log denom_ij - sim[i,j] / temp )       (n floats; loss = sum / (n (n - 1)))
 *   dsim[i,k]  = ( s_ik * T_ik - [k != i] ) / (temp * n * (n - 1)),    T_ik = sum_{j != i, dist[i,j] <= dist[i,k]}
 *                                                                              1 / denom_ij
 * dsim (n x n, the gradient of the mean loss with respect to sim, diagonal included) may be NULL: the
 * forward only.  dist takes part in comparisons only (as floats: -0 == +0) and gets no gradient.
 * One workgroup per row sorts it by dist descending (a fixed bitonic network in LDS) and scans it;
 * O(n^2) memory, no n x n x n mask.  Every sum runs in a fixed order: two calls on the same inputs return
 * the same bits.  Non-finite entries are not checked (the result is then unspecified; the call ends).
 * nt_rnc_max_n() is the largest n a workgroup's LDS and thread count hold (>= 4096).
 * Checked on the host before any device call: NULL sim / dist / row_nll, n < 0, temp not finite or
 * <= 0 (NT_EINVAL); n > nt_rnc_max_n() (NT_EUNSUPPORTED); n == 0 launches nothing.  Rows move as
 * 16-byte vectors when n % 4 == 0 and the pointers are 16-byte aligned, else by element.
 */
NT_API int nt_rnc_max_n(void);
NT_API int nt_rnc_rank(const float* sim, const float* dist, int64_t n, float temp, float eps, float* row_nll,
                       float* dsim, void* stream);

/*
 * nt_rnc_rank for longer rows (csrc/rnc_long.hip; additive to ABI 8): the same arguments, results, host
 * checks and guarantees, for 0 <= n <= nt_rnc_long_max_n() = 16384.  Still one workgroup per row, with 8
 * sorted positions per thread up to n = 8192 and 16 above, in 8 P + 256 bytes of LDS (P = max(512, next
 * power of two >= n): 64.25 KiB at 8192, 128.25 KiB at 16384, set with the dynamic-LDS attribute).  The
 * sums run in an order fixed by (n, position) that differs from nt_rnc_rank's in the per-thread part, so the
 * two agree to fp32 rounding, not bit for bit.  n > nt_rnc_long_max_n() is NT_EUNSUPPORTED.  One launch,
 * no allocation, no synchronisation.
 */
NT_API int nt_rnc_long_max_n(void);
NT_API int nt_rnc_rank_long(const float* sim, const float* dist, int64_t n, float temp, float eps,
                            float* row_nll, float* dsim, void* stream);

/*
 * The task losses and regression metrics of notorch/nn/loss/loss.py and notorch/nn/metrics.py: element
 * loss, masked weighted reduction and the gradient of the reduced loss (csrc/task_loss.hip).
 *
 * preds: b x t x c, contiguous, preds_dtype NT_F32 or NT_BF16 (widened as loaded); targets: b x t fp32.
 * mask, lt_mask, gt_mask: b x t bytes (0 = false), each may be NULL; sample_weights: b fp32 or NULL.
 * kind selects the element loss L[i,j] of preds[i,j,:] = p and targets[i,j] = y:
 *   NT_LOSS_MSE  (c = 1)  (p - y)^2
 *   NT_LOSS_MAE  (c = 1)  |p - y|
 *   NT_LOSS_RMSE (c = 1)  sqrt((p - y)^2): the reference's literal definition, equal to MAE
 *   NT_LOSS_BCE  (c = 1)  max(p, 0) - p y + log1p(exp(-|p|))        (binary_cross_entropy_with_logits)
 *   NT_LOSS_MVE  (c = 2)  p = (m, v): (m - y)^2 / (2 v) + log(2 pi v) / 2
 *   NT_LOSS_EVIDENTIAL (c = 4)  p = (m, v, alpha, beta), r = y - m, B = 2 beta (1 + v):
 *                         log(pi / v) / 2 - alpha log B + (alpha + 1/2) log(v r^2 + B) + lgamma(alpha)
 *                         - lgamma(alpha + 1/2) + v_kl ((2 v + alpha) |r| - eps)
 *   NT_LOSS_XENT (c >= 1) logsumexp(p) - p[(int)y]; a class index outside [0, c) makes the element NaN
 * With lt_mask / gt_mask (MSE, MAE, RMSE only) p is first replaced by y where (p < y and lt) or (p > y and
 * gt); such an element has zero loss and zero gradient.  v_kl and eps are read by NT_LOSS_EVIDENTIAL only.
 *   loss[0]       = sum_ij L[i,j] w[i] m[i,j] / den,   den = sum_ij m[i,j]  (mask) or b t (mask == NULL)
 *   dpreds[i,j,:] = dL[i,j]/dp * (w[i] m[i,j] / den)                       (preds_dtype; NULL: loss only)
 * w = 1 without sample_weights.  An all-false mask gives NaN (0 / 0), as in the reference.  MAE and RMSE
 * take the gradient sign(p - y), 0 at p == y.  Evidential's digamma is the recurrence up to x >= 6 followed
 * by the asymptotic series (NaN for alpha <= 0).  Non-finite inputs are not checked.
 *
 * b t <= nt_task_loss_single_max(): ONE launch of one workgroup, no workspace.  Above it: one workgroup per
 * nt_task_loss_single_max() elements writes a partial sum and a partial mask count, one workgroup adds them
 * in index order and leaves 1 / den in the workspace, and (with dpreds) a third launch writes the gradient.
 * Every sum runs in an order fixed by (b, t): per-thread partials in index order (fp64), a fixed shuffle
 * tree, the waves in order; no float atomics; two calls return the same bits.  Nothing is read back.
 * workspace: nt_task_loss_workspace(b, t) bytes (0 in the one-launch case: NULL is accepted then) of
 * caller-owned device memory, 16-byte aligned.
 * Checked on the host before any device call: NULL preds / targets / loss, b, t < 0 or c < 1 or sizes beyond
 * 2^40 elements, a c that does not fit the kind, bounds with another kind than MSE / MAE / RMSE, a short or
 * missing workspace (NT_EINVAL); an unknown kind or preds_dtype (NT_EUNSUPPORTED).  b t == 0 launches
 * nothing (loss is not written).
 */
enum { NT_LOSS_MSE = 0, NT_LOSS_MAE = 1, NT_LOSS_RMSE = 2, NT_LOSS_BCE = 3, NT_LOSS_MVE = 4,
       NT_LOSS_EVIDENTIAL = 5, NT_LOSS_XENT = 6 };
NT_API int64_t nt_task_loss_single_max(void);
/* bytes of workspace for these sizes; -1 for bad sizes */
NT_API int64_t nt_task_loss_workspace(int64_t b, int64_t t);
NT_API int nt_task_loss(const void* preds, int preds_dtype, const float* targets, const uint8_t* mask,
                        const float* sample_weights, const uint8_t* lt_mask, const uint8_t* gt_mask, int64_t b,
                        int64_t t, int64_t c, int kind, float v_kl, float eps, float* loss, void* dpreds,
                        void* workspace, int64_t workspace_bytes, void* stream);

/*
 * AUROC and average precision of the columns of scores and targets (both n x t fp32, contiguous), one
 * workgroup per column (csrc/rank_metric.hip).  The label of an entry is ignored where mask (n x t bytes,
 * may be NULL) is 0, else positive where (int)target == 1, negative where (int)target == 0, ignored otherwise.
 * The column is sorted by score descending (the bitonic network of nt_rnc_rank; -0 == +0; ignored entries
 * are padding behind everything), the prefix counts tp and fp of positives and negatives are integers, and
 * both metrics are evaluated at the end g of each group of equal scores:
 *   AUROC = sum_g (fp_g - fp_{g-1}) (tp_g + tp_{g-1}) / (2 P N)      (the trapezoid over distinct thresholds
 *           = Mann-Whitney with ties counted half; the sum is exact in 64-bit integers, divided once)
 *   AP    = sum_g ((tp_g - tp_{g-1}) / P) tp_g / (tp_g + fp_g)       (fp64, in a fixed order)
 * out: t x 4 fp32: AUROC, AP, P, N of each column; AUROC and AP are NaN when P == 0 or N == 0.
 * Two calls return the same bits.  Checked on the host before any device call: NULL scores / targets / out,
 * n < 0 or t < 0 or t >= 2^31 (NT_EINVAL); n > nt_rank_metric_max_n() (>= 4096; NT_EUNSUPPORTED).  t == 0
 * launches nothing; n == 0 writes NaN, NaN, 0, 0.
 */
NT_API int nt_rank_metric_max_n(void);
NT_API int nt_rank_metric(const float* scores, const float* targets, const uint8_t* mask, int64_t n, int64_t t,
                          float* out, void* stream);

/*
 * nt_rank_metric for columns of any n up to nt_rank_metric_long_max_n() = 2^24 (P and N return as fp32
 * counts, exact up to 2^24): same arguments, label rule, formulas and output layout, on several workgroups
 * per column (csrc/rank_metric_long.hip).  With tile = 4096 positions and tiles = ceil(n / 4096), one call is
 * a fixed chain of 5 + ceil(log2 tiles) launches on the caller's stream:
 *   runs     one workgroup per (tile, column) sorts its 4096 words (nt_rank_metric's word with the global
 *            row, so all words of a column are distinct; padding counts on past n behind every score);
 *   merge    ceil(log2 tiles) passes between two word buffers: neighbouring sorted sequences of length L
 *            become one of length 2 L, one workgroup per 4096-word output tile, split by merge path;
 *   scan     tile partials (total counts, the local counts at the tile's last end of a group of equal
 *            scores), then per column the carries (the exclusive prefix of the totals; the counts at the
 *            latest group end before the tile), then every tile's AUROC and AP terms from those carries,
 *            then per column their sum: the integers exactly, the fp64 terms in a fixed order.
 * Every ordering between workgroups is a launch boundary: no workgroup waits for another inside a launch,
 * and there are no floating-point atomics; two calls return the same bits, whatever the workspace held.
 * Stream-ordered: no synchronisation, no allocation.  AUROC, P and N have the bits nt_rank_metric returns
 * where both take n; AP is the same fp64 sum in another fixed order.
 * workspace: nt_rank_metric_long_workspace(n, t) = tiles * t * (2 * 32768 + 48) bytes of caller-owned device
 * memory, 16-byte aligned (two word buffers; partials, carries and terms); the query answers -1 for sizes
 * the call refuses.
 * Checked on the host before any device call, in this order: NULL scores / targets / out (NT_EINVAL);
 * n < 0, t < 0, t >= 2^31 or tiles * t >= 2^31 (NT_EINVAL, "bad sizes"); n > nt_rank_metric_long_max_n()
 * (NT_EUNSUPPORTED); t == 0 launches nothing (NT_OK); n == 0 writes NaN, NaN, 0, 0 per column and reads no
 * workspace; otherwise a NULL, misaligned or short workspace (NT_EINVAL).
 */
NT_API int64_t nt_rank_metric_long_max_n(void);
/* bytes of workspace for these sizes; -1 for bad sizes */
NT_API int64_t nt_rank_metric_long_workspace(int64_t n, int64_t t);
NT_API int nt_rank_metric_long(const float* scores, const float* targets, const uint8_t* mask, int64_t n,
                               int64_t t, float* out, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NOTORCH_AMD_TRAIN_H */
