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

#ifdef __cplusplus
}
#endif
#endif /* NOTORCH_AMD_TRAIN_H */
