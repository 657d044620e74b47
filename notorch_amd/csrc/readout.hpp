// The launches of nt_softmax_pool_backward (readout.hip) that read no key, for bf16 rows: shared with
// nt_softmax_pool_backward_mixed (mixed.hip), whose own kernel is only the per-node one that reads the
// fp32 key.  Same kernels, same grids: the bits of the plain entry point.
#pragma once

#include "common.hpp"

namespace nt {

// stats[3 g] = (max_g, normaliser_g, <dout[g], pooled[g]>) of every molecule, pooled[g] the row out[g] was
// rounded from (summed again from X as the forward does); vec: 16-byte pieces
int launch_pool_stats_bf16(bool vec, const void* X, const float* s, const int32_t* seg_ptr,
                           const int32_t* perm, const void* out, const void* dout, int64_t nseg, int64_t h,
                           float* stats, hipStream_t stream);
// P[g] = sum_{v in g} ds[v] X[v] (fp32), ascending node order
int launch_weighted_pool_bf16(bool vec, const void* X, const float* ds, const int32_t* seg_ptr,
                              const int32_t* perm, int64_t nseg, int64_t h, float* P, hipStream_t stream);

}  // namespace nt
