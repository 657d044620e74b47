// Rank-N-Contrast loss (notorch/nn/loss/rnc.py): the ranking part, one workgroup per anchor row.
//
// For the anchor row i of Sim and D (both n x n fp32), with s_k = exp(Sim[i,k] / temp):
//   denom_j = eps + sum_{k : D[i,k] >= D[i,j]} s_k                  (k over all of 0..n-1)
//   row_nll[i] = sum_{j != i} ( log denom_j - Sim[i,j] / temp )
//   dSim[i,k]  = ( s_k * T_k - [k != i] ) * scale,  T_k = sum_{j != i, D[i,j] <= D[i,k]} 1 / denom_j
// The reference builds the n x n x n mask of the comparison; here the row is sorted once by D[i,.]
// descending, after which the >= set of j is the prefix that ends where j's tie group ends and the <=
// set of k is the suffix that starts where k's tie group starts: a prefix sum of s, a suffix sum of
// 1 / denom, and the two group bounds.
//
// The sort (sort_scan.hpp, shared with rank_metric.hip) is a fixed bitonic network over P = max(256, next power of two >= n) 64-bit words
// (key << 32 | column): the key is the bit pattern of D mapped so that unsigned order is descending
// float order (-0 first made +0, so floats that compare equal have equal keys), the column breaks ties
// ascending, so all words are distinct, the order is total, and a NaN is just one more bit pattern: the
// network cannot loop.  Padding words carry the key of -inf and columns >= n (behind every real -inf)
// and s = 0.  Each thread owns 4 consecutive sorted positions (P / 4 threads, at most 1024): the stages
// with partner distance 2 and 1 run in registers on those, the others through LDS, two stages per barrier
// (4 words a quarter of the upper distance apart per thread): 40 barriers at P = 4096.  Every sum runs in
// an order fixed by (n, position): two calls return the same bits.
//
// LDS: 8 P (sort words; reused for the two scan results once the words sit in registers) + 4 P (the Sim
// row, then the dSim row) + 256 B of scan scratch: 48.25 KiB at P = 4096, two workgroups per CU.
#include "../../include/notorch_amd_train.h"
#include "common.hpp"
#include "sort_scan.hpp"

#include <cmath>

namespace nt {
namespace {

constexpr int kRncMaxN = kSortMaxN;
constexpr int kRncMinP = kSortMinP;

// VEC: n % 4 == 0 and 16-byte aligned rows (16-byte loads and stores); else by element
template <bool VEC>
__global__ __launch_bounds__(1024) void rnc_rank_kernel(const float* __restrict__ sim,
                                                        const float* __restrict__ dist, int n, int P,
                                                        float temp, float eps, float scale,
                                                        float* __restrict__ row_nll, float* __restrict__ dsim) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint64_t* comp = reinterpret_cast<uint64_t*>(lds);          // P sort words
  float* cbuf = reinterpret_cast<float*>(lds);                // P prefix sums   (over comp, after the sort)
  float* rbuf = cbuf + P;                                     // P suffix sums   (over comp, after the sort)
  float* simv = reinterpret_cast<float*>(lds + 8 * (size_t)P);  // P: the Sim row, later the dSim row
  float* redf = reinterpret_cast<float*>(lds + 12 * (size_t)P);  // 64 words of scan scratch
  int* redi = reinterpret_cast<int*>(redf);

  const int row = blockIdx.x, tid = threadIdx.x, T = blockDim.x, base = 4 * tid;
  const float* drow = dist + (size_t)row * n;
  const float* srow = sim + (size_t)row * n;

  // ---- load the two rows; positions >= n are padding
  float d[4], sv[4];
  if (VEC && base < n) {
    const float4 dv = *reinterpret_cast<const float4*>(drow + base);
    const float4 s4 = *reinterpret_cast<const float4*>(srow + base);
    d[0] = dv.x, d[1] = dv.y, d[2] = dv.z, d[3] = dv.w;
    sv[0] = s4.x, sv[1] = s4.y, sv[2] = s4.z, sv[3] = s4.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = base + e < n;
      d[e] = in ? drow[base + e] : -INFINITY;
      sv[e] = in ? srow[base + e] : 0.f;
    }
  }
  uint64_t c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    simv[base + e] = sv[e];
    c[e] = ((uint64_t)rnc_desc_key(d[e]) << 32) | (uint32_t)(base + e);
  }
  block_bitonic_sort4(c, comp, P);

  // ---- c[] holds sorted positions base .. base + 3: D descending, column ascending among equals
  uint32_t key[4], col[4];
  bool valid[4], pair[4];  // a real column; a (row, column) pair of the loss (column != row)
  float sm[4], s[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    key[e] = (uint32_t)(c[e] >> 32);
    col[e] = (uint32_t)c[e];
    valid[e] = col[e] < (uint32_t)n;
    pair[e] = valid[e] && col[e] != (uint32_t)row;
    sm[e] = valid[e] ? simv[col[e]] / temp : 0.f;
    s[e] = valid[e] ? expf(sm[e]) : 0.f;
  }
  // tie groups: a position starts one when the key before it differs, ends one when the key after does
  const bool first = base == 0, last = base + 4 == P;
  const uint32_t kprev = first ? 0u : (uint32_t)(comp[base - 1] >> 32);
  const uint32_t knext = last ? 0u : (uint32_t)(comp[base + 4] >> 32);
  bool st[4], en[4];
  st[0] = first || key[0] != kprev;
  en[3] = last || key[3] != knext;
#pragma unroll
  for (int e = 1; e < 4; ++e) st[e] = en[e - 1] = key[e] != key[e - 1];
  __syncthreads();  // comp and simv are read; their memory is reused below

  // start of each position's group (prefix max of the start positions), end of it (suffix min of the ends)
  int gs[4], ge[4];
  {
    int vmax = -1, vmin = P;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (st[e]) vmax = base + e;
      if (en[3 - e]) vmin = base + 3 - e;
    }
    const int cs = rnc_block_scan<int, false>(vmax, -1, RncMax{}, redi);
    const int ce = rnc_block_scan<int, true>(vmin, P, RncMin{}, redi);
    gs[0] = st[0] ? base : cs;
    ge[3] = en[3] ? base + 3 : ce;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
      gs[e] = st[e] ? base + e : gs[e - 1];
      ge[3 - e] = en[3 - e] ? base + 3 - e : ge[4 - e];
    }
  }

  // ---- forward: inclusive prefix sum of s, denom at the end of the own group
  {
    float loc[4];
    loc[0] = s[0];
#pragma unroll
    for (int e = 1; e < 4; ++e) loc[e] = loc[e - 1] + s[e];
    const float off = rnc_block_scan<float, false>(loc[3], 0.f, RncAdd{}, redf);
#pragma unroll
    for (int e = 0; e < 4; ++e) cbuf[base + e] = off + loc[e];
  }
  __syncthreads();
  float r[4], nll[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float denom = eps + cbuf[ge[e]];
    nll[e] = pair[e] ? logf(denom) - sm[e] : 0.f;
    r[e] = pair[e] ? 1.f / denom : 0.f;
  }
  {
    float v = (nll[0] + nll[1]) + (nll[2] + nll[3]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) redf[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
      for (int q = 1; q < (T >> 6); ++q) v += redf[q];
      row_nll[row] = v;
    }
    __syncthreads();
  }
  if (dsim == nullptr) return;

  // ---- gradient: suffix sum of 1 / denom over the pairs, read at the start of the own group
  {
    float loc[4];
    loc[3] = r[3];
#pragma unroll
    for (int e = 2; e >= 0; --e) loc[e] = loc[e + 1] + r[e];
    const float off = rnc_block_scan<float, true>(loc[0], 0.f, RncAdd{}, redf);
#pragma unroll
    for (int e = 0; e < 4; ++e) rbuf[base + e] = off + loc[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (valid[e]) simv[col[e]] = (s[e] * rbuf[gs[e]] - (pair[e] ? 1.f : 0.f)) * scale;
  __syncthreads();
  float* grow = dsim + (size_t)row * n;
  if (VEC) {
    if (base < n) *reinterpret_cast<float4*>(grow + base) = *reinterpret_cast<const float4*>(simv + base);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (base + e < n) grow[base + e] = simv[base + e];
  }
}

}  // namespace
}  // namespace nt

extern "C" int nt_rnc_max_n(void) { return nt::kRncMaxN; }

extern "C" int nt_rnc_rank(const float* sim, const float* dist, int64_t n, float temp, float eps,
                           float* row_nll, float* dsim, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(sim && dist && row_nll, NT_EINVAL, "NULL pointer (sim, dist and row_nll are required)");
  NT_REQUIRE(n >= 0, NT_EINVAL, "bad sizes: n < 0");
  NT_REQUIRE(std::isfinite(temp) && temp > 0.f, NT_EINVAL, "temp must be finite and > 0");
  NT_REQUIRE(n <= kRncMaxN, NT_EUNSUPPORTED,
             "n above nt_rnc_max_n() = " + std::to_string(kRncMaxN) + " (one row per workgroup, sorted in LDS)");
  if (n == 0) return NT_OK;
  int P = kRncMinP;
  while (P < n) P <<= 1;
  const size_t lds = 12 * (size_t)P + 256;
  const double pairs = (double)n * (double)(n - 1);
  const float scale = n > 1 ? (float)(1.0 / ((double)temp * pairs)) : 0.f;
  const bool vec = n % 4 == 0 && aligned16(sim) && aligned16(dist) && (dsim == nullptr || aligned16(dsim));
  hipStream_t stream = as_stream(stream_);
  if (vec)
    rnc_rank_kernel<true><<<(int)n, P / 4, lds, stream>>>(sim, dist, (int)n, P, temp, eps, scale, row_nll, dsim);
  else
    rnc_rank_kernel<false><<<(int)n, P / 4, lds, stream>>>(sim, dist, (int)n, P, temp, eps, scale, row_nll, dsim);
  NT_LAUNCH_CHECK();
  return NT_OK;
}
