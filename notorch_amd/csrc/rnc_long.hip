// Rank-N-Contrast loss above nt_rnc_max_n(): the ranking part of rnc.hip for rows of up to 16384, still one
// workgroup per anchor row, sorted and scanned in LDS.  The mathematics and its guarantees are rnc.hip's
// (see its header): the key is rnc_desc_key, the column breaks ties, padding sorts behind every real entry
// and carries s = 0, the tie-group bounds are a prefix max and a suffix min, denom is an inclusive prefix
// sum of s read at the group end, T a suffix sum of 1 / denom over the pairs read at the group start, and
// every sum runs in an order fixed by (n, position): two calls return the same bits.
//
// A thread owns E consecutive sorted positions, E = 8 for P <= 8192 and E = 16 for P = 16384, where
// P = max(512, next power of two >= n) and the workgroup has P / E threads (64 .. 1024).  The sort
// (block_bitonic_sort_wide, sort_scan.hpp) runs the stages with partner distance < E in registers and the
// others through LDS, log2(E) stages between two barriers: 33 barriers at P = 8192, 29 at P = 16384
// (rnc.hip: 40 at P = 4096).
//
// LDS: 8 P + 256 bytes (64.25 KiB at P = 8192, 128.25 KiB at P = 16384), the 8 P used as
//   1. the P sort words (only the dist row is loaded before the sort); then, the words in registers,
//   2. lower half: the first and last key of every thread (the neighbours' tie-group edges);
//      upper half: the Sim row, loaded coalesced, from which sim[col] is gathered;
//   3. lower half: the prefix sums of s (denom is read at the group ends; sim[col] is gathered once more
//      for the nll term, which is cheaper than holding it in registers; the row's nll is reduced);
//   4. upper half: the suffix sums of 1 / denom (read at the group starts);
//      lower half: the dSim row, scattered by column, which leaves as whole 16-byte pieces.
// The last 256 bytes are the scans' per-wave slots.
#include "../../include/notorch_amd_train.h"
#include "common.hpp"
#include "sort_scan.hpp"

#include <cmath>

namespace nt {
namespace {

constexpr int kRncLongMaxN = 16384;  // 16 positions per thread, 1024 threads; 128.25 KiB of the CU's 160 KiB
constexpr int kRncLongMinP = 512;    // 8 positions per thread, one wave

// VEC: n % 4 == 0 and 16-byte aligned rows (16-byte loads and stores); else by element.
// E = 8 is held to 8 waves per SIMD (64 VGPRs), so that two workgroups of 64.25 KiB share a CU: measured
// 1.4 to 1.5 times faster than one workgroup at 75 VGPRs.
template <int E, bool VEC>
__global__ __launch_bounds__(1024, E == 8 ? 8 : 4) void rnc_rank_long_kernel(
    const float* __restrict__ sim, const float* __restrict__ dist, int n, int P, float temp, float eps,
    float scale, float* __restrict__ row_nll, float* __restrict__ dsim) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint64_t* comp = reinterpret_cast<uint64_t*>(lds);           // P sort words
  float* lo = reinterpret_cast<float*>(lds);                   // P floats: edge keys, prefix sums, dSim row
  float* hi = lo + P;                                          // P floats: Sim row, suffix sums
  uint32_t* edge = reinterpret_cast<uint32_t*>(lds);           // 2 per thread, over lo
  float* redf = reinterpret_cast<float*>(lds + 8 * (size_t)P);  // 64 words of scan scratch
  int* redi = reinterpret_cast<int*>(redf);

  const int row = blockIdx.x, tid = threadIdx.x, T = blockDim.x, base = E * tid;
  const float* drow = dist + (size_t)row * n;
  const float* srow = sim + (size_t)row * n;

  // ---- the dist row as sort words; positions >= n are padding
  uint64_t c[E];
#pragma unroll
  for (int q = 0; q < E; q += 4) {
    float d[4];
    if (VEC && base + q < n) {
      const float4 dv = *reinterpret_cast<const float4*>(drow + base + q);
      d[0] = dv.x, d[1] = dv.y, d[2] = dv.z, d[3] = dv.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = base + q + e < n ? drow[base + q + e] : -INFINITY;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) c[q + e] = ((uint64_t)rnc_desc_key(d[e]) << 32) | (uint32_t)(base + q + e);
  }
  block_bitonic_sort_wide<E>(c, comp, P);

  // ---- c[] holds sorted positions base .. base + E - 1: D descending, column ascending among equals
  // tie groups: a position starts one when the key before it differs, ends one when the key after does
  // (bit e of stm / enm; the thread's two outer bits wait for the neighbours' keys)
  uint32_t col[E], stm = 0, enm = 0, validm = 0, pairm = 0;
  const uint32_t key0 = (uint32_t)(c[0] >> 32), keyl = (uint32_t)(c[E - 1] >> 32);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    col[e] = (uint32_t)c[e];
    if (col[e] < (uint32_t)n) validm |= 1u << e;                               // a real column
    if (col[e] < (uint32_t)n && col[e] != (uint32_t)row) pairm |= 1u << e;     // a pair of the loss
    if (e > 0 && (uint32_t)(c[e] >> 32) != (uint32_t)(c[e - 1] >> 32)) stm |= 1u << e, enm |= 1u << (e - 1);
  }
  __syncthreads();  // every thread has read its sort words; their memory is reused below
  edge[2 * tid] = key0, edge[2 * tid + 1] = keyl;
  if (VEC) {
    for (int i = tid; 4 * i < n; i += T)
      reinterpret_cast<float4*>(hi)[i] = reinterpret_cast<const float4*>(srow)[i];
  } else {
    for (int i = tid; i < n; i += T) hi[i] = srow[i];
  }
  __syncthreads();
  const bool first = tid == 0, last = tid == T - 1;
  if (first || key0 != edge[first ? 0 : 2 * tid - 1]) stm |= 1u;
  if (last || keyl != edge[last ? 0 : 2 * tid + 2]) enm |= 1u << (E - 1);
  float s[E];
#pragma unroll
  for (int e = 0; e < E; ++e) s[e] = ((validm >> e) & 1u) ? expf(hi[col[e]] / temp) : 0.f;

  // start of each position's group (prefix max of the start positions), end of it (suffix min of the ends);
  // the scans' barriers also separate the reads of edge and hi above from the writes below
  int cs, ce;
  {
    int vmax = -1, vmin = P;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if ((stm >> e) & 1u) vmax = base + e;
      if ((enm >> (E - 1 - e)) & 1u) vmin = base + E - 1 - e;
    }
    cs = rnc_block_scan<int, false>(vmax, -1, RncMax{}, redi);
    ce = rnc_block_scan<int, true>(vmin, P, RncMin{}, redi);
  }

  // ---- forward: inclusive prefix sum of s, denom at the end of the own group
  {
    float loc[E];
    loc[0] = s[0];
#pragma unroll
    for (int e = 1; e < E; ++e) loc[e] = loc[e - 1] + s[e];
    const float off = rnc_block_scan<float, false>(loc[E - 1], 0.f, RncAdd{}, redf);
#pragma unroll
    for (int e = 0; e < E; ++e) lo[base + e] = off + loc[e];
  }
  __syncthreads();
  float r[E];  // 1 / denom over the pairs; first the nll terms
  {
    int ge = ce;
    float nll[E];
#pragma unroll
    for (int e = E - 1; e >= 0; --e) {
      if ((enm >> e) & 1u) ge = base + e;
      const bool pair = (pairm >> e) & 1u;
      const float denom = eps + lo[ge];
      nll[e] = pair ? logf(denom) - hi[col[e]] / temp : 0.f;  // gathered again: 8 registers fewer held
      r[e] = pair ? 1.f / denom : 0.f;
    }
#pragma unroll
    for (int w = 1; w < E; w <<= 1) {  // pairwise, as rnc.hip's (nll0 + nll1) + (nll2 + nll3)
#pragma unroll
      for (int e = 0; e < E; e += 2 * w) nll[e] += nll[e + w];
    }
    float v = nll[0];
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
#pragma unroll
    for (int e = E - 2; e >= 0; --e) r[e] += r[e + 1];
    const float off = rnc_block_scan<float, true>(r[0], 0.f, RncAdd{}, redf);
#pragma unroll
    for (int e = 0; e < E; ++e) hi[base + e] = off + r[e];
  }
  __syncthreads();
  {
    int gs = cs;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if ((stm >> e) & 1u) gs = base + e;
      if ((validm >> e) & 1u) lo[col[e]] = (s[e] * hi[gs] - (((pairm >> e) & 1u) ? 1.f : 0.f)) * scale;
    }
  }
  __syncthreads();
  float* grow = dsim + (size_t)row * n;
  if (VEC) {
    for (int i = tid; 4 * i < n; i += T)
      reinterpret_cast<float4*>(grow)[i] = reinterpret_cast<const float4*>(lo)[i];
  } else {
    for (int i = tid; i < n; i += T) grow[i] = lo[i];
  }
}

template <int E>
int launch_long(const float* sim, const float* dist, int n, int P, float temp, float eps, float scale,
                float* row_nll, float* dsim, bool vec, hipStream_t stream) {
  const size_t lds = 8 * (size_t)P + 256;
  auto kern = vec ? rnc_rank_long_kernel<E, true> : rnc_rank_long_kernel<E, false>;
  if (lds > 64 * 1024)
    NT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<n, P / E, lds, stream>>>(sim, dist, n, P, temp, eps, scale, row_nll, dsim);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

}  // namespace
}  // namespace nt

extern "C" int nt_rnc_long_max_n(void) { return nt::kRncLongMaxN; }

extern "C" int nt_rnc_rank_long(const float* sim, const float* dist, int64_t n, float temp, float eps,
                                float* row_nll, float* dsim, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(sim && dist && row_nll, NT_EINVAL, "NULL pointer (sim, dist and row_nll are required)");
  NT_REQUIRE(n >= 0, NT_EINVAL, "bad sizes: n < 0");
  NT_REQUIRE(std::isfinite(temp) && temp > 0.f, NT_EINVAL, "temp must be finite and > 0");
  NT_REQUIRE(n <= kRncLongMaxN, NT_EUNSUPPORTED,
             "n above nt_rnc_long_max_n() = " + std::to_string(kRncLongMaxN) +
                 " (one row per workgroup, sorted in LDS)");
  if (n == 0) return NT_OK;
  int P = kRncLongMinP;
  while (P < n) P <<= 1;
  const double pairs = (double)n * (double)(n - 1);
  const float scale = n > 1 ? (float)(1.0 / ((double)temp * pairs)) : 0.f;
  const bool vec = n % 4 == 0 && aligned16(sim) && aligned16(dist) && (dsim == nullptr || aligned16(dsim));
  hipStream_t stream = as_stream(stream_);
  if (P > 8192) return launch_long<16>(sim, dist, (int)n, P, temp, eps, scale, row_nll, dsim, vec, stream);
  return launch_long<8>(sim, dist, (int)n, P, temp, eps, scale, row_nll, dsim, vec, stream);
}
