// One workgroup sorts and scans a row in LDS: the fixed bitonic network and the block scan shared by the
// Rank-N-Contrast kernel (rnc.hip) and the ranking metrics (rank_metric.hip; rank_metric_long.hip sorts its
// runs with it and merges them with the network's last iteration, block_bitonic_merge4).
//
// The network runs over P = a power of two >= 256 64-bit words, (key << 32 | payload), in P / 4 threads
// (at most 1024, so P <= 4096): each thread owns 4 consecutive sorted positions, the stages with partner
// distance 2 and 1 run in registers on those, the others through LDS, two stages per barrier (4 words a
// quarter of the upper distance apart per thread): 40 barriers at P = 4096.  The order is the unsigned order
// of the words; equal words are interchangeable, a NaN key is just one more bit pattern: the network cannot
// loop.
#pragma once

#include "common.hpp"

namespace nt {

constexpr int kSortMaxN = 4096;  // 4 positions per thread, 1024 threads per workgroup
constexpr int kSortMinP = 256;

// bit pattern of d mapped so that unsigned order is descending float order; -0 is first made +0, so floats
// that compare equal have equal keys
__device__ __forceinline__ uint32_t rnc_desc_key(float d) {
  const uint32_t u = __float_as_uint(d == 0.f ? 0.f : d);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

// compare-exchange of two words: ascending when up
__device__ __forceinline__ void rnc_cmpx(uint64_t& a, uint64_t& b, bool up) {
  if ((a > b) == up) {
    const uint64_t t = a;
    a = b;
    b = t;
  }
}

struct RncAdd {
  __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};
struct RncAddInt {
  __device__ __forceinline__ int operator()(int a, int b) const { return a + b; }
};
struct RncMax {
  __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; }
};
struct RncMin {
  __device__ __forceinline__ int operator()(int a, int b) const { return a < b ? a : b; }
};

// Exclusive scan of one value per thread over the workgroup, towards higher threads (REV: towards lower):
// wave shuffles, one LDS slot per wave, the other waves' totals folded in a fixed order.  Every thread of
// the block calls it (two barriers; red is free again on return).
template <typename V, bool REV, typename Op>
__device__ __forceinline__ V rnc_block_scan(V v, V ident, Op op, V* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  V incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V t = REV ? __shfl_down(incl, o) : __shfl_up(incl, o);
    if (REV ? lane + o < 64 : lane >= o) incl = op(incl, t);
  }
  V excl = REV ? __shfl_down(incl, 1) : __shfl_up(incl, 1);
  if (lane == (REV ? 63 : 0)) excl = ident;
  if (lane == (REV ? 0 : 63)) red[w] = incl;
  __syncthreads();
  V pre = ident;
  if (REV) {
    for (int q = nw - 1; q > w; --q) pre = op(pre, red[q]);
  } else {
    for (int q = 0; q < w; ++q) pre = op(pre, red[q]);
  }
  __syncthreads();
  return op(pre, excl);
}

// Sorts the P words of the workgroup ascending: c[e] is the word of position 4 * threadIdx.x + e on entry
// and the sorted word of that position on return, when comp[0 .. P) (LDS) holds all sorted words and every
// thread has passed a barrier.  blockDim.x == P / 4; every thread of the block calls it.
__device__ __forceinline__ void block_bitonic_sort4(uint64_t (&c)[4], uint64_t* comp, int P) {
  const int tid = threadIdx.x, T = blockDim.x, base = 4 * tid;
  // k = 2 and k = 4 of the network: the thread's 4 words sorted, ascending in even threads
  {
    const bool up = (tid & 1) == 0;
    rnc_cmpx(c[0], c[1], up), rnc_cmpx(c[2], c[3], up);
    rnc_cmpx(c[0], c[2], up), rnc_cmpx(c[1], c[3], up);
    rnc_cmpx(c[1], c[2], up);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) comp[base + e] = c[e];
  __syncthreads();

  // ---- bitonic merges k = 8 .. P
  for (int k = 8; k <= P; k <<= 1) {
    int j = k >> 1;
    // two stages (partner distances j and j / 2) per barrier: the thread's 4 words sit h = j / 2 apart
    for (; j >= 8; j >>= 2) {
      const int h = j >> 1, a = ((tid & ~(h - 1)) << 2) | (tid & (h - 1));
      const bool up = (a & k) == 0;
      uint64_t w0 = comp[a], w1 = comp[a + h], w2 = comp[a + 2 * h], w3 = comp[a + 3 * h];
      rnc_cmpx(w0, w2, up), rnc_cmpx(w1, w3, up);
      rnc_cmpx(w0, w1, up), rnc_cmpx(w2, w3, up);
      comp[a] = w0, comp[a + h] = w1, comp[a + 2 * h] = w2, comp[a + 3 * h] = w3;
      __syncthreads();
    }
    if (j == 4) {  // an odd number of LDS stages: the last one alone
      for (int u = tid; u < (P >> 1); u += T) {
        const int lo = ((u & ~3) << 1) | (u & 3), hi = lo | 4;
        const uint64_t a = comp[lo], b = comp[hi];
        if ((a > b) == ((lo & k) == 0)) comp[lo] = b, comp[hi] = a;
      }
      __syncthreads();
    }
    const bool up = (base & k) == 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = comp[base + e];
    rnc_cmpx(c[0], c[2], up), rnc_cmpx(c[1], c[3], up);
    rnc_cmpx(c[0], c[1], up), rnc_cmpx(c[2], c[3], up);
#pragma unroll
    for (int e = 0; e < 4; ++e) comp[base + e] = c[e];
    __syncthreads();
  }
}

// The k = P iteration of the network above on its own: comp[0 .. P) (LDS) holds a BITONIC sequence (ascending,
// then descending: two sorted runs, the second reversed) and every thread has passed a barrier; on return c[e]
// is the ascending sorted word of position 4 * threadIdx.x + e.  comp is left mid-network (not rewritten after
// the register stages).  blockDim.x == P / 4; every thread of the block calls it.  6 barriers at P = 4096.
__device__ __forceinline__ void block_bitonic_merge4(uint64_t (&c)[4], uint64_t* comp, int P) {
  const int tid = threadIdx.x, T = blockDim.x, base = 4 * tid;
  int j = P >> 1;
  for (; j >= 8; j >>= 2) {
    const int h = j >> 1, a = ((tid & ~(h - 1)) << 2) | (tid & (h - 1));
    uint64_t w0 = comp[a], w1 = comp[a + h], w2 = comp[a + 2 * h], w3 = comp[a + 3 * h];
    rnc_cmpx(w0, w2, true), rnc_cmpx(w1, w3, true);
    rnc_cmpx(w0, w1, true), rnc_cmpx(w2, w3, true);
    comp[a] = w0, comp[a + h] = w1, comp[a + 2 * h] = w2, comp[a + 3 * h] = w3;
    __syncthreads();
  }
  if (j == 4) {
    for (int u = tid; u < (P >> 1); u += T) {
      const int lo = ((u & ~3) << 1) | (u & 3), hi = lo | 4;
      const uint64_t a = comp[lo], b = comp[hi];
      if (a > b) comp[lo] = b, comp[hi] = a;
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) c[e] = comp[base + e];
  rnc_cmpx(c[0], c[2], true), rnc_cmpx(c[1], c[3], true);
  rnc_cmpx(c[0], c[1], true), rnc_cmpx(c[2], c[3], true);
}

// ---- wide rows (rnc_long.hip): the same network with E = 8 or 16 consecutive positions per thread, so
// P = E * blockDim.x reaches 8192 or 16384.  The stages with partner distance < E run in registers on the
// thread's own words; the others go through LDS, log2(E) stages between two barriers.

// The stages with partner distances G / 2 .. 1 of one merge on G words in registers, all in direction up.
template <int G>
__device__ __forceinline__ void rnc_reg_stages(uint64_t (&w)[G], bool up) {
#pragma unroll
  for (int d = G / 2; d >= 1; d >>= 1) {
#pragma unroll
    for (int m = 0; m < G; ++m)
      if ((m & d) == 0) rnc_cmpx(w[m], w[m | d], up);
  }
}

// NS stages of merge k (partner distances j, j / 2, .., h = j >> (NS - 1)) on comp[0 .. E * blockDim.x),
// then a barrier.  A thread takes E >> NS groups of 2^NS words that sit h apart, which are exactly the
// words those stages connect.  k >= 2 j, so the direction is the same for the whole group.
template <int E, int NS>
__device__ __forceinline__ void rnc_lds_stages(uint64_t* comp, int k, int j) {
  constexpr int G = 1 << NS;
  const int h = j >> (NS - 1);
#pragma unroll
  for (int g = 0; g < E / G; ++g) {
    const int u = (int)threadIdx.x + g * (int)blockDim.x;
    const int a = ((u & ~(h - 1)) << NS) | (u & (h - 1));
    uint64_t w[G];
#pragma unroll
    for (int m = 0; m < G; ++m) w[m] = comp[a + m * h];
    rnc_reg_stages<G>(w, (a & k) == 0);
#pragma unroll
    for (int m = 0; m < G; ++m) comp[a + m * h] = w[m];
  }
  __syncthreads();
}

// Sorts the P = E * blockDim.x words of the workgroup ascending: c[e] is the word of position
// E * threadIdx.x + e on entry and the sorted word of that position on return.  comp[0 .. P) (LDS) is left
// mid-network and NO barrier follows the last read of it: the caller places one before it reuses comp.
// P >= 2 E; every thread of the block calls it.  Barriers: 32 at P = 8192 (E = 8), 28 at P = 16384 (E = 16).
template <int E>
__device__ __forceinline__ void block_bitonic_sort_wide(uint64_t (&c)[E], uint64_t* comp, int P) {
  static_assert(E == 8 || E == 16, "8 or 16 positions per thread");
  constexpr int S = E == 16 ? 4 : 3;  // log2(E): LDS stages between two barriers
  const int tid = threadIdx.x, base = E * tid;
  // k = 2 .. E of the network: the thread's words sorted, ascending in even threads
#pragma unroll
  for (int k = 2; k <= E; k <<= 1) {
#pragma unroll
    for (int d = k / 2; d >= 1; d >>= 1) {
#pragma unroll
      for (int m = 0; m < E; ++m)
        if ((m & d) == 0) rnc_cmpx(c[m], c[m | d], k < E ? (m & k) == 0 : (tid & 1) == 0);
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) comp[base + e] = c[e];
  __syncthreads();

  // ---- bitonic merges k = 2 E .. P: `stages` partner distances k / 2 .. E through LDS, the rest in registers
  int stages = 1;
  for (int k = 2 * E; k <= P; k <<= 1, ++stages) {
    int j = k >> 1, left = stages;
    for (; left >= S; left -= S, j >>= S) rnc_lds_stages<E, S>(comp, k, j);
    if (left == 1) rnc_lds_stages<E, 1>(comp, k, j);
    if (left == 2) rnc_lds_stages<E, 2>(comp, k, j);
    if (S == 4 && left == 3) rnc_lds_stages<E, 3>(comp, k, j);
#pragma unroll
    for (int e = 0; e < E; ++e) c[e] = comp[base + e];
    rnc_reg_stages<E>(c, (base & k) == 0);
    if (k < P) {
#pragma unroll
      for (int e = 0; e < E; ++e) comp[base + e] = c[e];
      __syncthreads();
    }
  }
}

}  // namespace nt
