// AUROC and average precision of columns longer than one workgroup sorts (rank_metric.hip stops at 4096
// rows): sorted runs, merge-path passes and a tiled scan, a fixed chain of launches on the caller's stream.
//
// tile = 4096 positions, tiles = ceil(n / 4096), npad = 4096 tiles words per column.  Every ordering between
// workgroups is a launch boundary: no workgroup waits on, polls or spins for another, and there are no
// floating-point atomics, so the bits of the result are a function of the inputs alone.
//   runs     one workgroup per (tile, column) builds the words of rank_metric.hip (key << 32 | row << 2 |
//            label; row is the global row, so all words of a column are distinct; ignored entries and the
//            padding rows n .. npad - 1 carry the key 0xffffffff) and sorts them with block_bitonic_sort4.
//   merge    ceil(log2 tiles) passes, ping-pong between two buffers: sequences of length L become sequences
//            of length 2 L, a sequence without a partner is copied.  One workgroup per 4096-word output tile
//            finds where the tile's two bounding diagonals cut the pair (merge path: a search on global
//            memory, unambiguous because words are distinct), loads its part of the first sequence ascending
//            and its part of the second reversed into LDS, which is bitonic, and runs the network's last
//            iteration (block_bitonic_merge4).
//   scan     counts are (positives << 32 | negatives) in one 64-bit word (each < 2^25; the pairs along a
//            column are ordered componentwise, so the word's max is the pair's max).
//            (a) partials: a tile's total counts and its local counts at its last group end (bit 63: it has
//                one).  A position ends a group of equal keys when the next position's key differs (the next
//                tile's first word is read from global memory); the last position of all always does.
//            (b) carries, one workgroup per column: the exclusive prefix of the totals, and the counts at
//                the latest group end before the tile = the prefix max of (prefix + local at end).
//            (c) terms: every tile redoes its scan from the two carries and adds, at each group end g,
//                  auc += (fp_g - fp_{g-1}) (tp_g + tp_{g-1})        (64-bit integers)
//                  ap  += (tp_g - tp_{g-1}) tp_g / (tp_g + fp_g)     (fp64: per thread in position order, a
//                                                                     fixed shuffle tree, the waves in order)
//            (d) finish, one workgroup per column: the integers and, thread q taking tiles q, q + 1024, ...
//                in that order and then block_sum's fixed tree, the fp64 terms; writes AUROC, AP, P, N.
// 5 + ceil(log2 tiles) launches.  Workspace: tiles t (2 * 32768 + 48) bytes (two word buffers; 16 B each of
// partials, carries and terms per tile).  LDS: 32 KiB of words + 128 B of scan scratch, static.
#include "../../include/notorch_amd_train.h"
#include "common.hpp"
#include "sort_scan.hpp"

#include <cmath>

namespace nt {
namespace {

constexpr int kTile = kSortMaxN;  // positions per workgroup: 4 per thread, 1024 threads
constexpr int64_t kLongMaxN = (int64_t)1 << 24;  // P and N return as fp32: exact up to 2^24
constexpr int64_t kTileBytes = 2 * 8 * (int64_t)kTile + 48;  // workspace per (tile, column)
constexpr uint32_t kIgnored = 2u;
constexpr uint64_t kHasEnd = 1ull << 63;

struct U64Add {
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};
struct U64Max {
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

// max of one value per thread over the workgroup, to every thread (block_sum's shape; two barriers)
__device__ __forceinline__ uint64_t block_max(uint64_t v, uint64_t* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t m = red[0];
  for (int q = 1; q < (int)(blockDim.x >> 6); ++q) m = red[q] > m ? red[q] : m;
  __syncthreads();
  return m;
}

__global__ __launch_bounds__(1024) void rank_long_runs_kernel(const float* __restrict__ scores,
                                                              const float* __restrict__ targets,
                                                              const uint8_t* __restrict__ mask, int64_t n, int64_t t,
                                                              int64_t tiles, uint64_t* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) uint64_t comp[kTile];
  const int base = 4 * threadIdx.x;
  const int64_t col = blockIdx.x / tiles, tile = blockIdx.x % tiles;

  uint64_t c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t row = tile * kTile + base + e;
    uint32_t key = 0xffffffffu, lab = kIgnored;
    if (row < n) {
      const int64_t at = row * t + col;
      if (mask == nullptr || mask[at] != 0) {
        const float y = truncf(targets[at]);
        lab = y == 1.f ? 1u : y == 0.f ? 0u : kIgnored;
      }
      if (lab != kIgnored) key = rnc_desc_key(scores[at]);
    }
    c[e] = ((uint64_t)key << 32) | ((uint32_t)row << 2) | lab;
  }
  block_bitonic_sort4(c, comp, kTile);
  uint64_t* o = dst + (col * tiles + tile) * kTile + base;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = c[e];
}

// How many of the first d words of the merge of A (la words) and B (lb words), both ascending and with no
// word in common, come from A.  The whole wave calls it: 64 probes a step (pred(i) = A[i] < B[d - 1 - i]
// is true exactly below the answer), so 2^24 words take 5 steps.  Reads A[i] and B[d - 1 - i] only for
// max(0, d - lb) <= i < min(d, la): inside both.
__device__ __forceinline__ int64_t merge_path_wave(const uint64_t* __restrict__ A, int64_t la,
                                                   const uint64_t* __restrict__ B, int64_t lb, int64_t d) {
  const int lane = threadIdx.x & 63;
  int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const int64_t stride = (hi - lo + 63) >> 6, i = lo + lane * stride;
    const bool p = i < hi && A[i] < B[d - 1 - i];
    const int cnt = __popcll(__ballot(p));  // pred is monotone: lanes 0 .. cnt - 1
    if (cnt == 0) {
      hi = lo;
    } else {
      const int64_t top = lo + cnt * stride;
      lo += (cnt - 1) * stride + 1;
      hi = top < hi ? top : hi;
    }
  }
  return lo;
}

__global__ __launch_bounds__(1024) void rank_long_merge_kernel(const uint64_t* __restrict__ src,
                                                               uint64_t* __restrict__ dst, int64_t L,
                                                               int64_t tiles) {
  __shared__ __attribute__((aligned(16))) uint64_t comp[kTile];
  __shared__ int64_t cut[2];
  const int tid = threadIdx.x, base = 4 * tid;
  const int64_t col = blockIdx.x / tiles, tile = blockIdx.x % tiles, npad = tiles * kTile;
  const int64_t o0 = tile * kTile, s = o0 / (2 * L) * (2 * L);  // the output tile; its pair starts at s
  const int64_t la = npad - s < L ? npad - s : L, lb = npad - s - la < L ? npad - s - la : L;
  const uint64_t* A = src + col * npad + s;
  uint64_t* o = dst + col * npad + o0 + base;
  uint64_t c[4];
  if (lb == 0) {  // no partner: copied through (the whole workgroup takes this branch)
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = A[o0 - s + base + e];
    return;
  }
  const uint64_t* B = A + la;
  const int64_t d0 = o0 - s;  // d0 + kTile <= la + lb: npad is a multiple of kTile
  if (tid < 128) {            // wave 0: the tile's lower diagonal, wave 1: its upper one
    const int64_t i = merge_path_wave(A, la, B, lb, d0 + (tid >> 6) * kTile);
    if ((tid & 63) == 0) cut[tid >> 6] = i;
  }
  __syncthreads();
  const int64_t i0 = cut[0], j0 = d0 - i0;
  const int na = (int)(cut[1] - i0);  // A[i0 .. i0 + na) and B[j0 .. j0 + kTile - na) make the tile
  for (int k = tid; k < kTile; k += 1024) comp[k] = k < na ? A[i0 + k] : B[j0 + (kTile - 1 - k)];
  __syncthreads();
  block_bitonic_merge4(c, comp, kTile);
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = c[e];
}

// The thread's 4 sorted positions of a tile: cum[e] = its own inclusive counts (positives << 32 | negatives),
// en[e] = the position ends a group of equal keys.
__device__ __forceinline__ void tile_counts(const uint64_t* __restrict__ words, int64_t tile, int64_t tiles,
                                            uint64_t (&cum)[4], bool (&en)[4]) {
  const int64_t p0 = tile * kTile + 4 * threadIdx.x;
  const bool last = p0 + 4 == tiles * kTile;
  uint32_t key[5];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint64_t w = words[p0 + e];
    key[e] = (uint32_t)(w >> 32);
    const uint32_t lab = (uint32_t)w & 3u;
    const uint64_t one = lab == 1u ? (1ull << 32) : lab == 0u ? 1ull : 0ull;
    cum[e] = e == 0 ? one : cum[e - 1] + one;
  }
  key[4] = last ? 0u : (uint32_t)(words[p0 + 4] >> 32);
#pragma unroll
  for (int e = 0; e < 4; ++e) en[e] = key[e + 1] != key[e];
  if (last) en[3] = true;
}

__global__ __launch_bounds__(1024) void rank_long_partials_kernel(const uint64_t* __restrict__ sorted, int64_t tiles,
                                                                  uint64_t* __restrict__ part) {
  __shared__ uint64_t red[16];
  const int64_t col = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  uint64_t cum[4];
  bool en[4];
  tile_counts(sorted + col * tiles * kTile, tile, tiles, cum, en);
  const uint64_t off = rnc_block_scan<uint64_t, false>(cum[3], 0ull, U64Add{}, red);
  uint64_t at_end = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (en[e]) at_end = kHasEnd | (cum[e] + off);
  at_end = block_max(at_end, red);
  if (threadIdx.x == 1023) {
    part[2 * (int64_t)blockIdx.x] = off + cum[3];
    part[2 * (int64_t)blockIdx.x + 1] = at_end;
  }
}

__global__ __launch_bounds__(1024) void rank_long_carries_kernel(const uint64_t* __restrict__ part, int64_t tiles,
                                                                 uint64_t* __restrict__ carry) {
  __shared__ uint64_t red[16];
  const uint64_t* p = part + 2 * (int64_t)blockIdx.x * tiles;
  uint64_t* c = carry + 2 * (int64_t)blockIdx.x * tiles;
  uint64_t run_pre = 0, run_prev = 0;
  for (int64_t i0 = 0; i0 < tiles; i0 += 1024) {
    const int64_t i = i0 + threadIdx.x;
    const uint64_t tot = i < tiles ? p[2 * i] : 0, end = i < tiles ? p[2 * i + 1] : 0;
    const uint64_t pre = run_pre + rnc_block_scan<uint64_t, false>(tot, 0ull, U64Add{}, red);
    const uint64_t cand = (end & kHasEnd) ? pre + (end & ~kHasEnd) : 0;
    const uint64_t before = rnc_block_scan<uint64_t, false>(cand, 0ull, U64Max{}, red);
    if (i < tiles) {
      c[2 * i] = pre;
      c[2 * i + 1] = before > run_prev ? before : run_prev;
    }
    if (i0 + 1024 < tiles) {
      run_pre += block_sum(tot, red);
      const uint64_t m = block_max(cand, red);
      run_prev = m > run_prev ? m : run_prev;
    }
  }
}

__global__ __launch_bounds__(1024) void rank_long_terms_kernel(const uint64_t* __restrict__ sorted, int64_t tiles,
                                                               const uint64_t* __restrict__ carry,
                                                               uint64_t* __restrict__ terms) {
  __shared__ uint64_t red[16];
  const int64_t col = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  uint64_t cum[4];
  bool en[4];
  tile_counts(sorted + col * tiles * kTile, tile, tiles, cum, en);
  const uint64_t off = carry[2 * (int64_t)blockIdx.x] + rnc_block_scan<uint64_t, false>(cum[3], 0ull, U64Add{}, red);
  uint64_t at_end = 0;  // counts at the thread's last group end
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cum[e] += off;
    if (en[e]) at_end = cum[e];
  }
  uint64_t prev = rnc_block_scan<uint64_t, false>(at_end, 0ull, U64Max{}, red);  // at the group end before
  const uint64_t before = carry[2 * (int64_t)blockIdx.x + 1];
  prev = before > prev ? before : prev;

  unsigned long long auc = 0;
  double ap = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!en[e]) continue;
    const uint32_t tp = (uint32_t)(cum[e] >> 32), fp = (uint32_t)cum[e];
    const uint32_t ptp = (uint32_t)(prev >> 32), pfp = (uint32_t)prev;
    auc += (unsigned long long)(fp - pfp) * (unsigned long long)(tp + ptp);
    if (tp > ptp) ap += (double)(tp - ptp) * (double)tp / ((double)tp + (double)fp);
    prev = cum[e];
  }
  auc = block_sum(auc, reinterpret_cast<unsigned long long*>(red));
  ap = block_sum(ap, reinterpret_cast<double*>(red));
  if (threadIdx.x == 0) {
    terms[2 * (int64_t)blockIdx.x] = auc;
    terms[2 * (int64_t)blockIdx.x + 1] = (uint64_t)__double_as_longlong(ap);
  }
}

// tiles == 0 (n == 0) reads nothing: NaN, NaN, 0, 0
__global__ __launch_bounds__(1024) void rank_long_finish_kernel(const uint64_t* __restrict__ part,
                                                                const uint64_t* __restrict__ carry,
                                                                const uint64_t* __restrict__ terms, int64_t tiles,
                                                                float* __restrict__ out) {
  __shared__ uint64_t red[16];
  const int64_t first = (int64_t)blockIdx.x * tiles;
  unsigned long long auc = 0;
  double ap = 0.0;
  for (int64_t i = threadIdx.x; i < tiles; i += 1024) {
    auc += terms[2 * (first + i)];
    ap += __longlong_as_double((long long)terms[2 * (first + i) + 1]);
  }
  auc = block_sum(auc, reinterpret_cast<unsigned long long*>(red));
  ap = block_sum(ap, reinterpret_cast<double*>(red));
  if (threadIdx.x == 0) {
    const int64_t at = 2 * (first + tiles - 1);
    const uint64_t total = tiles > 0 ? carry[at] + part[at] : 0;
    const uint32_t np = (uint32_t)(total >> 32), nn = (uint32_t)total;
    const bool both = np > 0 && nn > 0;
    float* o = out + 4 * (int64_t)blockIdx.x;
    o[0] = both ? (float)((double)auc / (2.0 * (double)np * (double)nn)) : NAN;
    o[1] = both ? (float)(ap / (double)np) : NAN;
    o[2] = (float)np;
    o[3] = (float)nn;
  }
}

// tiles of n rows, or -1 where (n, t) are bad sizes: negative, t >= 2^31 or tiles * t >= 2^31 (the grid)
int64_t long_tiles(int64_t n, int64_t t) {
  if (n < 0 || t < 0 || t > INT32_MAX) return -1;
  const int64_t tiles = n / kTile + (n % kTile != 0);
  if (tiles > INT32_MAX || tiles * t > INT32_MAX) return -1;
  return tiles;
}

}  // namespace
}  // namespace nt

extern "C" int64_t nt_rank_metric_long_max_n(void) { return nt::kLongMaxN; }

extern "C" int64_t nt_rank_metric_long_workspace(int64_t n, int64_t t) {
  const int64_t tiles = nt::long_tiles(n, t);
  return tiles < 0 || n > nt::kLongMaxN ? -1 : tiles * t * nt::kTileBytes;
}

extern "C" int nt_rank_metric_long(const float* scores, const float* targets, const uint8_t* mask, int64_t n,
                                   int64_t t, float* out, void* workspace, int64_t workspace_bytes, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(scores && targets && out, NT_EINVAL, "NULL pointer (scores, targets and out are required)");
  const int64_t tiles = long_tiles(n, t);
  NT_REQUIRE(tiles >= 0, NT_EINVAL, "bad sizes: n < 0, t < 0, t >= 2^31 or ceil(n / 4096) * t >= 2^31");
  NT_REQUIRE(n <= kLongMaxN, NT_EUNSUPPORTED,
             "n above nt_rank_metric_long_max_n() = " + std::to_string(kLongMaxN) +
                 " (P and N return as fp32 counts, exact up to 2^24)");
  if (t == 0) return NT_OK;
  hipStream_t stream = as_stream(stream_);
  if (n == 0) {
    rank_long_finish_kernel<<<(unsigned)t, 1024, 0, stream>>>(nullptr, nullptr, nullptr, 0, out);
    NT_LAUNCH_CHECK();
    return NT_OK;
  }
  NT_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= tiles * t * kTileBytes, NT_EINVAL,
             "workspace missing, not 16-byte aligned or below nt_rank_metric_long_workspace(n, t) = " +
                 std::to_string(tiles * t * kTileBytes) + " bytes");
  const int64_t words = tiles * t * kTile;
  uint64_t* a = static_cast<uint64_t*>(workspace);
  uint64_t* b = a + words;
  uint64_t* part = b + words;
  uint64_t* carry = part + 2 * tiles * t;
  uint64_t* terms = carry + 2 * tiles * t;
  const unsigned grid = (unsigned)(tiles * t);

  rank_long_runs_kernel<<<grid, 1024, 0, stream>>>(scores, targets, mask, n, t, tiles, a);
  NT_LAUNCH_CHECK();
  for (int64_t L = kTile; L < tiles * kTile; L *= 2) {
    rank_long_merge_kernel<<<grid, 1024, 0, stream>>>(a, b, L, tiles);
    NT_LAUNCH_CHECK();
    uint64_t* s = a;
    a = b, b = s;
  }
  rank_long_partials_kernel<<<grid, 1024, 0, stream>>>(a, tiles, part);
  NT_LAUNCH_CHECK();
  rank_long_carries_kernel<<<(unsigned)t, 1024, 0, stream>>>(part, tiles, carry);
  NT_LAUNCH_CHECK();
  rank_long_terms_kernel<<<grid, 1024, 0, stream>>>(a, tiles, carry, terms);
  NT_LAUNCH_CHECK();
  rank_long_finish_kernel<<<(unsigned)t, 1024, 0, stream>>>(part, carry, terms, tiles, out);
  NT_LAUNCH_CHECK();
  return NT_OK;
}
