// AUROC and average precision (notorch/nn/metrics.py AUROC, AUPRC) by sort and scan, one workgroup per column.
//
// The column's n scores are sorted descending with the network of sort_scan.hpp over P = max(256, next power
// of two >= n) words (key << 32 | row << 2 | label): the key is rnc_desc_key of the score (-0 == +0), the label
// 1 (positive), 0 (negative) or 2 (ignored: masked, or a target that is neither 0 nor 1).  Ignored entries and
// padding carry the largest key, so they sit behind every real score and count nothing.  The prefix counts of
// positives and negatives run as ONE integer scan of (positive << 16 | negative) (both <= 4096), a prefix
// max of the counts at the group ends gives every group end the counts of the group end before it (counts
// never decrease, so the max is the latest), and at the end g of each group of equal scores
//   auc += (fp_g - fp_{g-1}) (tp_g + tp_{g-1})                (64-bit integers: exact, any order)
//   ap  += (tp_g - tp_{g-1}) tp_g / (tp_g + fp_g)             (fp64: per thread in position order, a fixed
//                                                               shuffle tree, the waves in order)
// AUROC = auc / (2 P N), AP = ap / P.  LDS: 8 P + 256 B of scan scratch (32.25 KiB at P = 4096).
#include "../../include/notorch_amd_train.h"
#include "common.hpp"
#include "sort_scan.hpp"

#include <cmath>

namespace nt {
namespace {

constexpr int kRankMaxN = kSortMaxN;
constexpr uint32_t kIgnored = 2u;

__global__ __launch_bounds__(1024) void rank_metric_kernel(const float* __restrict__ scores,
                                                           const float* __restrict__ targets,
                                                           const uint8_t* __restrict__ mask, int n, int64_t t, int P,
                                                           float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint64_t* comp = reinterpret_cast<uint64_t*>(lds);                                  // P sort words
  int* redi = reinterpret_cast<int*>(lds + 8 * (size_t)P);                            // 16 ints
  unsigned long long* redu = reinterpret_cast<unsigned long long*>(lds + 8 * (size_t)P + 64);  // 16 x 8 B
  double* redd = reinterpret_cast<double*>(redu);

  const int tid = threadIdx.x, base = 4 * tid;
  const int64_t col = blockIdx.x;

  uint64_t c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = base + e;
    uint32_t key = 0xffffffffu, lab = kIgnored;
    if (row < n) {
      const int64_t at = (int64_t)row * t + col;
      if (mask == nullptr || mask[at] != 0) {
        const float y = truncf(targets[at]);
        lab = y == 1.f ? 1u : y == 0.f ? 0u : kIgnored;
      }
      if (lab != kIgnored) key = rnc_desc_key(scores[at]);
    }
    c[e] = ((uint64_t)key << 32) | ((uint32_t)row << 2) | lab;
  }
  block_bitonic_sort4(c, comp, P);

  // ---- c[] holds sorted positions base .. base + 3: score descending, ignored and padding last
  const bool last = base + 4 == P;
  const uint32_t knext = last ? 0u : (uint32_t)(comp[base + 4] >> 32);
  uint32_t key[4];
  bool en[4];  // the position ends a group of equal scores
  int cum[4];  // inclusive counts (positives << 16 | negatives), first within the thread
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    key[e] = (uint32_t)(c[e] >> 32);
    const uint32_t lab = (uint32_t)c[e] & 3u;
    const int one = lab == 1u ? (1 << 16) : lab == 0u ? 1 : 0;
    cum[e] = e == 0 ? one : cum[e - 1] + one;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) en[e] = key[e + 1] != key[e];
  en[3] = last || key[3] != knext;

  const int own = cum[3];
  const int off = rnc_block_scan<int, false>(own, 0, RncAddInt{}, redi);
  int at_end = 0;  // counts at the thread's last group end
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cum[e] += off;
    if (en[e]) at_end = cum[e];
  }
  int prev = rnc_block_scan<int, false>(at_end, 0, RncMax{}, redi);  // counts at the group end before base

  unsigned long long auc = 0;
  double ap = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!en[e]) continue;
    const int tp = cum[e] >> 16, fp = cum[e] & 0xffff, ptp = prev >> 16, pfp = prev & 0xffff;
    auc += (unsigned long long)(fp - pfp) * (unsigned long long)(tp + ptp);
    if (tp > ptp) ap += (double)(tp - ptp) * (double)tp / (double)(tp + fp);
    prev = cum[e];
  }
  const int total = block_sum(own, redi);
  auc = block_sum(auc, redu);
  ap = block_sum(ap, redd);
  if (tid == 0) {
    const int np = total >> 16, nn = total & 0xffff;
    const bool both = np > 0 && nn > 0;
    float* o = out + 4 * col;
    o[0] = both ? (float)((double)auc / (2.0 * (double)np * (double)nn)) : NAN;
    o[1] = both ? (float)(ap / (double)np) : NAN;
    o[2] = (float)np;
    o[3] = (float)nn;
  }
}

}  // namespace
}  // namespace nt

extern "C" int nt_rank_metric_max_n(void) { return nt::kRankMaxN; }

extern "C" int nt_rank_metric(const float* scores, const float* targets, const uint8_t* mask, int64_t n, int64_t t,
                              float* out, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(scores && targets && out, NT_EINVAL, "NULL pointer (scores, targets and out are required)");
  NT_REQUIRE(n >= 0 && t >= 0 && t <= INT32_MAX, NT_EINVAL, "bad sizes: n < 0, t < 0 or t >= 2^31");
  NT_REQUIRE(n <= kRankMaxN, NT_EUNSUPPORTED,
             "n above nt_rank_metric_max_n() = " + std::to_string(kRankMaxN) +
                 " (one column per workgroup, sorted in LDS)");
  if (t == 0) return NT_OK;
  int P = kSortMinP;
  while (P < n) P <<= 1;
  const size_t lds = 8 * (size_t)P + 256;
  rank_metric_kernel<<<(unsigned)t, P / 4, lds, as_stream(stream_)>>>(scores, targets, mask, (int)n, t, P, out);
  NT_LAUNCH_CHECK();
  return NT_OK;
}
