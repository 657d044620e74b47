// Task losses and regression metrics (notorch/nn/loss/loss.py, notorch/nn/metrics.py): the element loss,
// the masked weighted reduction and the gradient of the reduced loss from one launch.
//
//   loss   = sum_e L[e] w[e / t] m[e] / den,   den = sum_e m[e]  (or n = b t without a mask)
//   dpreds = dL[e]/dp * (w[e / t] m[e] / den)
// over the n = b t elements e = i t + j; the element math is task_loss_math.hpp.
//
// n <= kSingleMax (8192): one workgroup of 1024 threads.  It counts the mask (integers), so 1 / den is known
// before the one pass that evaluates L and writes the scaled gradient; thread q takes the elements
// q, q + 1024, ... in that order into an fp64 partial, the partials are added by a fixed xor-shuffle tree
// in each wave and the 16 wave totals in wave order.  Nothing but 16 doubles and 16 ints of LDS.
// n > kSingleMax: workgroup g of the partial launch does the same over the elements [g, g + 1) * 8192 and
// writes its sum and count to the workspace; one workgroup adds those in g order (same thread / tree / wave
// order) and leaves the loss and 1 / den; the gradient launch re-evaluates the elements with that scale.
// The loads are per element (c values each): at these sizes the launch, not the bandwidth, is the cost.
#include "task_loss_math.hpp"

#include "common.hpp"

namespace nt {
namespace {

constexpr int kThreads = 1024;
constexpr int64_t kSingleMax = 8192;   // elements per workgroup: 8 per thread
constexpr int64_t kMaxElems = (int64_t)1 << 40;

enum { kModeSingle = 0, kModePartial = 1, kModeGrad = 2 };

struct TaskLossArgs {
  const void* preds;
  const float* targets;
  const uint8_t* mask;
  const float* weights;
  const uint8_t* lt;
  const uint8_t* gt;
  int64_t n, t;
  int c;
  float v_kl, eps;
  float* loss;
  void* dpreds;
  float* inv_den;       // workspace: 1 / den (written by the finalize, read by the gradient launch)
  double* part_sum;     // workspace: one per workgroup of the partial launch
  long long* part_cnt;  // workspace: likewise
};

template <int KIND, typename P>
__global__ __launch_bounds__(kThreads) void task_loss_kernel(TaskLossArgs a, int mode) {
  __shared__ double redd[kThreads / 64];
  __shared__ long long redc[kThreads / 64];
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * kSingleMax;
  const int64_t hi = a.n - lo < kSingleMax ? a.n : lo + kSingleMax;

  double den = (double)a.n;
  float inv = 0.f;
  if (mode == kModeGrad) {
    inv = *a.inv_den;
  } else if (mode == kModeSingle) {
    if (a.mask) {
      long long cnt = 0;
      for (int64_t e = lo + tid; e < hi; e += kThreads) cnt += a.mask[e] != 0;
      den = (double)block_sum(cnt, redc);
    }
    inv = (float)(1.0 / den);
  }

  const bool want_grad = mode != kModePartial && a.dpreds != nullptr;
  if (mode == kModeGrad && !want_grad) return;
  const P* preds = static_cast<const P*>(a.preds);
  P* dpreds = static_cast<P*>(a.dpreds);
  double acc = 0.0;
  long long cnt = 0;
  for (int64_t e = lo + tid; e < hi; e += kThreads) {
    const bool on = a.mask == nullptr || a.mask[e] != 0;
    const float m = on ? 1.f : 0.f;
    const float w = a.weights ? a.weights[e / a.t] : 1.f;
    const bool lt = a.lt != nullptr && a.lt[e] != 0, gt = a.gt != nullptr && a.gt[e] != 0;
    const float L = task_loss_element<KIND, P>(preds + e * a.c, a.targets[e], a.c, a.v_kl, a.eps, lt, gt,
                                               w * m * inv, want_grad ? dpreds + e * a.c : nullptr);
    acc += (double)((L * w) * m);
    cnt += on;
  }
  if (mode == kModeGrad) return;
  const double total = block_sum(acc, redd);
  if (mode == kModeSingle) {
    if (tid == 0) a.loss[0] = (float)(total / den);
    return;
  }
  const long long count = block_sum(cnt, redc);
  if (tid == 0) {
    a.part_sum[blockIdx.x] = total;
    a.part_cnt[blockIdx.x] = count;
  }
}

__global__ __launch_bounds__(kThreads) void task_loss_finalize_kernel(const double* __restrict__ part_sum,
                                                                      const long long* __restrict__ part_cnt,
                                                                      int64_t nparts, float* __restrict__ loss,
                                                                      float* __restrict__ inv_den) {
  __shared__ double redd[kThreads / 64];
  __shared__ long long redc[kThreads / 64];
  double acc = 0.0;
  long long cnt = 0;
  for (int64_t g = threadIdx.x; g < nparts; g += kThreads) {
    acc += part_sum[g];
    cnt += part_cnt[g];
  }
  const double total = block_sum(acc, redd);
  const double den = (double)block_sum(cnt, redc);
  if (threadIdx.x == 0) {
    loss[0] = (float)(total / den);
    inv_den[0] = (float)(1.0 / den);
  }
}

inline int64_t num_parts(int64_t n) { return (n + kSingleMax - 1) / kSingleMax; }

// bytes: 16 (1 / den) + 8 per partial sum + 8 per partial count
inline int64_t workspace_bytes_for(int64_t n) { return n <= kSingleMax ? 0 : 16 + 16 * num_parts(n); }

inline bool sizes_ok(int64_t b, int64_t t) {
  return b >= 0 && t >= 0 && b <= kMaxElems && t <= kMaxElems && (b == 0 || t <= kMaxElems / b);
}

template <int KIND, typename P>
int launch(const TaskLossArgs& a, hipStream_t stream) {
  if (a.n <= kSingleMax) {
    task_loss_kernel<KIND, P><<<1, kThreads, 0, stream>>>(a, kModeSingle);
    NT_LAUNCH_CHECK();
    return NT_OK;
  }
  const int64_t parts = num_parts(a.n);
  task_loss_kernel<KIND, P><<<(unsigned)parts, kThreads, 0, stream>>>(a, kModePartial);
  NT_LAUNCH_CHECK();
  task_loss_finalize_kernel<<<1, kThreads, 0, stream>>>(a.part_sum, a.part_cnt, parts, a.loss, a.inv_den);
  NT_LAUNCH_CHECK();
  if (a.dpreds) {
    task_loss_kernel<KIND, P><<<(unsigned)parts, kThreads, 0, stream>>>(a, kModeGrad);
    NT_LAUNCH_CHECK();
  }
  return NT_OK;
}

template <typename P>
int launch_kind(int kind, const TaskLossArgs& a, hipStream_t stream) {
  switch (kind) {
    case NT_LOSS_MSE: return launch<NT_LOSS_MSE, P>(a, stream);
    case NT_LOSS_MAE: return launch<NT_LOSS_MAE, P>(a, stream);
    case NT_LOSS_RMSE: return launch<NT_LOSS_RMSE, P>(a, stream);
    case NT_LOSS_BCE: return launch<NT_LOSS_BCE, P>(a, stream);
    case NT_LOSS_MVE: return launch<NT_LOSS_MVE, P>(a, stream);
    case NT_LOSS_EVIDENTIAL: return launch<NT_LOSS_EVIDENTIAL, P>(a, stream);
    default: return launch<NT_LOSS_XENT, P>(a, stream);
  }
}

}  // namespace
}  // namespace nt

extern "C" int64_t nt_task_loss_single_max(void) { return nt::kSingleMax; }

extern "C" int64_t nt_task_loss_workspace(int64_t b, int64_t t) {
  if (!nt::sizes_ok(b, t)) return -1;
  return nt::workspace_bytes_for(b * t);
}

extern "C" int nt_task_loss(const void* preds, int preds_dtype, const float* targets, const uint8_t* mask,
                            const float* sample_weights, const uint8_t* lt_mask, const uint8_t* gt_mask, int64_t b,
                            int64_t t, int64_t c, int kind, float v_kl, float eps, float* loss, void* dpreds,
                            void* workspace, int64_t workspace_bytes, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(preds && targets && loss, NT_EINVAL, "NULL pointer (preds, targets and loss are required)");
  NT_REQUIRE(kind >= NT_LOSS_MSE && kind <= NT_LOSS_XENT, NT_EUNSUPPORTED,
             "unknown kind " + std::to_string(kind) + " (NT_LOSS_MSE .. NT_LOSS_XENT)");
  NT_REQUIRE(preds_dtype == NT_F32 || preds_dtype == NT_BF16, NT_EUNSUPPORTED,
             "preds dtype " + std::to_string(preds_dtype) + " (NT_F32 or NT_BF16)");
  NT_REQUIRE(sizes_ok(b, t) && c >= 1 && c <= INT32_MAX && (b * t == 0 || c <= kMaxElems / (b * t)), NT_EINVAL,
             "bad sizes: b, t >= 0 and c >= 1 with at most 2^40 elements");
  const int64_t want_c = kind == NT_LOSS_MVE ? 2 : kind == NT_LOSS_EVIDENTIAL ? 4 : kind == NT_LOSS_XENT ? c : 1;
  NT_REQUIRE(c == want_c, NT_EINVAL,
             "c = " + std::to_string(c) + " does not fit the kind (it takes c = " + std::to_string(want_c) + ")");
  NT_REQUIRE((!lt_mask && !gt_mask) || kind <= NT_LOSS_RMSE, NT_EINVAL,
             "lt_mask / gt_mask bound NT_LOSS_MSE, NT_LOSS_MAE and NT_LOSS_RMSE only");
  const int64_t n = b * t;
  if (n == 0) return NT_OK;
  const int64_t need = workspace_bytes_for(n);
  NT_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && aligned16(workspace)), NT_EINVAL,
             "workspace missing, misaligned or below nt_task_loss_workspace(b, t) = " + std::to_string(need));
  TaskLossArgs a{};
  a.preds = preds, a.targets = targets, a.mask = mask, a.weights = sample_weights, a.lt = lt_mask, a.gt = gt_mask;
  a.n = n, a.t = t, a.c = (int)c, a.v_kl = v_kl, a.eps = eps, a.loss = loss, a.dpreds = dpreds;
  if (need) {
    char* ws = static_cast<char*>(workspace);
    a.inv_den = reinterpret_cast<float*>(ws);
    a.part_sum = reinterpret_cast<double*>(ws + 16);
    a.part_cnt = reinterpret_cast<long long*>(ws + 16 + 8 * num_parts(n));
  }
  hipStream_t stream = as_stream(stream_);
  return preds_dtype == NT_F32 ? launch_kind<float>(kind, a, stream) : launch_kind<uint16_t>(kind, a, stream);
}
