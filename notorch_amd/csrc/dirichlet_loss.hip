// The Dirichlet loss (notorch/nn/loss/loss.py: Dirichlet), its masked weighted reduction and the gradient of the
// reduced loss, class-parallel: an element has k classes and three special functions per class, so the classes
// are the parallel dimension, where nt_task_loss gives an element to one thread.
//
//   loss   = sum_e L[e] w[e / t] m[e] / den,   den = sum_e m[e]  (or n = b t without a mask)
//   dpreds = dL[e]/dx * (w[e / t] m[e] / den)
// over the n = b t elements e = i t + j; the class and element math is dirichlet_math.hpp.
//
// Groups.  Element e belongs to the W consecutive lanes [e W, (e + 1) W) of the launch ("lane slots"), W the
// smallest power of two >= k, at most 64: a group lies inside one wave and starts at a multiple of W.  Lane l
// of the group evaluates the classes l, l + W, ...: one class when k <= 64, whose a, sigmoid, KL term and
// (a - 1) psi'(a) then stay in registers from the forward sums to the gradient store, so nothing is evaluated
// twice; with k > 64 the lane keeps its first class and re-evaluates the later ones for the gradient.  The five
// sums of an element (DirichletSums) go through an xor-shuffle tree over the group's lanes (offsets W/2 .. 1), after
// which every lane holds them, finishes the element and stores the gradients of its own classes: consecutive
// lanes read and write consecutive logits.
//
// Reduction: task_loss.hip's.  n W <= kSingleSlots (8192): one workgroup of 1024 threads counts the mask
// (integers), so 1 / den is known before the one pass; a group's lane 0 adds L w m into its thread's fp64 partial,
// elements in ascending order, the partials meet in block_sum's fixed tree.  Above: workgroup g of the partial
// launch does the slots [g, g + 1) * 8192 and writes its sum and count to the workspace; one workgroup adds those
// in g order and leaves the loss and 1 / den; the gradient launch re-evaluates the elements with that scale.
#include "dirichlet_math.hpp"

#include "common.hpp"

namespace nt {
namespace {

constexpr int kThreads = 1024;
constexpr int64_t kSingleSlots = 8192;  // lane slots per workgroup: 8 per thread
constexpr int64_t kMaxElems = (int64_t)1 << 40;

enum { kModeSingle = 0, kModePartial = 1, kModeGrad = 2 };

struct DirichletArgs {
  const void* preds;
  const float* targets;
  const uint8_t* mask;
  const float* weights;
  int64_t n, t;
  int k, log2w;
  float v_kl;
  DirichletK kc;
  float* loss;
  void* dpreds;
  float* inv_den;       // workspace: 1 / den (written by the finalize, read by the gradient launch)
  double* part_sum;     // workspace: one per workgroup of the partial launch
  long long* part_cnt;  // workspace: likewise
};

template <typename P>
__global__ __launch_bounds__(kThreads) void dirichlet_loss_kernel(DirichletArgs a, int mode) {
  __shared__ double redd[kThreads / 64];
  __shared__ long long redc[kThreads / 64];
  const int tid = threadIdx.x, W = 1 << a.log2w, lane = tid & (W - 1);
  // this workgroup's elements [lo, hi): kSingleSlots / W of them, the group of thread tid takes lo + tid / W first
  const int64_t per = kSingleSlots >> a.log2w, lo = (int64_t)blockIdx.x * per;
  const int64_t hi = a.n - lo < per ? a.n : lo + per;

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
  // every lane of a group is in range or none is (the slots end at a multiple of W), so the shuffles below only
  // read lanes that run the same trip
  for (int64_t e = lo + (tid >> a.log2w); e < hi; e += kThreads >> a.log2w) {
    const bool on = a.mask == nullptr || a.mask[e] != 0;
    const float m = on ? 1.f : 0.f;
    const float w = a.weights ? a.weights[e / a.t] : 1.f;
    const int cls = dirichlet_target(a.targets[e], a.k);
    const P* x = preds + e * a.k;

    DirichletSums s{};
    DirichletClass first{};
    if (lane < a.k) {
      first = dirichlet_class(load_pred(x + lane), want_grad);
      s.add(first, lane == cls);
    }
    for (int c = lane + W; c < a.k; c += W) s.add(dirichlet_class(load_pred(x + c), false), c == cls);
    for (int o = W >> 1; o >= 1; o >>= 1) {
      s.S += __shfl_xor(s.S, o);
      s.A2 += __shfl_xor(s.A2, o);
      s.E += __shfl_xor(s.E, o);
      s.T += __shfl_xor(s.T, o);
      s.ay += __shfl_xor(s.ay, o);
    }
    const DirichletElement el = dirichlet_finish(s, a.kc, a.v_kl, want_grad);

    if (want_grad) {
      const float scale = w * m * inv;
      P* g = dpreds + e * a.k;
      if (lane < a.k) store_grad(g + lane, cls < 0 ? NAN : dirichlet_grad(first, lane == cls, el, a.v_kl) * scale);
      for (int c = lane + W; c < a.k; c += W)
        store_grad(g + c, cls < 0 ? NAN
                                  : dirichlet_grad(dirichlet_class(load_pred(x + c), true), c == cls, el, a.v_kl) * scale);
    }
    if (lane == 0) {
      acc += (double)(((cls < 0 ? NAN : el.L) * w) * m);
      cnt += on;
    }
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

__global__ __launch_bounds__(kThreads) void dirichlet_loss_finalize_kernel(const double* __restrict__ part_sum,
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

// log2 of the group width: the smallest power of two >= k, at most 64
inline int group_log2(int64_t k) {
  int l = 0;
  while (l < 6 && ((int64_t)1 << l) < k) ++l;
  return l;
}

inline int64_t num_parts(int64_t n, int log2w) {
  const int64_t per = kSingleSlots >> log2w;
  return (n + per - 1) / per;
}

// bytes: 16 (1 / den) + 8 per partial sum + 8 per partial count
inline int64_t workspace_bytes_for(int64_t n, int log2w) {
  return n <= (kSingleSlots >> log2w) ? 0 : 16 + 16 * num_parts(n, log2w);
}

inline bool sizes_ok(int64_t b, int64_t t, int64_t k) {
  return b >= 0 && t >= 0 && b <= kMaxElems && t <= kMaxElems && (b == 0 || t <= kMaxElems / b) && k >= 1 &&
         k <= INT32_MAX && (b * t == 0 || k <= kMaxElems / (b * t));
}

template <typename P>
int launch(const DirichletArgs& a, hipStream_t stream) {
  const int64_t parts = num_parts(a.n, a.log2w);
  if (parts == 1) {
    dirichlet_loss_kernel<P><<<1, kThreads, 0, stream>>>(a, kModeSingle);
    NT_LAUNCH_CHECK();
    return NT_OK;
  }
  dirichlet_loss_kernel<P><<<(unsigned)parts, kThreads, 0, stream>>>(a, kModePartial);
  NT_LAUNCH_CHECK();
  dirichlet_loss_finalize_kernel<<<1, kThreads, 0, stream>>>(a.part_sum, a.part_cnt, parts, a.loss, a.inv_den);
  NT_LAUNCH_CHECK();
  if (a.dpreds) {
    dirichlet_loss_kernel<P><<<(unsigned)parts, kThreads, 0, stream>>>(a, kModeGrad);
    NT_LAUNCH_CHECK();
  }
  return NT_OK;
}

}  // namespace
}  // namespace nt

extern "C" int64_t nt_dirichlet_loss_workspace(int64_t b, int64_t t, int64_t k) {
  if (!nt::sizes_ok(b, t, k)) return -1;
  return nt::workspace_bytes_for(b * t, nt::group_log2(k));
}

extern "C" int nt_dirichlet_loss(const void* preds, int preds_dtype, const float* targets, const uint8_t* mask,
                                 const float* sample_weights, int64_t b, int64_t t, int64_t k, float v_kl,
                                 float* loss, void* dpreds, void* workspace, int64_t workspace_bytes,
                                 void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(preds && targets && loss, NT_EINVAL, "NULL pointer (preds, targets and loss are required)");
  NT_REQUIRE(preds_dtype == NT_F32 || preds_dtype == NT_BF16, NT_EUNSUPPORTED,
             "preds dtype " + std::to_string(preds_dtype) + " (NT_F32 or NT_BF16)");
  NT_REQUIRE(sizes_ok(b, t, k), NT_EINVAL, "bad sizes: b, t >= 0 and k >= 1 with at most 2^40 elements");
  const int64_t n = b * t;
  if (n == 0) return NT_OK;
  const int log2w = group_log2(k);
  const int64_t need = workspace_bytes_for(n, log2w);
  NT_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && aligned16(workspace)), NT_EINVAL,
             "workspace missing, misaligned or below nt_dirichlet_loss_workspace(b, t, k) = " + std::to_string(need));
  DirichletArgs a{};
  a.preds = preds, a.targets = targets, a.mask = mask, a.weights = sample_weights;
  a.n = n, a.t = t, a.k = (int)k, a.log2w = log2w, a.v_kl = v_kl, a.kc = dirichlet_k((int)k);
  a.loss = loss, a.dpreds = dpreds;
  if (need) {
    char* ws = static_cast<char*>(workspace);
    a.inv_den = reinterpret_cast<float*>(ws);
    a.part_sum = reinterpret_cast<double*>(ws + 16);
    a.part_cnt = reinterpret_cast<long long*>(ws + 16 + 8 * num_parts(n, log2w));
  }
  hipStream_t stream = as_stream(stream_);
  return preds_dtype == NT_F32 ? launch<float>(a, stream) : launch<uint16_t>(a, stream);
}
