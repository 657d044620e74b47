// The boundary between fp32 leaves and the bf16 storage path (mixed precision: an fp32 block under
// torch.autocast(dtype=bfloat16)).  The conversions run inside the kernels that consume the data, so
// no E x h or h x h bf16 copy of an fp32 tensor is written and read back:
//
//   nt_dmpnn_pack_weights_mixed  the bf16 B-fragment images (layout of bf16.hip pack_bf16) of up to 16
//                                h x h weights in fp32 or bf16, of their transposes if asked, and the
//                                bf16 copies of their biases, in ONE launch
//   nt_dmpnn_init_mixed          H0[e] = bf16(Xv[src e] + Xe[e]) from fp32 Xv / Xe (added in fp32, rounded
//                                once), optionally with S[v] = R_{e->v} act(H0[e]) as init_aggregate_bf16
//   nt_dmpnn_init_embed_mixed    the same from fp32 embedding tables and the type indices (bags summed
//                                in fp32 in ascending j): nt_embed_bag (fp32) twice + nt_dmpnn_init_mixed,
//                                bit for bit, with Xv / Xe never written
//   nt_node_scores_mixed         the readout scores of bf16 rows against an fp32 key (Gated's a / a_bias,
//                                SDPAttention's Q), the key rounded as it is loaded: nt_node_scores (bf16)
//                                on the bf16 copy of the key, bit for bit
//   nt_softmax_pool_backward_mixed  the same for nt_softmax_pool_backward: its per-node kernel with the fp32
//                                key; the per-molecule statistics and P are readout.hip's own launches
//
// Every rounding is round-to-nearest-even (v_cvt_pk_bf16_f32), the rounding of torch's .to(bfloat16).
// All kernels of this file are new; no kernel of another translation unit changes.
#include "../../include/notorch_amd_train.h"
#include "bf16.hpp"
#include "readout.hpp"
#include "rows.hpp"

namespace nt {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;  // raw bf16 storage

__device__ __forceinline__ bf16_t f2bf(float x) { return __builtin_bit_cast(bf16_t, (__bf16)x); }
__device__ __forceinline__ float rbf(float x) { return __uint_as_float((unsigned)f2bf(x) << 16); }

// W consecutive fp32 (W = 8: two 16-B loads, W = 4: one, 16-B aligned; W = 1: one element)
template <int W>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, float (&x)[W]) {
  if constexpr (W == 8) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  } else if constexpr (W == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
  } else {
    x[0] = *p;
  }
}

// W consecutive bf16 from fp32 registers (W = 8: one 16-B store, W = 4: one 8-B store), each rounded once
template <int W>
__device__ __forceinline__ void store_bf16(bf16_t* __restrict__ p, const float (&x)[W]) {
  if constexpr (W == 8) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (__bf16)x[i];
    *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, v);
  } else if constexpr (W == 4) {
    bf16x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (__bf16)x[i];
    *reinterpret_cast<uint2*>(p) = __builtin_bit_cast(uint2, v);
  } else {
    *p = f2bf(x[0]);
  }
}

// ------------------------------------------------------------------------------ weight images
constexpr int kMaxLayers = 16;

struct PackArgs {
  const void* W[kMaxLayers];
  uint4* Wp[kMaxLayers];
  uint4* WpT[kMaxLayers];   // NULL: no transpose image
  const void* b[kMaxLayers];  // NULL: no bias
  bf16_t* b16[kMaxLayers];
};

template <bool SRC_BF16>
__device__ __forceinline__ bf16_t weight_elem(const void* W, int64_t i) {
  if constexpr (SRC_BF16) return reinterpret_cast<const bf16_t*>(W)[i];
  else return f2bf(reinterpret_cast<const float*>(W)[i]);
}

// Work items [0, nlayers * nimg * per_layer): one 16-B fragment piece of an image, laid out as
// pack_bf16 (bf16.hip): Wp[ks][nt][lane] = 8 bf16 of M[n][k], n = 16 nt + (lane & 15),
// k = 32 ks + 8 (lane >> 4) + j, zero outside [0, h); M = W (image 0) or W^T (image 1, read from W:
// M[n][k] = W[k][n]).  Work items past them: one bias element each.
template <bool SRC_BF16>
__global__ void __launch_bounds__(256) pack_mixed_kernel(PackArgs a, int nlayers, int nimg, int64_t h,
                                                         int KS, int NTn) {
  const int64_t per_layer = (int64_t)KS * NTn * 64;
  const int64_t nfrag = (int64_t)nlayers * nimg * per_layer;
  const int64_t total = nfrag + (int64_t)nlayers * h;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    if (t >= nfrag) {
      const int64_t r = t - nfrag;
      const int l = (int)(r / h);
      const int64_t c = r - (int64_t)l * h;
      if (a.b[l] != nullptr) a.b16[l][c] = weight_elem<SRC_BF16>(a.b[l], c);
      continue;
    }
    const int64_t li = t / per_layer;
    int64_t r = t - li * per_layer;
    const int l = (int)(li / nimg), img = (int)(li - (int64_t)l * nimg);
    const int lane = (int)(r & 63);
    r >>= 6;
    const int nt = (int)(r % NTn);
    const int ks = (int)(r / NTn);
    const int64_t n = 16 * nt + (lane & 15);
    const int64_t k0 = 32 * ks + 8 * (lane >> 4);
    const void* Wl = a.W[l];
    // image 0: 8 consecutive elements of row n; image 1: column n of rows k0 .. k0 + 7 (lanes 0-15
    // of a fragment read 16 consecutive elements of one row of W)
    const int64_t base = img == 0 ? n * h + k0 : k0 * h + n, step = img == 0 ? 1 : h;
    unsigned short v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = (n < h && k0 + j < h) ? weight_elem<SRC_BF16>(Wl, base + j * step) : (bf16_t)0;
    uint4 o;
    o.x = v[0] | ((unsigned)v[1] << 16);
    o.y = v[2] | ((unsigned)v[3] << 16);
    o.z = v[4] | ((unsigned)v[5] << 16);
    o.w = v[6] | ((unsigned)v[7] << 16);
    (img == 0 ? a.Wp[l] : a.WpT[l])[((int64_t)ks * NTn + nt) * 64 + lane] = o;
  }
}

// ------------------------------------------------------------------------------ init
// init_aggregate_bf16 / init_only_bf16 (bf16.hip) with fp32 loads: one thread per W-element piece of
// a node row walks the node's in-edges in CSR order.
template <int R, int ACT, int W>
__global__ void __launch_bounds__(256) init_aggregate_mixed(
    const float* __restrict__ Xv, const float* __restrict__ Xe, const int64_t* __restrict__ src,
    const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ perm, int64_t V, int64_t h,
    int act, float alpha, bf16_t* __restrict__ H0, bf16_t* __restrict__ S) {
  const int64_t hw = h / W;
  const int64_t total = V * hw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = t / hw, c = (t - v * hw) * W;
    const int32_t b = seg_ptr[v], e = seg_ptr[v + 1];
    Reducer<R> r[W];
#pragma unroll
    for (int i = 0; i < W; ++i) r[i].init();
    for (int32_t j = b; j < e; ++j) {
      const int64_t ed = perm[j];
      float xv[W], xe[W], x[W];
      load_f32<W>(Xv + src[ed] * h + c, xv);
      load_f32<W>(Xe + ed * h + c, xe);
#pragma unroll
      for (int i = 0; i < W; ++i) x[i] = rbf(xv[i] + xe[i]);  // H0 as stored: one rounding
      store_bf16<W>(H0 + ed * h + c, x);
#pragma unroll
      for (int i = 0; i < W; ++i) r[i].push(act_t<ACT>(x[i], act, alpha));
    }
    float y[W];
#pragma unroll
    for (int i = 0; i < W; ++i) y[i] = r[i].result();
    store_bf16<W>(S + v * h + c, y);
  }
}

template <int W>
__global__ void __launch_bounds__(256) init_only_mixed(const float* __restrict__ Xv,
                                                       const float* __restrict__ Xe,
                                                       const int64_t* __restrict__ src, int64_t E,
                                                       int64_t h, bf16_t* __restrict__ H0) {
  const int64_t hw = h / W;
  const int64_t total = E * hw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / hw, c = (t - e * hw) * W;
    float xv[W], xe[W];
    load_f32<W>(Xv + src[e] * h + c, xv);
    load_f32<W>(Xe + e * h + c, xe);
#pragma unroll
    for (int i = 0; i < W; ++i) xv[i] += xe[i];
    store_bf16<W>(H0 + e * h + c, xv);
  }
}

// ------------------------------------------------------------------------------ embedded init
struct EmbedMixedArgs {
  const float* Tv;
  int64_t nv;
  const int64_t* vtypes;
  int64_t kv;
  const float* Te;
  int64_t ne;
  const int64_t* etypes;
  int64_t ke;
};

// one bag in fp32, ascending j from +0.0 (the sum nt_embed_bag stores for an fp32 table)
template <int W>
__device__ __forceinline__ void bag_sum_f32(const float* __restrict__ table, int64_t ntypes,
                                            const int64_t* __restrict__ idx, int64_t k, int64_t h,
                                            int64_t c, float (&x)[W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) x[i] = 0.f;
  for (int64_t j = 0; j < k; ++j) {
    const int64_t t = idx[j];
    if (t < 0 || t >= ntypes) continue;  // validated on the host; never read out of bounds
    float y[W];
    load_f32<W>(table + t * h + c, y);
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] += y[i];
  }
}

// the fp32 sum Xv[src e] + Xe[e] of edge e, column piece c (not yet rounded)
template <int W>
__device__ __forceinline__ void h0_sum(const EmbedMixedArgs& a, const int64_t* __restrict__ src,
                                       int64_t e, int64_t h, int64_t c, float (&x)[W]) {
  float xv[W], xe[W];
  bag_sum_f32<W>(a.Tv, a.nv, a.vtypes + src[e] * a.kv, a.kv, h, c, xv);
  bag_sum_f32<W>(a.Te, a.ne, a.etypes + e * a.ke, a.ke, h, c, xe);
#pragma unroll
  for (int i = 0; i < W; ++i) x[i] = xv[i] + xe[i];
}

template <int R, int ACT, int W>
__global__ void __launch_bounds__(256) init_embed_aggregate_mixed(
    EmbedMixedArgs a, const int64_t* __restrict__ src, const int32_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ perm, int64_t V, int64_t h, int act, float alpha,
    bf16_t* __restrict__ H0, bf16_t* __restrict__ S) {
  const int64_t hw = h / W;
  const int64_t total = V * hw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = t / hw, c = (t - v * hw) * W;
    const int32_t b = seg_ptr[v], en = seg_ptr[v + 1];
    Reducer<R> r[W];
#pragma unroll
    for (int i = 0; i < W; ++i) r[i].init();
    for (int32_t j = b; j < en; ++j) {
      const int64_t e = perm[j];
      float x[W];
      h0_sum<W>(a, src, e, h, c, x);
#pragma unroll
      for (int i = 0; i < W; ++i) x[i] = rbf(x[i]);
      store_bf16<W>(H0 + e * h + c, x);
#pragma unroll
      for (int i = 0; i < W; ++i) r[i].push(act_t<ACT>(x[i], act, alpha));
    }
    float y[W];
#pragma unroll
    for (int i = 0; i < W; ++i) y[i] = r[i].result();
    store_bf16<W>(S + v * h + c, y);
  }
}

template <int W>
__global__ void __launch_bounds__(256) init_embed_only_mixed(EmbedMixedArgs a,
                                                             const int64_t* __restrict__ src, int64_t E,
                                                             int64_t h, bf16_t* __restrict__ H0) {
  const int64_t hw = h / W;
  const int64_t total = E * hw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / hw, c = (t - e * hw) * W;
    float x[W];
    h0_sum<W>(a, src, e, h, c, x);
    store_bf16<W>(H0 + e * h + c, x);
  }
}

// ------------------------------------------------------------------------------ attention readouts
// node_scores_kernel and pool_node_backward_kernel of readout.hip at T = bf16 with the key (Gated's a
// and a_bias, SDPAttention's Q) read from fp32: N key elements (N = 8: two 16-B loads per lane) rounded
// to bf16 as they are loaded.  Everything after the load is those kernels' code (same lane -> column
// map, same fmaf chain, same butterfly), so the bits are theirs on the bf16 copy of the key.
template <bool VEC>
struct KeyPiece {
  static constexpr int N = VEC ? 8 : 1;
  __device__ __forceinline__ static void load(const float* __restrict__ p, float (&y)[N]) {
    load_f32<N>(p, y);
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = rbf(y[i]);
  }
};

template <bool VEC, bool SDPA>
__global__ void __launch_bounds__(256) node_scores_mixed_kernel(
    const bf16_raw* __restrict__ X, const int64_t* __restrict__ node_seg, int64_t n, int64_t h,
    const float* __restrict__ a, const float* __restrict__ a_bias, const float* __restrict__ Q,
    float sqrt_key, float* __restrict__ s) {
  constexpr int N = Piece<bf16_raw, VEC>::N;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = wave; v < n; v += nwaves) {
    const float* q = a;
    if constexpr (SDPA) q = Q + node_seg[v] * h;
    float part = 0.f;
    for (int64_t c = (int64_t)lane * N; c < h; c += 64 * N) {
      float x[N], y[N];
      Piece<bf16_raw, VEC>::load(X + v * h + c, x);
      KeyPiece<VEC>::load(q + c, y);
#pragma unroll
      for (int i = 0; i < N; ++i) part = fmaf(x[i], y[i], part);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) {
      float sc = part;
      if constexpr (SDPA) {
        sc = sc / sqrt_key;
      } else if (a_bias) {
        sc += rbf(*a_bias);
      }
      s[v] = sc;
    }
  }
}

template <bool VEC, bool SDPA>
__global__ void __launch_bounds__(256) pool_node_backward_mixed_kernel(
    const bf16_raw* __restrict__ X, const float* __restrict__ s, const int64_t* __restrict__ node_seg,
    const float* __restrict__ stats, const bf16_raw* __restrict__ dout, int64_t n, int64_t h,
    const float* __restrict__ a, const float* __restrict__ Q, float sqrt_key, bf16_raw* __restrict__ dX,
    float* __restrict__ ds) {
  constexpr int N = Piece<bf16_raw, VEC>::N;
  const int lane = threadIdx.x & 63;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = wave; v < n; v += nwaves) {
    const int64_t g = node_seg[v];
    const float alpha = expf(s[v] - stats[3 * g]) / stats[3 * g + 1];
    float part = 0.f;
    for (int64_t c = (int64_t)lane * N; c < h; c += 64 * N) {
      float x[N], y[N];
      Piece<bf16_raw, VEC>::load(X + v * h + c, x);
      Piece<bf16_raw, VEC>::load(dout + g * h + c, y);
#pragma unroll
      for (int i = 0; i < N; ++i) part = fmaf(x[i], y[i], part);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    const float dsv = alpha * (part - stats[3 * g + 2]);
    for (int64_t c = (int64_t)lane * N; c < h; c += 64 * N) {
      float k[N], y[N], o[N];
      Piece<bf16_raw, VEC>::load(dout + g * h + c, y);
      if constexpr (SDPA) {
        KeyPiece<VEC>::load(Q + g * h + c, k);
#pragma unroll
        for (int i = 0; i < N; ++i) k[i] /= sqrt_key;
      } else {
        KeyPiece<VEC>::load(a + c, k);
      }
#pragma unroll
      for (int i = 0; i < N; ++i) o[i] = fmaf(alpha, y[i], dsv * k[i]);
      Piece<bf16_raw, VEC>::store(dX + v * h + c, o);
    }
    if (lane == 0) ds[v] = dsv;
  }
}

template <bool VEC>
int launch_scores_mixed(const void* X, const int64_t* node_seg, int64_t n, int64_t h, const void* a,
                        const void* a_bias, const void* Q, float sqrt_key, float* s, hipStream_t stream) {
  const int grid = grid_for(n * 64, 256, 256 * 32);
  if (Q)
    node_scores_mixed_kernel<VEC, true><<<grid, 256, 0, stream>>>(
        (const bf16_raw*)X, node_seg, n, h, nullptr, nullptr, (const float*)Q, sqrt_key, s);
  else
    node_scores_mixed_kernel<VEC, false><<<grid, 256, 0, stream>>>(
        (const bf16_raw*)X, nullptr, n, h, (const float*)a, (const float*)a_bias, nullptr, 1.f, s);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

template <bool VEC>
int launch_node_backward_mixed(const void* X, const float* s, const int64_t* node_seg, const float* stats,
                               const void* dout, int64_t n, int64_t h, const void* a, const void* Q,
                               float sqrt_key, void* dX, float* ds, hipStream_t stream) {
  const int grid = grid_for(n * 64, 256, 256 * 32);
  if (Q)
    pool_node_backward_mixed_kernel<VEC, true><<<grid, 256, 0, stream>>>(
        (const bf16_raw*)X, s, node_seg, stats, (const bf16_raw*)dout, n, h, nullptr, (const float*)Q, sqrt_key,
        (bf16_raw*)dX, ds);
  else
    pool_node_backward_mixed_kernel<VEC, false><<<grid, 256, 0, stream>>>(
        (const bf16_raw*)X, s, node_seg, stats, (const bf16_raw*)dout, n, h, (const float*)a, nullptr, 1.f,
        (bf16_raw*)dX, ds);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

#define NT_MX_DISPATCH_A(ACT, LAUNCH)                                          \
  do {                                                                           \
    if ((ACT) == NT_ACT_IDENTITY) { constexpr int A_ = NT_ACT_IDENTITY; LAUNCH; } \
    else if ((ACT) == NT_ACT_RELU) { constexpr int A_ = NT_ACT_RELU; LAUNCH; }    \
    else { constexpr int A_ = -1; LAUNCH; }                                      \
  } while (0)
#define NT_MX_DISPATCH_RA(REDUCE, ACT, LAUNCH)                                            \
  do {                                                                                    \
    switch (REDUCE) {                                                                     \
      case NT_SUM: { constexpr int R_ = NT_SUM; NT_MX_DISPATCH_A(ACT, LAUNCH); } break;   \
      case NT_MEAN: { constexpr int R_ = NT_MEAN; NT_MX_DISPATCH_A(ACT, LAUNCH); } break; \
      case NT_MAX: { constexpr int R_ = NT_MAX; NT_MX_DISPATCH_A(ACT, LAUNCH); } break;   \
      default: { constexpr int R_ = NT_MIN; NT_MX_DISPATCH_A(ACT, LAUNCH); } break;       \
    }                                                                                     \
  } while (0)

}  // namespace
}  // namespace nt

extern "C" int nt_dmpnn_pack_weights_mixed(const void* const* W, int64_t nlayers, int64_t h, int src_dtype,
                                           void* const* Wp, void* const* WpT, const void* const* b,
                                           void* const* b16, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(src_dtype == NT_F32 || src_dtype == NT_BF16, NT_EUNSUPPORTED,
             "src_dtype must be NT_F32 or NT_BF16");
  NT_REQUIRE(nlayers >= 1 && nlayers <= kMaxLayers && h > 0, NT_EINVAL, "bad sizes (1 <= nlayers <= 16, h >= 1)");
  NT_REQUIRE(bf16_update_supported(h), NT_EUNSUPPORTED, NT_BF16_H_RULE);
  NT_REQUIRE(W && Wp, NT_EINVAL, "NULL pointer array");
  NT_REQUIRE((b == nullptr) == (b16 == nullptr), NT_EINVAL, "NULL pointer array: b and b16 go together");
  PackArgs a;
  for (int l = 0; l < kMaxLayers; ++l) {
    a.W[l] = nullptr;
    a.Wp[l] = a.WpT[l] = nullptr;
    a.b[l] = nullptr;
    a.b16[l] = nullptr;
  }
  for (int64_t l = 0; l < nlayers; ++l) {
    NT_REQUIRE(W[l] && Wp[l] && aligned16(Wp[l]) && (WpT == nullptr || (WpT[l] && aligned16(WpT[l]))), NT_EINVAL,
               "NULL or misaligned pointer");
    // a layer without a bias has b[l] == NULL; a bias needs its destination
    NT_REQUIRE(b == nullptr || b[l] == nullptr || b16[l] != nullptr, NT_EINVAL, "NULL pointer: b16 of a given bias");
    a.W[l] = W[l];
    a.Wp[l] = (uint4*)Wp[l];
    a.WpT[l] = WpT ? (uint4*)WpT[l] : nullptr;
    a.b[l] = b ? b[l] : nullptr;
    a.b16[l] = (b && b[l]) ? (bf16_t*)b16[l] : nullptr;
  }
  const int KS = (int)((h + 31) / 32), NTn = (int)((h + 15) / 16);
  const int nimg = WpT ? 2 : 1;
  const int64_t total = nlayers * nimg * (int64_t)KS * NTn * 64 + nlayers * h;
  hipStream_t stream = as_stream(stream_);
  if (src_dtype == NT_BF16)
    pack_mixed_kernel<true><<<grid_for(total, 256), 256, 0, stream>>>(a, (int)nlayers, nimg, h, KS, NTn);
  else
    pack_mixed_kernel<false><<<grid_for(total, 256), 256, 0, stream>>>(a, (int)nlayers, nimg, h, KS, NTn);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

extern "C" int nt_dmpnn_init_mixed(const void* Xv, const void* Xe, const int64_t* src, const int32_t* seg_ptr,
                                   const int32_t* perm, int64_t V, int64_t E, int64_t h, int act,
                                   float act_alpha, int reduce, void* H0, void* S, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(reduce >= NT_SUM && reduce <= NT_MIN, NT_EINVAL, "bad reduce code");
  NT_REQUIRE(act >= NT_ACT_IDENTITY && act <= NT_ACT_SIGMOID, NT_EINVAL, "bad act code");
  NT_REQUIRE(V >= 0 && E >= 0 && h > 0 && E < (int64_t(1) << 31), NT_EINVAL, "bad sizes");
  NT_REQUIRE(bf16_update_supported(h), NT_EUNSUPPORTED, NT_BF16_H_RULE);
  NT_REQUIRE(S == nullptr || (seg_ptr && (perm || E == 0)), NT_EINVAL, "NULL pointer: fused aggregation needs the dst CSR");
  NT_REQUIRE(E == 0 || (Xv && Xe && src && H0), NT_EINVAL, "NULL pointer");
  hipStream_t stream = as_stream(stream_);
  const float* xv = (const float*)Xv;
  const float* xe = (const float*)Xe;
  const int vec = row_piece(h, aligned16(Xv) && aligned16(Xe) && aligned16(H0) && (S == nullptr || aligned16(S)));
  if (S != nullptr) {
    if (V == 0) return NT_OK;
    if (vec == 8) {
      const int grid = grid_for(V * (h / 8), 256, 256 * 32);
      NT_MX_DISPATCH_RA(reduce, act,
                        (init_aggregate_mixed<R_, A_, 8><<<grid, 256, 0, stream>>>(
                            xv, xe, src, seg_ptr, perm, V, h, act, act_alpha, (bf16_t*)H0, (bf16_t*)S)));
    } else if (vec == 4) {
      const int grid = grid_for(V * (h / 4), 256, 256 * 32);
      NT_MX_DISPATCH_RA(reduce, act,
                        (init_aggregate_mixed<R_, A_, 4><<<grid, 256, 0, stream>>>(
                            xv, xe, src, seg_ptr, perm, V, h, act, act_alpha, (bf16_t*)H0, (bf16_t*)S)));
    } else {
      const int grid = grid_for(V * h, 256, 256 * 32);
      NT_MX_DISPATCH_RA(reduce, act,
                        (init_aggregate_mixed<R_, A_, 1><<<grid, 256, 0, stream>>>(
                            xv, xe, src, seg_ptr, perm, V, h, act, act_alpha, (bf16_t*)H0, (bf16_t*)S)));
    }
  } else {
    if (E == 0) return NT_OK;
    if (vec == 8)
      init_only_mixed<8><<<grid_for(E * (h / 8), 256, 256 * 32), 256, 0, stream>>>(xv, xe, src, E, h,
                                                                                  (bf16_t*)H0);
    else if (vec == 4)
      init_only_mixed<4><<<grid_for(E * (h / 4), 256, 256 * 32), 256, 0, stream>>>(xv, xe, src, E, h,
                                                                                  (bf16_t*)H0);
    else
      init_only_mixed<1><<<grid_for(E * h, 256, 256 * 32), 256, 0, stream>>>(xv, xe, src, E, h, (bf16_t*)H0);
  }
  NT_LAUNCH_CHECK();
  return NT_OK;
}

extern "C" int nt_dmpnn_init_embed_mixed(const void* node_table, int64_t num_node_types,
                                         const int64_t* node_types, int64_t kv, const void* edge_table,
                                         int64_t num_edge_types, const int64_t* edge_types, int64_t ke,
                                         const int64_t* src, const int32_t* seg_ptr, const int32_t* perm,
                                         int64_t V, int64_t E, int64_t h, int act, float act_alpha,
                                         int reduce, void* H0, void* S, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(reduce >= NT_SUM && reduce <= NT_MIN, NT_EINVAL, "bad reduce code");
  NT_REQUIRE(act >= NT_ACT_IDENTITY && act <= NT_ACT_SIGMOID, NT_EINVAL, "bad act code");
  NT_REQUIRE(V >= 0 && E >= 0 && h > 0 && E < (int64_t(1) << 31) && kv >= 0 && ke >= 0 &&
                 num_node_types >= 0 && num_edge_types >= 0,
             NT_EINVAL, "bad sizes");
  NT_REQUIRE(bf16_update_supported(h), NT_EUNSUPPORTED, NT_BF16_H_RULE);
  NT_REQUIRE(S == nullptr || (seg_ptr && (perm || E == 0)), NT_EINVAL, "NULL pointer: fused aggregation needs the dst CSR");
  NT_REQUIRE(E == 0 || (node_table && edge_table && src && H0 && (node_types || kv == 0) &&
                        (edge_types || ke == 0)),
             NT_EINVAL, "NULL pointer");
  hipStream_t stream = as_stream(stream_);
  const EmbedMixedArgs a{(const float*)node_table, num_node_types, node_types, kv,
                         (const float*)edge_table, num_edge_types, edge_types, ke};
  const bool vec = h % 8 == 0 && aligned16(node_table) && aligned16(edge_table) && aligned16(H0) &&
                   (S == nullptr || aligned16(S));
  if (S != nullptr) {
    if (V == 0) return NT_OK;
    if (vec) {
      const int grid = grid_for(V * (h / 8), 256, 256 * 32);
      NT_MX_DISPATCH_RA(reduce, act,
                        (init_embed_aggregate_mixed<R_, A_, 8><<<grid, 256, 0, stream>>>(
                            a, src, seg_ptr, perm, V, h, act, act_alpha, (bf16_t*)H0, (bf16_t*)S)));
    } else {
      const int grid = grid_for(V * h, 256, 256 * 32);
      NT_MX_DISPATCH_RA(reduce, act,
                        (init_embed_aggregate_mixed<R_, A_, 1><<<grid, 256, 0, stream>>>(
                            a, src, seg_ptr, perm, V, h, act, act_alpha, (bf16_t*)H0, (bf16_t*)S)));
    }
  } else {
    if (E == 0) return NT_OK;
    if (vec)
      init_embed_only_mixed<8><<<grid_for(E * (h / 8), 256, 256 * 32), 256, 0, stream>>>(a, src, E, h,
                                                                                        (bf16_t*)H0);
    else
      init_embed_only_mixed<1><<<grid_for(E * h, 256, 256 * 32), 256, 0, stream>>>(a, src, E, h, (bf16_t*)H0);
  }
  NT_LAUNCH_CHECK();
  return NT_OK;
}

extern "C" int nt_node_scores_mixed(const void* X, int64_t n, int64_t h, const void* a, const void* a_bias,
                                    const void* Q, const int64_t* node_seg, float sqrt_key, int dtype,
                                    float* scores, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(dtype == NT_BF16, NT_EUNSUPPORTED, "dtype (of X) must be NT_BF16; the keys are fp32");
  NT_REQUIRE(n >= 0 && h > 0, NT_EINVAL, "bad sizes");
  NT_REQUIRE((a == nullptr) != (Q == nullptr), NT_EINVAL, "exactly one of a (Gated) and Q (SDPA)");
  NT_REQUIRE(Q == nullptr || (node_seg && sqrt_key > 0.f), NT_EINVAL, "SDPA needs node_seg, sqrt_key > 0");
  if (n == 0) return NT_OK;
  NT_REQUIRE(X && scores, NT_EINVAL, "NULL pointer");
  hipStream_t stream = as_stream(stream_);
  const bool vec = h % 8 == 0 && aligned16(X) && aligned16(a ? a : Q);
  return vec ? launch_scores_mixed<true>(X, node_seg, n, h, a, a_bias, Q, sqrt_key, scores, stream)
             : launch_scores_mixed<false>(X, node_seg, n, h, a, a_bias, Q, sqrt_key, scores, stream);
}

extern "C" int nt_softmax_pool_backward_mixed(const void* X, const float* scores, const int32_t* seg_ptr,
                                              const int32_t* perm, const int64_t* node_seg, int64_t nseg,
                                              int64_t n, int64_t h, const void* out, const void* dout,
                                              const void* a, const void* Q, float sqrt_key, int dtype,
                                              float* stats, void* dX, float* ds, float* P, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(dtype == NT_BF16, NT_EUNSUPPORTED, "dtype (of X, out, dout, dX) must be NT_BF16; the key is fp32");
  NT_REQUIRE(nseg >= 0 && n >= 0 && h > 0, NT_EINVAL, "bad sizes");
  NT_REQUIRE((a == nullptr) != (Q == nullptr), NT_EINVAL, "exactly one of a (Gated) and Q (SDPA)");
  NT_REQUIRE(Q == nullptr || sqrt_key > 0.f, NT_EINVAL, "SDPA needs sqrt_key > 0");
  if (nseg == 0) return NT_OK;
  NT_REQUIRE(X && scores && seg_ptr && node_seg && out && dout && stats && dX && ds && P, NT_EINVAL,
             "NULL pointer");
  hipStream_t stream = as_stream(stream_);
  const bool vec = h % 8 == 0 && aligned16(X) && aligned16(out) && aligned16(dout) && aligned16(dX) &&
                   aligned16(a ? a : Q);
  // the three launches of nt_softmax_pool_backward; only the per-node kernel reads the key
  int rc = launch_pool_stats_bf16(vec, X, scores, seg_ptr, perm, out, dout, nseg, h, stats, stream);
  if (rc != NT_OK) return rc;
  if (n > 0) {
    rc = vec ? launch_node_backward_mixed<true>(X, scores, node_seg, stats, dout, n, h, a, Q, sqrt_key, dX, ds, stream)
             : launch_node_backward_mixed<false>(X, scores, node_seg, stats, dout, n, h, a, Q, sqrt_key, dX, ds,
                                                 stream);
    if (rc != NT_OK) return rc;
  }
  return launch_weighted_pool_bf16(vec, X, ds, seg_ptr, perm, nseg, h, P, stream);
}
