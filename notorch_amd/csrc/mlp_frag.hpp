// What the fused MLP head's kernels share (csrc/mlp_head.hip: the forward, csrc/mlp_head_train.hip: the backward):
// the 16-row tile constants, bf16 rounding, the 16-byte fragment loader of a k-contiguous row, the MFMA step of
// both instances and the padded LDS row.
#pragma once
#include "common.hpp"

namespace nt {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short bf16_t;  // raw bf16 storage

constexpr int kRows = 16;  // R
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kCT = 4;  // column tiles a wave accumulates on one A fragment
constexpr int kMaxLayers = 8;
constexpr int64_t kLds = 160 * 1024;
constexpr int64_t kMaxIn = 8192, kMaxWidth = 1264;

__device__ __forceinline__ bf16_t f2bf(float x) { return __builtin_bit_cast(bf16_t, (__bf16)x); }
__device__ __forceinline__ float bf2f(bf16_t u) { return __uint_as_float((unsigned)u << 16); }
__device__ __forceinline__ float rbf(float x) { return bf2f(f2bf(x)); }

// bytes of an LDS row that holds w activations: whole 64-byte k steps and the bank padding
inline int lds_row_bytes(int64_t w, bool bf) { return (int)(bf ? (w + 31) / 32 * 64 + 16 : (w + 15) / 16 * 64 + 32); }

// A lane's 16-byte fragment of the k step at k (4 floats, or 8 bf16) from a row of K elements in global memory;
// a NULL row (past the rows of x, or the columns of W) and k past K are zeros.
template <bool BF, typename T>
__device__ __forceinline__ uint4 load_frag(const T* __restrict__ row, int k, int K, bool vec) {
  if (row == nullptr || k >= K) return make_uint4(0u, 0u, 0u, 0u);
  if constexpr (sizeof(T) == 2) {
    if (vec && k + 8 <= K) return *reinterpret_cast<const uint4*>(row + k);
    unsigned v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = k + j < K ? row[k + j] : 0u;
    return make_uint4(v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16, v[6] | v[7] << 16);
  } else {
    constexpr int E = BF ? 8 : 4;
    float v[E];
#pragma unroll
    for (int p = 0; p < E; p += 4) {
      if (vec && k + p + 4 <= K) {
        const float4 f = *reinterpret_cast<const float4*>(row + k + p);
        v[p] = f.x, v[p + 1] = f.y, v[p + 2] = f.z, v[p + 3] = f.w;
      } else {
#pragma unroll
        for (int j = p; j < p + 4; ++j) v[j] = k + j < K ? row[k + j] : 0.f;
      }
    }
    if constexpr (BF) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];
      return __builtin_bit_cast(uint4, o);
    } else {
      return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    }
  }
}

template <bool BF>
__device__ __forceinline__ void mma(f32x4& acc, const uint4& a, const uint4& b) {
  if constexpr (BF) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc,
                                                  0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
}

template <typename T>
__device__ __forceinline__ float load_param(const T* p) {
  if constexpr (sizeof(T) == 2) return bf2f(*p);
  else return *p;
}

inline bool dtype_ok(int d) { return d == NT_F32 || d == NT_BF16; }

}  // namespace
}  // namespace nt
