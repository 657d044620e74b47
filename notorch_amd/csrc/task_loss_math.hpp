// Element losses of nt_task_loss and their derivatives, one (i, j) element at a time, in fp32.
// __host__ __device__: the same text compiles for the host, where it can be checked without a device.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/notorch_amd_train.h"

namespace nt {

// digamma for x > 0 (NaN otherwise): psi(x) = psi(x + k) - sum_{i < k} 1 / (x + i) up to x + k >= 6 (at
// most 6 steps), then ln x - 1/(2x) - 1/(12 x^2) + 1/(120 x^4) - 1/(252 x^6), whose first omitted term is
// 1 / (240 x^8) <= 2.5e-9 there
__host__ __device__ inline float digammaf(float x) {
  if (!(x > 0.f)) return NAN;
  float acc = 0.f;
  for (int i = 0; i < 6 && x < 6.f; ++i) {
    acc += 1.f / x;
    x += 1.f;
  }
  const float r = 1.f / x, r2 = r * r;
  const float series = r2 * (1.f / 12.f - r2 * (1.f / 120.f - r2 * (1.f / 252.f)));
  return (logf(x) - 0.5f * r - series) - acc;
}

// bf16 <-> fp32: widening is exact, narrowing rounds to nearest even (a NaN stays a quiet NaN)
__host__ __device__ inline float bf16_bits_to_float(uint16_t u) {
  union { uint32_t i; float f; } v;
  v.i = (uint32_t)u << 16;
  return v.f;
}
__host__ __device__ inline uint16_t float_to_bf16_bits(float f) {
  union { uint32_t i; float f; } v;
  v.f = f;
  if ((v.i & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((v.i >> 16) | 0x0040u);
  return (uint16_t)((v.i + 0x7fffu + ((v.i >> 16) & 1u)) >> 16);
}

template <typename P>
__host__ __device__ inline float load_pred(const P* p);
template <>
__host__ __device__ inline float load_pred<float>(const float* p) { return *p; }
template <>
__host__ __device__ inline float load_pred<uint16_t>(const uint16_t* p) { return bf16_bits_to_float(*p); }

__host__ __device__ inline void store_grad(float* g, float v) { *g = v; }
__host__ __device__ inline void store_grad(uint16_t* g, float v) { *g = float_to_bf16_bits(v); }

// The loss of one element: p points at its c predictions, y is its target.  With g != nullptr also writes
// g[k] = dL/dp[k] * s for k < c (s: the element's weight in the reduced loss).
template <int KIND, typename P>
__host__ __device__ inline float task_loss_element(const P* p, float y, int c, float v_kl, float eps, bool lt,
                                                   bool gt, float s, P* g) {
  if constexpr (KIND == NT_LOSS_MSE || KIND == NT_LOSS_MAE || KIND == NT_LOSS_RMSE) {
    const float x = load_pred(p);
    const bool clamped = (x < y && lt) || (x > y && gt);
    const float d = clamped ? 0.f : x - y;
    float L, dL;
    if constexpr (KIND == NT_LOSS_MSE) {
      L = d * d, dL = 2.f * d;
    } else {
      L = KIND == NT_LOSS_MAE ? fabsf(d) : sqrtf(d * d);
      dL = d > 0.f ? 1.f : d < 0.f ? -1.f : d;  // d itself at 0 (and for a NaN)
    }
    if (g) store_grad(g, clamped ? 0.f : dL * s);
    return L;
  } else if constexpr (KIND == NT_LOSS_BCE) {
    const float x = load_pred(p);
    const float e = expf(-fabsf(x));
    if (g) {
      const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      store_grad(g, (sig - y) * s);
    }
    return fmaxf(x, 0.f) - x * y + log1pf(e);
  } else if constexpr (KIND == NT_LOSS_MVE) {
    const float m = load_pred(p), v = load_pred(p + 1);
    const float d = m - y, iv = 1.f / v;
    if (g) {
      store_grad(g, d * iv * s);
      store_grad(g + 1, 0.5f * iv * (1.f - d * d * iv) * s);
    }
    return 0.5f * d * d * iv + 0.5f * logf(6.283185307179586f * v);
  } else if constexpr (KIND == NT_LOSS_EVIDENTIAL) {
    const float m = load_pred(p), v = load_pred(p + 1), al = load_pred(p + 2), be = load_pred(p + 3);
    const float r = y - m, ar = fabsf(r);
    const float B = 2.f * be * (1.f + v), A = v * r * r + B;
    const float lB = logf(B), lA = logf(A);
    if (g) {
      const float sr = r > 0.f ? 1.f : r < 0.f ? -1.f : r, iA = 1.f / A, a5 = al + 0.5f;
      store_grad(g, (-2.f * a5 * v * r * iA - v_kl * (2.f * v + al) * sr) * s);
      store_grad(g + 1, (-0.5f / v - al / (1.f + v) + a5 * (r * r + 2.f * be) * iA + 2.f * v_kl * ar) * s);
      store_grad(g + 2, (lA - lB + (digammaf(al) - digammaf(a5)) + v_kl * ar) * s);
      store_grad(g + 3, (-al / be + 2.f * a5 * (1.f + v) * iA) * s);
    }
    const float nll = 0.5f * logf(3.141592653589793f / v) - al * lB + (al + 0.5f) * lA +
                      (lgammaf(al) - lgammaf(al + 0.5f));
    return nll + v_kl * ((2.f * v + al) * ar - eps);
  } else {  // NT_LOSS_XENT
    float mx = load_pred(p);
    for (int k = 1; k < c; ++k) mx = fmaxf(mx, load_pred(p + k));
    float se = 0.f;
    for (int k = 0; k < c; ++k) se += expf(load_pred(p + k) - mx);
    const bool ok = y >= 0.f && y < (float)c;  // false for a NaN
    const int cls = ok ? (int)y : 0;
    if (g) {
      const float ise = 1.f / se;
      for (int k = 0; k < c; ++k)
        store_grad(g + k, ok ? (expf(load_pred(p + k) - mx) * ise - (k == cls ? 1.f : 0.f)) * s : NAN);
    }
    return ok ? (logf(se) + mx) - load_pred(p + cls) : NAN;
  }
}

}  // namespace nt
