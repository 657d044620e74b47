// Element losses of nt_task_loss and their derivatives, one (i, j) element at a time, in fp32.
// __host__ __device__: the same text compiles for the host, where it can be checked without a device:
// tests/test_task_loss_host.py builds tests/host/task_loss_host.cpp around this header and holds every kind to
// torch in fp64 (1e-5 per element on loss and gradient) over grids that reach alpha = 1e4, v = 1e-6 .. 1e6,
// |x| = 200 and logits of 1e4.  One point is a convention, not autograd's value: RMSE at x == y has the
// gradient 0, as MAE does, where autograd of sqrt(d^2) gives 0 * inf = NaN.
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

// lgamma(x) - lgamma(x + 1/2) for x > 0.  Below 6 the two lgammaf are small and their difference keeps fp32's
// precision; from 6 on they grow like x ln x while the difference stays near -ln(x) / 2, so it is the series
// -ln(x) / 2 + 1/(8x) - 1/(192 x^3) + 1/(640 x^5) - 17/(14336 x^7), whose error is below 2e-10 there
__host__ __device__ inline float lgamma_half_step(float x) {
  if (x < 6.f) return lgammaf(x) - lgammaf(x + 0.5f);
  const float r = 1.f / x, r2 = r * r;
  return r * (1.f / 8.f - r2 * (1.f / 192.f - r2 * (1.f / 640.f - r2 * (17.f / 14336.f)))) - 0.5f * logf(x);
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
      // (v - d^2) / (2 v^2): the fma rounds v - d^2 once, so it keeps its digits where d^2 is close to v
      store_grad(g + 1, 0.5f * iv * (fmaf(-d, d, v) * iv) * s);
    }
    return 0.5f * d * d * iv + 0.5f * logf(6.283185307179586f * v);
  } else if constexpr (KIND == NT_LOSS_EVIDENTIAL) {
    const float m = load_pred(p), v = load_pred(p + 1), al = load_pred(p + 2), be = load_pred(p + 3);
    const float r = y - m, ar = fabsf(r);
    const float B = 2.f * be * (1.f + v), A = v * r * r + B;
    // The literal forms cancel at large alpha: -al ln B + (al + 1/2) ln A is two terms of size al ln B whose
    // difference is al ln(A / B) + ln(A) / 2, and dL/dv and dL/dbeta hold -al / (1 + v) and -al / be against terms
    // that take them back.  Here ln(A / B) = log1p(v r^2 / B) and the gradients are in the form in which those
    // terms have been cancelled by hand:
    //   dL/dv    = al r^2 / (A (1 + v)) - be / (v A)        dL/dbe = (1 + v) / A - al v r^2 / (be A)
    const float lAB = log1pf(v * r * r / B), lA = logf(A);
    if (g) {
      const float sr = r > 0.f ? 1.f : r < 0.f ? -1.f : r, iA = 1.f / A, a5 = al + 0.5f;
      store_grad(g, (-2.f * a5 * v * r * iA - v_kl * (2.f * v + al) * sr) * s);
      store_grad(g + 1, (al * r * r * iA / (1.f + v) - be * iA / v + 2.f * v_kl * ar) * s);
      store_grad(g + 2, (lAB + (digammaf(al) - digammaf(a5)) + v_kl * ar) * s);
      store_grad(g + 3, ((1.f + v) * iA - al * v * r * r * iA / be) * s);
    }
    const float nll = 0.5f * logf(3.141592653589793f / v) + al * lAB + 0.5f * lA + lgamma_half_step(al);
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
    return ok ? logf(se) + (mx - load_pred(p + cls)) : NAN;  // mx - p[cls] first: exact where the two are close
  }
}

}  // namespace nt
