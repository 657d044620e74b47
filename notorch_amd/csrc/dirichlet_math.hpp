// Element math of nt_dirichlet_loss (nn/loss/loss.py's Dirichlet: Sensoy et al., NeurIPS 2018) and its
// derivative, in fp32, split the way the class-parallel kernel of dirichlet_loss.hip uses it: one class at a
// time (dirichlet_class), five sums over the classes (DirichletSums), the element from the sums
// (dirichlet_finish) and one class's gradient (dirichlet_grad).  dirichlet_element is the same pieces in class
// order.  __host__ __device__: tests/test_dirichlet_host.py builds tests/host/dirichlet_host.cpp around this
// header and holds it to Dirichlet._element and autograd in fp64.
//
// For the logits x[0..k) and the true class y:  a_c = softplus(x_c) + 1,  S = sum a_c,  p_c = a_c / S,
// q = sum p_c^2,  E = sum_{c != y} softplus(x_c),  St = E + k  (the Dirichlet strength without y's evidence)
//   L_mse = (1 - 2 p_y + q) + (1 - q) / (S + 1)
//   KL    = lgamma(St) - lgamma(k) - E psi(St) + sum_{c != y} u(a_c),   u(a) = -lgamma(a) + (a - 1) psi(a)
//   L     = L_mse + v_kl KL
// The literal KL cancels at large a: lgamma(St) and sum u(a_c) each grow like a, KL like k ln St.  From a = 6 on
// a class therefore adds the Stirling series of u(a) without its linear term,
//   u(a) - a = -ln(a)/2 - (1 + ln 2pi)/2 + 1/(3a) + 1/(12a^2) + 1/(90a^3) - 1/(120a^4) - 1/(210a^5) + 1/(252a^6)
// (first omitted term 1/(210 a^7) <= 1.8e-8), and from St = 6 on lgamma(St) - E psi(St) is the series
//   (k - 1/2) ln St - St + ln(2pi)/2 + corr(St) + E r(St),   corr(x) = lgamma(x) - ((x - 1/2) ln x - x + ln(2pi)/2),
// r(x) = ln x - psi(x).  The linear terms meet by hand: -St + sum_{big} a_c = -k - sum_{small} softplus(x_c) +
// n_big, so a big class adds 1 and a small one -softplus(x_c) to its term, and with lgamma(k) written the same way
//   KL = (k - 1/2) log1p(E / k) + corr(St) - corr(k) + E r(St) + sum_{c != y} term_c          (St >= 6)
// in which nothing grows faster than k ln St and everything is 0 when every a_c is 1.  corr(k) comes from the host
// in fp64 (DirichletK).  Below St = 6 (then k < 6 and every class is small) the literal form has nothing to cancel.
//   dL_mse/da_c = 2 (p_c - q) / (S + 1) + 2 p_y / S - (1 - q) / (S + 1)^2 - 2 [c == y] / S
//   dKL/da_c    = (a_c - 1) psi'(a_c) - E psi'(St)  for c != y,  0 for c == y;     da_c/dx_c = sigmoid(x_c)
// A target that is no class (y < 0, y >= k, NaN) makes the loss and all k gradients NaN, as NT_LOSS_XENT does.
#pragma once

#include "task_loss_math.hpp"

namespace nt {

// trigamma for x >= 1: psi'(x) = psi'(x + 1) + 1 / x^2 up to x >= 6 (at most 5 steps), then 1/x + 1/(2x^2) +
// 1/(6x^3) - 1/(30x^5) + 1/(42x^7) - 1/(30x^9), whose first omitted term is 5 / (66 x^11) <= 2.1e-10 there
__host__ __device__ inline float trigammaf(float x) {
  float acc = 0.f;
  for (int i = 0; i < 5 && x < 6.f; ++i) {
    const float r = 1.f / x;
    acc += r * r;
    x += 1.f;
  }
  const float r = 1.f / x, r2 = r * r;
  return r + r2 * (0.5f + r * (1.f / 6.f - r2 * (1.f / 30.f - r2 * (1.f / 42.f - r2 * (1.f / 30.f))))) + acc;
}

// lgamma(x) - ((x - 1/2) ln x - x + ln(2 pi) / 2) for x >= 6: 1/(12x) - 1/(360x^3) + 1/(1260x^5) - 1/(1680x^7)
__host__ __device__ inline float stirling_corr(float x) {
  const float r = 1.f / x, r2 = r * r;
  return r * (1.f / 12.f - r2 * (1.f / 360.f - r2 * (1.f / 1260.f - r2 * (1.f / 1680.f))));
}

// ln(x) - psi(x) for x >= 6, in the series digammaf ends with (the difference itself would cancel):
// 1/(2x) + 1/(12x^2) - 1/(120x^4) + 1/(252x^6)
__host__ __device__ inline float log_minus_digamma(float x) {
  const float r = 1.f / x, r2 = r * r;
  return r * (0.5f + r * (1.f / 12.f - r2 * (1.f / 120.f - r2 * (1.f / 252.f))));
}

// what the element needs of the class count: k, lgamma(k) and corr(k), from fp64
struct DirichletK {
  float k, lgk, corr;
};
__host__ __device__ inline DirichletK dirichlet_k(int k) {
  const double x = (double)k, lg = lgamma(x);
  return DirichletK{(float)k, (float)lg, (float)(lg - ((x - 0.5) * log(x) - x + 0.9189385332046727))};
}

// one class: a, sigmoid(x), its term of the KL sum and (a - 1) psi'(a) (0 without want_grad)
struct DirichletClass {
  float a, sp, sig, term, dpsi;
};
__host__ __device__ inline DirichletClass dirichlet_class(float x, bool want_grad) {
  DirichletClass c;
  const float e = expf(-fabsf(x));
  c.sp = fmaxf(x, 0.f) + log1pf(e);
  c.a = c.sp + 1.f;
  c.sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  if (c.a < 6.f) {
    c.term = c.sp * (digammaf(c.a) - 1.f) - lgammaf(c.a);
  } else {
    const float r = 1.f / c.a;
    const float series =
        r * (1.f / 3.f + r * (1.f / 12.f + r * (1.f / 90.f - r * (1.f / 120.f + r * (1.f / 210.f - r * (1.f / 252.f))))));
    c.term = (series - 0.4189385332046727f) - 0.5f * logf(c.a);
  }
  c.dpsi = want_grad ? c.sp * trigammaf(c.a) : 0.f;
  return c;
}

// the sums over the classes of one element; a lane of the kernel adds its classes, then the lanes are added
struct DirichletSums {
  float S, A2, E, T, ay;  // sum a, sum a^2, and over c != y: sum softplus(x), sum term; a_y
  __host__ __device__ inline void add(const DirichletClass& c, bool is_y) {
    S += c.a;
    A2 += c.a * c.a;
    E += is_y ? 0.f : c.sp;
    T += is_y ? 0.f : c.term;
    ay += is_y ? c.a : 0.f;
  }
};

// the element's loss and what every class's gradient shares
struct DirichletElement {
  float L, iS, q, c1, g0, ekl;  // c1 = 2 / (S + 1), g0 = 2 p_y / S - (1 - q) / (S + 1)^2, ekl = v_kl E psi'(St)
};
__host__ __device__ inline DirichletElement dirichlet_finish(const DirichletSums& s, const DirichletK& kc,
                                                             float v_kl, bool want_grad) {
  DirichletElement o;
  o.iS = 1.f / s.S;
  o.q = s.A2 * o.iS * o.iS;
  const float py = s.ay * o.iS, iS1 = 1.f / (s.S + 1.f);
  const float mse = (1.f - 2.f * py + o.q) + (1.f - o.q) * iS1;
  const float St = s.E + kc.k;
  float kl;
  if (St < 6.f) {
    kl = (lgammaf(St) - kc.lgk) - s.E * digammaf(St) + (s.T + s.E);
  } else {
    kl = (kc.k - 0.5f) * log1pf(s.E / kc.k) + (stirling_corr(St) - kc.corr) + s.E * log_minus_digamma(St) + s.T;
  }
  o.L = mse + v_kl * kl;
  o.c1 = 2.f * iS1;
  o.g0 = 2.f * py * o.iS - (1.f - o.q) * iS1 * iS1;
  o.ekl = want_grad ? v_kl * s.E * trigammaf(St) : 0.f;
  return o;
}

// dL/dx_c of one class
__host__ __device__ inline float dirichlet_grad(const DirichletClass& c, bool is_y, const DirichletElement& o,
                                                float v_kl) {
  const float gm = o.c1 * (c.a * o.iS - o.q) + o.g0;
  return (is_y ? gm - 2.f * o.iS : gm + (v_kl * c.dpsi - o.ekl)) * c.sig;
}

// a target's class, or -1 when it is none (y < 0, y >= k, NaN)
__host__ __device__ inline int dirichlet_target(float y, int k) { return y >= 0.f && y < (float)k ? (int)y : -1; }

// One element in class order: x points at its k logits.  With g != nullptr also writes g[c] = dL/dx[c] * s.
template <typename P>
__host__ __device__ inline float dirichlet_element(const P* x, float y, int k, float v_kl, float s, P* g) {
  const DirichletK kc = dirichlet_k(k);
  const int cls = dirichlet_target(y, k);
  DirichletSums sums{};
  for (int c = 0; c < k; ++c) sums.add(dirichlet_class(load_pred(x + c), false), c == cls);
  const DirichletElement o = dirichlet_finish(sums, kc, v_kl, g != nullptr);
  if (g)
    for (int c = 0; c < k; ++c)
      store_grad(g + c, cls < 0 ? NAN : dirichlet_grad(dirichlet_class(load_pred(x + c), true), c == cls, o, v_kl) * s);
  return cls < 0 ? NAN : o.L;
}

}  // namespace nt
