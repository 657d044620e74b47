// The dropout mask shared by nt_dropout_residual (dropout.hip) and the layer kernels that apply it in
// their epilogue (nt_dmpnn_update_fused_dropout: update_fk.hpp, bf16.hip).  keep() is a counter-based
// hash of (seed, element index): the splitmix64 finaliser of seed + (i + 1) * golden-ratio; an element
// is kept when its top 32 bits are >= p * 2^32, i.e. with probability 1 - p (p = 1 drops all, like
// torch.nn.Dropout(1.0)).  The mask is never stored: every kernel that needs it regenerates it from
// (seed, offset + dense element index), so all of them must take the decision from this header.
#pragma once

#include <stdint.h>

#include "common.hpp"

namespace nt {

__device__ __forceinline__ uint32_t drop_hash(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}

// launch constants of one dropout (p, seed, offset), computed on the host
struct DropMask {
  uint64_t seed = 0, offset = 0;
  uint32_t thr = 0;   // keep when drop_hash >= thr
  int drop_all = 0;   // p >= 1
  float scale = 1.f;  // 1 / (1 - p) (0 when everything is dropped)
};

inline DropMask drop_mask(float p, uint64_t seed, uint64_t offset) {
  DropMask m;
  m.seed = seed;
  m.offset = offset;
  m.drop_all = p >= 1.f;
  const double t = (double)p * 4294967296.0;
  m.thr = m.drop_all ? 0u : (uint32_t)(t >= 4294967295.0 ? 4294967295.0 : t);
  m.scale = m.drop_all ? 0.f : 1.f / (1.f - p);
  return m;
}

// the mask's decision for dense element index i (offset added here)
__device__ __forceinline__ bool drop_keep(const DropMask& m, uint64_t i) {
  return !m.drop_all && drop_hash(m.seed, m.offset + i) >= m.thr;
}

// keep(i) * y / (1 - p)
__device__ __forceinline__ float drop_apply(const DropMask& m, uint64_t i, float y) {
  return drop_keep(m, i) ? y * m.scale : 0.f;
}

}  // namespace nt
