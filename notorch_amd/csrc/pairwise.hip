// Pairwise p-norm of the rows of A (n x d) against the rows of B (m x d), p in {1, 2}, in the direct
// difference form, and its gradient (nn/loss/rnc.py PNorm; the inputs of RankNContrastLoss):
//   X[i,j]  = s (sum_k |a_i[k] - b_j[k]|^p)^(1/p),  s = -1 with negate
//   dA[i,k] = sum_j w_ij phi(a_i[k] - b_j[k]),      p = 1: phi = sign (sign(0) = 0), w = g
//                                                    p = 2: phi(t) = t, w = g / |X| (0 where X == 0)
// No matrix instruction: the Gram form |a|^2 + |b|^2 - 2ab that would put p = 2 on MFMA is the cancelling
// form this file replaces, and p = 1 has no matrix form.
//
// Forward: one 256-thread workgroup per 128 x 128 tile of X; thread (tx, ty) = (tid & 15, tid >> 4) owns the
// 8 x 8 register tile of rows ty + 16 r and columns tx + 16 c, so for one k a wave reads 4 distinct a values
// (broadcasts) and 16 consecutive b values (conflict-free).  A and B move in k chunks of 16, staged k-major in
// LDS with a row pitch of 132 floats (the transposing stores of a wave then hit 64 distinct banks), in two
// buffers: the next chunk's global loads are issued before the current chunk's arithmetic and stored after
// it, one barrier per chunk.  The k tail and the rows past n / m are zero in LDS.  The sum over k runs in
// ascending k for every (i, j), so |a_i - a_j| and |a_j - a_i| are the same bits and a row against itself is
// exactly 0.  Self mode (B == NULL) computes the tiles J >= I only and writes each off-diagonal tile a second
// time, transposed through LDS, to X[J, I]: X is bitwise symmetric.  All stores go through a 32-row LDS
// buffer and leave as whole 16-byte row pieces when m % 4 == 0 and X is 16-byte aligned, else by element.
//
// Backward: a workgroup owns TI rows x TK columns of dA (64 x 64, or 256 x 16 for d <= 16) with its a values
// in registers, a thread a 4 x 4 (i, k) tile.  It walks j in chunks of 32: w is formed once per pair while it
// is staged (G and X at [i, j], and / or at [j, i], read along i and added in LDS), the b chunk is staged
// beside it, and each thread adds the chunk's sum to its running sum (two levels: the rounding error of a
// long j grows with the chunk count, not with m).  j ascends, there are no atomics, and every order is fixed
// by the shape.  When the tiles are fewer than kSplitBelow, j is split over workgroups that write partial
// sums to the caller's workspace, and a second launch adds them in split order.
#include "../../include/notorch_amd_train.h"
#include "common.hpp"

#include <climits>

namespace nt {
namespace {

constexpr int kTile = 128;             // rows and columns of X per workgroup
constexpr int kKC = 16;                // k chunk
constexpr int kLd = kTile + 4;         // LDS row pitch of a staged chunk (floats)
constexpr int kFwdLds = 2 * 2 * kKC * kLd;  // two buffers of an A and a B chunk (33 KiB)
constexpr int kOutRows = 32;           // rows of X per store pass
constexpr int kLdOut = kTile + 16;     // pitch of the store buffer, direct (ty * 16 + tx: 64 banks)
constexpr int kLdOutT = kTile + 4;     // the same, transposed (tx * 4 + ty: 64 banks)
static_assert(kOutRows * kLdOut <= kFwdLds, "the store buffer reuses the staging memory");

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// 4 consecutive elements of row `row` from column k, widened; 0 past the rows or past d.
// VEC: d % 4 == 0 and a base aligned to 4 elements, so a piece is whole or absent and moves in one load.
template <typename T, bool VEC>
__device__ __forceinline__ float4 load_piece(const T* __restrict__ M, int64_t row, int64_t rows, int64_t d,
                                             int64_t k) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row >= rows || k >= d) return v;
  const T* p = M + row * d + k;
  if constexpr (VEC && sizeof(T) == 4) {
    v = *reinterpret_cast<const float4*>(p);
  } else if constexpr (VEC) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    v = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                    __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
  } else {
    v.x = widen(p[0]);
    if (k + 1 < d) v.y = widen(p[1]);
    if (k + 2 < d) v.z = widen(p[2]);
    if (k + 3 < d) v.w = widen(p[3]);
  }
  return v;
}

// Store 32-row passes of the thread tiles through `buf`: rows orow0.. of X take acc's rows (TR = false) or
// acc's columns (TR = true: the tile lands transposed).  Every thread of the workgroup calls it.
template <bool TR>
__device__ __forceinline__ void store_tile(const float (&acc)[8][8], float* buf, float* __restrict__ X,
                                           int64_t ldx, int64_t orow0, int64_t ocol0, int64_t orows,
                                           int64_t ocols, bool vec) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  constexpr int LD = TR ? kLdOutT : kLdOut;
#pragma unroll
  for (int p = 0; p < kTile / kOutRows; ++p) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (TR) buf[(tx + 16 * h) * LD + ty + 16 * e] = acc[e][2 * p + h];
        else buf[(ty + 16 * h) * LD + tx + 16 * e] = acc[2 * p + h][e];
      }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kOutRows * kTile / 4 / 256; ++u) {
      const int q = tid + 256 * u, rl = q >> 5, pc = (q & 31) * 4;
      const int64_t grow = orow0 + kOutRows * p + rl, gcol = ocol0 + pc;
      if (grow >= orows || gcol >= ocols) continue;
      const float4 v = *reinterpret_cast<const float4*>(buf + rl * LD + pc);
      float* out = X + grow * ldx + gcol;
      if (vec) {
        *reinterpret_cast<float4*>(out) = v;
      } else {
        out[0] = v.x;
        if (gcol + 1 < ocols) out[1] = v.y;
        if (gcol + 2 < ocols) out[2] = v.z;
        if (gcol + 3 < ocols) out[3] = v.w;
      }
    }
    __syncthreads();
  }
}

template <typename T, int P, bool VEC>
__global__ __launch_bounds__(256, 4) void pairwise_fwd_kernel(const T* __restrict__ A, const T* __restrict__ B,
                                                           int64_t n, int64_t m, int64_t d, int tiles_m,
                                                           int self, int negate, int xvec,
                                                           float* __restrict__ X) {
  __shared__ __attribute__((aligned(16))) float lds[kFwdLds];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int I = blockIdx.x / tiles_m, J = blockIdx.x % tiles_m;
  if (self && J < I) return;  // the whole workgroup: written by tile (J, I)
  const int64_t row0 = (int64_t)I * kTile, col0 = (int64_t)J * kTile;

  // staging: a chunk of a tile is 128 rows x 4 pieces; thread pieces q = tid, tid + 256
  float4 pa[2], pb[2];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = tid + 256 * u;
      pa[u] = load_piece<T, VEC>(A, row0 + (q >> 2), n, d, k0 + (q & 3) * 4);
      pb[u] = load_piece<T, VEC>(B, col0 + (q >> 2), m, d, k0 + (q & 3) * 4);
    }
  };
  auto stage = [&](int b) {
    float* as = lds + b * 2 * kKC * kLd;
    float* bs = as + kKC * kLd;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = tid + 256 * u, r = q >> 2, k = (q & 3) * 4;
      as[(k + 0) * kLd + r] = pa[u].x, as[(k + 1) * kLd + r] = pa[u].y;
      as[(k + 2) * kLd + r] = pa[u].z, as[(k + 3) * kLd + r] = pa[u].w;
      bs[(k + 0) * kLd + r] = pb[u].x, bs[(k + 1) * kLd + r] = pb[u].y;
      bs[(k + 2) * kLd + r] = pb[u].z, bs[(k + 3) * kLd + r] = pb[u].w;
    }
  };

  float acc[8][8];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;

  const int chunks = (int)((d + kKC - 1) / kKC);
  fetch(0);
  stage(0);
  __syncthreads();
  for (int ch = 0; ch < chunks; ++ch) {
    const bool more = ch + 1 < chunks;
    if (more) fetch((int64_t)(ch + 1) * kKC);  // in flight across the arithmetic below
    const float* as = lds + (ch & 1) * 2 * kKC * kLd;
    const float* bs = as + kKC * kLd;
#pragma unroll 2
    for (int k = 0; k < kKC; ++k) {
      float a[8], b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[e] = as[k * kLd + ty + 16 * e];
        b[e] = bs[k * kLd + tx + 16 * e];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float t = a[r] - b[c];
          if constexpr (P == 2) acc[r][c] = fmaf(t, t, acc[r][c]);
          else acc[r][c] += fabsf(t);
        }
    }
    // the other buffer was last read before the barrier that ended the previous chunk
    if (more) stage((ch + 1) & 1);
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float v = acc[r][c];
      if constexpr (P == 2) v = sqrtf(v);
      acc[r][c] = negate ? 0.f - v : v;  // 0 stays +0
    }
  store_tile<false>(acc, lds, X, m, row0, col0, n, m, xvec);
  if (self && J > I) store_tile<true>(acc, lds, X, m, col0, row0, m, n, xvec);
}

// ---------------------------------------------------------------------------------------- backward
constexpr int kJC = 32;            // j chunk
constexpr int kLdW = kJC + 4;      // pitch of the staged w rows (16-byte rows)
constexpr int kSplitBelow = 256;   // fewer (row, k) tiles than this: split j over workgroups ...
constexpr int kSplitTarget = 512;  // ... to about this many workgroups (constants: the order is the shape's)

// w of one pair from g and X at the same index
template <int P>
__device__ __forceinline__ float pair_weight(const float* __restrict__ G, const float* __restrict__ X,
                                             int64_t idx) {
  const float g = G[idx];
  if constexpr (P == 1) return g;
  const float x = X[idx];
  return x != 0.f ? g / fabsf(x) : 0.f;
}

template <typename T, int P, int TK, bool VEC>
__global__ __launch_bounds__(256, 3) void pairwise_bwd_kernel(const T* __restrict__ A, const T* __restrict__ B,
                                                           const float* __restrict__ X,
                                                           const float* __restrict__ G, int64_t n, int64_t m,
                                                           int64_t d, int tiles_k, int splits,
                                                           int chunks_per_split, int negate, int use_g,
                                                           int use_gt, float* __restrict__ out) {
  constexpr int KT = TK / 4, RT = 256 / KT, TI = RT * 4;
  __shared__ __attribute__((aligned(16))) float ws[TI * kLdW];
  __shared__ __attribute__((aligned(16))) float bs[kJC * TK];
  const int tid = threadIdx.x, tk = tid % KT, ti = tid / KT;
  int bid = blockIdx.x;
  const int split = bid % splits;
  bid /= splits;
  const int64_t k0 = (int64_t)(bid % tiles_k) * TK, i0 = (int64_t)(bid / tiles_k) * TI;
  const int64_t kk = k0 + tk * 4;

  float4 a[4];
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    a[r] = load_piece<T, VEC>(A, i0 + ti + RT * r, n, d, kk);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  }

  const int chunks = (int)((m + kJC - 1) / kJC);
  const int first = split * chunks_per_split;
  const int last = first + chunks_per_split < chunks ? first + chunks_per_split : chunks;
  for (int ch = first; ch < last; ++ch) {
    const int64_t j0 = (int64_t)ch * kJC;
    // w at [i, j]: a wave reads 32 consecutive j of two rows
#pragma unroll 4
    for (int u = 0; u < TI * kJC / 256; ++u) {
      const int q = tid + 256 * u, ii = q / kJC, jj = q % kJC;
      const int64_t gi = i0 + ii, gj = j0 + jj;
      float w = 0.f;
      if (use_g && gi < n && gj < m) w = pair_weight<P>(G, X, gi * m + gj);
      ws[ii * kLdW + jj] = negate ? -w : w;
    }
    for (int q = tid; q < kJC * KT; q += 256) {
      const int jj = q / KT, kp = (q % KT) * 4;
      *reinterpret_cast<float4*>(bs + jj * TK + kp) = load_piece<T, VEC>(B, j0 + jj, m, d, k0 + kp);
    }
    __syncthreads();
    if (use_gt) {  // w at [j, i] of the m x n matrices, read along i, added to its pair's slot
#pragma unroll 4
      for (int u = 0; u < TI * kJC / 256; ++u) {
        const int q = tid + 256 * u, jj = q / TI, ii = q % TI;
        const int64_t gi = i0 + ii, gj = j0 + jj;
        if (gi < n && gj < m) {
          const float w = pair_weight<P>(G, X, gj * n + gi);
          ws[ii * kLdW + jj] += negate ? -w : w;
        }
      }
      __syncthreads();
    }

    float part[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) part[r][c] = 0.f;
#pragma unroll 1
    for (int jj = 0; jj < kJC; jj += 4) {
      float w[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(ws + (ti + RT * r) * kLdW + jj);
        w[r][0] = v.x, w[r][1] = v.y, w[r][2] = v.z, w[r][3] = v.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float4 bv = *reinterpret_cast<const float4*>(bs + (jj + e) * TK + tk * 4);
        const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float av[4] = {a[r].x, a[r].y, a[r].z, a[r].w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float t = av[c] - b[c];
            if constexpr (P == 2) {
              part[r][c] = fmaf(w[r][e], t, part[r][c]);
            } else {
              const float s = t > 0.f ? w[r][e] : t < 0.f ? -w[r][e] : 0.f;
              part[r][c] += s;
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] += part[r][c];
    __syncthreads();
  }

  float* dst = out + (int64_t)split * n * d;  // split > 0 only with a workspace of splits x n x d
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t gi = i0 + ti + RT * r;
    if (gi >= n || kk >= d) continue;
    float* o = dst + gi * d + kk;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(o) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (kk + c < d) o[c] = acc[r][c];
    }
  }
}

// dA = the partial sums of the j splits, added in split order
__global__ __launch_bounds__(256) void pairwise_combine_kernel(const float* __restrict__ part, int64_t count,
                                                               int splits, float* __restrict__ dA) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
    float v = part[e];
    for (int s = 1; s < splits; ++s) v += part[(int64_t)s * count + e];
    dA[e] = v;
  }
}

struct BwdPlan {
  int tk, tiles_k, splits, chunks_per_split;
  int64_t tiles;  // (row, k) tiles
};

// the shape's plan: the narrow k tile for d <= 16; a j split when the tiles alone leave CUs idle
BwdPlan bwd_plan(int64_t n, int64_t m, int64_t d) {
  BwdPlan p;
  p.tk = d <= 16 ? 16 : 64;
  const int ti = p.tk == 16 ? 256 : 64;
  p.tiles_k = (int)((d + p.tk - 1) / p.tk);
  p.tiles = ((n + ti - 1) / ti) * p.tiles_k;
  const int64_t chunks = (m + kJC - 1) / kJC;
  int64_t splits = 1;
  if (p.tiles < kSplitBelow) splits = (kSplitTarget + p.tiles - 1) / p.tiles;
  if (splits > chunks) splits = chunks;
  p.chunks_per_split = (int)((chunks + splits - 1) / splits);
  p.splits = (int)((chunks + p.chunks_per_split - 1) / p.chunks_per_split);
  return p;
}

const char* kShapeRule = "p must be 1 or 2 and dtype NT_F32 or NT_BF16 (fp32 arithmetic either way)";

bool sizes_ok(int64_t n, int64_t m, int64_t d) {
  const int64_t lim = (int64_t)1 << 40;
  return n >= 0 && m >= 0 && d >= 0 && n < lim && m < lim && d < ((int64_t)1 << 31) &&
         (n == 0 || m < lim / n) && (n == 0 || d == 0 || d < lim / n) && (m == 0 || d == 0 || d < lim / m);
}

template <typename T, int P>
void launch_fwd(const void* A, const void* B, int64_t n, int64_t m, int64_t d, int tiles_m, int64_t blocks,
                int self, int negate, bool vec, bool xvec, float* X, hipStream_t stream) {
  const T* a = static_cast<const T*>(A);
  const T* b = static_cast<const T*>(B);
  if (vec)
    pairwise_fwd_kernel<T, P, true><<<(int)blocks, 256, 0, stream>>>(a, b, n, m, d, tiles_m, self, negate, xvec, X);
  else
    pairwise_fwd_kernel<T, P, false><<<(int)blocks, 256, 0, stream>>>(a, b, n, m, d, tiles_m, self, negate, xvec, X);
}

template <typename T, int P, int TK>
void launch_bwd_tk(const void* A, const void* B, const float* X, const float* G, int64_t n, int64_t m,
                   int64_t d, const BwdPlan& p, int negate, int use_g, int use_gt, bool vec, float* out,
                   hipStream_t stream) {
  const T* a = static_cast<const T*>(A);
  const T* b = static_cast<const T*>(B);
  const int blocks = (int)(p.tiles * p.splits);
  if (vec)
    pairwise_bwd_kernel<T, P, TK, true><<<blocks, 256, 0, stream>>>(
        a, b, X, G, n, m, d, p.tiles_k, p.splits, p.chunks_per_split, negate, use_g, use_gt, out);
  else
    pairwise_bwd_kernel<T, P, TK, false><<<blocks, 256, 0, stream>>>(
        a, b, X, G, n, m, d, p.tiles_k, p.splits, p.chunks_per_split, negate, use_g, use_gt, out);
}

template <typename T, int P>
void launch_bwd(const void* A, const void* B, const float* X, const float* G, int64_t n, int64_t m, int64_t d,
                const BwdPlan& p, int negate, int use_g, int use_gt, bool vec, float* out, hipStream_t stream) {
  if (p.tk == 16) launch_bwd_tk<T, P, 16>(A, B, X, G, n, m, d, p, negate, use_g, use_gt, vec, out, stream);
  else launch_bwd_tk<T, P, 64>(A, B, X, G, n, m, d, p, negate, use_g, use_gt, vec, out, stream);
}

// rows move as whole pieces of 4 elements: d % 4 == 0 and both bases aligned to a piece
bool rows_vec(const void* A, const void* B, int64_t d, int dtype) {
  const uintptr_t mask = dtype == NT_F32 ? 15u : 7u;
  return d % 4 == 0 && ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & mask) == 0;
}

}  // namespace
}  // namespace nt

extern "C" int nt_pairwise_pnorm(const void* A, const void* B, int64_t n, int64_t m, int64_t d, int dtype,
                                 int p, int negate, float* X, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(p == 1 || p == 2, NT_EUNSUPPORTED, std::string("unsupported p: ") + kShapeRule);
  NT_REQUIRE(dtype == NT_F32 || dtype == NT_BF16, NT_EUNSUPPORTED, std::string("unsupported dtype: ") + kShapeRule);
  NT_REQUIRE(A && X, NT_EINVAL, "NULL pointer (A and X are required; B == NULL means B = A)");
  NT_REQUIRE(sizes_ok(n, m, d), NT_EINVAL, "bad sizes: n, m or d < 0, or beyond 2^40 elements");
  NT_REQUIRE(B || n == m, NT_EINVAL, "bad sizes: B == NULL (B = A) needs m == n");
  if (n == 0 || m == 0) return NT_OK;
  const int self = B == nullptr;
  if (self) B = A;
  const int64_t tiles_n = (n + kTile - 1) / kTile, tiles_m = (m + kTile - 1) / kTile;
  NT_REQUIRE(tiles_n * tiles_m <= INT_MAX, NT_EINVAL, "bad sizes: more than 2^31 tiles of 128 x 128");
  const bool vec = rows_vec(A, B, d, dtype), xvec = m % 4 == 0 && aligned16(X);
  hipStream_t stream = as_stream(stream_);
  const int64_t blocks = tiles_n * tiles_m;
  if (dtype == NT_F32) {
    if (p == 2) launch_fwd<float, 2>(A, B, n, m, d, (int)tiles_m, blocks, self, negate, vec, xvec, X, stream);
    else launch_fwd<float, 1>(A, B, n, m, d, (int)tiles_m, blocks, self, negate, vec, xvec, X, stream);
  } else {
    if (p == 2) launch_fwd<uint16_t, 2>(A, B, n, m, d, (int)tiles_m, blocks, self, negate, vec, xvec, X, stream);
    else launch_fwd<uint16_t, 1>(A, B, n, m, d, (int)tiles_m, blocks, self, negate, vec, xvec, X, stream);
  }
  NT_LAUNCH_CHECK();
  return NT_OK;
}

extern "C" int64_t nt_pairwise_pnorm_backward_workspace(int64_t n, int64_t m, int64_t d) {
  using namespace nt;
  if (!sizes_ok(n, m, d)) return -1;
  if (n == 0 || m == 0 || d == 0) return 0;
  const BwdPlan p = bwd_plan(n, m, d);
  return p.splits > 1 ? (int64_t)p.splits * n * d * (int64_t)sizeof(float) : 0;
}

extern "C" int nt_pairwise_pnorm_backward(const void* A, const void* B, const float* X, const float* G,
                                          int64_t n, int64_t m, int64_t d, int dtype, int p, int negate,
                                          int use_g, int use_gt, float* dA, void* workspace,
                                          int64_t workspace_bytes, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(p == 1 || p == 2, NT_EUNSUPPORTED, std::string("unsupported p: ") + kShapeRule);
  NT_REQUIRE(dtype == NT_F32 || dtype == NT_BF16, NT_EUNSUPPORTED, std::string("unsupported dtype: ") + kShapeRule);
  NT_REQUIRE(A && B && G && dA && (X || p == 1), NT_EINVAL,
             "NULL pointer (A, B, G and dA are required, X with p = 2; self mode passes A twice)");
  NT_REQUIRE(sizes_ok(n, m, d), NT_EINVAL, "bad sizes: n, m or d < 0, or beyond 2^40 elements");
  NT_REQUIRE(use_g || use_gt, NT_EINVAL, "neither use_g nor use_gt: no gradient to read");
  NT_REQUIRE(!(use_g && use_gt) || n == m, NT_EINVAL, "bad sizes: use_g with use_gt (G[i,j] + G[j,i]) needs m == n");
  if (n == 0 || m == 0 || d == 0) return NT_OK;  // m == 0: the empty sum is the caller's zero-fill
  const BwdPlan plan = bwd_plan(n, m, d);
  NT_REQUIRE(plan.tiles * plan.splits <= INT_MAX, NT_EINVAL, "bad sizes: more than 2^31 workgroups");
  const int64_t need = plan.splits > 1 ? (int64_t)plan.splits * n * d * (int64_t)sizeof(float) : 0;
  NT_REQUIRE(need == 0 || (workspace && aligned16(workspace) && workspace_bytes >= need), NT_EINVAL,
             "workspace missing, misaligned or shorter than nt_pairwise_pnorm_backward_workspace(n, m, d)");
  const bool split = need > 0;
  float* out = split ? static_cast<float*>(workspace) : dA;
  const bool vec = rows_vec(A, B, d, dtype) && aligned16(out);
  hipStream_t stream = as_stream(stream_);
  if (dtype == NT_F32) {
    if (p == 2) launch_bwd<float, 2>(A, B, X, G, n, m, d, plan, negate, use_g, use_gt, vec, out, stream);
    else launch_bwd<float, 1>(A, B, X, G, n, m, d, plan, negate, use_g, use_gt, vec, out, stream);
  } else {
    if (p == 2) launch_bwd<uint16_t, 2>(A, B, X, G, n, m, d, plan, negate, use_g, use_gt, vec, out, stream);
    else launch_bwd<uint16_t, 1>(A, B, X, G, n, m, d, plan, negate, use_g, use_gt, vec, out, stream);
  }
  NT_LAUNCH_CHECK();
  if (split) {
    const int64_t count = n * d;
    pairwise_combine_kernel<<<grid_for(count, 256), 256, 0, stream>>>(out, count, plan.splits, dA);
    NT_LAUNCH_CHECK();
  }
  return NT_OK;
}
