// Backward of GraphEmbedding's sum-mode EmbeddingBag tables (notorch/nn/gnn/embed.py:20-24,29), the
// reduction the embedded encoder's training step ends in:
//
//   nt_embed_bag_backward  dT[t] = sum_{i, j : idx[i][j] = t} R[i],  R[i] = dX[i]  or, with a CSR,
//                          R[i] = sum_{p in seg i} dX[perm[p]]       (include/notorch_amd_train.h)
//
// The fused encoder calls it twice on G = dL/dH0 (E x h): the edge table without a CSR (idx =
// edge_types), the node table with the src CSR (idx = node_types; R[v] = dXv[v] is formed in registers,
// never written).  n x k indices fall on a few dozen table rows, the worst case of an atomic scatter,
// so nothing here is atomic:
//
//   embed_bwd_partial  one workgroup per contiguous row range [r0, r1) and per chunk of type rows; the
//                      chunk's fp32 partial table lives in LDS; lane = column (c = threadIdx.x, + blockDim
//                      for h > 1024), so every (t, c) address is accumulated by one lane in program
//                      order: ascending i, then ascending j.  No barrier, no LDS atomic.  Rows are
//                      taken kU at a time with every index and row load of the kU issued before the
//                      first LDS update (the row index, the CSR range and the type indices are
//                      wave-uniform: scalar loads).
//   embed_bwd_combine  dT[t][c] = sum_p partial[p][t][c], p ascending within four slices, the four
//                      slice sums added in slice order; rounded once to the table's dtype.
//
// Same inputs -> same bits.  Empty work (n = 0, an empty row range, an empty segment, an unused type)
// leaves zeros in the partial and so in dT.
#include <algorithm>

#include "../../include/notorch_amd_train.h"
#include "rows.hpp"

namespace nt {
namespace {

constexpr int kU = 8;                  // rows in flight per lane
constexpr int kD = 4;                  // CSR entries per row loaded ahead (longer segments loop)
constexpr int kMinRows = 64;           // rows per part at least (small inputs: few partials)
constexpr int64_t kMaxParts = 1024;    // parts at most
constexpr int64_t kPartBytes = 32 << 20;  // ... and about this much workspace for one table
constexpr int kLdsS = 16 * 1024, kLdsM = 52 * 1024, kLdsL = 96 * 1024;  // partial-table instances
constexpr int kMaxThreads = 1024;

__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ inline int64_t mn(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t mx(int64_t a, int64_t b) { return a > b ? a : b; }

// number of row ranges: ceil(n / kMinRows), capped by kMaxParts and by kPartBytes of partial tables
inline int64_t parts_for(int64_t n, int64_t ntypes, int64_t h) {
  const int64_t table = std::max<int64_t>(ntypes * h * 4, 1);
  const int64_t cap = std::min(kMaxParts, std::max<int64_t>(64, kPartBytes / table));
  return std::max<int64_t>(1, std::min(cap, cdiv(n, kMinRows)));
}

template <typename T>
__device__ __forceinline__ float load1(const T* p) {
  float x[1];
  Piece<T, false>::load(p, x);
  return x[0];
}

// K > 0: k known at compile time (the reference featurisation's 7 atom and 2 bond columns); 0: runtime
template <typename T, bool CSR, int K, int LDSB>
__global__ void __launch_bounds__(kMaxThreads) embed_bwd_partial(
    const T* __restrict__ dX, int64_t ld, int64_t n_dx, const int64_t* __restrict__ idx, int64_t n, int64_t k_,
    int64_t ntypes, int64_t h, const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ perm,
    int64_t rows_per_part, int64_t chunk_types, float* __restrict__ partial) {
  __shared__ float tab[LDSB / 4];
  const int64_t k = K > 0 ? K : k_;
  const int64_t t0 = (int64_t)blockIdx.y * chunk_types;
  const int64_t nt = mn(chunk_types, ntypes - t0);  // > 0: the grid has cdiv(ntypes, chunk_types) chunks
  const int64_t r0 = mn((int64_t)blockIdx.x * rows_per_part, n);
  int64_t r1 = mn(r0 + rows_per_part, n);
  if (CSR && n_dx == 0) r1 = r0;  // no rows of dX: every segment is empty (perm may be NULL)
  float* __restrict__ mine = partial + ((int64_t)blockIdx.x * ntypes + t0) * h;
  for (int64_t c = threadIdx.x; c < h; c += blockDim.x) {  // this lane's column: no other lane touches it
    for (int64_t t = 0; t < nt; ++t) tab[t * h + c] = 0.f;
    for (int64_t i = r0; i < r1; i += kU) {
      float r[kU];
      int64_t row[kU];  // clamped: loads stay inside idx / seg_ptr; rows past r1 are masked below
#pragma unroll
      for (int u = 0; u < kU; ++u) row[u] = mn(i + u, r1 - 1);
      if constexpr (!CSR) {
#pragma unroll
        for (int u = 0; u < kU; ++u) r[u] = load1<T>(dX + row[u] * ld + c);
      } else {
        int64_t b[kU], len[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          b[u] = mn(mx((int64_t)seg_ptr[row[u]], 0), n_dx);
          const int64_t e = mn((int64_t)seg_ptr[row[u] + 1], n_dx);
          len[u] = (i + u < r1 && e > b[u]) ? e - b[u] : 0;
        }
        float x[kU][kD];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
#pragma unroll
          for (int d = 0; d < kD; ++d) {  // unconditional loads of clamped entries, masked at the add
            const int64_t p = perm[mn(b[u] + d, n_dx - 1)];
            x[u][d] = load1<T>(dX + mn(mx(p, 0), n_dx - 1) * ld + c);
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          r[u] = 0.f;
#pragma unroll
          for (int d = 0; d < kD; ++d) r[u] += d < len[u] ? x[u][d] : 0.f;
          for (int64_t d = kD; d < len[u]; ++d) {  // hubs: the rest of a long segment, in order
            const int64_t p = perm[b[u] + d];
            r[u] += load1<T>(dX + mn(mx(p, 0), n_dx - 1) * ld + c);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (i + u >= r1) break;
        const int64_t* __restrict__ ti = idx + row[u] * k;
        if constexpr (K > 0) {
          int64_t t[K];
#pragma unroll
          for (int j = 0; j < K; ++j) t[j] = ti[j] - t0;
#pragma unroll
          for (int j = 0; j < K; ++j)
            if (t[j] >= 0 && t[j] < nt) tab[t[j] * h + c] += r[u];  // out of range / another chunk: skipped
        } else {
          for (int64_t j = 0; j < k; ++j) {
            const int64_t t = ti[j] - t0;
            if (t >= 0 && t < nt) tab[t * h + c] += r[u];
          }
        }
      }
    }
    for (int64_t t = 0; t < nt; ++t) mine[t * h + c] = tab[t * h + c];
  }
}

// 64 outputs per workgroup, 4 slices of the parts (one wave each), combined through LDS in slice order
template <typename T>
__global__ void __launch_bounds__(256) embed_bwd_combine(const float* __restrict__ partial, int64_t parts,
                                                         int64_t total, T* __restrict__ out) {
  __shared__ float sm[4][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int64_t o = (int64_t)blockIdx.x * 64 + lane;
  const int64_t per = cdiv(parts, 4);
  const int64_t p0 = mn(s * per, parts), p1 = mn(p0 + per, parts);
  float acc = 0.f;
  if (o < total) {
    int64_t p = p0;
    for (; p + 8 <= p1; p += 8) {
      float x[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = partial[(p + q) * total + o];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc += x[q];
    }
    for (; p < p1; ++p) acc += partial[p * total + o];
  }
  sm[s][lane] = acc;
  __syncthreads();
  if (s == 0 && o < total) {
    const float y[1] = {((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane]};
    Piece<T, false>::store(out + o, y);
  }
}

template <typename T, bool CSR, int K>
int launch_partial(const void* dX, int64_t ld, int64_t n_dx, const int64_t* idx, int64_t n, int64_t k,
                   int64_t ntypes, int64_t h, const int32_t* seg_ptr, const int32_t* perm, int64_t parts,
                   float* partial, hipStream_t stream) {
  const int64_t table = ntypes * h * 4;
  const int lds = table <= kLdsS ? kLdsS : table <= kLdsM ? kLdsM : kLdsL;
  const int64_t chunk_types = std::min(ntypes, (int64_t)lds / (h * 4));  // >= 1: h * 4 <= kLdsL checked
  const int64_t chunks = cdiv(ntypes, chunk_types);
  const int threads = (int)std::min<int64_t>(kMaxThreads, cdiv(h, kWave) * kWave);
  const int64_t rpp = std::max<int64_t>(1, cdiv(n, parts));
  const dim3 grid((unsigned)parts, (unsigned)chunks);
#define NT_EBP(L_)                                                                                        \
  embed_bwd_partial<T, CSR, K, L_><<<grid, threads, 0, stream>>>((const T*)dX, ld, n_dx, idx, n, k, ntypes, h, \
                                                                 seg_ptr, perm, rpp, chunk_types, partial)
  if (lds == kLdsS) NT_EBP(kLdsS);
  else if (lds == kLdsM) NT_EBP(kLdsM);
  else NT_EBP(kLdsL);
#undef NT_EBP
  NT_LAUNCH_CHECK();
  return NT_OK;
}

template <typename T, bool CSR>
int launch_partial_k(const void* dX, int64_t ld, int64_t n_dx, const int64_t* idx, int64_t n, int64_t k,
                     int64_t ntypes, int64_t h, const int32_t* seg_ptr, const int32_t* perm, int64_t parts,
                     float* partial, hipStream_t stream) {
  if (k == 7) return launch_partial<T, CSR, 7>(dX, ld, n_dx, idx, n, k, ntypes, h, seg_ptr, perm, parts, partial, stream);
  if (k == 2) return launch_partial<T, CSR, 2>(dX, ld, n_dx, idx, n, k, ntypes, h, seg_ptr, perm, parts, partial, stream);
  return launch_partial<T, CSR, 0>(dX, ld, n_dx, idx, n, k, ntypes, h, seg_ptr, perm, parts, partial, stream);
}

}  // namespace
}  // namespace nt

extern "C" int64_t nt_embed_bag_backward_workspace(int64_t n, int64_t num_types, int64_t h) {
  if (n < 0 || num_types < 0 || h <= 0) return -1;
  return std::max<int64_t>(16, nt::parts_for(n, num_types, h) * num_types * h * (int64_t)sizeof(float));
}

extern "C" int nt_embed_bag_backward(const void* dX, int64_t ld_dx, int64_t n_dx, const int64_t* idx, int64_t n,
                                     int64_t k, int64_t num_types, int64_t h, const int32_t* seg_ptr,
                                     const int32_t* perm, int dx_dtype, int out_dtype, void* out, void* workspace,
                                     int64_t workspace_bytes, void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE((dx_dtype == NT_F32 || dx_dtype == NT_BF16) && (out_dtype == NT_F32 || out_dtype == NT_BF16),
             NT_EUNSUPPORTED, "dx_dtype and out_dtype must be NT_F32 or NT_BF16");
  NT_REQUIRE(n >= 0 && n_dx >= 0 && k >= 0 && num_types >= 0 && h > 0 && ld_dx >= h &&
                 n < (int64_t(1) << 31) && n_dx < (int64_t(1) << 31),
             NT_EINVAL, "bad sizes");
  NT_REQUIRE(h * 4 <= kLdsL, NT_EUNSUPPORTED, "one fp32 table row must fit the LDS partial (h <= 24576)");
  NT_REQUIRE(cdiv(num_types, std::max<int64_t>(1, kLdsL / (h * 4))) <= 65535, NT_EUNSUPPORTED,
             "too many type chunks for one launch");
  const bool csr = seg_ptr != nullptr;
  NT_REQUIRE(csr || n_dx == n, NT_EINVAL, "bad sizes: without a CSR dX has one row per index row");
  if (num_types == 0) return NT_OK;
  NT_REQUIRE(out && (n == 0 || k == 0 || idx) && (n_dx == 0 || n == 0 || dX) && (!csr || n_dx == 0 || perm),
             NT_EINVAL, "NULL pointer");
  NT_REQUIRE(workspace && aligned16(workspace) &&
                 workspace_bytes >= nt_embed_bag_backward_workspace(n, num_types, h),
             NT_EINVAL, "workspace missing, misaligned or too small (nt_embed_bag_backward_workspace)");
  hipStream_t stream = as_stream(stream_);
  const int64_t parts = parts_for(n, num_types, h);
  float* partial = (float*)workspace;
  int rc;
  if (dx_dtype == NT_F32) {
    rc = csr ? launch_partial_k<float, true>(dX, ld_dx, n_dx, idx, n, k, num_types, h, seg_ptr, perm, parts, partial, stream)
             : launch_partial_k<float, false>(dX, ld_dx, n_dx, idx, n, k, num_types, h, seg_ptr, perm, parts, partial, stream);
  } else {
    rc = csr ? launch_partial_k<bf16_raw, true>(dX, ld_dx, n_dx, idx, n, k, num_types, h, seg_ptr, perm, parts, partial, stream)
             : launch_partial_k<bf16_raw, false>(dX, ld_dx, n_dx, idx, n, k, num_types, h, seg_ptr, perm, parts, partial, stream);
  }
  if (rc != NT_OK) return rc;
  const int64_t total = num_types * h;
  const int64_t grid = cdiv(total, 64);
  NT_REQUIRE(grid < (int64_t(1) << 31), NT_EINVAL, "table too large");
  if (out_dtype == NT_F32)
    embed_bwd_combine<float><<<(unsigned)grid, 256, 0, stream>>>(partial, parts, total, (float*)out);
  else
    embed_bwd_combine<bf16_raw><<<(unsigned)grid, 256, 0, stream>>>(partial, parts, total, (bf16_raw*)out);
  NT_LAUNCH_CHECK();
  return NT_OK;
}
