// Dropout of the layer update fused with its residual add (the training path of
// chemprop.py:26 `update = Sequential(Linear, Dropout(p))` under residual.py:28 `H + module(H)`):
//
//   out[i] = (base ? base[i] : 0) + keep(seed, offset + i) * Y[i] / (1 - p)
//
// keep() is a counter-based hash of (seed, element index): the mask is never stored, the backward
// regenerates it from the same (seed, offset) (dY = keep * G / (1 - p) is this kernel with
// base = NULL).  The hash, the threshold and the scale live in dropout.hpp, shared with the layer
// kernels that apply the same mask in their epilogue (nt_dmpnn_update_fused_dropout); p = 1 drops
// all, out = base, like torch.nn.Dropout(1.0).  HBM-bound: 2-3 rows of traffic per row.
#include "common.hpp"
#include "dropout.hpp"
#include "rows.hpp"

namespace nt {

namespace {

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) dropout_residual_kernel(const T* __restrict__ base,
                                                               const T* __restrict__ Y, int64_t n,
                                                               DropMask m, T* __restrict__ out) {
  using P = Piece<T, VEC>;
  constexpr int N = P::N;
  const int64_t pieces = n / N;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < pieces;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = t * N;
    float y[N], b[N];
    P::load(Y + i0, y);
    if (base) P::load(base + i0, b);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float v = drop_apply(m, (uint64_t)(i0 + k), y[k]);
      y[k] = base ? b[k] + v : v;
    }
    P::store(out + i0, y);
  }
}

template <typename T>
void launch_dropout(const void* base, const void* Y, int64_t n, float p, uint64_t seed,
                    uint64_t offset, void* out, hipStream_t stream) {
  const DropMask m = drop_mask(p, seed, offset);
  constexpr int NV = 16 / sizeof(T);
  const bool vec = n % NV == 0 && aligned16(Y) && aligned16(out) && (!base || aligned16(base));
  const int grid = grid_for(vec ? n / NV : n, 256, 256 * 32);
  if (vec)
    dropout_residual_kernel<T, true><<<grid, 256, 0, stream>>>(
        (const T*)base, (const T*)Y, n, m, (T*)out);
  else
    dropout_residual_kernel<T, false><<<grid, 256, 0, stream>>>(
        (const T*)base, (const T*)Y, n, m, (T*)out);
}

}  // namespace

}  // namespace nt

using namespace nt;

extern "C" int nt_dropout_residual(const void* base, const void* Y, int64_t n, float p,
                                   uint64_t seed, uint64_t offset, int dtype, void* out,
                                   void* stream_) {
  clear_error();
  NT_REQUIRE(dtype == NT_F32 || dtype == NT_BF16, NT_EUNSUPPORTED, "dtype must be NT_F32 or NT_BF16");
  NT_REQUIRE(n >= 0, NT_EINVAL, "bad sizes");
  NT_REQUIRE(p >= 0.f && p <= 1.f, NT_EINVAL, "dropout probability must be in [0, 1]");
  if (n == 0) return NT_OK;
  NT_REQUIRE(Y && out, NT_EINVAL, "NULL pointer");
  hipStream_t stream = as_stream(stream_);
  if (dtype == NT_BF16)
    launch_dropout<bf16_raw>(base, Y, n, p, seed, offset, out, stream);
  else
    launch_dropout<float>(base, Y, n, p, seed, offset, out, stream);
  NT_LAUNCH_CHECK();
  return NT_OK;
}
