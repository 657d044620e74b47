// The MLP predictor head (nn/mlp.py) in one launch: y = L_n(act(... act(L_1(x)) ...)), L_i(v) = v W_i^T + b_i,
// up to 8 linear layers: the inference forward, and the training forward (SAVE), which is the same chain and also
// stores every hidden layer's pre-activation z_l (after the bias and, in the bf16 instance, the rounding) for the
// backward of csrc/mlp_head_train.hip.
//
// Work split.  A workgroup (4 waves) owns a tile of R = 16 rows of x, one MFMA row tile: B = 4096 rows are 256
// tiles, one per CU of the chip (R = 32 would leave half of it idle, R = 64 three quarters).  Tiles beyond the
// grid are walked grid-stride.  Inside a layer the waves split the 16-wide output column tiles round-robin (wave
// w takes the tiles w, w + 4, ...), up to kCT = 4 of them at a time on one A fragment, so the 19 tiles of a
// 300-wide layer go 5 / 5 / 5 / 4.
//
// Data movement.  Layer 1 takes its A fragments straight from the rows of x in global memory; every later layer
// takes them from an LDS activation tile that the epilogue of the layer before wrote (bias, rounding, activation
// on the accumulators).  Two tiles ping-pong: layer l reads tile (l - 1) & 1 and writes tile l & 1, one barrier
// per layer, so hidden activations never reach global memory.  The last layer stores to global memory without an
// activation.  W stays in nn.Linear's [out, in] layout: output column n is the k-contiguous row n of W, which is
// the B fragment order of both MFMA shapes, so a lane loads its fragment as one or two 16-byte pieces (by element
// where a row is not 16-byte aligned, and for the piece that crosses the end of a row); the next k step's
// fragments are loaded ahead of the MFMAs of this one.  Every workgroup reads the same W: L2 serves it after
// the first tile.
//
// A k step is 64 bytes of an LDS row in both instances, and a lane's fragment the 16 bytes at 16 (lane >> 4):
//   fp32   16 floats; four v_mfma_f32_16x16x4_f32, the j-th on element j of the lanes' float4 (k is permuted
//          inside the step, for A and B alike); the exact fp32 fma chain
//   bf16   32 bf16; one v_mfma_f32_16x16x32_bf16, fp32 accumulation.  fp32 x and fp32 master parameters are
//          rounded to bf16 as loaded; a layer's output is rounded to bf16 once after the bias, then the
//          activation is applied and rounded, as autocast's nn.Linear and activation modules do.
// LDS rows are padded (32 bytes fp32, 16 bytes bf16) so the 16 rows of a fragment read spread over the banks.
//
// Tails are predicates: rows past B load zeros and are not stored; k past `in` loads zeros on both operands;
// columns past `out` load zero weights and write zeros into the LDS tile up to the next layer's k step, so that
// layer multiplies zeros, never stale LDS.
//
// Limits (nt_mlp_head_supported).  The first layer's `in` comes from global memory: up to 8192.  Every other
// width sits in the two LDS tiles: 2 * 16 rows * (64 ceil(w / 16) + 32) bytes <= 160 KiB = 163840 in fp32, so
// ceil(w / 16) <= 79 and w <= 1264 (1265 takes 164864 bytes).  The bf16 tiles take half of that; one bound
// serves both instances.
#include "mlp_frag.hpp"

#include <algorithm>
#include <type_traits>

#include "../../include/notorch_amd_train.h"

namespace nt {
int cu_count();  // csrc/tile_plan.hip: the current device's CU count, queried once per device
namespace {

struct MlpLayer {
  const void* W;  // [out, in]
  const void* b;  // [out] or NULL
  void* z;        // SAVE: [rows, out] pre-activations of a hidden layer, in the instance's dtype
  int in, out;
};

struct MlpArgs {
  MlpLayer L[kMaxLayers];
  const void* x;
  void* out;
  int64_t rows, x_pitch;
  int nlayers, act;
  float alpha;
  int lds_row;     // bytes of one row of an activation tile
  unsigned x_vec;  // x rows load as 16-byte pieces
  unsigned w_vec;  // bit l: so do the rows of layer l's W
};

// BF: the bf16 instance.  XT / PT: the storage of x and of the parameters (float, or bf16_t in the bf16 instance).
// SAVE: the training forward.
template <bool BF, typename XT, typename PT, bool SAVE>
__global__ __launch_bounds__(kThreads) void mlp_head_kernel(const MlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KS = BF ? 32 : 16;  // elements of a k step
  constexpr int FE = KS / 4;        // elements of a lane's fragment
  using OT = typename std::conditional<BF, bf16_t, float>::type;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;  // A row / B column of the fragment, and its quarter of the k step
  const int64_t ntiles = (a.rows + kRows - 1) / kRows;
  const int tile_bytes = kRows * a.lds_row;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kRows;
    const XT* xrow = r0 + lr < a.rows ? static_cast<const XT*>(a.x) + (r0 + lr) * a.x_pitch : nullptr;

    for (int l = 0; l < a.nlayers; ++l) {
      const PT* W = static_cast<const PT*>(a.L[l].W);
      const PT* bias = static_cast<const PT*>(a.L[l].b);
      const int K = a.L[l].in, N = a.L[l].out;
      const bool first = l == 0, last = l + 1 == a.nlayers;
      const bool wvec = (a.w_vec >> l) & 1u;
      const int KB = (K + KS - 1) / KS;
      const int NT = (N + 15) / 16;
      // column tiles to write: up to the next layer's whole k steps (zeros past N); the last layer's own only
      const int NTW = last ? NT : (N + KS - 1) / KS * (KS / 16);
      // layer l reads tile (l - 1) & 1 == (l + 1) & 1 and writes tile l & 1
      const unsigned char* ain = smem + ((l + 1) & 1) * tile_bytes + lr * a.lds_row + 16 * lq;
      unsigned char* aout = smem + (l & 1) * tile_bytes;

      for (int t0 = wave; t0 < NTW; t0 += kWaves * kCT) {
        // this pass: the tiles t0 + 4 c, c < kCT; the first nact of them hold columns below N (wave-uniform)
        const int nact = t0 < NT ? min(kCT, (NT - t0 + kWaves - 1) / kWaves) : 0;
        const PT* wrow[kCT];
        f32x4 acc[kCT];
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
          const int n = 16 * (t0 + kWaves * c) + lr;
          wrow[c] = n < N ? W + (int64_t)n * K : nullptr;
          acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

        if (nact > 0) {
          uint4 a_next, b_next[kCT];
          a_next = first ? load_frag<BF, XT>(xrow, FE * lq, K, a.x_vec) : *reinterpret_cast<const uint4*>(ain);
#pragma unroll
          for (int c = 0; c < kCT; ++c) b_next[c] = load_frag<BF, PT>(wrow[c], FE * lq, K, wvec);
          for (int kb = 0; kb < KB; ++kb) {
            const uint4 a_cur = a_next;
            uint4 b_cur[kCT];
#pragma unroll
            for (int c = 0; c < kCT; ++c) b_cur[c] = b_next[c];
            if (kb + 1 < KB) {
              const int k = KS * (kb + 1) + FE * lq;
              a_next = first ? load_frag<BF, XT>(xrow, k, K, a.x_vec)
                             : *reinterpret_cast<const uint4*>(ain + 64 * (kb + 1));
#pragma unroll
              for (int c = 0; c < kCT; ++c) b_next[c] = load_frag<BF, PT>(wrow[c], k, K, wvec);
            }
#pragma unroll
            for (int c = 0; c < kCT; ++c)
              if (c < nact) mma<BF>(acc[c], a_cur, b_cur[c]);
          }
        }

        // epilogue (C layout: column lane & 15, rows 4 (lane >> 4) + j): bias, rounding, then the activation into
        // the LDS tile, or the last layer's store
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
          const int t = t0 + kWaves * c;
          if (t >= NTW) continue;
          const int col = 16 * t + lr;
          float bv = col < N && bias != nullptr ? load_param(bias + col) : 0.f;
          if constexpr (BF) bv = rbf(bv);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = 4 * lq + j;
            float v = acc[c][j] + bv;
            if constexpr (BF) v = rbf(v);
            if (last) {
              if (col < N && r0 + row < a.rows) {
                OT* o = static_cast<OT*>(a.out) + (r0 + row) * N + col;
                if constexpr (BF) *o = f2bf(v);
                else *o = v;
              }
            } else {
              if constexpr (SAVE) {
                if (col < N && r0 + row < a.rows) {
                  OT* z = static_cast<OT*>(a.L[l].z) + (r0 + row) * N + col;
                  if constexpr (BF) *z = f2bf(v);
                  else *z = v;
                }
              }
              v = col < N ? act_apply(v, a.act, a.alpha) : 0.f;
              OT* o = reinterpret_cast<OT*>(aout + row * a.lds_row) + col;
              if constexpr (BF) *o = f2bf(v);
              else *o = v;
            }
          }
        }
      }
      __syncthreads();  // the tile this layer wrote is whole; the tile it read is free for the layer after next
    }
  }
}

template <bool BF, typename XT, typename PT, bool SAVE>
int launch(const MlpArgs& a, int grid, size_t lds, hipStream_t stream) {
  auto kern = mlp_head_kernel<BF, XT, PT, SAVE>;
  if (lds > 64 * 1024)
    NT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, kThreads, lds, stream>>>(a);
  NT_LAUNCH_CHECK();
  if (SAVE) set_last_kernel(BF ? "mlp_head_train_bf16" : "mlp_head_train_f32");
  else set_last_kernel(BF ? "mlp_head_bf16" : "mlp_head_f32");
  return NT_OK;
}

template <bool SAVE>
int dispatch(const MlpArgs& a, bool bf, int x_dtype, int param_dtype, int grid, size_t lds, hipStream_t stream) {
  if (!bf) return launch<false, float, float, SAVE>(a, grid, lds, stream);
  if (x_dtype == NT_F32)
    return param_dtype == NT_F32 ? launch<true, float, float, SAVE>(a, grid, lds, stream)
                                 : launch<true, float, bf16_t, SAVE>(a, grid, lds, stream);
  return param_dtype == NT_F32 ? launch<true, bf16_t, float, SAVE>(a, grid, lds, stream)
                               : launch<true, bf16_t, bf16_t, SAVE>(a, grid, lds, stream);
}

}  // namespace
}  // namespace nt

extern "C" int nt_mlp_head_supported(int x_dtype, int param_dtype, int nlayers, const int64_t* dims) {
  using namespace nt;
  if (!dtype_ok(x_dtype) || !dtype_ok(param_dtype) || nlayers < 1 || nlayers > kMaxLayers || dims == nullptr)
    return 0;
  if (dims[0] < 1 || dims[0] > kMaxIn) return 0;
  for (int l = 1; l <= nlayers; ++l)
    if (dims[l] < 1 || dims[l] > kMaxWidth) return 0;
  return 1;
}

namespace nt {
namespace {
// the two forwards' checks and launch; train: the training forward, which fills saved[l] for every hidden layer
int mlp_head_forward(const void* x, int x_dtype, int64_t rows, int64_t x_pitch, int nlayers,
                     const void* const* W, const void* const* b, int param_dtype, const int64_t* dims, int act,
                     float act_alpha, void* out, int out_dtype, bool train, void* const* saved, int saved_dtype,
                     void* stream_) {
  clear_error();
  NT_REQUIRE(x && W && dims && out, NT_EINVAL, "NULL pointer (x, W, dims and out are required)");
  NT_REQUIRE(nlayers >= 1 && nlayers <= kMaxLayers, NT_EINVAL,
             "nlayers " + std::to_string(nlayers) + " (1 to " + std::to_string(kMaxLayers) + ")");
  for (int l = 0; l < nlayers; ++l) NT_REQUIRE(W[l], NT_EINVAL, "NULL pointer (W[" + std::to_string(l) + "])");
  bool positive = rows >= 0;
  for (int l = 0; l <= nlayers; ++l) positive = positive && dims[l] >= 1;
  NT_REQUIRE(positive, NT_EINVAL, "bad sizes: rows >= 0 and every entry of dims >= 1");
  NT_REQUIRE(dtype_ok(x_dtype) && dtype_ok(param_dtype) && dtype_ok(out_dtype), NT_EUNSUPPORTED,
             "dtype (NT_F32 or NT_BF16 for x, the parameters and out)");
  const bool bf = out_dtype == NT_BF16;
  NT_REQUIRE(bf || (x_dtype == NT_F32 && param_dtype == NT_F32), NT_EUNSUPPORTED,
             "dtype: an fp32 out takes fp32 x and fp32 parameters (the bf16 instance writes bf16)");
  NT_REQUIRE(act >= NT_ACT_IDENTITY && act <= NT_ACT_SIGMOID, NT_EINVAL, "act code " + std::to_string(act));
  if (train) {
    NT_REQUIRE(nlayers == 1 || saved, NT_EINVAL, "NULL pointer (saved: one buffer per hidden layer)");
    for (int l = 0; l + 1 < nlayers; ++l)
      NT_REQUIRE(saved[l], NT_EINVAL, "NULL pointer (saved[" + std::to_string(l) + "])");
    NT_REQUIRE(saved_dtype == out_dtype, NT_EUNSUPPORTED, "dtype: saved pre-activations have the dtype of out");
  }
  const int64_t xbytes = x_dtype == NT_BF16 ? 2 : 4, pbytes = param_dtype == NT_BF16 ? 2 : 4;
  NT_REQUIRE(x_pitch >= dims[0], NT_EINVAL,
             "x pitch " + std::to_string(x_pitch) + " below dims[0] = " + std::to_string(dims[0]));
  NT_REQUIRE(x_pitch == dims[0] || x_pitch * xbytes % 16 == 0, NT_EINVAL,
             "x pitch " + std::to_string(x_pitch) + ": padded rows start at multiples of 16 bytes");
  NT_REQUIRE(nt_mlp_head_supported(x_dtype, param_dtype, nlayers, dims), NT_EUNSUPPORTED,
             "widths beyond the limits: dims[0] <= " + std::to_string(kMaxIn) + " and every later width <= " +
                 std::to_string(kMaxWidth) + " (two 16-row activation tiles in 160 KiB of LDS)");
  if (rows == 0) return NT_OK;

  MlpArgs a{};
  int64_t widest = 0;
  for (int l = 0; l < nlayers; ++l) {
    a.L[l] = MlpLayer{W[l], b ? b[l] : nullptr, train && l + 1 < nlayers ? saved[l] : nullptr, (int)dims[l],
                      (int)dims[l + 1]};
    if (aligned16(W[l]) && dims[l] * pbytes % 16 == 0) a.w_vec |= 1u << l;
    if (l + 1 < nlayers && dims[l + 1] > widest) widest = dims[l + 1];
  }
  a.x = x, a.out = out, a.rows = rows, a.x_pitch = x_pitch;
  a.nlayers = nlayers, a.act = act, a.alpha = act_alpha;
  a.x_vec = aligned16(x) && x_pitch * xbytes % 16 == 0;
  a.lds_row = nlayers > 1 ? lds_row_bytes(widest, bf) : 0;
  const size_t lds = (size_t)2 * kRows * a.lds_row;
  // as many workgroups per CU as their tiles leave room for, up to one per SIMD's worth of four
  const int64_t per_cu = lds == 0 ? 4 : std::min<int64_t>(4, std::max<int64_t>(1, kLds / (int64_t)lds));
  const int64_t ntiles = (rows + kRows - 1) / kRows;
  const int cus = cu_count() > 0 ? cu_count() : 256;
  const int grid = (int)std::min<int64_t>(ntiles, per_cu * cus);
  hipStream_t stream = as_stream(stream_);
  return train ? dispatch<true>(a, bf, x_dtype, param_dtype, grid, lds, stream)
               : dispatch<false>(a, bf, x_dtype, param_dtype, grid, lds, stream);
}
}  // namespace
}  // namespace nt

extern "C" int nt_mlp_head_forward(const void* x, int x_dtype, int64_t rows, int64_t x_pitch, int nlayers,
                                   const void* const* W, const void* const* b, int param_dtype, const int64_t* dims,
                                   int act, float act_alpha, void* out, int out_dtype, void* stream) {
  return nt::mlp_head_forward(x, x_dtype, rows, x_pitch, nlayers, W, b, param_dtype, dims, act, act_alpha, out,
                              out_dtype, false, nullptr, 0, stream);
}

extern "C" int nt_mlp_head_forward_train(const void* x, int x_dtype, int64_t rows, int64_t x_pitch, int nlayers,
                                         const void* const* W, const void* const* b, int param_dtype,
                                         const int64_t* dims, int act, float act_alpha, void* out, int out_dtype,
                                         void* const* saved, int saved_dtype, void* stream) {
  return nt::mlp_head_forward(x, x_dtype, rows, x_pitch, nlayers, W, b, param_dtype, dims, act, act_alpha, out,
                              out_dtype, true, saved, saved_dtype, stream);
}
