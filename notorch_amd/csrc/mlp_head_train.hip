// Backward of the fused MLP head (csrc/mlp_head.hip holds the forward and its training variant, which saves every
// hidden layer's pre-activation z_l): dx, every dW_l and every db_l in at most three launches, whatever the depth.
// Layer l is L_l(v) = v W_l^T + b_l, W_l of [out_l, in_l]; a_l = act(z_l) is recomputed from the saved z_l, so one
// backward serves every NT_ACT_* code.
//
// Launch 1, the dX chain (mlp_head_dx_kernel).  The forward's split: a workgroup (4 waves) owns 16 rows, and the
// gradient of those rows stays in two ping-pong LDS tiles from layer to layer.  dZ_n = dY comes from global memory
// as the A fragments of the top layer; then, for l = n ... 2, dA_{l-1} = dZ_l W_l on MFMA, and the epilogue turns the
// accumulators into dZ_{l-1} = dA_{l-1} act'(z_{l-1}) (z from the saved buffer), writes it to the next LDS tile and
// to the global dZ workspace that launch 2 reads.  Last, dX = dZ_1 W_1 goes straight to global memory (the step is
// left out when dx is NULL).  One barrier per layer.
//   The B operand.  Here k runs over `out`, the slow axis of nn.Linear's [out, in] layout, and the output column n
//   over `in`, the contiguous one: the forward's "row n of W is the B fragment" does not hold.  W is read in place,
//   one element per (k, n): at a fixed k the 16 column lanes of a fragment read 16 consecutive elements of row k of
//   W, a 64-byte run (32 bytes for bf16 parameters).  fp32: the j-th v_mfma_f32_16x16x4_f32 of a k step takes
//   k = 16 kb + 4 (lane >> 4) + j, so a k step is four such loads per column tile and no shuffle.  bf16: a lane's
//   fragment of v_mfma_f32_16x16x32_bf16 is 8 consecutive k, so eight loads per column tile and k step, rounded to bf16 and
//   packed in registers.  Why not an LDS transpose of W k-slabs: every workgroup reads the same W, at most
//   1264 x 1264 and 300 x 300 at the head's sizes, so after the first tile the loads are L2 hits in whole 64-byte
//   runs; a slab staged through LDS would add two barriers per slab to a kernel whose whole layer has one, and the
//   LDS is taken by the gradient tiles at the width bound.  No packing launch of W^T.  The next k step's fragments
//   are loaded ahead of this one's MFMAs, as in the forward.
//
// Launch 2, every weight and bias gradient (mlp_head_wgrad_kernel): dW_l = dZ_l^T A_{l-1}, db_l = sum_rows dZ_l,
// A_0 = x, A_l = act(z_l).  One work list of (layer, 64 x 64 tile of dW, row chunk) items, one workgroup each, so a
// two-layer head fills the chip in one launch.  k is the row index, the slow axis of both operands, so a workgroup
// stages a k step (16 rows fp32, 32 rows bf16) of its 64 dZ columns and its 64 A columns through LDS transposed:
// global reads run along the columns (256-byte runs), the LDS stores put column c's k step into 64 contiguous bytes
// (pitch 80: the 16 columns of a fragment read fall on distinct banks), the activation is applied once per element
// on the way, and the fragments are then the forward's 16-byte LDS reads.  Wave w owns the 16 dW rows 16 w ... of
// the tile and four column tiles on one A fragment.  Two staging buffers, one barrier per k step.  The 64 threads
// of wave 0 sum the staged dZ columns for db (in the tiles of the first tile column).  fp32: v_mfma_f32_16x16x4_f32;
// bf16: v_mfma_f32_16x16x32_bf16 on bf16 dZ / A with fp32 accumulation.
//   Split-K.  Rows are cut into chunks (chunk_rule: at least 128 rows, at most 64 chunks, a multiple of 32).  One
//   chunk: the tile is written as dW / db in the parameters' dtype.  More: fp32 partials per chunk in the
//   workspace, and launch 3 (mlp_head_reduce_kernel) adds them in chunk order and writes dW / db, from fp32, in the
//   parameters' dtype.  No atomics: two calls give the same bits.
//
// bf16 instance (the head under bf16 autocast): dY, the saved z and dZ are bf16; dA is rounded to bf16 and so is
// dZ = dA act'(z), where autocast's modules round; W, x and fp32 parameters are rounded as loaded.  dx is written
// in x's dtype from the fp32 accumulators (rounded once when x is bf16).
//
// Tails are predicates everywhere: rows past B, k past `out` (chain) or the chunk's rows (wgrad) and columns past a
// width load zeros and are not stored; the chain writes zeros into the LDS tile up to the next step's k step.  W,
// x, dZ and z load by element in the staging and the B fragments, so no alignment is asked of them; dY loads as
// 16-byte pieces where its rows allow and by element otherwise.
//
// Limits (nt_mlp_head_train_supported).  The chain keeps dZ of the hidden layers in the two 16-row tiles the
// forward keeps their activations in: 2 * 16 * (64 ceil(w / 16) + 32) bytes <= 160 KiB, w <= 1264 (1265 takes
// 164864 bytes); the bf16 tiles take half.  The weight gradient's staging is 20 KiB whatever the widths.  dims[0]
// is read from and written to global memory only: up to 8192, as in the forward, whose limits these are.
#include "mlp_frag.hpp"

#include <algorithm>
#include <type_traits>

#include "../../include/notorch_amd_train.h"

namespace nt {
int cu_count();  // csrc/tile_plan.hip
namespace {

constexpr int64_t kChunkRows = 128;  // the smallest row chunk of the weight-gradient split
constexpr int64_t kMaxChunks = 64;
constexpr int kTile = 64;   // the weight gradient's workgroup tile: 64 x 64 of dW
constexpr int kPitch = 80;  // bytes between staged columns: a 64-byte k step and 16 of padding
constexpr int kStage = kTile * kPitch;

struct BwdLayer {
  const void* W;   // [out, in]
  const void* z;   // saved pre-activation of the layer below, [rows, in]; NULL for layer 0
  void* dz;        // dZ of the layer below, [rows, in]; NULL for layer 0
  int in, out;
};

struct ChainArgs {
  BwdLayer L[kMaxLayers];
  const void* dy;  // [rows, out of the top layer]
  void* dx;        // [rows, in of layer 0]; the chain stops above layer 0 without it
  int64_t rows;
  int nlayers, stop, act;  // stop: the lowest layer whose step runs
  float alpha;
  int lds_row;
  unsigned dy_vec;
};

// A lane's fragment of the k step at k from column `col` of a [K, ld] matrix: elements (k + j, col), j < 4 or 8,
// each ld apart (at a fixed j the 16 column lanes read a contiguous run).  A NULL column and k past K are zeros.
template <bool BF, typename PT>
__device__ __forceinline__ uint4 load_frag_t(const PT* __restrict__ col, int k, int K, int64_t ld) {
  constexpr int E = BF ? 8 : 4;
  float v[E];
#pragma unroll
  for (int j = 0; j < E; ++j) v[j] = col != nullptr && k + j < K ? load_param(col + (int64_t)(k + j) * ld) : 0.f;
  if constexpr (BF) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)v[j];
    return __builtin_bit_cast(uint4, o);
  } else {
    return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
  }
}

template <typename T>
__device__ __forceinline__ void store_as(T* p, float v) {
  if constexpr (sizeof(T) == 2) *p = f2bf(v);
  else *p = v;
}

// BF: the bf16 instance.  XT / PT: the storage of dx and of the parameters.
template <bool BF, typename XT, typename PT>
__global__ __launch_bounds__(kThreads) void mlp_head_dx_kernel(const ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KS = BF ? 32 : 16;
  constexpr int FE = KS / 4;
  using T = typename std::conditional<BF, bf16_t, float>::type;  // dY, z, dZ
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int64_t ntiles = (a.rows + kRows - 1) / kRows;
  const int tile_bytes = kRows * a.lds_row;
  const int NY = a.L[a.nlayers - 1].out;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kRows;
    const T* dyrow = r0 + lr < a.rows ? static_cast<const T*>(a.dy) + (r0 + lr) * NY : nullptr;

    for (int l = a.nlayers - 1, s = 0; l >= a.stop; --l, ++s) {
      const PT* W = static_cast<const PT*>(a.L[l].W);
      const T* zsav = static_cast<const T*>(a.L[l].z);
      T* dzg = static_cast<T*>(a.L[l].dz);
      const int K = a.L[l].out, N = a.L[l].in;
      const bool first = s == 0, last = l == 0;
      const int KB = (K + KS - 1) / KS;
      const int NT = (N + 15) / 16;
      // column tiles to write: up to the next step's whole k steps (zeros past N); dx's own only
      const int NTW = last ? NT : (N + KS - 1) / KS * (KS / 16);
      // step s reads tile (s + 1) & 1 and writes tile s & 1
      const unsigned char* ain = smem + ((s + 1) & 1) * tile_bytes + lr * a.lds_row + 16 * lq;
      unsigned char* aout = smem + (s & 1) * tile_bytes;

      for (int t0 = wave; t0 < NTW; t0 += kWaves * kCT) {
        const int nact = t0 < NT ? min(kCT, (NT - t0 + kWaves - 1) / kWaves) : 0;
        const PT* wcol[kCT];
        f32x4 acc[kCT];
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
          const int n = 16 * (t0 + kWaves * c) + lr;
          wcol[c] = n < N ? W + n : nullptr;
          acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

        if (nact > 0) {
          uint4 a_next, b_next[kCT];
          a_next = first ? load_frag<BF, T>(dyrow, FE * lq, K, a.dy_vec) : *reinterpret_cast<const uint4*>(ain);
#pragma unroll
          for (int c = 0; c < kCT; ++c) b_next[c] = load_frag_t<BF, PT>(wcol[c], FE * lq, K, N);
          for (int kb = 0; kb < KB; ++kb) {
            const uint4 a_cur = a_next;
            uint4 b_cur[kCT];
#pragma unroll
            for (int c = 0; c < kCT; ++c) b_cur[c] = b_next[c];
            if (kb + 1 < KB) {
              const int k = KS * (kb + 1) + FE * lq;
              a_next = first ? load_frag<BF, T>(dyrow, k, K, a.dy_vec)
                             : *reinterpret_cast<const uint4*>(ain + 64 * (kb + 1));
#pragma unroll
              for (int c = 0; c < kCT; ++c) b_next[c] = load_frag_t<BF, PT>(wcol[c], k, K, N);
            }
#pragma unroll
            for (int c = 0; c < kCT; ++c)
              if (c < nact) mma<BF>(acc[c], a_cur, b_cur[c]);
          }
        }

        // epilogue (C layout: column lane & 15, rows 4 (lane >> 4) + j): dx to global memory, or
        // dZ = dA act'(z) to the LDS tile and the dZ workspace
#pragma unroll
        for (int c = 0; c < kCT; ++c) {
          const int t = t0 + kWaves * c;
          if (t >= NTW) continue;
          const int col = 16 * t + lr;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = 4 * lq + j;
            const bool live = col < N && r0 + row < a.rows;
            float v = acc[c][j];
            if (last) {
              if (live) store_as(static_cast<XT*>(a.dx) + (r0 + row) * N + col, v);
            } else {
              float g = 0.f;
              if (live) {
                const int64_t at = (r0 + row) * N + col;
                if constexpr (BF) v = rbf(v);
                g = v * act_grad(load_param(zsav + at), a.act, a.alpha);
                if constexpr (BF) g = rbf(g);
                store_as(dzg + at, g);
              }
              store_as(reinterpret_cast<T*>(aout + row * a.lds_row) + col, g);
            }
          }
        }
      }
      __syncthreads();  // the tile this step wrote is whole; the tile it read is free for the step after next
    }
  }
}

struct WgLayer {
  const void* dz;  // [rows, out]: dY for the top layer, else the chain's dZ workspace
  const void* a;   // [rows, in], rows a_pitch apart: x for layer 0, else the saved z of the layer below
  void* dW;        // [out, in]
  void* db;        // [out] or NULL
  float* pW;       // nchunks x [out, in] partials (nchunks > 1)
  float* pb;       // nchunks x [out]
  int64_t a_pitch;
  int in, out;
  int item0;    // the layer's first work item
  int tiles_i;  // 64-column tiles across `in`
};

struct WgArgs {
  WgLayer L[kMaxLayers];
  int64_t rows, chunk_rows;
  int nlayers, nchunks, act;
  float alpha;
  int param_bf16;
  int64_t total;  // reduce: elements of every dW and db together
};

__device__ __forceinline__ void store_param(void* base, int64_t at, float v, bool bf) {
  if (bf) static_cast<bf16_t*>(base)[at] = f2bf(v);
  else static_cast<float*>(base)[at] = v;
}

// One k step (rows k0 ... k0 + KS, below `re`) of 64 columns from c0 of a [rows, width] matrix, transposed into
// `dst`: column c's k step at dst + c * kPitch.  ACT: the activation (and, in the bf16 instance, its rounding) on
// the way.  Thread t takes column t & 63 of the rows (t >> 6) + 4 j.
template <bool BF, typename ST, bool ACT>
__device__ __forceinline__ void stage(unsigned char* dst, const ST* __restrict__ src, int64_t pitch, int width, int c0,
                                      int64_t k0, int64_t re, int act, float alpha) {
  constexpr int KS = BF ? 32 : 16;
  using T = typename std::conditional<BF, bf16_t, float>::type;
  const int c = threadIdx.x & 63;
  const bool col_ok = c0 + c < width;
  T* out = reinterpret_cast<T*>(dst + c * kPitch);
#pragma unroll
  for (int j = 0; j < KS / 4; ++j) {
    const int rr = (threadIdx.x >> 6) + 4 * j;
    float v = 0.f;
    if (col_ok && k0 + rr < re) {
      v = load_param(src + (k0 + rr) * pitch + c0 + c);
      if constexpr (ACT) v = act_apply(v, act, alpha);
    }
    store_as(out + rr, v);
  }
}

// BF: the bf16 instance.  XT: the storage of x.
template <bool BF, typename XT>
__global__ __launch_bounds__(kThreads) void mlp_head_wgrad_kernel(const WgArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char sm[2][2][kStage];  // [buffer][dZ, A]
  constexpr int KS = BF ? 32 : 16;
  using T = typename std::conditional<BF, bf16_t, float>::type;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;

  int l = a.nlayers - 1;
  while (l > 0 && (int)blockIdx.x < a.L[l].item0) --l;
  const WgLayer& L = a.L[l];
  const int idx = (int)blockIdx.x - L.item0;
  const int chunk = idx % a.nchunks, tile = idx / a.nchunks;
  const int o0 = kTile * (tile / L.tiles_i), i0 = kTile * (tile % L.tiles_i);
  const int64_t rb = chunk * a.chunk_rows, re = rb + a.chunk_rows < a.rows ? rb + a.chunk_rows : a.rows;
  const int steps = (int)((re - rb + KS - 1) / KS);
  const bool wave_live = o0 + 16 * wave < L.out;     // this wave's 16 dW rows hold at least one real row
  const bool bias = L.db != nullptr && i0 == 0;      // this item also sums db (wave 0, a column per lane)

  auto stage_step = [&](int buf, int64_t k0) {
    stage<BF, T, false>(sm[buf][0], static_cast<const T*>(L.dz), L.out, L.out, o0, k0, re, a.act, a.alpha);
    if (l == 0) stage<BF, XT, false>(sm[buf][1], static_cast<const XT*>(L.a), L.a_pitch, L.in, i0, k0, re, 0, 0.f);
    else stage<BF, T, true>(sm[buf][1], static_cast<const T*>(L.a), L.a_pitch, L.in, i0, k0, re, a.act, a.alpha);
  };

  f32x4 acc[kCT];
#pragma unroll
  for (int c = 0; c < kCT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  stage_step(0, rb);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) stage_step(buf ^ 1, rb + (int64_t)(s + 1) * KS);
    if (wave_live) {
      const uint4 af = *reinterpret_cast<const uint4*>(sm[buf][0] + (16 * wave + lr) * kPitch + 16 * lq);
#pragma unroll
      for (int c = 0; c < kCT; ++c) {
        const uint4 bfrag = *reinterpret_cast<const uint4*>(sm[buf][1] + (16 * c + lr) * kPitch + 16 * lq);
        mma<BF>(acc[c], af, bfrag);
      }
    }
    if (bias && wave == 0) {
      const T* col = reinterpret_cast<const T*>(sm[buf][0] + lane * kPitch);
#pragma unroll
      for (int k = 0; k < KS; ++k) bsum += load_param(col + k);
    }
    __syncthreads();  // this buffer is read; the other one is whole
  }

  const bool direct = a.nchunks == 1;
  if (wave_live) {
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
      const int i = i0 + 16 * c + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = o0 + 16 * wave + 4 * lq + j;
        if (o < L.out && i < L.in) {
          if (direct) store_param(L.dW, (int64_t)o * L.in + i, acc[c][j], a.param_bf16 != 0);
          else L.pW[((int64_t)chunk * L.out + o) * L.in + i] = acc[c][j];
        }
      }
    }
  }
  if (bias && wave == 0 && o0 + lane < L.out) {
    if (direct) store_param(L.db, o0 + lane, bsum, a.param_bf16 != 0);
    else L.pb[(int64_t)chunk * L.out + o0 + lane] = bsum;
  }
}

// dW / db = the sum of the chunks' partials in chunk order, written in the parameters' dtype; nchunks == 0 writes
// zeros (the backward of no rows).  One thread per element of every dW and db.
__global__ __launch_bounds__(256) void mlp_head_reduce_kernel(const WgArgs a) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.total) return;
  int l = 0;
  for (;; ++l) {
    const int64_t n = (int64_t)a.L[l].out * a.L[l].in + (a.L[l].db != nullptr ? a.L[l].out : 0);
    if (e < n) break;
    e -= n;
  }
  const WgLayer& L = a.L[l];
  const int64_t nW = (int64_t)L.out * L.in;
  const bool is_b = e >= nW;
  const int64_t at = is_b ? e - nW : e, n = is_b ? L.out : nW;
  const float* p = is_b ? L.pb : L.pW;
  float sum = 0.f;
  for (int c = 0; c < a.nchunks; ++c) sum += p[c * n + at];
  store_param(is_b ? L.db : L.dW, at, sum, a.param_bf16 != 0);
}

inline int64_t align16(int64_t n) { return (n + 15) / 16 * 16; }

// The row chunks of the weight-gradient split: as many chunks of at least kChunkRows rows as there are, at most
// kMaxChunks, each a multiple of 32 rows (a whole k step of both instances) but the last.
inline void chunk_rule(int64_t rows, int64_t& chunk_rows, int& nchunks) {
  const int64_t want = std::max<int64_t>(1, std::min(kMaxChunks, (rows + kChunkRows - 1) / kChunkRows));
  chunk_rows = std::max<int64_t>(32, ((rows + want - 1) / want + 31) / 32 * 32);
  nchunks = (int)std::max<int64_t>(1, (rows + chunk_rows - 1) / chunk_rows);
}

// The workspace: dZ of every hidden layer ([rows, dims[l]], the instance's dtype), then, with more than one chunk,
// per layer the fp32 partials of dW and of db.  Every piece starts at a multiple of 16 bytes.
struct Plan {
  int64_t chunk_rows, dz[kMaxLayers], pW[kMaxLayers], pb[kMaxLayers], bytes;
  int nchunks;
};

inline Plan plan(int64_t rows, int nlayers, const int64_t* dims, bool bf) {
  Plan p{};
  chunk_rule(rows, p.chunk_rows, p.nchunks);
  int64_t at = 0;
  for (int l = 1; l < nlayers; ++l) p.dz[l] = at, at += align16(rows * dims[l] * (bf ? 2 : 4));
  if (p.nchunks > 1)
    for (int l = 0; l < nlayers; ++l) {
      p.pW[l] = at, at += align16(p.nchunks * dims[l + 1] * dims[l] * 4);
      p.pb[l] = at, at += align16(p.nchunks * dims[l + 1] * 4);
    }
  p.bytes = at;
  return p;
}

inline bool sizes_ok(int64_t rows, int nlayers, const int64_t* dims) {
  if (rows < 0 || rows > (int64_t)1 << 31 || nlayers < 1 || nlayers > kMaxLayers || dims == nullptr) return false;
  for (int l = 0; l <= nlayers; ++l)
    if (dims[l] < 1) return false;
  return true;
}

template <bool BF, typename XT, typename PT>
int launch_chain(const ChainArgs& a, int grid, size_t lds, hipStream_t stream) {
  auto kern = mlp_head_dx_kernel<BF, XT, PT>;
  if (lds > 64 * 1024)
    NT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, kThreads, lds, stream>>>(a);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

}  // namespace
}  // namespace nt

extern "C" int nt_mlp_head_train_supported(int x_dtype, int param_dtype, int nlayers, const int64_t* dims) {
  // the chain's two dZ tiles are the forward's two activation tiles, and the weight gradient has no width limit
  return nt_mlp_head_supported(x_dtype, param_dtype, nlayers, dims);
}

extern "C" int64_t nt_mlp_head_backward_workspace(int64_t rows, int nlayers, const int64_t* dims, int dtype) {
  using namespace nt;
  if (!sizes_ok(rows, nlayers, dims) || !dtype_ok(dtype)) return -1;
  return plan(rows, nlayers, dims, dtype == NT_BF16).bytes;
}

extern "C" int nt_mlp_head_backward(const void* dy, int dtype, const void* x, int x_dtype, int64_t rows,
                                    int64_t x_pitch, int nlayers, const void* const* saved, const void* const* W,
                                    int param_dtype, const int64_t* dims, int act, float act_alpha, void* dx,
                                    void* const* dW, void* const* db, void* workspace, int64_t workspace_bytes,
                                    void* stream_) {
  using namespace nt;
  clear_error();
  NT_REQUIRE(dy && x && W && dims && dW, NT_EINVAL, "NULL pointer (dy, x, W, dims and dW are required)");
  NT_REQUIRE(nlayers >= 1 && nlayers <= kMaxLayers, NT_EINVAL,
             "nlayers " + std::to_string(nlayers) + " (1 to " + std::to_string(kMaxLayers) + ")");
  NT_REQUIRE(nlayers == 1 || saved, NT_EINVAL, "NULL pointer (saved: one buffer per hidden layer)");
  for (int l = 0; l < nlayers; ++l) {
    NT_REQUIRE(W[l] && dW[l], NT_EINVAL, "NULL pointer (W[" + std::to_string(l) + "] / dW[" + std::to_string(l) + "])");
    NT_REQUIRE(l + 1 == nlayers || saved[l], NT_EINVAL, "NULL pointer (saved[" + std::to_string(l) + "])");
  }
  NT_REQUIRE(sizes_ok(rows, nlayers, dims), NT_EINVAL,
             "bad sizes: 0 <= rows <= 2^31 and every entry of dims >= 1");
  NT_REQUIRE(dtype_ok(dtype) && dtype_ok(x_dtype) && dtype_ok(param_dtype), NT_EUNSUPPORTED,
             "dtype (NT_F32 or NT_BF16 for dy, x and the parameters)");
  const bool bf = dtype == NT_BF16;
  NT_REQUIRE(bf || (x_dtype == NT_F32 && param_dtype == NT_F32), NT_EUNSUPPORTED,
             "dtype: an fp32 dy takes fp32 x and fp32 parameters (the bf16 instance reads bf16)");
  NT_REQUIRE(act >= NT_ACT_IDENTITY && act <= NT_ACT_SIGMOID, NT_EINVAL, "act code " + std::to_string(act));
  const int64_t xbytes = x_dtype == NT_BF16 ? 2 : 4, ebytes = bf ? 2 : 4;
  NT_REQUIRE(x_pitch >= dims[0], NT_EINVAL,
             "x pitch " + std::to_string(x_pitch) + " below dims[0] = " + std::to_string(dims[0]));
  NT_REQUIRE(x_pitch == dims[0] || x_pitch * xbytes % 16 == 0, NT_EINVAL,
             "x pitch " + std::to_string(x_pitch) + ": padded rows start at multiples of 16 bytes");
  NT_REQUIRE(nt_mlp_head_train_supported(x_dtype, param_dtype, nlayers, dims), NT_EUNSUPPORTED,
             "widths beyond the limits: dims[0] <= " + std::to_string(kMaxIn) + " and every later width <= " +
                 std::to_string(kMaxWidth) + " (two 16-row gradient tiles in 160 KiB of LDS)");
  const Plan p = plan(rows, nlayers, dims, bf);
  NT_REQUIRE(p.bytes == 0 || (workspace && aligned16(workspace) && workspace_bytes >= p.bytes), NT_EINVAL,
             "workspace: " + std::to_string(p.bytes) + " bytes at a multiple of 16 (nt_mlp_head_backward_workspace)");
  hipStream_t stream = as_stream(stream_);
  unsigned char* ws = static_cast<unsigned char*>(workspace);

  WgArgs w{};
  int64_t items = 0;
  for (int l = 0; l < nlayers; ++l) {
    WgLayer& L = w.L[l];
    L.in = (int)dims[l], L.out = (int)dims[l + 1];
    L.dz = l + 1 == nlayers ? dy : ws + p.dz[l + 1];
    L.a = l == 0 ? x : saved[l - 1];
    L.a_pitch = l == 0 ? x_pitch : dims[l];
    L.dW = dW[l], L.db = db ? db[l] : nullptr;
    if (p.nchunks > 1) L.pW = reinterpret_cast<float*>(ws + p.pW[l]), L.pb = reinterpret_cast<float*>(ws + p.pb[l]);
    L.tiles_i = (L.in + kTile - 1) / kTile;
    L.item0 = (int)items;
    items += (int64_t)L.tiles_i * ((L.out + kTile - 1) / kTile) * p.nchunks;
    w.total += dims[l + 1] * dims[l] + (L.db ? dims[l + 1] : 0);
  }
  w.rows = rows, w.chunk_rows = p.chunk_rows, w.nlayers = nlayers, w.nchunks = p.nchunks;
  w.act = act, w.alpha = act_alpha, w.param_bf16 = param_dtype == NT_BF16;
  const int reduce_grid = (int)((w.total + 255) / 256);
  if (rows == 0) {  // no rows: the gradients are zeros
    w.nchunks = 0;
    mlp_head_reduce_kernel<<<reduce_grid, 256, 0, stream>>>(w);
    NT_LAUNCH_CHECK();
    return NT_OK;
  }

  ChainArgs c{};
  int64_t widest = 0;
  for (int l = 0; l < nlayers; ++l) {
    c.L[l] = BwdLayer{W[l], l == 0 ? nullptr : saved[l - 1], l == 0 ? nullptr : ws + p.dz[l], (int)dims[l],
                      (int)dims[l + 1]};
    if (l >= 1 && dims[l] > widest) widest = dims[l];
  }
  c.dy = dy, c.dx = dx, c.rows = rows, c.nlayers = nlayers, c.stop = dx ? 0 : 1;
  c.act = act, c.alpha = act_alpha;
  c.dy_vec = aligned16(dy) && dims[nlayers] * ebytes % 16 == 0;
  c.lds_row = nlayers > 1 ? lds_row_bytes(widest, bf) : 0;
  if (c.stop < nlayers) {
    const size_t lds = (size_t)2 * kRows * c.lds_row;
    const int64_t per_cu = lds == 0 ? 4 : std::min<int64_t>(4, std::max<int64_t>(1, kLds / (int64_t)lds));
    const int64_t ntiles = (rows + kRows - 1) / kRows;
    const int cus = cu_count() > 0 ? cu_count() : 256;
    const int grid = (int)std::min<int64_t>(ntiles, per_cu * cus);
    int rc;
    if (!bf) rc = launch_chain<false, float, float>(c, grid, lds, stream);
    else if (x_dtype == NT_F32)
      rc = param_dtype == NT_F32 ? launch_chain<true, float, float>(c, grid, lds, stream)
                                 : launch_chain<true, float, bf16_t>(c, grid, lds, stream);
    else
      rc = param_dtype == NT_F32 ? launch_chain<true, bf16_t, float>(c, grid, lds, stream)
                                 : launch_chain<true, bf16_t, bf16_t>(c, grid, lds, stream);
    if (rc != NT_OK) return rc;
  }

  if (!bf) mlp_head_wgrad_kernel<false, float><<<(int)items, kThreads, 0, stream>>>(w);
  else if (x_dtype == NT_F32) mlp_head_wgrad_kernel<true, float><<<(int)items, kThreads, 0, stream>>>(w);
  else mlp_head_wgrad_kernel<true, bf16_t><<<(int)items, kThreads, 0, stream>>>(w);
  NT_LAUNCH_CHECK();
  if (p.nchunks > 1) {
    mlp_head_reduce_kernel<<<reduce_grid, 256, 0, stream>>>(w);
    NT_LAUNCH_CHECK();
  }
  set_last_kernel(bf ? "mlp_head_backward_bf16" : "mlp_head_backward_f32");
  return NT_OK;
}
