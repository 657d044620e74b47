// bf16 storage path of the D-MPNN forward (BASELINE config 3: ZINC-shaped batches, depth 5,
// hidden 512, bf16).  Same math as the fp32 kernels (chemprop.py:28-43,81-88, residual.py:27-28,
// agg.py:23-47); feature rows, weights and bias are bf16 in HBM, every sum and product runs in fp32
// and each stored element is rounded to bf16 once (round-to-nearest-even, v_cvt_pk_bf16_f32).
//
//   init_bf16          H0[e] = Xv[src e] + Xe[e];  S[v] = R_{e->v} act(H0[e])          (3E+V rows)
//   segment_reduce     out[s] = R_{j in s} act(X[perm j])                                 (E+V rows)
//   update_bf16        H'[e] = H[e] + W (S[src e] - act(H[rev e])) + b                    (4 rows/edge)
//
// update_bf16 is a 64-edge-tile MFMA kernel (v_mfma_f32_16x16x32_bf16, fp32 accumulators):
//   1. gather: the four waves form A = S[src] - act(H[rev]) for the tile's 64 edges (one wave per
//      row, 16 B per lane, so a 512-wide bf16 row is one 1 KiB coalesced read) and store it as bf16
//      into LDS (row stride Kp*2 + 16 B: the fragment reads below are bank-conflict free);
//   2. MFMA: wave w owns column tiles w, w+4, ... (<= 8 of 16 columns) for all 64 rows: per 32-deep
//      k step it reads 4 A fragments from LDS and streams its B fragments from the packed weight
//      image (L2-resident: 512 KiB per layer at h = 512; one 1 KiB coalesced load per fragment,
//      prefetched one k step ahead);
//   3. epilogue: accumulators are staged through LDS (fp32, 256 columns per pass) and written as
//      whole 16-B row pieces with + bias + residual, rounded to bf16 once.
// Two workgroups per CU (66.5 KiB LDS each) overlap one tile's gather with the other's MFMAs.
// HBM bytes per edge: 4 rows x 2h (read H, gather S[src], gather H[rev], write H') + 16 B indices.
// h > 512 (h % 8 == 0, <= 8192): update_bf16_wide_kernel walks the same tile in column passes and
// K chunks of 512 (see there).
// h % 4 == 0, h % 8 != 0 (h <= 512): the same kernel on 8-B row pieces (W = 4: every 16-B global access
// as two 8-B halves; the half past a row's end is never loaded into A, stored or reduced).
#include "bf16.hpp"

namespace nt {

int cu_count();   // tile_plan.hip
int xcd_count();  // tile_plan.hip

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;  // raw bf16 storage

__device__ __forceinline__ float bf2f(bf16_t u) { return __uint_as_float((unsigned)u << 16); }
__device__ __forceinline__ bf16_t f2bf(float x) { return __builtin_bit_cast(bf16_t, (__bf16)x); }

// W consecutive bf16 (W = 8: one 16-B piece, 16-B aligned; W = 4: one 8-B piece, 8-B aligned; W = 1:
// one element) <-> fp32
template <int W>
__device__ __forceinline__ void load_chunk(const bf16_t* __restrict__ p, float (&x)[W]) {
  if constexpr (W == 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = __uint_as_float(u[i] << 16);
      x[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  } else if constexpr (W == 4) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    const unsigned u[2] = {v.x, v.y};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      x[2 * i] = __uint_as_float(u[i] << 16);
      x[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  } else {
    x[0] = bf2f(*p);
  }
}

template <int W>
__device__ __forceinline__ void store_chunk(bf16_t* __restrict__ p, const float (&x)[W]) {
  if constexpr (W == 8) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (__bf16)x[i];
    *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, v);
  } else if constexpr (W == 4) {
    bf16x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (__bf16)x[i];
    *reinterpret_cast<uint2*>(p) = __builtin_bit_cast(uint2, v);
  } else {
    *p = f2bf(x[0]);
  }
}

// round-trip through bf16 (the value a bf16 tensor would hold)
__device__ __forceinline__ float rbf(float x) { return bf2f(f2bf(x)); }

// ------------------------------------------------------------------------------ segment reduce
template <int R, int ACT, int W>
__global__ void __launch_bounds__(256) segment_reduce_bf16(
    const bf16_t* __restrict__ X, const int32_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ perm, int64_t nseg, int64_t h, int act, float alpha,
    bf16_t* __restrict__ out) {
  const int64_t hw = h / W;
  const int64_t total = nseg * hw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = t / hw, c = (t - s * hw) * W;
    const int32_t b = seg_ptr[s], e = seg_ptr[s + 1];
    Reducer<R> r[W];
#pragma unroll
    for (int i = 0; i < W; ++i) r[i].init();
    for (int32_t j = b; j < e; ++j) {
      const int64_t row = perm ? perm[j] : j;
      float x[W];
      load_chunk<W>(X + row * h + c, x);
#pragma unroll
      for (int i = 0; i < W; ++i) r[i].push(act_t<ACT>(x[i], act, alpha));
    }
    float y[W];
#pragma unroll
    for (int i = 0; i < W; ++i) y[i] = r[i].result();
    store_chunk<W>(out + s * h + c, y);
  }
}

// ------------------------------------------------------------------------------ init
template <int R, int ACT, int W>
__global__ void __launch_bounds__(256) init_aggregate_bf16(
    const bf16_t* __restrict__ Xv, const bf16_t* __restrict__ Xe, const int64_t* __restrict__ src,
    const int32_t* __restrict__ seg_ptr, const int32_t* __restrict__ perm, int64_t V, int64_t h,
    int act, float alpha, bf16_t* __restrict__ H0, bf16_t* __restrict__ S) {
  const int64_t hw = h / W;
  const int64_t total = V * hw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = t / hw, c = (t - v * hw) * W;
    const int32_t b = seg_ptr[v], e = seg_ptr[v + 1];
    Reducer<R> r[W];
#pragma unroll
    for (int i = 0; i < W; ++i) r[i].init();
    for (int32_t j = b; j < e; ++j) {
      const int64_t ed = perm[j];
      float xv[W], xe[W], x[W];
      load_chunk<W>(Xv + src[ed] * h + c, xv);
      load_chunk<W>(Xe + ed * h + c, xe);
#pragma unroll
      for (int i = 0; i < W; ++i) x[i] = rbf(xv[i] + xe[i]);  // H0 as stored
      store_chunk<W>(H0 + ed * h + c, x);
#pragma unroll
      for (int i = 0; i < W; ++i) r[i].push(act_t<ACT>(x[i], act, alpha));
    }
    float y[W];
#pragma unroll
    for (int i = 0; i < W; ++i) y[i] = r[i].result();
    store_chunk<W>(S + v * h + c, y);
  }
}

template <int W>
__global__ void __launch_bounds__(256) init_only_bf16(const bf16_t* __restrict__ Xv,
                                                      const bf16_t* __restrict__ Xe,
                                                      const int64_t* __restrict__ src, int64_t E,
                                                      int64_t h, bf16_t* __restrict__ H0) {
  const int64_t hw = h / W;
  const int64_t total = E * hw;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / hw, c = (t - e * hw) * W;
    float xv[W], xe[W];
    load_chunk<W>(Xv + src[e] * h + c, xv);
    load_chunk<W>(Xe + e * h + c, xe);
#pragma unroll
    for (int i = 0; i < W; ++i) xv[i] += xe[i];
    store_chunk<W>(H0 + e * h + c, xv);
  }
}

// ------------------------------------------------------------------------------ weight image
// Wp[ks][nt][lane] = 8 bf16: W[n][k], n = 16 nt + (lane & 15), k = 32 ks + 8 (lane >> 4) + j
// (zero outside [0, h)) — exactly the B fragment of v_mfma_f32_16x16x32_bf16 for out = A W^T.
__global__ void __launch_bounds__(256) pack_bf16(const bf16_t* __restrict__ W, int64_t nlayers,
                                                 int64_t h, int KS, int NTn, int64_t layer_stride16,
                                                 uint4* __restrict__ Wp) {
  const int64_t per_layer = (int64_t)KS * NTn * 64;
  const int64_t total = nlayers * per_layer;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = t / per_layer;
    int64_t r = t - l * per_layer;
    const int lane = (int)(r & 63);
    r >>= 6;
    const int nt = (int)(r % NTn);
    const int ks = (int)(r / NTn);
    const int64_t n = 16 * nt + (lane & 15);
    const int64_t k0 = 32 * ks + 8 * (lane >> 4);
    const bf16_t* Wl = W + l * h * h;
    unsigned short v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (n < h && k0 + j < h) ? Wl[n * h + k0 + j] : (bf16_t)0;
    uint4 o;
    o.x = v[0] | ((unsigned)v[1] << 16);
    o.y = v[2] | ((unsigned)v[3] << 16);
    o.z = v[4] | ((unsigned)v[5] << 16);
    o.w = v[6] | ((unsigned)v[7] << 16);
    Wp[l * layer_stride16 + ((int64_t)ks * NTn + nt) * 64 + lane] = o;
  }
}

// ------------------------------------------------------------------------------ update
constexpr int kM = 64;        // edges per tile
constexpr int kThreads = 256;  // 4 waves
constexpr int kNWMax = 8;     // column tiles per wave at h = 512 (NW = ceil(ceil(h/16) / 4))
constexpr int kSO = 260;      // staging row stride (floats): 256 columns + 4 (conflict-free writes)
constexpr int kStageB = kM * kSO * 4;  // 66,560 B

__host__ __device__ constexpr int a_row_bytes(int KS) { return KS * 64 + 16; }
inline int lds_bytes_bf16(int KS) {
  const int a = kM * a_row_bytes(KS);
  return a > kStageB ? a : kStageB;
}

// Fused aggregation of the layer output (nt_dmpnn_update_fused): tiles are the tile plan's cuts of
// the dst-sorted edge order, so every node's in-edges are consecutive rows of one tile.
struct BfAgg {
  const int* tile_ptr;   // ntiles + 1 positions
  const int* perm;       // dst CSR permutation: position -> edge
  const int* dsts;       // position -> destination node
  int reduce, aact;
  float aalpha;
  bf16_t* S_out;         // V x h, rows of in-degree-0 nodes pre-zeroed by the caller
};

// S_out[node] piece = R over rows [r0, r1) of the staged values (already aact(stored H')); N = 4: the
// first half of a piece whose second half lies past the row (W == 4, h % 8 == 4)
template <int R, int N = 8>
__device__ __forceinline__ void reduce_rows(const float* stage, int r0, int r1, int c, float (&y)[N]) {
  Reducer<R> red[N];
#pragma unroll
  for (int q = 0; q < N; ++q) red[q].init();
  for (int r = r0; r < r1; ++r) {
    const float* st = stage + r * kSO + c;
#pragma unroll
    for (int q = 0; q < N; ++q) red[q].push(st[q]);
  }
#pragma unroll
  for (int q = 0; q < N; ++q) y[q] = red[q].result();
}

// the same with the reduce chosen at run time
template <int N>
__device__ __forceinline__ void reduce_rows_by(int reduce, const float* stage, int r0, int r1, int c,
                                               float (&y)[N]) {
  switch (reduce) {
    case NT_SUM: reduce_rows<NT_SUM, N>(stage, r0, r1, c, y); break;
    case NT_MEAN: reduce_rows<NT_MEAN, N>(stage, r0, r1, c, y); break;
    case NT_MAX: reduce_rows<NT_MAX, N>(stage, r0, r1, c, y); break;
    default: reduce_rows<NT_MIN, N>(stage, r0, r1, c, y); break;
  }
}

// AGG: 0 = no aggregation; 1 = fused aggregation of the stored H' (final node scatter, identity);
// 2 = fused aggregation of act(H') (the next layer's chemprop.py:37-39, same act as this layer)
// DROP (nt_dmpnn_update_fused_dropout): the update passes the dropout mask `drop` (dropout.hpp, dense
// element index e h + j) before the residual is added, H' = H + keep (stage + bias) / (1 - p), in fp32
// with one rounding; the aggregation reads the rounded value as without dropout.
template <int ACT, int W, int NW, int AGG, bool DROP = false>
__global__ void __launch_bounds__(kThreads, 2) update_bf16_kernel(
    const bf16_t* __restrict__ H, const bf16_t* __restrict__ S, const int64_t* __restrict__ src,
    const int64_t* __restrict__ rev, const uint4* __restrict__ Wp, const bf16_t* __restrict__ bias,
    int64_t V, int64_t E, int h, int KS, int NTn, int residual, int act, float alpha,
    bf16_t* __restrict__ out, BfAgg agg, int ntiles, int nxcd, DropMask drop) {
  static_assert(!DROP || (W == 8 && AGG != 0), "dropout: the fused kernel on whole 16-B pieces only");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ int64_t soff[kM], qoff[kM], erow[kM];
  __shared__ int nstart[kM + 1], nnode[kM], nseg;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lda = a_row_bytes(KS);
  const int G = gridDim.x;
  // Column tile j of this wave is nt = w + 4 j, j < NW.  A wave's last tile may lie past NTn (h not
  // a multiple of 64): its loads are clamped to a valid fragment and its result is never stored,
  // so every load and MFMA below is unconditional (no branch for hipcc to drain vmcnt in front of).
  // (recomputed where used, not kept in registers: the column tile of fragment j, clamped)
  auto boff = [&](int j) { return (w + 4 * j < NTn ? w + 4 * j : NTn - 1) * 64 + lane; };
  const int64_t kstride = (int64_t)NTn * 64;

  // Persistent loop over tiles t = blockIdx.x + i G.  Wave 0 lane r holds row r's indices of the
  // NEXT tile, fetched in three dependent stages spread over the current tile (tile bounds before
  // the gather, edge / node ids before the MFMAs, src / rev before the epilogue) so the index
  // chain tile_ptr -> perm -> src, rev never stalls the pipeline.
  int cT = 0, cn = 0;           // stage A: tile start position and size
  int ce = -1;                  // stage B: edge of row `lane` (E < 2^31)
  int cnode = -1, cprev = -2;   // stage B: its destination node, and that of the row before
  int cs = -1, cq = -1;         // stage C: src / rev of that edge (-1 when out of range)
  auto stage_a = [&](int t) {
    if constexpr (AGG != 0) {
      cT = agg.tile_ptr[t];
      cn = agg.tile_ptr[t + 1] - cT;
    } else {
      cT = t * kM;
      cn = E - (int64_t)cT < kM ? (int)(E - cT) : kM;
    }
  };
  auto stage_b = [&]() {
    ce = -1;
    cnode = -1;
    cprev = -2;
    if (lane < cn) {
      if constexpr (AGG != 0) {
        ce = agg.perm[cT + lane];
        cnode = agg.dsts[cT + lane];
        cprev = lane > 0 ? agg.dsts[cT + lane - 1] : -2;
      } else {
        ce = cT + lane;
      }
    }
  };
  auto stage_c = [&]() {
    // dense mode (src = rev = NULL, nt_dmpnn_dense_matmul): row e of A is S[e]
    const int64_t s = ce >= 0 ? (src ? src[ce] : (int64_t)ce) : -1, q = (ce >= 0 && rev) ? rev[ce] : -1;
    cs = (s >= 0 && s < V) ? (int)s : -1;
    cq = (q >= 0 && q < E) ? (int)q : -1;
  };
  // XCD-aware walk (as update_fk.hip): blocks b and b + nxcd share an XCD; each XCD takes one
  // contiguous 1/nxcd of the tiles, so rows shared by neighbouring tiles stay in its L2.
  int t_first = blockIdx.x, t_step = G, t_end = ntiles;
  if (nxcd > 1 && G % nxcd == 0) {
    const int x = (int)blockIdx.x % nxcd, chunk = (ntiles + nxcd - 1) / nxcd;
    t_first = x * chunk + (int)blockIdx.x / nxcd;
    t_step = G / nxcd;
    t_end = min(ntiles, x * chunk + chunk);
  }
  if (w == 0 && t_first < t_end) {
    stage_a(t_first);
    stage_b();
    stage_c();
  }

  for (int t = t_first; t < t_end; t += t_step) {
    const bool has_next = t + t_step < t_end;
    if (w == 0) {  // publish this tile's indices (the previous tile's epilogue ended with a barrier)
      erow[lane] = ce;
      soff[lane] = cs >= 0 ? (int64_t)cs * h : -1;
      qoff[lane] = cq >= 0 ? (int64_t)cq * h : -1;
      if constexpr (AGG != 0) {  // segment starts of the tile's nodes (ballot + prefix popcount)
        const bool first = lane < cn && cnode != cprev;
        const unsigned long long m = __ballot(first);
        const int k = __popcll(m & ((1ull << lane) - 1ull));
        if (first) {
          nstart[k] = lane;
          nnode[k] = cnode;
        }
        if (lane == 0) {
          nseg = __popcll(m);
          nstart[__popcll(m)] = cn;
        }
      }
      if (has_next) stage_a(t + t_step);
    }
    // B fragments of the first k step, in flight during the gather
    uint4 bcur[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) bcur[j] = Wp[boff(j)];
    __syncthreads();

  // ---- 1. gather A = S[src] - act(H[rev]) (fp32) -> bf16 LDS tile [64][Kp] ----
  if constexpr (W == 8) {
    // wave w owns rows 16 w .. 16 w + 15; lane c takes the c-th 16-B piece of each row, and all 32
    // loads of the wave are issued before the first is consumed (latency hidden by depth)
    const int chunks = KS * 4;
    constexpr int kRG = 8;  // rows in flight per round (2 rounds of 8: 64 VGPRs of raw pieces)
    for (int idx = lane; idx < chunks * (16 / kRG); idx += 64) {
      const int c = idx % chunks, r0 = 16 * w + kRG * (idx / chunks);
      const int k0 = c * 8;
      const int kc = k0 < h ? k0 : h - 8;  // clamped, unconditional loads
      uint4 sraw[kRG], qraw[kRG];
#pragma unroll
      for (int u = 0; u < kRG; ++u) {
        const int64_t so = soff[r0 + u], qo = qoff[r0 + u];
        sraw[u] = *reinterpret_cast<const uint4*>(S + (so >= 0 ? so : 0) + kc);
        qraw[u] = *reinterpret_cast<const uint4*>(H + (qo >= 0 ? qo : 0) + kc);
      }
#pragma unroll
      for (int u = 0; u < kRG; ++u) {
        const int r = r0 + u;
        const bool sok = soff[r] >= 0 && k0 < h, qok = qoff[r] >= 0 && k0 < h;
        const unsigned su[4] = {sraw[u].x, sraw[u].y, sraw[u].z, sraw[u].w};
        const unsigned qu[4] = {qraw[u].x, qraw[u].y, qraw[u].z, qraw[u].w};
        bf16x8 a;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const unsigned sb = (i & 1) ? (su[i >> 1] & 0xffff0000u) : (su[i >> 1] << 16);
          const unsigned qb = (i & 1) ? (qu[i >> 1] & 0xffff0000u) : (qu[i >> 1] << 16);
          const float sv = sok ? __uint_as_float(sb) : 0.f;
          const float qv = qok ? __uint_as_float(qb) : 0.f;
          a[i] = (__bf16)(sv - act_t<ACT>(qv, act, alpha));
        }
        *reinterpret_cast<uint4*>(lds + r * lda + c * 16) = __builtin_bit_cast(uint4, a);
      }
    }
  } else if constexpr (W == 4) {
    // h % 4 == 0: rows are whole 8-B pieces.  The ownership of the W == 8 gather (lane c takes the
    // c-th 8-column piece, 8 rows in flight, one 16-B LDS store per piece), each piece loaded as two
    // 8-B halves.  The second half of a row's last piece lies past the row when h % 8 == 4: its
    // address is clamped to the first half's (the load stays unconditional) and its four A values
    // are the zeros of k >= h, never the loaded bits (they belong to the next row).
    const int chunks = KS * 4;
    constexpr int kRG = 8;
    for (int idx = lane; idx < chunks * (16 / kRG); idx += 64) {
      const int c = idx % chunks, r0 = 16 * w + kRG * (idx / chunks);
      const int k0 = c * 8;
      const bool in0 = k0 < h, in1 = k0 + 4 < h;
      const int kc0 = in0 ? k0 : h - 4, kc1 = in1 ? k0 + 4 : kc0;
      uint2 sraw[kRG][2], qraw[kRG][2];
#pragma unroll
      for (int u = 0; u < kRG; ++u) {
        const int64_t so = soff[r0 + u], qo = qoff[r0 + u];
        const bf16_t* sp = S + (so >= 0 ? so : 0);
        const bf16_t* qp = H + (qo >= 0 ? qo : 0);
        sraw[u][0] = *reinterpret_cast<const uint2*>(sp + kc0);
        sraw[u][1] = *reinterpret_cast<const uint2*>(sp + kc1);
        qraw[u][0] = *reinterpret_cast<const uint2*>(qp + kc0);
        qraw[u][1] = *reinterpret_cast<const uint2*>(qp + kc1);
      }
#pragma unroll
      for (int u = 0; u < kRG; ++u) {
        const int r = r0 + u;
        const bool sok[2] = {soff[r] >= 0 && in0, soff[r] >= 0 && in1};
        const bool qok[2] = {qoff[r] >= 0 && in0, qoff[r] >= 0 && in1};
        const unsigned su[4] = {sraw[u][0].x, sraw[u][0].y, sraw[u][1].x, sraw[u][1].y};
        const unsigned qu[4] = {qraw[u][0].x, qraw[u][0].y, qraw[u][1].x, qraw[u][1].y};
        bf16x8 a;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const unsigned sb = (i & 1) ? (su[i >> 1] & 0xffff0000u) : (su[i >> 1] << 16);
          const unsigned qb = (i & 1) ? (qu[i >> 1] & 0xffff0000u) : (qu[i >> 1] << 16);
          const float sv = sok[i >> 2] ? __uint_as_float(sb) : 0.f;
          const float qv = qok[i >> 2] ? __uint_as_float(qb) : 0.f;
          a[i] = (__bf16)(sv - act_t<ACT>(qv, act, alpha));
        }
        *reinterpret_cast<uint4*>(lds + r * lda + c * 16) = __builtin_bit_cast(uint4, a);
      }
    }
  } else {
    const int chunks = KS * 4;  // 8-element pieces per padded row
    constexpr int kRU = 4;      // rows in flight per wave
    for (int r0 = w * kRU; r0 < kM; r0 += 4 * kRU) {
      for (int c = lane; c < chunks; c += 64) {
        const int k0 = c * 8;
        float sv[kRU][8], qv[kRU][8];
#pragma unroll
        for (int u = 0; u < kRU; ++u) {
          const int64_t so = soff[r0 + u], qo = qoff[r0 + u];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const bool in = k0 + i < h;
            sv[u][i] = (in && so >= 0) ? bf2f(S[so + k0 + i]) : 0.f;
            qv[u][i] = (in && qo >= 0) ? bf2f(H[qo + k0 + i]) : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < kRU; ++u) {
          bf16x8 a;
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] = (__bf16)(sv[u][i] - act_t<ACT>(qv[u][i], act, alpha));
          *reinterpret_cast<uint4*>(lds + (r0 + u) * lda + c * 16) = __builtin_bit_cast(uint4, a);
        }
      }
    }
  }
  __syncthreads();

    if (w == 0 && has_next) stage_b();

  // ---- 2. MFMA over k: acc[mt][j] = rows 16 mt.., columns of tile w + 4 j ----
  f32x4 acc[4][NW];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < NW; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* arow = lds + (lane & 15) * lda + 16 * (lane >> 4);
  for (int ks = 0; ks < KS; ++ks) {
    // next step's fragments (the last step re-reads its own: no branch, no drain)
    const int64_t kn = (ks + 1 < KS ? ks + 1 : ks) * kstride;
    uint4 bnext[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) bnext[j] = Wp[kn + boff(j)];
    bf16x8 a[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
      a[mt] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(arow + 16 * mt * lda + 64 * ks));
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, bcur[j]);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b, acc[mt][j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) bcur[j] = bnext[j];
  }
    if (w == 0 && has_next) stage_c();
  __syncthreads();  // every wave is done with the A tile: its LDS becomes the staging tile

  // ---- 3. epilogue: 256 columns per pass through LDS, + bias + residual, bf16 rows ----
  float* stage = reinterpret_cast<float*>(lds);
  const int Np = NTn * 16;
  // p and jj fully unrolled: acc[][j] must only ever be indexed by constants, or it lands in scratch
#pragma unroll
  for (int p = 0; p < (NW + 3) / 4; ++p) {
    if (p * 256 >= Np) break;
    const int n0 = 256 * p;
    const int ncols = h - n0 < 256 ? h - n0 : 256;
    // W == 8: thread (tid) owns column piece c = 8 (tid & 31) of rows (tid >> 5) + 8 it, it < 8;
    // its residual pieces are loaded before the staging round trip so their latency overlaps it
    constexpr int kIt = kM * 32 / kThreads;
    const int cpiece = 8 * (tid & 31);
    const bool cok = cpiece < ncols;
    // all residual pieces are in flight across the staging round trip (halving that for the fused
    // aggregation did not remove its spill and cost ~5% at config 3)
    constexpr int kPre = kIt;
    auto load_res = [&](int it) {
      const int64_t e = erow[(tid >> 5) + 8 * it];
      const bool ok = cok && e >= 0 && residual;
      return *reinterpret_cast<const uint4*>(H + (ok ? e * h + n0 + cpiece : 0));
    };
    uint4 hres[kPre];
    if constexpr (W == 8) {
#pragma unroll
      for (int it = 0; it < kPre; ++it) hres[it] = load_res(it);
    }
    // W == 4: the same pieces as two 8-B halves.  chi: the piece's second half is inside the row (it
    // is not in the last piece of a row with h % 8 == 4: never loaded, stored or reduced then; its
    // residual load is clamped to the first half's address)
    const bool chi = cpiece + 4 < ncols;
    uint2 hres4[kPre][2];
    if constexpr (W == 4) {
#pragma unroll
      for (int it = 0; it < kPre; ++it) {
        const int64_t e = erow[(tid >> 5) + 8 * it];
        const bool ok = cok && e >= 0 && residual;
        const bf16_t* hp = H + (ok ? e * h + n0 + cpiece : 0);
        hres4[it][0] = *reinterpret_cast<const uint2*>(hp);
        hres4[it][1] = *reinterpret_cast<const uint2*>(hp + (ok && chi ? 4 : 0));
      }
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = 4 * p + jj;
      if (j < NW && w + 4 * j < NTn) {
        const int sc = 16 * w + 64 * jj + (lane & 15);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) stage[(16 * mt + 4 * (lane >> 4) + r) * kSO + sc] = acc[mt][j][r];
      }
    }
    __syncthreads();
    if constexpr (W == 8) {
      float bb[8];
      if (bias && cok) load_chunk<8>(bias + n0 + cpiece, bb);
      else for (int q = 0; q < 8; ++q) bb[q] = 0.f;
#pragma unroll
      for (int it = 0; it < kIt; ++it) {
        const int r = (tid >> 5) + 8 * it;
        const int64_t e = erow[r];
        if (cok && e >= 0) {
          float* st = stage + r * kSO + cpiece;
          const uint4 hr = it < kPre ? hres[it < kPre ? it : 0] : load_res(it);
          const unsigned hu[4] = {hr.x, hr.y, hr.z, hr.w};
          float y[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const unsigned hb = (q & 1) ? (hu[q >> 1] & 0xffff0000u) : (hu[q >> 1] << 16);
            float u = st[q] + bb[q];
            if constexpr (DROP) u = drop_apply(drop, (uint64_t)(e * h + n0 + cpiece + q), u);
            y[q] = u + (residual ? __uint_as_float(hb) : 0.f);
          }
          store_chunk<8>(out + e * h + n0 + cpiece, y);
          if constexpr (AGG != 0) {  // the aggregation reads the stored (bf16) value, as unfused
#pragma unroll
            for (int q = 0; q < 8; ++q) st[q] = AGG == 2 ? act_t<ACT>(rbf(y[q]), act, alpha) : rbf(y[q]);
          }
        }
      }
      if constexpr (AGG != 0) {
        __syncthreads();
        for (int k = tid >> 5; k < nseg; k += kThreads / 32) {
          if (!cok) continue;
          float y[8];
          switch (agg.reduce) {
            case NT_SUM: reduce_rows<NT_SUM>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
            case NT_MEAN: reduce_rows<NT_MEAN>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
            case NT_MAX: reduce_rows<NT_MAX>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
            default: reduce_rows<NT_MIN>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
          }
          store_chunk<8>(agg.S_out + (int64_t)nnode[k] * h + n0 + cpiece, y);
        }
      }
    } else if constexpr (W == 4) {
      // the W == 8 epilogue with 8-B global accesses; the half past the row (!chi) is computed on
      // whatever the staging tile holds there and dropped
      float bb[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) bb[q] = 0.f;
      if (bias && cok) {
        load_chunk<4>(bias + n0 + cpiece, *reinterpret_cast<float(*)[4]>(&bb[0]));
        if (chi) load_chunk<4>(bias + n0 + cpiece + 4, *reinterpret_cast<float(*)[4]>(&bb[4]));
      }
#pragma unroll
      for (int it = 0; it < kIt; ++it) {
        const int r = (tid >> 5) + 8 * it;
        const int64_t e = erow[r];
        if (cok && e >= 0) {
          float* st = stage + r * kSO + cpiece;
          const unsigned hu[4] = {hres4[it][0].x, hres4[it][0].y, hres4[it][1].x, hres4[it][1].y};
          float y[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const unsigned hb = (q & 1) ? (hu[q >> 1] & 0xffff0000u) : (hu[q >> 1] << 16);
            y[q] = st[q] + bb[q] + (residual ? __uint_as_float(hb) : 0.f);
          }
          bf16_t* op = out + e * h + n0 + cpiece;
          store_chunk<4>(op, *reinterpret_cast<const float(*)[4]>(&y[0]));
          if (chi) store_chunk<4>(op + 4, *reinterpret_cast<const float(*)[4]>(&y[4]));
          if constexpr (AGG != 0) {  // the aggregation reads the stored (bf16) value, as unfused
#pragma unroll
            for (int q = 0; q < 8; ++q) st[q] = AGG == 2 ? act_t<ACT>(rbf(y[q]), act, alpha) : rbf(y[q]);
          }
        }
      }
      if constexpr (AGG != 0) {
        __syncthreads();
        for (int k = tid >> 5; k < nseg; k += kThreads / 32) {
          if (!cok) continue;
          bf16_t* sp = agg.S_out + (int64_t)nnode[k] * h + n0 + cpiece;
          if (chi) {
            float y[8];
            reduce_rows_by<8>(agg.reduce, stage, nstart[k], nstart[k + 1], cpiece, y);
            store_chunk<4>(sp, *reinterpret_cast<const float(*)[4]>(&y[0]));
            store_chunk<4>(sp + 4, *reinterpret_cast<const float(*)[4]>(&y[4]));
          } else {
            float y[4];
            reduce_rows_by<4>(agg.reduce, stage, nstart[k], nstart[k + 1], cpiece, y);
            store_chunk<4>(sp, y);
          }
        }
      }
    } else {
      for (int i = tid; i < kM * 256; i += kThreads) {
        const int r = i >> 8, c = i & 255;
        const int64_t e = erow[r];
        if (c < ncols && e >= 0) {
          float y = stage[r * kSO + c];
          if (bias) y += bf2f(bias[n0 + c]);
          if (residual) y += bf2f(H[e * h + n0 + c]);
          out[e * h + n0 + c] = f2bf(y);
        }
      }
    }
    __syncthreads();
  }
  }  // tile loop
}

// ------------------------------------------------------------------------------ update, h > 512
// The same tile, wave split, fragment layout and epilogue as update_bf16_kernel<ACT, 8, 8, AGG>, in
// a kernel of its own so that the h <= 512 instantiations keep their code.  A wave still owns eight
// column tiles (128 accumulator VGPRs) and the A tile still holds 16 k steps (66.5 KB of LDS, two
// workgroups per CU), so a tile is walked as
//   for each column pass of <= 512 output columns:        acc = 0
//     for each K chunk of <= 16 k steps (512 input columns):
//       barrier, gather the chunk of A into the LDS tile, barrier, the chunk's MFMAs
//     epilogue of the pass's columns (two 256-column staging rounds)
// A is gathered once per column pass (ceil(h / 512) times per tile; the repeats hit L2), the B
// fragments stream from Wp[global k step][column tile] one k step ahead across chunk boundaries, and
// the index pipeline runs once per tile.  The MFMA order per output element is k ascending whatever
// AGG is, so the fused H' equals the plain kernel's bit for bit.
constexpr int kKSc = 16;                      // k steps per chunk
constexpr int kLdaW = a_row_bytes(kKSc);      // 1040 B
constexpr int kLdsW = kM * kLdaW > kStageB ? kM * kLdaW : kStageB;  // 66,560 B
constexpr int kNTp = 4 * kNWMax;              // column tiles per pass (32 = 512 columns)

template <int ACT, int AGG, bool DROP = false>
__global__ void __launch_bounds__(kThreads, 2) update_bf16_wide_kernel(
    const bf16_t* __restrict__ H, const bf16_t* __restrict__ S, const int64_t* __restrict__ src,
    const int64_t* __restrict__ rev, const uint4* __restrict__ Wp, const bf16_t* __restrict__ bias,
    int64_t V, int64_t E, int h, int KS, int NTn, int residual, int act, float alpha,
    bf16_t* __restrict__ out, BfAgg agg, int ntiles, int nxcd, DropMask drop) {
  static_assert(!DROP || AGG != 0, "dropout: the fused kernel only");
  constexpr int NW = kNWMax;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ int64_t soff[kM], qoff[kM], erow[kM];
  __shared__ int nstart[kM + 1], nnode[kM], nseg;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int G = gridDim.x;
  const int64_t kstride = (int64_t)NTn * 64;
  const int npass = (NTn + kNTp - 1) / kNTp, nchunk = (KS + kKSc - 1) / kKSc;

  // index pipeline of the next tile, as update_bf16_kernel (once per tile, not per pass)
  int cT = 0, cn = 0;
  int ce = -1;
  int cnode = -1, cprev = -2;
  int cs = -1, cq = -1;
  auto stage_a = [&](int t) {
    if constexpr (AGG != 0) {
      cT = agg.tile_ptr[t];
      cn = agg.tile_ptr[t + 1] - cT;
    } else {
      cT = t * kM;
      cn = E - (int64_t)cT < kM ? (int)(E - cT) : kM;
    }
  };
  auto stage_b = [&]() {
    ce = -1;
    cnode = -1;
    cprev = -2;
    if (lane < cn) {
      if constexpr (AGG != 0) {
        ce = agg.perm[cT + lane];
        cnode = agg.dsts[cT + lane];
        cprev = lane > 0 ? agg.dsts[cT + lane - 1] : -2;
      } else {
        ce = cT + lane;
      }
    }
  };
  auto stage_c = [&]() {
    const int64_t s = ce >= 0 ? (src ? src[ce] : (int64_t)ce) : -1, q = (ce >= 0 && rev) ? rev[ce] : -1;
    cs = (s >= 0 && s < V) ? (int)s : -1;
    cq = (q >= 0 && q < E) ? (int)q : -1;
  };
  int t_first = blockIdx.x, t_step = G, t_end = ntiles;
  if (nxcd > 1 && G % nxcd == 0) {
    const int x = (int)blockIdx.x % nxcd, chunk = (ntiles + nxcd - 1) / nxcd;
    t_first = x * chunk + (int)blockIdx.x / nxcd;
    t_step = G / nxcd;
    t_end = min(ntiles, x * chunk + chunk);
  }
  if (w == 0 && t_first < t_end) {
    stage_a(t_first);
    stage_b();
    stage_c();
  }

  for (int t = t_first; t < t_end; t += t_step) {
    const bool has_next = t + t_step < t_end;
    if (w == 0) {  // publish this tile's indices (the previous tile's epilogue ended with a barrier)
      erow[lane] = ce;
      soff[lane] = cs >= 0 ? (int64_t)cs * h : -1;
      qoff[lane] = cq >= 0 ? (int64_t)cq * h : -1;
      if constexpr (AGG != 0) {
        const bool first = lane < cn && cnode != cprev;
        const unsigned long long m = __ballot(first);
        const int k = __popcll(m & ((1ull << lane) - 1ull));
        if (first) {
          nstart[k] = lane;
          nnode[k] = cnode;
        }
        if (lane == 0) {
          nseg = __popcll(m);
          nstart[__popcll(m)] = cn;
        }
      }
      if (has_next) stage_a(t + t_step);
    }

    for (int pass = 0; pass < npass; ++pass) {
      // Column tile j of this wave in this pass is nt = 32 pass + w + 4 j.  Tiles past NTn (last
      // pass only) load a clamped fragment and are never stored: no branch in front of a load.
      const int nt0 = kNTp * pass + w;
      auto boff = [&](int j) { return (nt0 + 4 * j < NTn ? nt0 + 4 * j : NTn - 1) * 64 + lane; };
      // B fragments of the pass's first k step, in flight during the first gather
      uint4 bcur[NW];
#pragma unroll
      for (int j = 0; j < NW; ++j) bcur[j] = Wp[boff(j)];
      f32x4 acc[4][NW];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int j = 0; j < NW; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

      for (int kc = 0; kc < nchunk; ++kc) {
        const int ks0 = kKSc * kc;
        const int ksn = KS - ks0 < kKSc ? KS - ks0 : kKSc;
        // the indices are published (first chunk) / every wave is done with the previous chunk or
        // the previous pass's staging tile
        __syncthreads();
        // ---- 1. gather this chunk of A = S[src] - act(H[rev]) -> bf16 LDS tile [64][<= 512] ----
        {
          const int chunks = ksn * 4;  // 16-B pieces per row in this chunk
          // rows in flight per round: 4, not the narrow kernel's 8, because the accumulators are
          // live across this gather from the second chunk on (8 rows: 260-450 B of scratch per lane)
          constexpr int kRG = 4;
          for (int idx = lane; idx < chunks * (16 / kRG); idx += 64) {
            const int c = idx % chunks, r0 = 16 * w + kRG * (idx / chunks);
            const int k0 = 32 * ks0 + c * 8;
            const int kcl = k0 < h ? k0 : h - 8;  // clamped, unconditional loads
            uint4 sraw[kRG], qraw[kRG];
#pragma unroll
            for (int u = 0; u < kRG; ++u) {
              const int64_t so = soff[r0 + u], qo = qoff[r0 + u];
              sraw[u] = *reinterpret_cast<const uint4*>(S + (so >= 0 ? so : 0) + kcl);
              qraw[u] = *reinterpret_cast<const uint4*>(H + (qo >= 0 ? qo : 0) + kcl);
            }
#pragma unroll
            for (int u = 0; u < kRG; ++u) {
              const int r = r0 + u;
              const bool sok = soff[r] >= 0 && k0 < h, qok = qoff[r] >= 0 && k0 < h;
              const unsigned su[4] = {sraw[u].x, sraw[u].y, sraw[u].z, sraw[u].w};
              const unsigned qu[4] = {qraw[u].x, qraw[u].y, qraw[u].z, qraw[u].w};
              bf16x8 a;
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                const unsigned sb = (i & 1) ? (su[i >> 1] & 0xffff0000u) : (su[i >> 1] << 16);
                const unsigned qb = (i & 1) ? (qu[i >> 1] & 0xffff0000u) : (qu[i >> 1] << 16);
                const float sv = sok ? __uint_as_float(sb) : 0.f;
                const float qv = qok ? __uint_as_float(qb) : 0.f;
                a[i] = (__bf16)(sv - act_t<ACT>(qv, act, alpha));
              }
              *reinterpret_cast<uint4*>(lds + r * kLdaW + c * 16) = __builtin_bit_cast(uint4, a);
            }
          }
        }
        __syncthreads();
        if (w == 0 && has_next && pass == 0 && kc == 0) stage_b();

        // ---- 2. the chunk's MFMAs: acc[mt][j] += rows 16 mt.., columns of tile nt0 + 4 j ----
        const char* arow = lds + (lane & 15) * kLdaW + 16 * (lane >> 4);
        for (int ks = 0; ks < ksn; ++ks) {
          // next global k step's fragments (the last one re-reads its own: no branch, no drain)
          const int kg = ks0 + ks;
          const int64_t kn = (kg + 1 < KS ? kg + 1 : kg) * kstride;
          uint4 bnext[NW];
#pragma unroll
          for (int j = 0; j < NW; ++j) bnext[j] = Wp[kn + boff(j)];
          bf16x8 a[4];
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            a[mt] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(arow + 16 * mt * kLdaW + 64 * ks));
#pragma unroll
          for (int j = 0; j < NW; ++j) {
            const bf16x8 b = __builtin_bit_cast(bf16x8, bcur[j]);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
              acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b, acc[mt][j], 0, 0, 0);
          }
#pragma unroll
          for (int j = 0; j < NW; ++j) bcur[j] = bnext[j];
        }
        if (w == 0 && has_next && pass == 0 && kc == nchunk - 1) stage_c();
      }
      __syncthreads();  // every wave is done with the A tile: its LDS becomes the staging tile

      // ---- 3. epilogue of this pass: 256 columns per round through LDS, + bias + residual ----
      float* stage = reinterpret_cast<float*>(lds);
      // p and jj fully unrolled: acc[][j] must only ever be indexed by constants
#pragma unroll
      for (int p = 0; p < NW / 4; ++p) {
        const int n0 = 16 * kNTp * pass + 256 * p;
        if (n0 >= h) break;
        const int ncols = h - n0 < 256 ? h - n0 : 256;
        // thread (tid) owns column piece c = 8 (tid & 31) of rows (tid >> 5) + 8 it, it < 8; its
        // residual pieces are loaded before the staging round trip so their latency overlaps it
        constexpr int kIt = kM * 32 / kThreads;
        const int cpiece = 8 * (tid & 31);
        const bool cok = cpiece < ncols;
        auto load_res = [&](int it) {
          const int64_t e = erow[(tid >> 5) + 8 * it];
          const bool ok = cok && e >= 0 && residual;
          return *reinterpret_cast<const uint4*>(H + (ok ? e * h + n0 + cpiece : 0));
        };
        uint4 hres[kIt];
#pragma unroll
        for (int it = 0; it < kIt; ++it) hres[it] = load_res(it);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = 4 * p + jj;
          if (nt0 + 4 * j < NTn) {
            const int sc = 16 * w + 64 * jj + (lane & 15);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
              for (int r = 0; r < 4; ++r) stage[(16 * mt + 4 * (lane >> 4) + r) * kSO + sc] = acc[mt][j][r];
          }
        }
        __syncthreads();
        float bb[8];
        if (bias && cok) load_chunk<8>(bias + n0 + cpiece, bb);
        else for (int q = 0; q < 8; ++q) bb[q] = 0.f;
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
          const int r = (tid >> 5) + 8 * it;
          const int64_t e = erow[r];
          if (cok && e >= 0) {
            float* st = stage + r * kSO + cpiece;
            const uint4 hr = hres[it];
            const unsigned hu[4] = {hr.x, hr.y, hr.z, hr.w};
            float y[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const unsigned hb = (q & 1) ? (hu[q >> 1] & 0xffff0000u) : (hu[q >> 1] << 16);
              float u = st[q] + bb[q];
              if constexpr (DROP) u = drop_apply(drop, (uint64_t)(e * h + n0 + cpiece + q), u);
              y[q] = u + (residual ? __uint_as_float(hb) : 0.f);
            }
            store_chunk<8>(out + e * h + n0 + cpiece, y);
            if constexpr (AGG != 0) {  // the aggregation reads the stored (bf16) value, as unfused
#pragma unroll
              for (int q = 0; q < 8; ++q) st[q] = AGG == 2 ? act_t<ACT>(rbf(y[q]), act, alpha) : rbf(y[q]);
            }
          }
        }
        if constexpr (AGG != 0) {
          __syncthreads();
          for (int k = tid >> 5; k < nseg; k += kThreads / 32) {
            if (!cok) continue;
            float y[8];
            switch (agg.reduce) {
              case NT_SUM: reduce_rows<NT_SUM>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
              case NT_MEAN: reduce_rows<NT_MEAN>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
              case NT_MAX: reduce_rows<NT_MAX>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
              default: reduce_rows<NT_MIN>(stage, nstart[k], nstart[k + 1], cpiece, y); break;
            }
            store_chunk<8>(agg.S_out + (int64_t)nnode[k] * h + n0 + cpiece, y);
          }
        }
        __syncthreads();
      }
    }  // column passes
  }  // tile loop
}

static bool valid_reduce(int r) { return r >= NT_SUM && r <= NT_MIN; }

#define NT_BF_DISPATCH_A(ACT, LAUNCH)                                            \
  do {                                                                           \
    if ((ACT) == NT_ACT_IDENTITY) { constexpr int A_ = NT_ACT_IDENTITY; LAUNCH; } \
    else if ((ACT) == NT_ACT_RELU) { constexpr int A_ = NT_ACT_RELU; LAUNCH; }    \
    else { constexpr int A_ = -1; LAUNCH; }                                      \
  } while (0)
#define NT_BF_DISPATCH_RA(REDUCE, ACT, LAUNCH)                                                  \
  do {                                                                                          \
    switch (REDUCE) {                                                                           \
      case NT_SUM: { constexpr int R_ = NT_SUM; NT_BF_DISPATCH_A(ACT, LAUNCH); } break;   \
      case NT_MEAN: { constexpr int R_ = NT_MEAN; NT_BF_DISPATCH_A(ACT, LAUNCH); } break; \
      case NT_MAX: { constexpr int R_ = NT_MAX; NT_BF_DISPATCH_A(ACT, LAUNCH); } break;   \
      case NT_MIN: { constexpr int R_ = NT_MIN; NT_BF_DISPATCH_A(ACT, LAUNCH); } break;   \
    }                                                                                           \
  } while (0)

template <int ACT, int W, int NW, int AGG, bool DROP = false>
int launch_upd(const void* H, const void* S, const int64_t* src, const int64_t* rev, const void* Wp,
               const void* b, int64_t V, int64_t E, int64_t h, int residual, int act, float alpha,
               void* H_out, int64_t grid, const BfAgg& agg, hipStream_t stream, const DropMask& drop = DropMask{}) {
  const int KS = (int)((h + 31) / 32), NTn = (int)((h + 15) / 16);
  const int lds = lds_bytes_bf16(KS);
  auto kern = update_bf16_kernel<ACT, W, NW, AGG, DROP>;
  if (lds > 64 * 1024)
    NT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const int64_t slots = 2 * (int64_t)cu_count();  // two resident workgroups per CU (LDS-bound)
  const int64_t g = grid < slots ? grid : slots;
  set_last_kernel(DROP ? "update_bf16_kernel: two 4-wave workgroups per CU, 64-edge tiles, dropout in the epilogue"
                  : W == 4 ? "update_bf16_kernel: two 4-wave workgroups per CU, 64-edge tiles, 8-byte row pieces"
                           : "update_bf16_kernel: two 4-wave workgroups per CU, 64-edge tiles");
  kern<<<(unsigned)g, kThreads, lds, stream>>>(
      (const bf16_t*)H, (const bf16_t*)S, src, rev, (const uint4*)Wp, (const bf16_t*)b, V, E, (int)h,
      KS, NTn, residual, act, alpha, (bf16_t*)H_out, agg, (int)grid, xcd_count(), drop);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

}  // namespace

int launch_segment_reduce_bf16(const void* X, const int32_t* seg_ptr, const int32_t* perm,
                               int64_t nseg, int64_t h, int reduce, int act, float alpha, void* out,
                               hipStream_t stream) {
  NT_REQUIRE(valid_reduce(reduce), NT_EINVAL, "bad reduce code");
  const int vec = row_piece(h, aligned16(X) && aligned16(out));
  if (vec == 8) {
    const int grid = grid_for(nseg * (h / 8), 256, 256 * 32);
    NT_BF_DISPATCH_RA(reduce, act,
                      (segment_reduce_bf16<R_, A_, 8><<<grid, 256, 0, stream>>>(
                          (const bf16_t*)X, seg_ptr, perm, nseg, h, act, alpha, (bf16_t*)out)));
  } else if (vec == 4) {
    const int grid = grid_for(nseg * (h / 4), 256, 256 * 32);
    NT_BF_DISPATCH_RA(reduce, act,
                      (segment_reduce_bf16<R_, A_, 4><<<grid, 256, 0, stream>>>(
                          (const bf16_t*)X, seg_ptr, perm, nseg, h, act, alpha, (bf16_t*)out)));
  } else {
    const int grid = grid_for(nseg * h, 256, 256 * 32);
    NT_BF_DISPATCH_RA(reduce, act,
                      (segment_reduce_bf16<R_, A_, 1><<<grid, 256, 0, stream>>>(
                          (const bf16_t*)X, seg_ptr, perm, nseg, h, act, alpha, (bf16_t*)out)));
  }
  NT_LAUNCH_CHECK();
  return NT_OK;
}

int launch_init_bf16(const void* Xv, const void* Xe, const int64_t* src, const int32_t* seg_ptr,
                     const int32_t* perm, int64_t V, int64_t E, int64_t h, int act, float alpha,
                     int reduce, void* H0, void* S, hipStream_t stream) {
  NT_REQUIRE(valid_reduce(reduce), NT_EINVAL, "bad reduce code");
  const int vec = row_piece(h, aligned16(Xv) && aligned16(Xe) && aligned16(H0) && (S == nullptr || aligned16(S)));
  if (S != nullptr) {
    if (V == 0) return NT_OK;
    NT_REQUIRE(seg_ptr && (perm || E == 0), NT_EINVAL, "fused aggregation needs the dst CSR");
    NT_REQUIRE(E == 0 || (Xv && Xe && src && H0), NT_EINVAL, "NULL pointer");
    if (vec == 8) {
      const int grid = grid_for(V * (h / 8), 256, 256 * 32);
      NT_BF_DISPATCH_RA(reduce, act,
                        (init_aggregate_bf16<R_, A_, 8><<<grid, 256, 0, stream>>>(
                            (const bf16_t*)Xv, (const bf16_t*)Xe, src, seg_ptr, perm, V, h, act,
                            alpha, (bf16_t*)H0, (bf16_t*)S)));
    } else if (vec == 4) {
      const int grid = grid_for(V * (h / 4), 256, 256 * 32);
      NT_BF_DISPATCH_RA(reduce, act,
                        (init_aggregate_bf16<R_, A_, 4><<<grid, 256, 0, stream>>>(
                            (const bf16_t*)Xv, (const bf16_t*)Xe, src, seg_ptr, perm, V, h, act,
                            alpha, (bf16_t*)H0, (bf16_t*)S)));
    } else {
      const int grid = grid_for(V * h, 256, 256 * 32);
      NT_BF_DISPATCH_RA(reduce, act,
                        (init_aggregate_bf16<R_, A_, 1><<<grid, 256, 0, stream>>>(
                            (const bf16_t*)Xv, (const bf16_t*)Xe, src, seg_ptr, perm, V, h, act,
                            alpha, (bf16_t*)H0, (bf16_t*)S)));
    }
  } else {
    if (E == 0) return NT_OK;
    NT_REQUIRE(Xv && Xe && src && H0, NT_EINVAL, "NULL pointer");
    if (vec == 8)
      init_only_bf16<8><<<grid_for(E * (h / 8), 256, 256 * 32), 256, 0, stream>>>(
          (const bf16_t*)Xv, (const bf16_t*)Xe, src, E, h, (bf16_t*)H0);
    else if (vec == 4)
      init_only_bf16<4><<<grid_for(E * (h / 4), 256, 256 * 32), 256, 0, stream>>>(
          (const bf16_t*)Xv, (const bf16_t*)Xe, src, E, h, (bf16_t*)H0);
    else
      init_only_bf16<1><<<grid_for(E * h, 256, 256 * 32), 256, 0, stream>>>(
          (const bf16_t*)Xv, (const bf16_t*)Xe, src, E, h, (bf16_t*)H0);
  }
  NT_LAUNCH_CHECK();
  return NT_OK;
}

size_t bf16_image_bytes(int64_t h) {
  const int64_t KS = (h + 31) / 32, NTn = (h + 15) / 16;
  return (size_t)KS * NTn * 64 * 16;
}

int pack_weight_bf16(const void* W, int64_t nlayers, int64_t h, int64_t layer_stride_bytes, void* Wp,
                     hipStream_t stream) {
  NT_REQUIRE(layer_stride_bytes % 16 == 0, NT_EINVAL, "internal: layer stride");
  const int KS = (int)((h + 31) / 32), NTn = (int)((h + 15) / 16);
  const int64_t total = nlayers * KS * NTn * 64;
  pack_bf16<<<grid_for(total, 256), 256, 0, stream>>>((const bf16_t*)W, nlayers, h, KS, NTn,
                                                      layer_stride_bytes / 16, (uint4*)Wp);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

template <int ACT, int W, int AGG, bool DROP = false>
static int launch_upd_nw(const void* H, const void* S, const int64_t* src, const int64_t* rev,
                         const void* Wp, const void* b, int64_t V, int64_t E, int64_t h, int residual,
                         int act, float alpha, void* H_out, int64_t grid, const BfAgg& agg,
                         hipStream_t stream, const DropMask& drop = DropMask{}) {
  const int nw = (int)(((h + 15) / 16 + 3) / 4);
  switch (nw) {
#define NT_NW(N)                                                                                  \
  case N:                                                                                         \
    return launch_upd<ACT, W, N, AGG, DROP>(H, S, src, rev, Wp, b, V, E, h, residual, act, alpha, H_out, \
                                            grid, agg, stream, drop);
    NT_NW(1) NT_NW(2) NT_NW(3) NT_NW(4) NT_NW(5) NT_NW(6) NT_NW(7) NT_NW(8)
#undef NT_NW
  }
  set_error("bf16 update: no kernel for this hidden size");
  return NT_EUNSUPPORTED;
}

// h > 512: the column-pass / K-chunk kernel (whole 16-B pieces only)
template <int ACT, int AGG, bool DROP = false>
static int launch_upd_wide(const void* H, const void* S, const int64_t* src, const int64_t* rev,
                           const void* Wp, const void* b, int64_t V, int64_t E, int64_t h, int residual,
                           int act, float alpha, void* H_out, int64_t grid, const BfAgg& agg,
                           hipStream_t stream, const DropMask& drop = DropMask{}) {
  const int KS = (int)((h + 31) / 32), NTn = (int)((h + 15) / 16);
  auto kern = update_bf16_wide_kernel<ACT, AGG, DROP>;
  NT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsW));
  const int64_t slots = 2 * (int64_t)cu_count();
  const int64_t g = grid < slots ? grid : slots;
  set_last_kernel(DROP ? "update_bf16_kernel: wide (h > 512), column passes x K chunks of 512, 64-edge tiles, "
                         "dropout in the epilogue"
                       : "update_bf16_kernel: wide (h > 512), column passes x K chunks of 512, 64-edge tiles");
  kern<<<(unsigned)g, kThreads, kLdsW, stream>>>(
      (const bf16_t*)H, (const bf16_t*)S, src, rev, (const uint4*)Wp, (const bf16_t*)b, V, E, (int)h,
      KS, NTn, residual, act, alpha, (bf16_t*)H_out, agg, (int)grid, xcd_count(), drop);
  NT_LAUNCH_CHECK();
  return NT_OK;
}

bool bf16_update_supported(int64_t h) {
  return h >= 1 && (h <= 4 * kNWMax * 16 || (h % 8 == 0 && h <= 8192));
}

int launch_update_bf16(const void* H, const void* S, const int64_t* src, const int64_t* rev,
                       const void* Wp, const void* b, int64_t V, int64_t E, int64_t h, int residual,
                       int act, float alpha, void* H_out, hipStream_t stream) {
  NT_REQUIRE(bf16_update_supported(h), NT_EUNSUPPORTED, NT_BF16_H_RULE);
  const int64_t grid = (E + kM - 1) / kM;
  NT_REQUIRE(grid < (int64_t(1) << 31), NT_EINVAL, "too many edges");
  const int vec = row_piece(h, aligned16(H) && aligned16(S) && aligned16(H_out) && (b == nullptr || aligned16(b)));
  const BfAgg none{nullptr, nullptr, nullptr, 0, 0, 0.f, nullptr};
  if (h > 4 * kNWMax * 16) {
    NT_REQUIRE(vec == 8, NT_EINVAL, "bf16 with h > 512 needs 16-byte aligned feature pointers");
    NT_BF_DISPATCH_A(act, return (launch_upd_wide<A_, 0>(H, S, src, rev, Wp, b, V, E, h, residual, act,
                                                         alpha, H_out, grid, none, stream)));
  }
  if (vec == 8)
    NT_BF_DISPATCH_A(act, return (launch_upd_nw<A_, 8, 0>(H, S, src, rev, Wp, b, V, E, h, residual,
                                                              act, alpha, H_out, grid, none, stream)));
  else if (vec == 4)
    NT_BF_DISPATCH_A(act, return (launch_upd_nw<A_, 4, 0>(H, S, src, rev, Wp, b, V, E, h, residual,
                                                              act, alpha, H_out, grid, none, stream)));
  else
    NT_BF_DISPATCH_A(act, return (launch_upd_nw<A_, 1, 0>(H, S, src, rev, Wp, b, V, E, h, residual,
                                                              act, alpha, H_out, grid, none, stream)));
  return NT_OK;
}

bool bf16_fused_supported(int64_t h) {
  return (h % 8 == 0 && h >= 8 && h <= 8192) || (h % 4 == 0 && h >= 4 && h <= 4 * kNWMax * 16);
}

int launch_update_bf16_fused(const void* H, const void* S, const int64_t* src, const int64_t* rev,
                             const void* Wp, const void* b, int64_t V, int64_t E, int64_t h,
                             int residual, int act, float alpha, const int32_t* tile_ptr,
                             int64_t ntiles, const int32_t* perm, const int32_t* dsts, int reduce,
                             int aact, float aalpha, void* H_out, void* S_out, hipStream_t stream,
                             const DropMask* drop) {
  NT_REQUIRE(drop == nullptr || tile_ptr != nullptr, NT_EUNSUPPORTED, "the dropout layer kernel needs a tile plan");
  if (tile_ptr == nullptr)  // no plan: the plain (unfused) kernel computes H_out only
    return launch_update_bf16(H, S, src, rev, Wp, b, V, E, h, residual, act, alpha, H_out, stream);
  NT_REQUIRE(bf16_fused_supported(h) && (drop == nullptr || h % 8 == 0), NT_EUNSUPPORTED,
             "bf16 update_fused needs " NT_BF16_FUSED_H_RULE);
  NT_REQUIRE(perm && dsts && S_out && aligned16(S_out), NT_EINVAL, "fused aggregation needs perm, "
             "dst_sorted and a 16-byte aligned S_out");
  NT_REQUIRE(ntiles > 0 && ntiles < (int64_t(1) << 31), NT_EINVAL, "bad ntiles");
  // the kernel applies either identity (final node scatter) or this layer's own act (the next
  // layer's aggregation, which ChempropBlock guarantees uses the same activation)
  NT_REQUIRE(aact == NT_ACT_IDENTITY || (aact == act && aalpha == alpha), NT_EUNSUPPORTED,
             "bf16 update_fused: agg_act must be identity or equal to act");
  const BfAgg agg{tile_ptr, perm, dsts, reduce, aact, aalpha, (bf16_t*)S_out};
  if (drop) {
    // the same kernels, the update masked before the residual is added; relu or the run-time
    // activation switch (identity included) to keep the instance count down
#define NT_BF_DROP(KERN, ...)                                                                              \
  return act == NT_ACT_RELU ? KERN<NT_ACT_RELU, __VA_ARGS__>(H, S, src, rev, Wp, b, V, E, h, residual, act, \
                                                             alpha, H_out, ntiles, agg, stream, *drop)     \
                            : KERN<-1, __VA_ARGS__>(H, S, src, rev, Wp, b, V, E, h, residual, act, alpha,  \
                                                    H_out, ntiles, agg, stream, *drop)
    if (h > 4 * kNWMax * 16) {
      if (aact == NT_ACT_IDENTITY) NT_BF_DROP(launch_upd_wide, 1, true);
      NT_BF_DROP(launch_upd_wide, 2, true);
    }
    if (aact == NT_ACT_IDENTITY) NT_BF_DROP(launch_upd_nw, 8, 1, true);
    NT_BF_DROP(launch_upd_nw, 8, 2, true);
#undef NT_BF_DROP
  }
  if (h > 4 * kNWMax * 16) {
    NT_REQUIRE(aligned16(H) && aligned16(S) && aligned16(H_out) && (b == nullptr || aligned16(b)), NT_EINVAL,
               "bf16 with h > 512 needs 16-byte aligned feature pointers");
    if (aact == NT_ACT_IDENTITY)
      NT_BF_DISPATCH_A(act, return (launch_upd_wide<A_, 1>(H, S, src, rev, Wp, b, V, E, h, residual, act,
                                                           alpha, H_out, ntiles, agg, stream)));
    else
      NT_BF_DISPATCH_A(act, return (launch_upd_wide<A_, 2>(H, S, src, rev, Wp, b, V, E, h, residual, act,
                                                           alpha, H_out, ntiles, agg, stream)));
  }
  if (h % 8 != 0) {  // whole 8-B pieces (h % 4 == 0, h <= 512)
    NT_REQUIRE(aligned16(H) && aligned16(S) && aligned16(H_out) && (b == nullptr || aligned16(b)), NT_EINVAL,
               "bf16 update_fused needs 16-byte aligned feature pointers");
    if (aact == NT_ACT_IDENTITY)
      NT_BF_DISPATCH_A(act, return (launch_upd_nw<A_, 4, 1>(H, S, src, rev, Wp, b, V, E, h, residual,
                                                            act, alpha, H_out, ntiles, agg, stream)));
    else
      NT_BF_DISPATCH_A(act, return (launch_upd_nw<A_, 4, 2>(H, S, src, rev, Wp, b, V, E, h, residual,
                                                            act, alpha, H_out, ntiles, agg, stream)));
  }
  if (aact == NT_ACT_IDENTITY)
    NT_BF_DISPATCH_A(act, return (launch_upd_nw<A_, 8, 1>(H, S, src, rev, Wp, b, V, E, h, residual,
                                                          act, alpha, H_out, ntiles, agg, stream)));
  else
    NT_BF_DISPATCH_A(act, return (launch_upd_nw<A_, 8, 2>(H, S, src, rev, Wp, b, V, E, h, residual,
                                                          act, alpha, H_out, ntiles, agg, stream)));
  return NT_OK;
}

}  // namespace nt
