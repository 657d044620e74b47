// Internal interface between the nt_dmpnn_update* entry points (update_f32.hip) and the fk launchers
// (update_fk.hip).
#pragma once

#include <utility>

#include "common.hpp"
#include "dropout.hpp"

namespace nt {

struct UpdateArgs {
  const float* H;
  const float* S;
  const int64_t* src;
  const int64_t* rev;
  const void* Wp;   // packed fragment image (nt_dmpnn_pack_weight)
  const float* b;   // may be NULL
  int64_t V, E, h;
  int KB, NT;       // 16-deep k blocks, 16-wide column tiles
  int residual, act;
  float alpha;
  float* H_out;
  hipStream_t stream;
  // row pitches in elements (0: dense rows of h): H and S inputs, H_out and S_out outputs (fp32 fused
  // layer kernel only)
  int64_t ldi = 0, ldo = 0;
  float* S_part = nullptr;  // fused fp32: hub partial rows (row table entries < 0), see nt_dmpnn_update_fused
};

// fp16x3 persistent layer kernel (update_fk.hpp, built in update_fk.hip): any h % 4 == 0; tiles of
// at most fk_tile_rows(h, act, reduce, aact, fused) rows; Wimg = the fk image of the layer (header + fragment blocks).
int fk_tile_rows(int64_t h, int act, int reduce, int aact, bool fused);
// drop (fused plans only): the update passes this dropout mask before the residual is added
int launch_update_fk(const UpdateArgs& u, const void* Wimg, const float* amax_in, float* amax_out,
                     const int32_t* tile_ptr, int64_t ntiles, int tile_rows, int max_in_degree,
                     const void* row_table, int reduce, int aact, float aalpha, float* S_out,
                     const DropMask* drop = nullptr);
// fk images of nlayers separate weights (<= 16) and optionally of their transposes, one launch pair
int fk_pack_multi(const float* const* W, int64_t nlayers, int64_t h, char* const* img, char* const* imgT,
                  hipStream_t stream);
int fk_row_table(const int32_t* perm, const int32_t* dsts, const int64_t* src, const int64_t* rev, int64_t V,
                 int64_t E, void* out, hipStream_t stream);
int fk_pack(const float* W, int64_t nlayers, int64_t h, int64_t w_stride, int64_t img_stride, void* img,
            hipStream_t stream);
int fk_absmax(const float* X, int64_t n, float* out, hipStream_t stream);
// the caller's 2-float workspace ws := (max|H|, max|S|) on `stream` (H or S may be NULL: that entry is 0)
int amax_fill(float* ws, const float* H, int64_t nh, const float* S, int64_t ns, hipStream_t stream);
// bf16 storage on the same skeleton (PREC = 1): h % 8 == 0, h <= 512, tiles of <= 128 rows, Wimg =
// the bf16 fragment image; S_out / the row table exactly with a tile plan
bool fkb_supported(int64_t h);
int bf16_kernel_env();  // NT_BF16_KERNEL, read once: 0 default, 1 fk, 2 fk4
int launch_update_fk_bf16(const UpdateArgs& u, const void* Wimg, const int32_t* tile_ptr, int64_t ntiles,
                          int tile_rows, int max_in_degree, const void* row_table, int reduce, int aact,
                          float aalpha, void* S_out);
inline int64_t fk_image_bytes(int64_t h) { return 256 + ((h + 31) / 32) * ((h + 15) / 16) * 2 * 1024; }

}  // namespace nt
