// What the input kernels of input_ops.hip and input_resample.hip share: the staging limit, the normalisation and
// the store of a pixel, a sample's crop box and its source image, and the launch shapes.
#pragma once
#include "common.h"

namespace dbx {

constexpr int kRowMax = 4096;  // bytes of a source row that can be staged in LDS

// ----------------------------------------------------------------------------------------
// normalisation of a 0..255 value: (v/255 - mean)/std as v * 1/(255 std) - mean/std
// ----------------------------------------------------------------------------------------
struct Norm {
  float m0, m1, m2, s0, s1, s2, i0, i1, i2;
};
__device__ __forceinline__ Norm make_norm(float m0, float m1, float m2, float s0, float s1, float s2) {
  return Norm{m0, m1, m2, s0, s1, s2, 1.f / (255.f * s0), 1.f / (255.f * s1), 1.f / (255.f * s2)};
}
__device__ __forceinline__ void normalise(const Norm& nm, const float (&v)[3], float (&f)[3]) {
  f[0] = v[0] * nm.i0 - nm.m0 / nm.s0; f[1] = v[1] * nm.i1 - nm.m1 / nm.s1; f[2] = v[2] * nm.i2 - nm.m2 / nm.s2;
}
__device__ __forceinline__ void store_px(bf16* __restrict__ out, int row, int Wo, int ox, const float (&f)[3]) {
  bf16x4 o = {(bf16)f[0], (bf16)f[1], (bf16)f[2], (bf16)0.f};  // the pad channel: 0
  *reinterpret_cast<bf16x4*>(out + ((size_t)row * Wo + ox) * 4) = o;
}

struct AugBox {  // a source sample's crop box (y0, x0, h; sxs = w / Wo) and flip: read once per sample
  int sn;
  float by, bx, bh, sxs;
  bool fl;
};
__device__ __forceinline__ AugBox aug_box(const float* __restrict__ boxes, const unsigned char* __restrict__ flip, int sn,
                                          int Wo) {
  return AugBox{sn, boxes[4 * sn], boxes[4 * sn + 1], boxes[4 * sn + 2], boxes[4 * sn + 3] / Wo, flip && flip[sn]};
}
// One source image: where its rows are, its size and the bytes from one row to the next. Dense batch
// [N][Hin][Win][Cin]: sample sn of it (base = the batch, rows sn Hin + y: the addressing these kernels always had). Ragged batch: a byte arena of `arena16` 16-byte units and the table tab int32 [N][4] =
// (offset / 16, H, W, stride) (data/loader.py pack_layout: stride = ceil16(W Cin), offsets the running sum of
// H stride, so every row starts 16-byte aligned and a row of at most kRowMax bytes can be staged). A table row is
// unusable when its extent leaves the arena, H < 1, W < 1, stride < W Cin or stride % 16 != 0; it is then read as
// the row (0, 1, 1, 16) -- the arena's first pixel -- and never dereferenced (base = the image, sn = 0).
// Block-uniform either way.
struct SrcImg {
  const unsigned char* base;
  int sn, H, W, rb;
};
template <bool RAGGED>
__device__ __forceinline__ SrcImg src_img(const unsigned char* __restrict__ in, const int* __restrict__ tab,
                                          long long arena16, int sn, int Hin, int Win, int Cin) {
  if constexpr (!RAGGED) {
    return SrcImg{in, sn, Hin, Win, Win * Cin};
  } else {
    const long long off = tab[4 * sn];
    const int H = tab[4 * sn + 1], W = tab[4 * sn + 2], rb = tab[4 * sn + 3];
    const bool ok = off >= 0 && H >= 1 && W >= 1 && (rb & 15) == 0 && (long long)rb >= (long long)W * Cin &&
                    off + (((long long)H * rb) >> 4) <= arena16;
    return ok ? SrcImg{in + (size_t)off * 16, 0, H, W, rb} : SrcImg{in, 0, 1, 1, 16};
  }
}

}  // namespace dbx

// one block per output row (crop_resize_u8: per chunk of rows), at most 4096; a wave per 64 output columns
static inline dim3 row_grid(long long rows) { return dim3((unsigned)(rows < 4096 ? rows : 4096)); }
static inline dim3 row_block(int Wo) { return dim3(Wo >= 256 ? 256 : ((Wo + 63) / 64) * 64); }
