// The input stage of the native step (gfx950): uint8 NHWC images -> the bf16 NHWC4 batch the stem reads.
//
//   normalize_u8     (x/255 - mean)/std, optional flip, pad channel 0
//   augment_u8       per-sample crop box resized to Ho x Wo (bilinear, pixel-centre convention, edge clamp),
//                    optional flip, normalised: RandomResizedCrop / RandomCrop(pad) / Resize / CenterCrop +
//                    RandomHorizontalFlip + Normalize of the reference's CPU transform chains (SURVEY.md §2.4
//                    K20), and the CutMix paste (K18)
//   augment_mix_u8   its mixing form: the MixUp blend and random erasing on top
//   crop_resize_u8, ta_prepare, ta_apply_u8
//                    TrivialAugmentWide between the crop and the normalisation (see the section below)
//   ta_stage_u8      one more uint8 operation between ta_prepare and ta_apply_u8: the chains of RandAugment and
//                    AutoAugment
//
// Mixing (augment_mix_u8 and ta_apply_u8). With f_s(oy, ox) the normalised fp32 pixel of source sample s --
// the erase value where (oy, ox) lies in erase[s] = (y0, y1, x0, x1), output coordinates --
//   out[n] = f_perm[n]                              inside mixbox
//          = bf16(w f_n + (1 - w) f_perm[n])        elsewhere, w = blend[0] read from memory
// Erasing (and the TrivialAugment operation) belongs to the source sample (torchvision / timm erase before
// they mix; Composer pastes after the per-sample transforms), so it travels with a pasted or blended sample.
// w == 1 never reads the second sample (block-uniform) and then, like an all-empty erase table, gives the
// plain kernel's bits. Erase value: 0 (pixel == 0), or one N(0, 1) draw per pixel and channel from the Philox
// counter pix = (s Ho + oy) Wo + ox (Box-Muller on its four words, precise logf / sqrtf / cospif / sinpif): a
// function of (seed, offset, source sample, position), so a copy of a sample carries its noise.
//
// Every piece the kernels share -- row geometry, row staging, the bilinear sample, the normalisation, the
// erase value, the mixing state and its column loop -- is one __forceinline__ function below. None of them may
// sit inside a `#pragma clang fp contract(off)` scope (only the three TrivialAugment functions that carry it do).
#include "common.h"
#include "philox.h"
#include "entry.h"

namespace dbx {

constexpr int kRowMax = 4096;  // bytes of a source row that can be staged in LDS
constexpr int kTaRows = 16;    // output rows per block of crop_resize_u8
constexpr int kTile = 1024;    // output columns per pass of ta_apply_u8
constexpr int kTaKinds = 14;

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

// ----------------------------------------------------------------------------------------
// crop / resize: what is uniform over one output row of one source sample (with the row's erased columns of
// that sample), the staging of its two source rows in LDS with 16-byte loads (the bilinear taps are byte
// gathers), and the sample at one column
// ----------------------------------------------------------------------------------------
struct MixSrc {  // a source sample of an output row and the row's erased columns of it (empty: none)
  int s, ex0, ex1;
};
__device__ __forceinline__ MixSrc mix_src(const int* __restrict__ erase, int s, int oy) {
  MixSrc r{s, 0, 0};
  if (erase && oy >= erase[4 * s] && oy < erase[4 * s + 1]) {  // (an empty box erases no column either)
    r.ex0 = erase[4 * s + 2]; r.ex1 = erase[4 * s + 3];
  }
  return r;
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

struct AugRow {
  const unsigned char *g0, *g1;
  float bx, sxs, wy;
  int W, rb;  // the source's width and the bytes of a row of it
  bool fl;
  MixSrc src;
};
// `erase`: the erase table of the mixing form, else null
template <bool RAGGED>
__device__ __forceinline__ AugRow aug_row(const SrcImg& im, const AugBox& b, const int* __restrict__ erase, int oy,
                                          int Cin, int Ho) {
  AugRow r;
  r.bx = b.bx;
  r.fl = b.fl;
  float sy = b.by + (oy + 0.5f) * b.bh / Ho - 0.5f;
  sy = fminf(fmaxf(sy, 0.f), (float)(im.H - 1));
  const int y0 = (int)sy, y1 = min(y0 + 1, im.H - 1);
  r.wy = sy - y0;
  if constexpr (RAGGED) {
    r.g0 = im.base + (size_t)y0 * im.rb;
    r.g1 = im.base + (size_t)y1 * im.rb;
  } else {
    r.g0 = im.base + ((size_t)im.sn * im.H + y0) * im.W * Cin;
    r.g1 = im.base + ((size_t)im.sn * im.H + y1) * im.W * Cin;
  }
  r.W = im.W;
  r.rb = im.rb;
  r.sxs = b.sxs;
  r.src = mix_src(erase, b.sn, oy);
  return r;
}

// Stages A's two rows of A.rb bytes in srow[0..1] (and, with `two`, P's of P.rb bytes in srow[2..3]) when all can
// be: they fit and the 16-byte loads are aligned. Block-uniform; false: the caller gathers from global memory.
// Dense: both sources have the batch's row bytes. Ragged: each its own (a multiple of 16 by the table's guard).
template <bool RAGGED>
__device__ __forceinline__ bool stage_rows(unsigned char (*srow)[kRowMax], const AugRow& A, const AugRow& P, bool two) {
  const int rb = A.rb;
  bool staged = rb <= kRowMax && (rb & 15) == 0 &&
                (((size_t)A.g0 | (size_t)A.g1 | (size_t)P.g0 | (size_t)P.g1) & 15) == 0;
  if constexpr (RAGGED) staged = staged && P.rb <= kRowMax && (P.rb & 15) == 0;
  if (staged) {
    if constexpr (!RAGGED) {
      for (int o = threadIdx.x * 16; o < rb; o += blockDim.x * 16) {
        *reinterpret_cast<u32x4*>(&srow[0][o]) = *reinterpret_cast<const u32x4*>(A.g0 + o);
        *reinterpret_cast<u32x4*>(&srow[1][o]) = *reinterpret_cast<const u32x4*>(A.g1 + o);
        if (two) {
          *reinterpret_cast<u32x4*>(&srow[2][o]) = *reinterpret_cast<const u32x4*>(P.g0 + o);
          *reinterpret_cast<u32x4*>(&srow[3][o]) = *reinterpret_cast<const u32x4*>(P.g1 + o);
        }
      }
    } else {
      // one loop over the longer row, all four loads of a thread in flight together as in the dense form: past the
      // end of the shorter row the offset is clamped to its last 16 bytes (rb >= 16), which are staged again with
      // the same bytes
      const int rbp = two ? P.rb : rb, rbm = max(rb, rbp);
      for (int o = threadIdx.x * 16; o < rbm; o += blockDim.x * 16) {
        const int oa = min(o, rb - 16), op = min(o, rbp - 16);
        *reinterpret_cast<u32x4*>(&srow[0][oa]) = *reinterpret_cast<const u32x4*>(A.g0 + oa);
        *reinterpret_cast<u32x4*>(&srow[1][oa]) = *reinterpret_cast<const u32x4*>(A.g1 + oa);
        if (two) {
          *reinterpret_cast<u32x4*>(&srow[2][op]) = *reinterpret_cast<const u32x4*>(P.g0 + op);
          *reinterpret_cast<u32x4*>(&srow[3][op]) = *reinterpret_cast<const u32x4*>(P.g1 + op);
        }
      }
    }
    __syncthreads();
  }
  return staged;
}

// each(c, v), v in 0..255: the bilinear sample of output column ox from the row's two source rows r0 / r1, channel
// by channel (crop_resize_u8 rounds each value where it is made); below, all three into v[]
template <typename Each>
__device__ __forceinline__ void bilinear(const AugRow& r, const unsigned char* r0, const unsigned char* r1, int ox,
                                         int Cin, int Wo, Each each) {
  const int oxx = r.fl ? (Wo - 1 - ox) : ox;
  float sx = r.bx + (oxx + 0.5f) * r.sxs - 0.5f;
  sx = fminf(fmaxf(sx, 0.f), (float)(r.W - 1));
  const int x0 = (int)sx, x1 = min(x0 + 1, r.W - 1);
  const float wx = sx - x0, wy = r.wy;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int cc = Cin == 1 ? 0 : c;
    const float a = r0[x0 * Cin + cc], b = r0[x1 * Cin + cc];
    const float d = r1[x0 * Cin + cc], e = r1[x1 * Cin + cc];
    each(c, (a * (1.f - wx) + b * wx) * (1.f - wy) + (d * (1.f - wx) + e * wx) * wy);
  }
}
__device__ __forceinline__ void bilinear(const AugRow& r, const unsigned char* r0, const unsigned char* r1, int ox,
                                         int Cin, int Wo, float (&v)[3]) {
  bilinear(r, r0, r1, ox, Cin, Wo, [&](int c, float x) __attribute__((always_inline)) { v[c] = x; });
}

// ----------------------------------------------------------------------------------------
// mixing: the CutMix box, the erase value, a row's state and its column loop
// ----------------------------------------------------------------------------------------
struct MixBox {  // batch-wide [y0, y1) x [x0, x1), output coordinates; empty without a table
  int y0, y1, x0, x1;
};
__device__ __forceinline__ MixBox mix_box(const int* __restrict__ mixbox) {
  return MixBox{mixbox ? mixbox[0] : 0, mixbox ? mixbox[1] : 0, mixbox ? mixbox[2] : 0, mixbox ? mixbox[3] : 0};
}

struct AugMix {
  const float* blend;     // fp32[1]; null: 1
  const int* erase;       // int32 [N][4]; null: none
  const int* rng_offset;  // int32[1] (pixel mode)
  unsigned long long seed;
  int pixel;
};

__device__ __forceinline__ void erase_value(unsigned long long seed, unsigned roff, int s, int oy, int ox, int Ho,
                                            int Wo, int pixel, float (&f)[3]) {
  f[0] = f[1] = f[2] = 0.f;
  if (pixel) {
    unsigned u[4];
    philox4x32_10(((unsigned long long)s * Ho + oy) * Wo + ox, seed, roff, u);
    const float k24 = 1.f / 16777216.f;
    const float r01 = sqrtf(-2.f * logf((float)((u[0] >> 8) + 1u) * k24));
    const float a01 = 2.f * ((float)(u[1] >> 8) * k24);
    f[0] = r01 * cospif(a01);
    f[1] = r01 * sinpif(a01);
    f[2] = sqrtf(-2.f * logf((float)((u[2] >> 8) + 1u) * k24)) * cospif(2.f * ((float)(u[3] >> 8) * k24));
  }
}

struct Mix {  // grid-uniform
  MixBox box;
  float w;
  bool blendrow;
  unsigned roff;
};
__device__ __forceinline__ Mix make_mix(const int* __restrict__ perm, const int* __restrict__ mixbox, const AugMix& am) {
  Mix m;
  m.box = mix_box(mixbox);
  m.w = (am.blend && perm) ? am.blend[0] : 1.f;
  m.blendrow = m.w != 1.f;
  m.roff = am.pixel ? (unsigned)am.rng_offset[0] : 0u;
  return m;
}

struct MixRow {  // block-uniform state of output row oy of sample n
  bool mixrow, two;  // the row crosses the box; it reads a second sample
  int other;         // that sample, perm[n] (n when unread)
};
__device__ __forceinline__ MixRow mix_row(const Mix& m, const int* __restrict__ perm, int n, int oy, int N) {
  MixRow r;
  r.mixrow = perm && oy >= m.box.y0 && oy < m.box.y1 && m.box.x0 < m.box.x1;
  r.two = r.mixrow || m.blendrow;
  r.other = r.two ? min(max(perm[n], 0), N - 1) : n;
  return r;
}

// Output columns [x0, x1) of row `row` = n Ho + oy. px(k, ox, f): the normalised value of source k (0: s0, sample
// n; 1: s1, the other sample) at column ox, asked for outside that source's erase box only.
template <typename Px>
__device__ __forceinline__ void mix_columns(const Mix& m, const MixRow& r, const AugMix& am, const MixSrc& s0,
                                            const MixSrc& s1, bf16* __restrict__ out, int row, int oy, int Ho, int Wo,
                                            int x0, int x1, Px px) {
  auto src = [&](int k, int ox, float (&f)[3]) __attribute__((always_inline)) {
    const MixSrc& s = k ? s1 : s0;
    if (ox >= s.ex0 && ox < s.ex1) erase_value(am.seed, m.roff, s.s, oy, ox, Ho, Wo, am.pixel, f);
    else px(k, ox, f);
  };
  for (int ox = x0 + threadIdx.x; ox < x1; ox += blockDim.x) {
    float f[3];
    if (r.mixrow && ox >= m.box.x0 && ox < m.box.x1) {
      src(1, ox, f);
    } else {
      src(0, ox, f);
      if (m.blendrow) {
        float q[3];
        src(1, ox, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = m.w * f[c] + (1.f - m.w) * q[c];
      }
    }
    store_px(out, row, Wo, ox, f);
  }
}

// ----------------------------------------------------------------------------------------
// normalize_u8: uint8 NHWC [N][H][W][Cin] -> bf16 NHWC4, optional per-sample horizontal flip (flip[n] != 0)
// ----------------------------------------------------------------------------------------
__global__ void normalize_u8_kernel(const unsigned char* __restrict__ in, bf16* __restrict__ out,
                                    const unsigned char* __restrict__ flip, int N, int H, int W, int Cin,
                                    float m0, float m1, float m2, float s0, float s1, float s2) {
  const long long total = (long long)N * H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int w = (int)(i % W);
    const long long nh = i / W;
    const int n = (int)(nh / H);
    const int ws = (flip && flip[n]) ? (W - 1 - w) : w;
    const unsigned char* src = in + ((nh * W) + ws) * Cin;
    float f0, f1, f2;
    if (Cin == 1) { f0 = f1 = f2 = src[0] * (1.f / 255.f); }
    else { f0 = src[0] * (1.f / 255.f); f1 = src[1] * (1.f / 255.f); f2 = src[2] * (1.f / 255.f); }
    bf16x4 o = {(bf16)((f0 - m0) / s0), (bf16)((f1 - m1) / s1), (bf16)((f2 - m2) / s2), (bf16)0.f};
    *reinterpret_cast<bf16x4*>(out + i * 4) = o;
  }
}

// ----------------------------------------------------------------------------------------
// augment_u8: uint8 NHWC [N][Hin][Win][Cin] -> bf16 NHWC4 [N][Ho][Wo][4]. One block per output row (n, oy):
// the box, flip and the two source rows are block-uniform, so per pixel only the column interpolation is
// computed (32-bit index math throughout). CutMix (Composer's CutMix(alpha=1),
// `03_composer/01_cifar_composer_resnet.ipynb:430`): with perm / mixbox set, output pixels inside the box come
// from sample perm[n] -- sampled with ITS crop box and flip, i.e. exactly the pixels of the augmented image
// perm[n] at the same output position.
// RAGGED (this kernel, the mixing form and crop_resize_u8): `in` is the arena and every source sample has its own
// geometry in `tab` (src_img above; Hin / Win are unread); the dense instantiation never reads tab / arena16.
// ----------------------------------------------------------------------------------------
template <bool RAGGED>
__global__ __launch_bounds__(256) void augment_u8_kernel(const unsigned char* __restrict__ in, bf16* __restrict__ out,
                                                         const float* __restrict__ boxes,
                                                         const unsigned char* __restrict__ flip, int N, int Hin,
                                                         int Win, int Cin, int Ho, int Wo, float m0, float m1,
                                                         float m2, float s0, float s1, float s2,
                                                         const int* __restrict__ perm, const int* __restrict__ mixbox,
                                                         const int* __restrict__ tab, long long arena16) {
  __shared__ __attribute__((aligned(16))) unsigned char srow[2][kRowMax];
  const MixBox box = mix_box(mixbox);
  const Norm nm = make_norm(m0, m1, m2, s0, s1, s2);
  for (int row = blockIdx.x; row < N * Ho; row += gridDim.x) {  // row = n * Ho + oy
    const int n = row / Ho, oy = row - n * Ho;
    const bool mixrow = perm && oy >= box.y0 && oy < box.y1 && box.x0 < box.x1;  // block-uniform
    // pass 0: sample n outside the box (everywhere when not mixing); pass 1: sample perm[n] inside
    for (int pass = 0; pass < (mixrow ? 2 : 1); ++pass) {
      const int xlo = pass ? box.x0 : 0, xhi = pass ? box.x1 : Wo;
      const int sn = pass ? perm[n] : n;
      const AugRow r = aug_row<RAGGED>(src_img<RAGGED>(in, tab, arena16, sn, Hin, Win, Cin),
                                       aug_box(boxes, flip, sn, Wo), nullptr, oy, Cin, Ho);
      const bool staged = stage_rows<RAGGED>(srow, r, r, false);
      auto body = [&](const unsigned char* r0, const unsigned char* r1) __attribute__((always_inline)) {
        for (int ox = xlo + threadIdx.x; ox < xhi; ox += blockDim.x) {
          if (mixrow && !pass && ox >= box.x0 && ox < box.x1) continue;  // pasted by pass 1
          float v[3], f[3];
          bilinear(r, r0, r1, ox, Cin, Wo, v);
          normalise(nm, v, f);
          store_px(out, row, Wo, ox, f);
        }
      };
      if (staged) body(&srow[0][0], &srow[1][0]);  // LDS byte gathers (ds_read_u8)
      else body(r.g0, r.g1);
      __syncthreads();  // srow reuse by the next pass / row
    }
  }
}

// The mixing form: a row stages the two source rows of both samples (4 x 4096 B of LDS) when all four can be.
template <bool RAGGED>
__global__ __launch_bounds__(256) void augment_mix_u8_kernel(const unsigned char* __restrict__ in, bf16* __restrict__ out,
                                                             const float* __restrict__ boxes,
                                                             const unsigned char* __restrict__ flip, int N, int Hin,
                                                             int Win, int Cin, int Ho, int Wo, float m0, float m1,
                                                             float m2, float s0, float s1, float s2,
                                                             const int* __restrict__ perm,
                                                             const int* __restrict__ mixbox, const AugMix am,
                                                             const int* __restrict__ tab, long long arena16) {
  __shared__ __attribute__((aligned(16))) unsigned char srow[4][kRowMax];
  const Mix mix = make_mix(perm, mixbox, am);
  const Norm nm = make_norm(m0, m1, m2, s0, s1, s2);
  for (int row = blockIdx.x; row < N * Ho; row += gridDim.x) {  // row = n * Ho + oy
    const int n = row / Ho, oy = row - n * Ho;
    const MixRow R = mix_row(mix, perm, n, oy, N);
    const AugRow A = aug_row<RAGGED>(src_img<RAGGED>(in, tab, arena16, n, Hin, Win, Cin), aug_box(boxes, flip, n, Wo),
                                     am.erase, oy, Cin, Ho);
    const AugRow P = R.two ? aug_row<RAGGED>(src_img<RAGGED>(in, tab, arena16, R.other, Hin, Win, Cin),
                                             aug_box(boxes, flip, R.other, Wo), am.erase, oy, Cin, Ho)
                           : A;
    const bool staged = stage_rows<RAGGED>(srow, A, P, R.two);
    auto body = [&](const unsigned char* a0, const unsigned char* a1, const unsigned char* p0, const unsigned char* p1)
                    __attribute__((always_inline)) {
      auto px = [&](int k, int ox, float (&f)[3]) __attribute__((always_inline)) {
        float v[3];
        bilinear(k ? P : A, k ? p0 : a0, k ? p1 : a1, ox, Cin, Wo, v);
        normalise(nm, v, f);
      };
      mix_columns(mix, R, am, A.src, P.src, out, row, oy, Ho, Wo, 0, Wo, px);
    };
    if (staged) body(&srow[0][0], &srow[1][0], &srow[2][0], &srow[3][0]);  // LDS byte gathers
    else body(A.g0, A.g1, P.g0, P.g1);
    __syncthreads();  // srow reuse by the next row
  }
}

// ----------------------------------------------------------------------------------------
// TrivialAugmentWide
//
//   crop_resize_u8   source uint8 -> T uint8 [N][Ho][Wo][4] = (R, G, B, L), u8 = (int)(v + 0.5f) of the plain
//                    kernel's bilinear v, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Pillow's L), and
//                    the per-sample histograms int32 [N][4][256] (LDS histogram per block, integer global
//                    atomics: order-independent, so deterministic)
//   ta_prepare       histograms + op table -> per-sample lut uint8 [N][3][256] (identity unless the kind is
//                    Posterize / Solarize / AutoContrast / Equalize) and the gray mean int32 [N]
//   ta_apply_u8      the mixing kernel on T: per source sample its operation, then the erase value, the
//                    normalisation, the blend and the paste through the same mix_columns
//
// Op table: per sample eight 32-bit words (kind int32; p, a, b, c, d, e, f fp32 bits); kinds and formulas:
// ops/reference.py (the oracle these kernels match bit for bit). Integer arithmetic throughout, except
// blend() and the affine map (fp32, every product and sum rounded on its own: fp contraction is off in
// those functions) and AutoContrast's LUT (float64, likewise).
// ----------------------------------------------------------------------------------------
// crop_resize_u8: a block takes kTaRows consecutive output rows of one sample (one LDS histogram flush per
// chunk, not per row).
template <bool RAGGED>
__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const unsigned char* __restrict__ in,
                                                             unsigned* __restrict__ T, int* __restrict__ hist,
                                                             const float* __restrict__ boxes,
                                                             const unsigned char* __restrict__ flip, int N, int Hin,
                                                             int Win, int Ho, int Wo, const int* __restrict__ tab,
                                                             long long arena16) {
  constexpr int Cin = 3;
  __shared__ __attribute__((aligned(16))) unsigned char srow[2][kRowMax];
  __shared__ int sh[4 * 256];
  const int cps = (Ho + kTaRows - 1) / kTaRows;  // chunks per sample
  for (int chunk = blockIdx.x; chunk < N * cps; chunk += gridDim.x) {
    const int n = chunk / cps, r0 = (chunk - n * cps) * kTaRows, r1 = min(r0 + kTaRows, Ho);
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) sh[i] = 0;
    const AugBox b = aug_box(boxes, flip, n, Wo);
    const SrcImg im = src_img<RAGGED>(in, tab, arena16, n, Hin, Win, Cin);
    __syncthreads();
    for (int oy = r0; oy < r1; ++oy) {
      const AugRow r = aug_row<RAGGED>(im, b, nullptr, oy, Cin, Ho);
      const bool staged = stage_rows<RAGGED>(srow, r, r, false);
      auto body = [&](const unsigned char* r0p, const unsigned char* r1p) __attribute__((always_inline)) {
        for (int ox = threadIdx.x; ox < Wo; ox += blockDim.x) {
          int u[3];
          bilinear(r, r0p, r1p, ox, Cin, Wo,
                   [&](int c, float v) __attribute__((always_inline)) { u[c] = min(max((int)(v + 0.5f), 0), 255); });
          const int L = (19595 * u[0] + 38470 * u[1] + 7471 * u[2] + 0x8000) >> 16;  // <= 255
          T[((size_t)n * Ho + oy) * Wo + ox] = (unsigned)u[0] | ((unsigned)u[1] << 8) | ((unsigned)u[2] << 16) |
                                               ((unsigned)L << 24);
          atomicAdd(&sh[u[0]], 1);
          atomicAdd(&sh[256 + u[1]], 1);
          atomicAdd(&sh[512 + u[2]], 1);
          atomicAdd(&sh[768 + L], 1);
        }
      };
      if (staged) body(&srow[0][0], &srow[1][0]);
      else body(r.g0, r.g1);
      __syncthreads();  // srow reuse by the next row; the histogram is complete after the last
    }
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x)
      if (sh[i]) atomicAdd(&hist[(size_t)n * 1024 + i], sh[i]);
    __syncthreads();  // sh is zeroed by the next chunk
  }
}

// ----------------------------------------------------------------------------------------
// ta_prepare: one block of 256 threads per sample, thread x owns LUT entry x of each channel.
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ int autocontrast_entry(int x, int lo, int hi) {
#pragma clang fp contract(off)
  // float64 as Pillow's Python code evaluates it: scale = 255.0 / (hi - lo), offset = -lo * scale,
  // int(x * scale + offset), product and sum rounded separately
  const double scale = 255.0 / (double)(hi - lo);
  const double off = (double)(-lo) * scale;
  const double t = (double)x * scale + off;
  return min(max((int)t, 0), 255);
}

__global__ __launch_bounds__(256) void ta_prepare_kernel(const int* __restrict__ hist, const int* __restrict__ ops,
                                                         unsigned char* __restrict__ lut, int* __restrict__ tmean,
                                                         int N) {
  __shared__ int scan[2][256];
  __shared__ int s_lo, s_hi;
  __shared__ unsigned long long s_sum, s_cnt;
  const int n = blockIdx.x, x = threadIdx.x;
  if (n >= N) return;
  const int kind = min(max(ops[8 * n], 0), kTaKinds - 1);
  const float p = __int_as_float(ops[8 * n + 1]);
  if (x == 0) { s_sum = 0ull; s_cnt = 0ull; }
  __syncthreads();
  {  // the gray mean (2 sum L + n) / (2 n)
    const int h = hist[((size_t)n * 4 + 3) * 256 + x];
    if (h) {
      atomicAdd(&s_sum, (unsigned long long)h * (unsigned)x);
      atomicAdd(&s_cnt, (unsigned long long)h);
    }
  }
  __syncthreads();
  if (x == 0) tmean[n] = s_cnt ? (int)((2ull * s_sum + s_cnt) / (2ull * s_cnt)) : 0;
  for (int c = 0; c < 3; ++c) {  // (every branch below is block-uniform)
    int v = x;
    if (kind == 10) {
      const int bits = min(max((int)p, 0), 8);
      v = x & ((0xFF << (8 - bits)) & 0xFF);
    } else if (kind == 11) {
      v = ((float)x < p) ? x : 255 - x;
    } else if (kind >= 12) {
      const int h = hist[((size_t)n * 4 + c) * 256 + x];
      __syncthreads();  // (the previous channel's readers of s_lo / s_hi / scan are done)
      if (x == 0) { s_lo = 256; s_hi = -1; }
      scan[0][x] = h;
      __syncthreads();
      if (h) { atomicMin(&s_lo, x); atomicMax(&s_hi, x); }
      // inclusive Hillis-Steele scan of the histogram (ping-pong)
      int src = 0;
      for (int d = 1; d < 256; d <<= 1) {
        __syncthreads();
        scan[src ^ 1][x] = scan[src][x] + (x >= d ? scan[src][x - d] : 0);
        src ^= 1;
      }
      __syncthreads();
      const int lo = s_lo, hi = s_hi;
      if (lo < hi) {  // at least two non-zero bins
        if (kind == 12) {
          v = autocontrast_entry(x, lo, hi);
        } else {
          const int total = scan[src][255], last = scan[src][hi] - (hi ? scan[src][hi - 1] : 0);
          const int step = (total - last) / 255;
          if (step) v = min(255, (step / 2 + (scan[src][x] - h)) / step);
        }
      }
    }
    lut[((size_t)n * 3 + c) * 256 + x] = (unsigned char)v;
  }
}

// ----------------------------------------------------------------------------------------
// ta_apply_u8
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ int ta_blend(float d, float v, float p) {
#pragma clang fp contract(off)
  // Pillow's Image.blend: t = d + p (v - d), truncated inside [0, 1], clamped first outside
  const float t = d + p * (v - d);
  if (p >= 0.f && p <= 1.f) return min(max((int)t, 0), 255);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ void ta_affine_src(float a, float b, float c, float d, float e, float f, int x, int y,
                                              float& xi, float& yi) {
#pragma clang fp contract(off)
  const float xs = (float)x + 0.5f, ys = (float)y + 0.5f;
  xi = (a * xs + b * ys) + c;
  yi = (d * xs + e * ys) + f;
}

struct TaSrc {  // one source sample's operation
  int s, kind, mean;
  float p, co[6];
};

__device__ __forceinline__ TaSrc ta_src(const int* __restrict__ ops, const int* __restrict__ tmean, int s) {
  TaSrc r;
  r.s = s;
  r.kind = min(max(ops[8 * s], 0), kTaKinds - 1);
  r.p = __int_as_float(ops[8 * s + 1]);
#pragma unroll
  for (int i = 0; i < 6; ++i) r.co[i] = __int_as_float(ops[8 * s + 2 + i]);
  r.mean = tmean[s];
  return r;
}

__device__ __forceinline__ unsigned ta_pack3(int r, int g, int b) {
  return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// The augmented uint8 pixels (R | G << 8 | B << 16) of columns [x0, x1) of output row oy of source sample S
// into dst (LDS). The kind is block-uniform: one loop per operation class.
__device__ __forceinline__ void ta_row(const TaSrc& S, const unsigned* __restrict__ T, const unsigned char* lut,
                                       int oy, int Ho, int Wo, int x0, int x1, unsigned* dst) {
  const unsigned* img = T + (size_t)S.s * Ho * Wo;
  const unsigned* trow = img + (size_t)oy * Wo;
  const int tid = threadIdx.x, nt = blockDim.x;
  if (S.kind == 0) {
    for (int ox = x0 + tid; ox < x1; ox += nt) dst[ox - x0] = trow[ox] & 0xFFFFFFu;
  } else if (S.kind <= 5) {  // nearest-neighbour inverse affine map; outside the image: 0
    for (int ox = x0 + tid; ox < x1; ox += nt) {
      float xi, yi;
      ta_affine_src(S.co[0], S.co[1], S.co[2], S.co[3], S.co[4], S.co[5], ox, oy, xi, yi);
      const float xf = floorf(xi), yf = floorf(yi);
      unsigned u = 0u;
      if (xf >= 0.f && xf < (float)Wo && yf >= 0.f && yf < (float)Ho)
        u = img[(size_t)(int)yf * Wo + (int)xf] & 0xFFFFFFu;
      dst[ox - x0] = u;
    }
  } else if (S.kind <= 8) {  // Brightness / Color / Contrast: blend with 0 / L / the gray mean
    for (int ox = x0 + tid; ox < x1; ox += nt) {
      const unsigned u = trow[ox];
      const float d = S.kind == 6 ? 0.f : (S.kind == 7 ? (float)(u >> 24) : (float)S.mean);
      dst[ox - x0] = ta_pack3(ta_blend(d, (float)(u & 255u), S.p), ta_blend(d, (float)((u >> 8) & 255u), S.p),
                              ta_blend(d, (float)((u >> 16) & 255u), S.p));
    }
  } else if (S.kind == 9) {  // Sharpness: blend with Pillow's SMOOTH (borders keep the pixel)
    const bool edge_row = oy == 0 || oy == Ho - 1;
    for (int ox = x0 + tid; ox < x1; ox += nt) {
      const unsigned u = trow[ox];
      if (edge_row || ox == 0 || ox == Wo - 1) { dst[ox - x0] = u & 0xFFFFFFu; continue; }
      int sum[3] = {0, 0, 0};
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const unsigned q = trow[(ptrdiff_t)dy * Wo + ox + dx];
          const int wgt = (dy == 0 && dx == 0) ? 5 : 1;
          sum[0] += wgt * (int)(q & 255u); sum[1] += wgt * (int)((q >> 8) & 255u); sum[2] += wgt * (int)((q >> 16) & 255u);
        }
      dst[ox - x0] = ta_pack3(ta_blend((float)((sum[0] + 6) / 13), (float)(u & 255u), S.p),
                              ta_blend((float)((sum[1] + 6) / 13), (float)((u >> 8) & 255u), S.p),
                              ta_blend((float)((sum[2] + 6) / 13), (float)((u >> 16) & 255u), S.p));
    }
  } else {  // Posterize / Solarize / AutoContrast / Equalize: the sample's LUT
    for (int ox = x0 + tid; ox < x1; ox += nt) {
      const unsigned u = trow[ox];
      dst[ox - x0] = ta_pack3(lut[u & 255u], lut[256 + ((u >> 8) & 255u)], lut[512 + ((u >> 16) & 255u)]);
    }
  }
}

__global__ __launch_bounds__(256) void ta_apply_u8_kernel(const unsigned* __restrict__ T, bf16* __restrict__ out,
                                                          const int* __restrict__ ops,
                                                          const unsigned char* __restrict__ lut,
                                                          const int* __restrict__ tmean, int N, int Ho, int Wo, float m0,
                                                          float m1, float m2, float s0, float s1, float s2,
                                                          const int* __restrict__ perm, const int* __restrict__ mixbox,
                                                          const AugMix am) {
  __shared__ unsigned arow[2][kTile];
  __shared__ __attribute__((aligned(4))) unsigned char slut[2][768];
  const Mix mix = make_mix(perm, mixbox, am);
  const Norm nm = make_norm(m0, m1, m2, s0, s1, s2);
  for (int row = blockIdx.x; row < N * Ho; row += gridDim.x) {  // row = n * Ho + oy
    const int n = row / Ho, oy = row - n * Ho;
    const MixRow R = mix_row(mix, perm, n, oy, N);
    const int nsrc = R.two ? 2 : 1;
    const int sid[2] = {n, R.other};
    const MixSrc S0 = mix_src(am.erase, n, oy), S1 = mix_src(am.erase, R.other, oy);
#pragma unroll 1
    for (int k = 0; k < nsrc; ++k)
      if (min(max(ops[8 * sid[k]], 0), kTaKinds - 1) >= 10)
        for (int i = threadIdx.x; i < 192; i += blockDim.x)
          reinterpret_cast<unsigned*>(&slut[k][0])[i] = reinterpret_cast<const unsigned*>(lut + (size_t)sid[k] * 768)[i];
    __syncthreads();
    for (int x0 = 0; x0 < Wo; x0 += kTile) {
      const int x1 = min(x0 + kTile, Wo);
#pragma unroll 1
      for (int k = 0; k < nsrc; ++k) ta_row(ta_src(ops, tmean, sid[k]), T, &slut[k][0], oy, Ho, Wo, x0, x1, &arow[k][0]);
      __syncthreads();
      auto px = [&](int k, int ox, float (&f)[3]) __attribute__((always_inline)) {
        const unsigned q = arow[k][ox - x0];
        const float v[3] = {(float)(q & 255u), (float)((q >> 8) & 255u), (float)((q >> 16) & 255u)};
        normalise(nm, v, f);
      };
      mix_columns(mix, R, am, S0, S1, out, row, oy, Ho, Wo, x0, x1, px);
      __syncthreads();  // arow / slut reuse by the next pass / row
    }
  }
}

// ----------------------------------------------------------------------------------------
// ta_stage_u8: one operation of a chain (RandAugment, AutoAugment). T_in -> T_out, both (R, G, B, L): sample n's
// own operation through the same ta_row, L recomputed from the new pixel with crop_resize_u8's expression, and
// T_out's histograms ADDED to hist -- what the next ta_prepare and the next operation read. The shape is
// crop_resize_u8's (a block takes kTaRows rows of one sample; one LDS histogram and one integer-atomic flush per
// chunk), the row walk ta_apply_u8's (tiles of kTile columns, the LUT staged for kinds >= 10 only). The affine
// kinds and Sharpness read T_in outside the block's rows: T_out must not alias T_in.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ta_stage_u8_kernel(const unsigned* __restrict__ T_in, unsigned* __restrict__ T_out,
                                                          int* __restrict__ hist, const int* __restrict__ ops,
                                                          const unsigned char* __restrict__ lut,
                                                          const int* __restrict__ tmean, int N, int Ho, int Wo) {
  __shared__ unsigned arow[kTile];
  __shared__ __attribute__((aligned(4))) unsigned char slut[768];
  __shared__ int sh[4 * 256];
  const int cps = (Ho + kTaRows - 1) / kTaRows;  // chunks per sample
  for (int chunk = blockIdx.x; chunk < N * cps; chunk += gridDim.x) {
    const int n = chunk / cps, r0 = (chunk - n * cps) * kTaRows, r1 = min(r0 + kTaRows, Ho);
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) sh[i] = 0;
    const TaSrc S = ta_src(ops, tmean, n);
    if (S.kind >= 10)  // (block-uniform)
      for (int i = threadIdx.x; i < 192; i += blockDim.x)
        reinterpret_cast<unsigned*>(&slut[0])[i] = reinterpret_cast<const unsigned*>(lut + (size_t)n * 768)[i];
    __syncthreads();
    for (int oy = r0; oy < r1; ++oy) {
      for (int x0 = 0; x0 < Wo; x0 += kTile) {
        const int x1 = min(x0 + kTile, Wo);
        ta_row(S, T_in, &slut[0], oy, Ho, Wo, x0, x1, &arow[0]);
        __syncthreads();
        for (int ox = x0 + threadIdx.x; ox < x1; ox += blockDim.x) {
          const unsigned q = arow[ox - x0];
          const int r = q & 255u, g = (q >> 8) & 255u, b = (q >> 16) & 255u;
          const int L = (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16;  // <= 255
          T_out[((size_t)n * Ho + oy) * Wo + ox] = q | ((unsigned)L << 24);
          atomicAdd(&sh[r], 1);
          atomicAdd(&sh[256 + g], 1);
          atomicAdd(&sh[512 + b], 1);
          atomicAdd(&sh[768 + L], 1);
        }
        __syncthreads();  // arow reuse by the next tile / row; the histogram is complete after the last
      }
    }
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x)
      if (sh[i]) atomicAdd(&hist[(size_t)n * 1024 + i], sh[i]);
    __syncthreads();  // sh and slut are rewritten by the next chunk
  }
}

}  // namespace dbx

using namespace dbx;

// one block per output row (crop_resize_u8: per chunk of rows), at most 4096; a wave per 64 output columns
static inline dim3 row_grid(long long rows) { return dim3((unsigned)(rows < 4096 ? rows : 4096)); }
static inline dim3 row_block(int Wo) { return dim3(Wo >= 256 ? 256 : ((Wo + 63) / 64) * 64); }

extern "C" int dbx_normalize_u8(const unsigned char* in, bf16* out, const unsigned char* flip, int N, int H, int W,
                                int Cin, float m0, float m1, float m2, float s0, float s1, float s2, hipStream_t st) {
  const long long blocks = ((long long)N * H * W + 255) / 256;
  hipLaunchKernelGGL(normalize_u8_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks))), dim3(256),
                     0, st, in, out, flip, N, H, W, Cin, m0, m1, m2, s0, s1, s2);
  RET_LAST;
}
extern "C" int dbx_augment_u8(const unsigned char* in, bf16* out, const float* boxes, const unsigned char* flip, int N,
                              int Hin, int Win, int Cin, int Ho, int Wo, float m0, float m1, float m2, float s0, float s1,
                              float s2, const int* perm, const int* mixbox, hipStream_t st, const int* src_tab,
                              long long arena16) {
  if (src_tab)  // the ragged form: `in` is the arena of arena16 16-byte units, Hin / Win unread
    hipLaunchKernelGGL(augment_u8_kernel<true>, row_grid((long long)N * Ho), row_block(Wo), 0, st, in, out, boxes, flip,
                       N, Hin, Win, Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, perm, mixbox, src_tab, arena16);
  else
    hipLaunchKernelGGL(augment_u8_kernel<false>, row_grid(N * Ho), row_block(Wo), 0, st, in, out, boxes, flip, N, Hin, Win,
                       Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, perm, mixbox, nullptr, 0ll);
  RET_LAST;
}
extern "C" int dbx_augment_mix_u8(const unsigned char* in, bf16* out, const float* boxes, const unsigned char* flip,
                                  int N, int Hin, int Win, int Cin, int Ho, int Wo, float m0, float m1, float m2, float s0,
                                  float s1, float s2, const int* perm, const int* mixbox, const float* blend,
                                  const int* erase, int pixel, unsigned long long seed, const int* rng_offset,
                                  hipStream_t st, const int* src_tab, long long arena16) {
  const AugMix am{blend, erase, rng_offset, seed, pixel};
  if (src_tab)
    hipLaunchKernelGGL(augment_mix_u8_kernel<true>, row_grid((long long)N * Ho), row_block(Wo), 0, st, in, out, boxes,
                       flip, N, Hin, Win, Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, perm, mixbox, am, src_tab, arena16);
  else
    hipLaunchKernelGGL(augment_mix_u8_kernel<false>, row_grid(N * Ho), row_block(Wo), 0, st, in, out, boxes, flip, N, Hin,
                       Win, Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, perm, mixbox, am, nullptr, 0ll);
  RET_LAST;
}
extern "C" int dbx_crop_resize_u8(const unsigned char* in, unsigned char* T, int* hist, const float* boxes,
                                  const unsigned char* flip, int N, int Hin, int Win, int Ho, int Wo, hipStream_t st,
                                  const int* src_tab, long long arena16) {
  const dim3 grid = row_grid((long long)N * ((Ho + kTaRows - 1) / kTaRows));
  if (src_tab)
    hipLaunchKernelGGL(crop_resize_u8_kernel<true>, grid, row_block(Wo), 0, st, in, (unsigned*)T, hist, boxes, flip, N,
                       Hin, Win, Ho, Wo, src_tab, arena16);
  else
    hipLaunchKernelGGL(crop_resize_u8_kernel<false>, grid, row_block(Wo), 0, st, in, (unsigned*)T, hist, boxes, flip, N,
                       Hin, Win, Ho, Wo, nullptr, 0ll);
  RET_LAST;
}
extern "C" int dbx_ta_prepare(const int* hist, const int* ops, unsigned char* lut, int* tmean, int N, hipStream_t st) {
  hipLaunchKernelGGL(ta_prepare_kernel, dim3(N), dim3(256), 0, st, hist, ops, lut, tmean, N);
  RET_LAST;
}
extern "C" int dbx_ta_apply_u8(const unsigned char* T, bf16* out, const int* ops, const unsigned char* lut,
                               const int* tmean, int N, int Ho, int Wo, float m0, float m1, float m2, float s0, float s1,
                               float s2, const int* perm, const int* mixbox, const float* blend, const int* erase,
                               int pixel, unsigned long long seed, const int* rng_offset, hipStream_t st,
                               unsigned char* T_out, int* hist_out) {
  if (T_out) return dbx_ta_stage_u8(T, T_out, hist_out, ops, lut, tmean, N, Ho, Wo, st);
  const AugMix am{blend, erase, rng_offset, seed, pixel};
  hipLaunchKernelGGL(ta_apply_u8_kernel, row_grid(N * Ho), row_block(Wo), 0, st, (const unsigned*)T, out, ops, lut, tmean,
                     N, Ho, Wo, m0, m1, m2, s0, s1, s2, perm, mixbox, am);
  RET_LAST;
}
extern "C" int dbx_ta_stage_u8(const unsigned char* T_in, unsigned char* T_out, int* hist, const int* ops,
                               const unsigned char* lut, const int* tmean, int N, int Ho, int Wo, hipStream_t st) {
  hipLaunchKernelGGL(ta_stage_u8_kernel, row_grid((long long)N * ((Ho + kTaRows - 1) / kTaRows)), row_block(Wo), 0, st,
                     (const unsigned*)T_in, (unsigned*)T_out, hist, ops, lut, tmean, N, Ho, Wo);
  RET_LAST;
}
