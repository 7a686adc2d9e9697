// TrivialAugmentWide in the native step's input pipeline (torchvision's `--auto-augment ta_wide`): each
// training image gets one of fourteen operations at a random strength, on the uint8 image after crop /
// resize / flip and before normalisation, erasing and batch mixing. Contrast (gray mean), AutoContrast
// (min / max), Equalize (histogram) and Sharpness (3x3 neighbourhood) need the whole image, so the
// one-pass augment kernels of nn_ops.hip cannot host it; three kernels do:
//
//   crop_resize_u8   source uint8 -> T uint8 [N][Ho][Wo][4] = (R, G, B, L), u8 = (int)(v + 0.5f) of the plain
//                    kernel's bilinear v, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (Pillow's L), and
//                    the per-sample histograms int32 [N][4][256] (LDS histogram per block, integer global
//                    atomics: order-independent, so deterministic)
//   ta_prepare       histograms + op table -> per-sample lut uint8 [N][3][256] (identity unless the kind is
//                    Posterize / Solarize / AutoContrast / Equalize) and the gray mean int32 [N]
//   ta_apply_u8      the mixing kernel on T: per source sample its operation, the erase value, the
//                    normalisation; then the MixUp blend and the CutMix paste of augment_mix_u8_kernel
//
// Op table: per sample eight 32-bit words (kind int32; p, a, b, c, d, e, f fp32 bits); kinds and formulas:
// ops/reference.py (the oracle these kernels match bit for bit). Integer arithmetic throughout, except
// blend() and the affine map (fp32, every product and sum rounded on its own: fp contraction is off in
// those functions) and AutoContrast's LUT (float64, likewise).
#include "common.h"
#include "philox.h"

namespace dbx {

constexpr int kTaKinds = 14;

// ----------------------------------------------------------------------------------------
// crop_resize_u8: a block takes kTaRows consecutive output rows of one sample (one LDS histogram flush
// per chunk, not per row); per row the two source rows are staged in LDS as in augment_u8_kernel.
// ----------------------------------------------------------------------------------------
constexpr int kTaRows = 16;

__global__ __launch_bounds__(256) void crop_resize_u8_kernel(const unsigned char* __restrict__ in,
                                                             unsigned* __restrict__ T, int* __restrict__ hist,
                                                             const float* __restrict__ boxes,
                                                             const unsigned char* __restrict__ flip, int N, int Hin,
                                                             int Win, int Ho, int Wo) {
  constexpr int kRowMax = 4096, Cin = 3;
  __shared__ __attribute__((aligned(16))) unsigned char srow[2][kRowMax];
  __shared__ int sh[4 * 256];
  const int cps = (Ho + kTaRows - 1) / kTaRows;  // chunks per sample
  for (int chunk = blockIdx.x; chunk < N * cps; chunk += gridDim.x) {
    const int n = chunk / cps, r0 = (chunk - n * cps) * kTaRows, r1 = min(r0 + kTaRows, Ho);
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) sh[i] = 0;
    const float by = boxes[4 * n], bx = boxes[4 * n + 1], bh = boxes[4 * n + 2], bw = boxes[4 * n + 3];
    const bool fl = flip && flip[n];
    const float sxs = bw / Wo;
    __syncthreads();
    for (int oy = r0; oy < r1; ++oy) {
      float sy = by + (oy + 0.5f) * bh / Ho - 0.5f;
      sy = fminf(fmaxf(sy, 0.f), (float)(Hin - 1));
      const int y0 = (int)sy, y1 = min(y0 + 1, Hin - 1);
      const float wy = sy - y0;
      const unsigned char* g0 = in + ((size_t)n * Hin + y0) * Win * Cin;
      const unsigned char* g1 = in + ((size_t)n * Hin + y1) * Win * Cin;
      const int rb = Win * Cin;
      const bool staged = rb <= kRowMax && (((size_t)g0 | (size_t)g1) & 15) == 0 && (rb & 15) == 0;  // block-uniform
      if (staged) {
        for (int o = threadIdx.x * 16; o < rb; o += blockDim.x * 16) {
          *reinterpret_cast<u32x4*>(&srow[0][o]) = *reinterpret_cast<const u32x4*>(g0 + o);
          *reinterpret_cast<u32x4*>(&srow[1][o]) = *reinterpret_cast<const u32x4*>(g1 + o);
        }
        __syncthreads();
      }
      auto body = [&](const unsigned char* r0p, const unsigned char* r1p) __attribute__((always_inline)) {
        for (int ox = threadIdx.x; ox < Wo; ox += blockDim.x) {
          const int oxx = fl ? (Wo - 1 - ox) : ox;
          float sx = bx + (oxx + 0.5f) * sxs - 0.5f;
          sx = fminf(fmaxf(sx, 0.f), (float)(Win - 1));
          const int x0 = (int)sx, x1 = min(x0 + 1, Win - 1);
          const float wx = sx - x0;
          int u[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float a = r0p[x0 * Cin + c], b = r0p[x1 * Cin + c];
            const float d = r1p[x0 * Cin + c], e = r1p[x1 * Cin + c];
            const float v = (a * (1.f - wx) + b * wx) * (1.f - wy) + (d * (1.f - wx) + e * wx) * wy;  // 0..255
            u[c] = min(max((int)(v + 0.5f), 0), 255);
          }
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
      else body(g0, g1);
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
      if (xf >= 0.f && xf < (float)Wo && yf >= 0.f && yf < (float)Ho) u = img[(size_t)(int)yf * Wo + (int)xf] & 0xFFFFFFu;
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

struct TaMix {
  const float* blend;     // fp32[1]; null: 1
  const int* erase;       // int32 [N][4]; null: none
  const int* rng_offset;  // int32[1] (pixel mode)
  unsigned long long seed;
  int pixel;
};

__global__ __launch_bounds__(256) void ta_apply_u8_kernel(const unsigned* __restrict__ T, bf16* __restrict__ out,
                                                          const int* __restrict__ ops,
                                                          const unsigned char* __restrict__ lut,
                                                          const int* __restrict__ tmean, int N, int Ho, int Wo, float m0,
                                                          float m1, float m2, float s0, float s1, float s2,
                                                          const int* __restrict__ perm, const int* __restrict__ mixbox,
                                                          const TaMix am) {
  constexpr int kTile = 1024;  // output columns per pass
  __shared__ unsigned arow[2][kTile];
  __shared__ __attribute__((aligned(4))) unsigned char slut[2][768];
  const int my0 = mixbox ? mixbox[0] : 0, my1 = mixbox ? mixbox[1] : 0;
  const int mx0 = mixbox ? mixbox[2] : 0, mx1 = mixbox ? mixbox[3] : 0;
  const float i0 = 1.f / (255.f * s0), i1 = 1.f / (255.f * s1), i2 = 1.f / (255.f * s2);
  const float w = (am.blend && perm) ? am.blend[0] : 1.f;
  const bool blendrow = w != 1.f;  // grid-uniform
  const unsigned roff = am.pixel ? (unsigned)am.rng_offset[0] : 0u;
  for (int row = blockIdx.x; row < N * Ho; row += gridDim.x) {  // row = n * Ho + oy
    const int n = row / Ho, oy = row - n * Ho;
    const bool mixrow = perm && oy >= my0 && oy < my1 && mx0 < mx1;  // block-uniform
    const bool two = mixrow || blendrow;                              // the row reads sample perm[n]
    const int nsrc = two ? 2 : 1;
    const int sid[2] = {n, two ? min(max(perm[n], 0), N - 1) : n};
    int ex0[2] = {0, 0}, ex1[2] = {0, 0};  // this row's erased columns per source sample (empty: none)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int s = sid[k];
      if (am.erase && oy >= am.erase[4 * s] && oy < am.erase[4 * s + 1]) { ex0[k] = am.erase[4 * s + 2]; ex1[k] = am.erase[4 * s + 3]; }
    }
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
      // f_s at column ox: the erase value inside the sample's erase box, else the normalised augmented pixel
      auto px = [&](int k, int ox, float (&f)[3]) __attribute__((always_inline)) {
        if (ox >= ex0[k] && ox < ex1[k]) {
          f[0] = f[1] = f[2] = 0.f;
          if (am.pixel) {
            unsigned u[4];
            philox4x32_10(((unsigned long long)sid[k] * Ho + oy) * Wo + ox, am.seed, roff, u);
            const float k24 = 1.f / 16777216.f;
            const float r01 = sqrtf(-2.f * logf((float)((u[0] >> 8) + 1u) * k24));
            const float a01 = 2.f * ((float)(u[1] >> 8) * k24);
            f[0] = r01 * cospif(a01);
            f[1] = r01 * sinpif(a01);
            f[2] = sqrtf(-2.f * logf((float)((u[2] >> 8) + 1u) * k24)) * cospif(2.f * ((float)(u[3] >> 8) * k24));
          }
          return;
        }
        const unsigned q = arow[k][ox - x0];
        float v[3] = {(float)(q & 255u), (float)((q >> 8) & 255u), (float)((q >> 16) & 255u)};
        f[0] = v[0] * i0 - m0 / s0; f[1] = v[1] * i1 - m1 / s1; f[2] = v[2] * i2 - m2 / s2;
      };
      for (int ox = x0 + threadIdx.x; ox < x1; ox += blockDim.x) {
        float f[3];
        if (mixrow && ox >= mx0 && ox < mx1) {
          px(1, ox, f);
        } else {
          px(0, ox, f);
          if (blendrow) {
            float q[3];
            px(1, ox, q);
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = w * f[c] + (1.f - w) * q[c];
          }
        }
        bf16x4 o = {(bf16)f[0], (bf16)f[1], (bf16)f[2], (bf16)0.f};
        *reinterpret_cast<bf16x4*>(out + ((size_t)row * Wo + ox) * 4) = o;
      }
      __syncthreads();  // arow / slut reuse by the next pass / row
    }
  }
}

}  // namespace dbx

using namespace dbx;
#define RET_LAST return (int)hipGetLastError()

extern "C" int dbx_crop_resize_u8(const unsigned char* in, unsigned char* T, int* hist, const float* boxes,
                                  const unsigned char* flip, int N, int Hin, int Win, int Ho, int Wo, hipStream_t st) {
  const long long chunks = (long long)N * ((Ho + kTaRows - 1) / kTaRows);
  hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)(chunks < 4096 ? chunks : 4096)),
                     dim3(Wo >= 256 ? 256 : ((Wo + 63) / 64) * 64), 0, st, in, (unsigned*)T, hist, boxes, flip, N, Hin,
                     Win, Ho, Wo);
  RET_LAST;
}
extern "C" int dbx_ta_prepare(const int* hist, const int* ops, unsigned char* lut, int* tmean, int N, hipStream_t st) {
  hipLaunchKernelGGL(ta_prepare_kernel, dim3(N), dim3(256), 0, st, hist, ops, lut, tmean, N);
  RET_LAST;
}
extern "C" int dbx_ta_apply_u8(const unsigned char* T, bf16* out, const int* ops, const unsigned char* lut,
                               const int* tmean, int N, int Ho, int Wo, float m0, float m1, float m2, float s0, float s1,
                               float s2, const int* perm, const int* mixbox, const float* blend, const int* erase,
                               int pixel, unsigned long long seed, const int* rng_offset, hipStream_t st) {
  const TaMix am{blend, erase, rng_offset, seed, pixel};
  hipLaunchKernelGGL(ta_apply_u8_kernel, dim3(N * Ho < 4096 ? N * Ho : 4096),
                     dim3(Wo >= 256 ? 256 : ((Wo + 63) / 64) * 64), 0, st, (const unsigned*)T, out, ops, lut, tmean, N,
                     Ho, Wo, m0, m1, m2, s0, s1, s2, perm, mixbox, am);
  RET_LAST;
}
