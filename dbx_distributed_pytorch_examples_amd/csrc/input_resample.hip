// The resampling kernel of the input stage (gfx950): Pillow's antialiased bilinear and bicubic filters for the crop /
// resize of augment_u8 and crop_resize_u8 (input_ops.hip, whose entry points launch it). A file of its own because it
// is compiled without the packed fp32 instructions (build_ext.py), which the kernels of input_ops.hip keep.
#include "common.h"
#include "entry.h"
#include "input_common.h"

namespace dbx {

// ----------------------------------------------------------------------------------------
// resample_u8: the crop / resize of augment_u8 (MODE 0: bf16 NHWC4, normalised) and of crop_resize_u8 (MODE 1: T
// and the histograms) with Pillow's separable resampling filters instead of two taps per axis -- `filter` 1
// antialiased bilinear, 2 bicubic (a = -0.5), 3 antialiased bicubic. Per axis, with box start b, box length l,
// n outputs and source size W (Pillow's precompute_coeffs; ops/reference.py resample_axis is the definition):
//   scale = l / n; fs = antialias ? max(scale, 1) : 1; sup = S fs (S = 1 triangle, 2 cubic)
//   c = b + (o + 0.5) scale; lo = max(0, int(c - sup + 0.5)); hi = min(W, int(c + sup + 0.5))
//   k[x] = filter((x - c + 0.5) / fs) / sum over [lo, hi)   -- clipped to the image, not to the box
// and one tap of weight 1 at clamp(floor(c), 0, W - 1) when the window is empty or its sum is not positive.
// v = sum_y ky sum_x kx px in fp32, rounded ONCE: u8 = clamp((int)(v + 0.5f), 0, 255); everything after it (L,
// the histograms, the normalisation) is the bilinear kernels' code on that uint8 pixel.
//
// A row-streaming separable filter: a block takes kRsRows consecutive output rows of one sample and, per pass, one
// output column per thread (up to kRsTile). A column's window and weights do not depend on the row: the thread
// keeps lo / n in registers and its first kRsTaps weights in LDS (skx[t][thread]: conflict-free); a column with
// more taps recomputes them at every use (slow, correct). The block then walks the source rows of the chunk's
// union window once: row y + 1 is loaded (aligned 16-byte loads, registers) while row y, already in LDS, is
// filtered -- each thread forms its column's horizontal sums h[3] from LDS byte reads (rows that cannot be staged
// by the kRowMax rule: from global memory) and adds ky[r][y] h to the accumulators of the chunk rows r whose window
// holds y. ky is block-uniform: the first threads write it to LDS next to the staged row, the update reads it
// into scalar registers and skips the rows where it is 0. The horizontally filtered row lives in registers only.
// No matrix instructions: the taps are byte gathers at per-column offsets with per-column weights (2 to about 30
// of them), so an MFMA form would spend its time building operands.
// ----------------------------------------------------------------------------------------
constexpr int kRsRows = 16;   // output rows per chunk (48 fp32 accumulators per thread)
constexpr int kRsTile = 256;  // output columns per pass: one per thread
constexpr int kRsTaps = 16;   // taps per column whose weights are kept in LDS
constexpr int kRsPre = kRowMax / 16 / 64;  // 16-byte loads per thread that stage a row with the smallest block

__device__ __forceinline__ float rs_filter(float x, bool cubic) {
  x = fabsf(x);
  if (!cubic) return x < 1.f ? 1.f - x : 0.f;
  if (x < 1.f) return (1.5f * x - 2.5f) * x * x + 1.f;
  if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * -0.5f;
  return 0.f;
}
__device__ __forceinline__ int rs_int(float x) {  // (int)x, any box: inside +-2^30 (a NaN: the lower end)
  return (int)fminf(fmaxf(x, -1073741824.f), 1073741824.f);
}
struct RsAxis {  // one output position's window [lo, lo + n) and what its weights need; sum == 0: the guard tap
  int lo, n;
  float c, fs, sum;
};
__device__ __forceinline__ RsAxis rs_axis(float b, float scale, int o, int W, bool cubic, bool aa) {
  RsAxis a;
  a.fs = aa ? fmaxf(scale, 1.f) : 1.f;
  const float sup = (cubic ? 2.f : 1.f) * a.fs;
  a.c = b + ((float)o + 0.5f) * scale;
  const int lo = max(0, rs_int(a.c - sup + 0.5f)), hi = min(W, rs_int(a.c + sup + 0.5f));
  a.lo = lo;
  a.n = hi - lo;
  a.sum = 0.f;
  for (int x = lo; x < hi; ++x) a.sum += rs_filter(((float)x - a.c + 0.5f) / a.fs, cubic);
  if (a.n <= 0 || !(a.sum > 0.f)) {
    a.lo = min(max(rs_int(floorf(a.c)), 0), W - 1);
    a.n = 1;
    a.sum = 0.f;
  }
  return a;
}
__device__ __forceinline__ float rs_weight(const RsAxis& a, int x, bool cubic) {  // x in [lo, lo + n)
  return a.sum > 0.f ? rs_filter(((float)x - a.c + 0.5f) / a.fs, cubic) / a.sum : 1.f;
}

template <bool RAGGED, int MODE>
__global__ __launch_bounds__(256) void resample_u8_kernel(const unsigned char* __restrict__ in, void* __restrict__ outp,
                                                          int* __restrict__ hist, const float* __restrict__ boxes,
                                                          const unsigned char* __restrict__ flip, int N, int Hin,
                                                          int Win, int Cin, int Ho, int Wo, float m0, float m1,
                                                          float m2, float s0, float s1, float s2,
                                                          const int* __restrict__ tab, long long arena16, int filter) {
  __shared__ __attribute__((aligned(16))) unsigned char srow[2][kRowMax];
  __shared__ float skx[kRsTaps][kRsTile];
  __shared__ float sky[2][kRsRows];
  __shared__ int sylo[kRsRows], syhi[kRsRows];
  __shared__ int sh[MODE ? 4 * 256 : 1];
  const bool cubic = filter >= 2, aa = filter != 2;
  const int C = MODE ? 3 : Cin;
  const int tid = threadIdx.x, nt = blockDim.x;  // nt <= kRsTile
  const Norm nm = make_norm(m0, m1, m2, s0, s1, s2);
  const int cps = (Ho + kRsRows - 1) / kRsRows;  // chunks per sample
  for (int chunk = blockIdx.x; chunk < N * cps; chunk += gridDim.x) {
    const int n = chunk / cps, r0 = (chunk - n * cps) * kRsRows, nr = min(kRsRows, Ho - r0);
    if constexpr (MODE)
      for (int i = tid; i < 4 * 256; i += nt) sh[i] = 0;
    const AugBox b = aug_box(boxes, flip, n, Wo);
    const SrcImg im = src_img<RAGGED>(in, tab, arena16, n, Hin, Win, C);
    // thread r < nr: the vertical window of chunk row r (kept in its registers; the bounds go to LDS)
    RsAxis ay{0, 0, 0.f, 1.f, 0.f};
    if (tid < nr) {
      ay = rs_axis(b.by, b.bh / Ho, r0 + tid, im.H, cubic, aa);
      sylo[tid] = ay.lo;
      syhi[tid] = ay.lo + ay.n;
    }
    __syncthreads();
    int ylo = sylo[0], yhi = syhi[0];  // the union window: never empty, inside [0, H)
    for (int r = 1; r < nr; ++r) { ylo = min(ylo, sylo[r]); yhi = max(yhi, syhi[r]); }
    const unsigned char* g = im.base + (size_t)im.sn * im.H * im.rb;  // row y of the image: g + y rb
    const bool staged = im.rb <= kRowMax && (im.rb & 15) == 0 && ((size_t)g & 15) == 0;  // (block-uniform)
    u32x4 pre[kRsPre];
    auto fetch = [&](int y) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < kRsPre; ++i) {
        const int o = (tid + i * nt) * 16;
        if (o < im.rb) pre[i] = *reinterpret_cast<const u32x4*>(g + (size_t)y * im.rb + o);
      }
    };
    auto commit = [&](int buf, int y) __attribute__((always_inline)) {  // row y's bytes and its ky column
      if (staged) {
#pragma unroll
        for (int i = 0; i < kRsPre; ++i) {
          const int o = (tid + i * nt) * 16;
          if (o < im.rb) *reinterpret_cast<u32x4*>(&srow[buf][o]) = pre[i];
        }
      }
      if (tid < nr) sky[buf][tid] = (y >= ay.lo && y < ay.lo + ay.n) ? rs_weight(ay, y, cubic) : 0.f;
    };
    for (int x0 = 0; x0 < Wo; x0 += nt) {  // a pass: nt output columns
      const int ox = x0 + tid;
      const bool live = ox < Wo;
      RsAxis ax{0, 0, 0.f, 1.f, 0.f};
      if (live) ax = rs_axis(b.bx, b.sxs, b.fl ? (Wo - 1 - ox) : ox, im.W, cubic, aa);
      const bool inlds = ax.n <= kRsTaps;
      if (inlds)
        for (int t = 0; t < ax.n; ++t) skx[t][tid] = rs_weight(ax, ax.lo + t, cubic);  // (read by this thread only)
      float acc[kRsRows][3];
#pragma unroll
      for (int r = 0; r < kRsRows; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;
      if (staged) fetch(ylo);
      commit(0, ylo);
      __syncthreads();
      for (int y = ylo; y < yhi; ++y) {
        const int cur = (y - ylo) & 1;
        const bool more = y + 1 < yhi;
        if (staged && more) fetch(y + 1);  // in flight during this row's arithmetic
        float h[3] = {0.f, 0.f, 0.f};
        auto hsum = [&](const unsigned char* row) __attribute__((always_inline)) {
          const unsigned char* p = row + ax.lo * C;
          for (int t = 0; t < ax.n; ++t, p += C) {
            const float w = inlds ? skx[t][tid] : rs_weight(ax, ax.lo + t, cubic);
            h[0] += w * p[0];
            if (C == 3) { h[1] += w * p[1]; h[2] += w * p[2]; }
          }
        };
        if (staged) hsum(&srow[cur][0]);  // LDS byte gathers
        else hsum(g + (size_t)y * im.rb);
        if (C != 3) h[1] = h[2] = h[0];
#pragma unroll
        for (int r = 0; r < kRsRows; ++r) {
          if (r < nr) {
            const float k = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sky[cur][r])));
            if (k != 0.f) { acc[r][0] += k * h[0]; acc[r][1] += k * h[1]; acc[r][2] += k * h[2]; }
          }
        }
        if (more) commit(cur ^ 1, y + 1);
        __syncthreads();  // row y + 1 is staged; row y's buffer is free for row y + 2
      }
      if (live) {
#pragma unroll
        for (int r = 0; r < kRsRows; ++r) {
          if (r < nr) {
            const int oy = r0 + r;
            int u[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c] = min(max((int)(acc[r][c] + 0.5f), 0), 255);
            if constexpr (MODE) {
              const int L = (19595 * u[0] + 38470 * u[1] + 7471 * u[2] + 0x8000) >> 16;  // <= 255
              reinterpret_cast<unsigned*>(outp)[((size_t)n * Ho + oy) * Wo + ox] =
                  (unsigned)u[0] | ((unsigned)u[1] << 8) | ((unsigned)u[2] << 16) | ((unsigned)L << 24);
              atomicAdd(&sh[u[0]], 1);
              atomicAdd(&sh[256 + u[1]], 1);
              atomicAdd(&sh[512 + u[2]], 1);
              atomicAdd(&sh[768 + L], 1);
            } else {
              const float v[3] = {(float)u[0], (float)u[1], (float)u[2]};
              float f[3];
              normalise(nm, v, f);
              store_px(reinterpret_cast<bf16*>(outp), n * Ho + oy, Wo, ox, f);
            }
          }
        }
      }
    }
    if constexpr (MODE) {
      __syncthreads();  // the histogram is complete
      for (int i = tid; i < 4 * 256; i += nt)
        if (sh[i]) atomicAdd(&hist[(size_t)n * 1024 + i], sh[i]);
    }
    __syncthreads();  // sh, sylo / syhi are rewritten by the next chunk
  }
}

}  // namespace dbx

using namespace dbx;

// a block per chunk of kRsRows output rows, a thread per output column of a pass
template <int MODE>
static int launch_resample(const unsigned char* in, void* out, int* hist, const float* boxes, const unsigned char* flip,
                           int N, int Hin, int Win, int Cin, int Ho, int Wo, float m0, float m1, float m2, float s0,
                           float s1, float s2, hipStream_t st, const int* src_tab, long long arena16, int filter) {
  const dim3 grid = row_grid((long long)N * ((Ho + kRsRows - 1) / kRsRows));
  if (src_tab)
    hipLaunchKernelGGL((resample_u8_kernel<true, MODE>), grid, row_block(Wo), 0, st, in, out, hist, boxes, flip, N, Hin,
                       Win, Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, src_tab, arena16, filter);
  else
    hipLaunchKernelGGL((resample_u8_kernel<false, MODE>), grid, row_block(Wo), 0, st, in, out, hist, boxes, flip, N, Hin,
                       Win, Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, nullptr, 0ll, filter);
  RET_LAST;
}

int dbx_resample_u8(int mode, const unsigned char* in, void* out, int* hist, const float* boxes,
                    const unsigned char* flip, int N, int Hin, int Win, int Cin, int Ho, int Wo, float m0, float m1,
                    float m2, float s0, float s1, float s2, hipStream_t st, const int* src_tab, long long arena16,
                    int filter) {
  if (filter < 1 || filter > 3 || (mode == 1 && (Cin != 3 || !hist))) return -80;
  return mode ? launch_resample<1>(in, out, hist, boxes, flip, N, Hin, Win, Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, st,
                                   src_tab, arena16, filter)
              : launch_resample<0>(in, out, hist, boxes, flip, N, Hin, Win, Cin, Ho, Wo, m0, m1, m2, s0, s1, s2, st,
                                   src_tab, arena16, filter);
}
