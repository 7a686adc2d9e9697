// Anti-aliased down-sampling (BlurPool, Zhang 2019) for the NHWC bf16 programs: reflect-pad 1, depthwise
// [1,2,1] x [1,2,1] / 16, stride 2, fused with the passes that surround it in a ResNet block.
//
//   blur_fwd      out[n,p,q,c] = bf16( blur( relu(y*scale + shift) ) )       (fp32, one rounding; the BN output
//                                                                             at full resolution never reaches HBM)
//   blur_bwd      dx = blur^T(dout)                                          (the stem: a max-pool backward follows)
//   blur_bn_bwd   g = [relu(y*scale + shift) > 0] * blur^T(dpool), then
//                 reduce: stats += [sum g, sum g*xhat]     apply: dy = k1*g + k2*y + k3       (g is never written)
//
// Work split: a workgroup owns one image, a band of rows and a 64-channel slab; its 256 lanes are 32 pixels x 8
// channel groups, every lane moving 16 bytes (8 channels). The filter is separable, and the two halves sit on the two
// sides of LDS: the horizontal taps are taken on the way in (global -> registers -> fp32 row sums in LDS), the
// vertical taps on the way out (LDS -> registers -> global). The band is walked in column chunks so the staged rows
// fit: forward 2*TH + 1 source rows x QT output columns, backward TH + 1 gradient rows (one halo row) x WT input
// columns. Between neighbouring bands only the halo row is read twice.
//
// blur^T as a gather (no atomics): per dimension an input index h receives from at most two outputs,
//   h even: 2 * d[h/2]
//   h odd : 1 * d[(h-1)/2] + 1 * d[(h+1)/2]  (the second only if it exists)
// and reflection adds what the padded taps carry: index -1 is pixel 1 (so h == 1 takes d[0] twice) and, for odd H,
// index H is pixel H-2 (so h == H-2 takes d[P-1] twice). Border weights therefore differ from interior ones.
#include "common.h"
#include "entry.h"

namespace {

constexpr int kSlab = 64;     // channels of a workgroup
constexpr int kTH = 4;        // output rows of a forward band / gradient rows of a backward band
constexpr int kQT = 16;       // forward: output columns per chunk
constexpr int kWT = 32;       // backward: input columns per chunk
constexpr int kFwdRows = 2 * kTH + 1, kBwdRows = kTH + 1;
constexpr int kFwdLds = kFwdRows * kQT * kSlab, kBwdLds = kBwdRows * kWT * kSlab;  // floats: 36 KiB / 40 KiB
static_assert(kBwdLds >= 2 * 256 * 8, "the reduce form reuses the staging tile for its block reduction");

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// the (at most) two outputs that input index h of a length-H dimension receives from, with their weights
__device__ __forceinline__ void taps_t(int h, int H, int P, int& pa, float& wa, int& pb, float& wb) {
  pa = h >> 1;
  if (!(h & 1)) { wa = 2.f; pb = pa; wb = 0.f; return; }
  wa = h == 1 ? 2.f : 1.f;
  const bool has = pa + 1 < P;
  pb = has ? pa + 1 : pa;
  wb = has ? (((H & 1) && h == H - 2) ? 2.f : 1.f) : 0.f;
}

__device__ __forceinline__ void load8f(const float* p, float* f) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}
__device__ __forceinline__ void lds_put8(float* p, const float* f) {
  *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <bool PRO, bool RELU>
__device__ __forceinline__ void act8(const bf16* p, const float* s, const float* h, float* f) {
  unpack8(*reinterpret_cast<const u32x4*>(p), f);
  if (PRO) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = f[j] * s[j] + h[j];
      if (RELU) f[j] = fmaxf(f[j], 0.f);
    }
  }
}

template <bool PRO, bool RELU>
__global__ __launch_bounds__(256) void blur_fwd_kernel(const bf16* __restrict__ y, const float* __restrict__ sc,
                                                       const float* __restrict__ sh, bf16* __restrict__ out, int H,
                                                       int W, int C, int P, int Q) {
  __shared__ float hs[kFwdLds];  // [source row][output column][channel]: horizontal sums a + 2b + c
  const int tid = threadIdx.x, cg = tid & 7, px = tid >> 3;
  const int c0 = blockIdx.y * kSlab + cg * 8, n = blockIdx.z;
  const int p0 = blockIdx.x * kTH, th = min(kTH, P - p0), rows = 2 * th + 1;
  float s[8], h[8];
  if (PRO) { load8f(sc + c0, s); load8f(sh + c0, h); }
  const bf16* img = y + (size_t)n * H * W * C + c0;
  for (int q0 = 0; q0 < Q; q0 += kQT) {
    const int qn = min(kQT, Q - q0);
    for (int i = px; i < rows * qn; i += 32) {
      const int r = i / qn, q = i - r * qn;
      const int hh = reflect(2 * p0 - 1 + r, H), wc = 2 * (q0 + q);
      const bf16* row = img + (size_t)hh * W * C;
      float a[8], b[8], c[8];
      act8<PRO, RELU>(row + (size_t)reflect(wc - 1, W) * C, s, h, a);
      act8<PRO, RELU>(row + (size_t)wc * C, s, h, b);
      act8<PRO, RELU>(row + (size_t)reflect(wc + 1, W) * C, s, h, c);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = a[j] + 2.f * b[j] + c[j];
      lds_put8(hs + (r * kQT + q) * kSlab + cg * 8, a);
    }
    __syncthreads();
    for (int i = px; i < th * qn; i += 32) {
      const int p = i / qn, q = i - p * qn;
      const float* t = hs + (2 * p * kQT + q) * kSlab + cg * 8;
      float a[8], b[8], c[8];
      load8f(t, a); load8f(t + kQT * kSlab, b); load8f(t + 2 * kQT * kSlab, c);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = (a[j] + 2.f * b[j] + c[j]) * 0.0625f;
      *reinterpret_cast<u32x4*>(out + (((size_t)n * P + p0 + p) * Q + q0 + q) * C + c0) = pack8(a);
    }
    __syncthreads();
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
enum { kPlain = 0, kReduce = 1, kApply = 2 };

// MODE kPlain : out = blur^T(d)
//      kReduce: stats[shard] += [sum g, sum g * (y - c1) * c2]          (c1 = mean, c2 = invstd)
//      kApply : out = c1*g + c2*y + c3                                   (bn_bwd_coeff's k1, k2, k3)
template <int MODE>
__global__ __launch_bounds__(256) void blur_bwd_kernel(const bf16* __restrict__ d, const bf16* __restrict__ y,
                                                       const float* __restrict__ sc, const float* __restrict__ sh,
                                                       const float* __restrict__ c1, const float* __restrict__ c2,
                                                       const float* __restrict__ c3, bf16* __restrict__ out,
                                                       double* __restrict__ stats, int nshard, int H, int W, int C,
                                                       int P, int Q) {
  __shared__ float hs[kBwdLds];  // [gradient row][input column][channel]: horizontally transposed taps
  const int tid = threadIdx.x, cg = tid & 7, px = tid >> 3;
  const int c0 = blockIdx.y * kSlab + cg * 8, n = blockIdx.z;
  const int p0 = blockIdx.x * kTH, h0 = 2 * p0;
  const int rows = min(kBwdRows, P - p0), hn = min(2 * kTH, H - h0);
  float s_[8], h_[8], k1[8], k2[8], k3[8];
  if (MODE != kPlain) {
    load8f(sc + c0, s_); load8f(sh + c0, h_);
    load8f(c1 + c0, k1); load8f(c2 + c0, k2);
    if (MODE == kApply) load8f(c3 + c0, k3);
  }
  float as[8] = {0, 0, 0, 0, 0, 0, 0, 0}, aq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bf16* dimg = d + (size_t)n * P * Q * C + c0;
  const size_t xoff = (size_t)n * H * W * C + c0;
  for (int w0 = 0; w0 < W; w0 += kWT) {
    const int wn = min(kWT, W - w0);
    for (int i = px; i < rows * wn; i += 32) {
      const int r = i / wn, w = i - r * wn;
      int qa, qb;
      float wa, wb;
      taps_t(w0 + w, W, Q, qa, wa, qb, wb);
      const bf16* row = dimg + (size_t)(p0 + r) * Q * C;
      float a[8], b[8];
      unpack8(*reinterpret_cast<const u32x4*>(row + (size_t)qa * C), a);
      unpack8(*reinterpret_cast<const u32x4*>(row + (size_t)qb * C), b);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = wa * a[j] + wb * b[j];
      lds_put8(hs + (r * kWT + w) * kSlab + cg * 8, a);
    }
    __syncthreads();
    for (int i = px; i < hn * wn; i += 32) {
      const int hl = i / wn, w = i - hl * wn;
      int pa, pb;
      float va, vb;
      taps_t(h0 + hl, H, P, pa, va, pb, vb);  // pa, pb in [p0, p0 + rows): pb is clamped to an existing row
      float a[8], b[8], g[8];
      load8f(hs + ((pa - p0) * kWT + w) * kSlab + cg * 8, a);
      load8f(hs + ((pb - p0) * kWT + w) * kSlab + cg * 8, b);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = (va * a[j] + vb * b[j]) * 0.0625f;
      const size_t e = xoff + ((size_t)(h0 + hl) * W + w0 + w) * C;
      if (MODE == kPlain) {
        *reinterpret_cast<u32x4*>(out + e) = pack8(g);
      } else {
        float yv[8];
        unpack8(*reinterpret_cast<const u32x4*>(y + e), yv);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = (yv[j] * s_[j] + h_[j]) > 0.f ? g[j] : 0.f;
        if (MODE == kApply) {
          float o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = k1[j] * g[j] + k2[j] * yv[j] + k3[j];
          *reinterpret_cast<u32x4*>(out + e) = pack8(o);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) { as[j] += g[j]; aq[j] += g[j] * (yv[j] - k1[j]) * k2[j]; }
        }
      }
    }
    __syncthreads();
  }
  if (MODE == kReduce) {
    // the block's 32 pixel lanes of a channel in a fixed order, then one fp64 add per channel and moment into the
    // block's shard: bn_bwd_reduce's scheme
    float* red = hs;
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[tid * 8 + j] = as[j]; red[256 * 8 + tid * 8 + j] = aq[j]; }
    __syncthreads();
    const int bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    double* st = stats + (size_t)(bid % nshard) * 2 * C + blockIdx.y * kSlab;
    if (tid < kSlab) {
      const int gi = tid >> 3, j = tid & 7;
      float ss = 0.f, qq = 0.f;
      for (int r = 0; r < 32; ++r) { ss += red[(r * 8 + gi) * 8 + j]; qq += red[256 * 8 + (r * 8 + gi) * 8 + j]; }
      atomicAdd(st + tid, (double)ss);
      atomicAdd(st + C + tid, (double)qq);
    }
  }
}

}  // namespace

// op 1 blur_fwd (a = y; sc / sh null: no prologue), 2 blur_bwd (a = dout), 3 blur_bn_bwd reduce (c1 = mean, c2 =
// invstd), 4 blur_bn_bwd apply (c1, c2, c3 = k1, k2, k3); a is the [N,P,Q,C] tensor of ops 2-4, out the tensor written
extern "C" int dbx_blur_op(int op, const bf16* a, const bf16* y, const float* sc, const float* sh, const float* c1,
                           const float* c2, const float* c3, bf16* out, double* stats, int nshard, int N, int H, int W,
                           int C, int P, int Q, int relu, hipStream_t st) {
  if (C < kSlab || C % kSlab || H < 2 || W < 2 || N < 1) return -1;
  if (P != (H - 1) / 2 + 1 || Q != (W - 1) / 2 + 1) return -2;
  if ((long long)N * H * W * C >= (1LL << 31) || N > 65535 || C / kSlab > 65535) return -3;
  if (!a || (op != 3 && !out) || (op >= 3 && !(y && sc && sh && c1 && c2)) || (op == 4 && !c3)) return -4;
  if (op == 3 && (!stats || nshard < 1)) return -4;
  const dim3 grid((P + kTH - 1) / kTH, C / kSlab, N), block(256);
  switch (op) {
    case 1:
      if (!sc != !sh) return -4;
      if (!sc)
        hipLaunchKernelGGL((blur_fwd_kernel<false, false>), grid, block, 0, st, a, sc, sh, out, H, W, C, P, Q);
      else if (relu)
        hipLaunchKernelGGL((blur_fwd_kernel<true, true>), grid, block, 0, st, a, sc, sh, out, H, W, C, P, Q);
      else
        hipLaunchKernelGGL((blur_fwd_kernel<true, false>), grid, block, 0, st, a, sc, sh, out, H, W, C, P, Q);
      break;
    case 2:
      hipLaunchKernelGGL((blur_bwd_kernel<kPlain>), grid, block, 0, st, a, y, sc, sh, c1, c2, c3, out, stats, nshard,
                         H, W, C, P, Q);
      break;
    case 3:
      hipLaunchKernelGGL((blur_bwd_kernel<kReduce>), grid, block, 0, st, a, y, sc, sh, c1, c2, c3, out, stats, nshard,
                         H, W, C, P, Q);
      break;
    case 4:
      hipLaunchKernelGGL((blur_bwd_kernel<kApply>), grid, block, 0, st, a, y, sc, sh, c1, c2, c3, out, stats, nshard,
                         H, W, C, P, Q);
      break;
    default:
      return -5;
  }
  RET_LAST;
}
