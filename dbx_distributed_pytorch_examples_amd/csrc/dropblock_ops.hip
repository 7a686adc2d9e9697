// DropBlock (Ghiasi et al. 2018; timm's drop_block_2d with batchwise=False, with_noise=False) for the NHWC bf16
// programs: a site sits behind one BN, in front of its ReLU's consumer, on an activation [N, H, W, C].
//
//   dropblock_mask     bits[n,h,w,c/32] bit c%32 = keep(n,h,w,c); kept += number of ones     (reads no activation)
//   dropblock_fwd      out = bf16( relu(y*sc + sh) * keep * scale )                          (one pass, one rounding)
//   dropblock_bn_bwd   g = d * keep * scale * [y*sc + sh > 0], then
//                      reduce: stats += [sum g, sum g*xhat]     apply: dy = k1*g + k2*y + k3   (g is never written)
//   with scale = (float)(N*H*W*C / max(kept, 1)), formed by every lane from the site's integer counter.
//
// The mask does not depend on the data. Element (n,h,w,c) draws word idx % 4 of the Philox counter idx / 4 with
// idx = site * 2^48 + ((n*H + h)*W + w)*C + c (reference.philox_u32): four neighbouring channels share one
// philox4x32_10 call. It is a seed iff word < thr inside the valid interior r <= h < H - r, r <= w < W - r, and
// keep = 0 within the bs x bs window (r = bs / 2) around every seed of the same sample and channel.
//
// Mask kernel, work split: a workgroup owns one image, a 64-channel slab, a band of kBH rows and a chunk of kCW
// columns, plus an r-wide halo on every side. Each lane issues one Philox call per four channels and packs the four
// compare results into a nibble; eight lanes OR their nibbles through the wave, so LDS holds the SEED bits of the
// tile as two 32-bit words per pixel. The window is then separable and bitwise on those words: an OR over bs
// neighbouring columns (LDS -> LDS), an OR over bs rows on the way out, the complement stored -- no per-element
// arithmetic. __popc of the stored words is folded through LDS and one integer atomic add per workgroup goes into the
// site's counter: the count does not depend on the order of arrival.
//
// Apply kernels: 256 lanes = 32 pixels x 8 channel groups of a 64-channel slab, 16 bytes of y (and d) per lane, the
// per-channel coefficients in registers; one mask word serves 32 channels (four lanes). The reduce form folds the 32
// pixel lanes of a channel in a fixed order and adds one fp64 pair per channel into the block's shard, as
// bn_bwd_reduce and blur_bn_bwd_reduce do.
#include "common.h"
#include "entry.h"
#include "philox.h"

namespace {

using dbx::DropBlockArgs;

constexpr int kSlab = 64;                      // channels of a workgroup
constexpr int kBH = 16, kCW = 32;              // rows of a band, columns of a chunk
constexpr int kRMax = 3;                       // block sizes up to 7
constexpr int kSR = kBH + 2 * kRMax, kSC = kCW + 2 * kRMax;
constexpr int kPix = 256;                      // pixels of an apply workgroup: 8 rounds of 32

__global__ __launch_bounds__(256) void dropblock_mask_kernel(const DropBlockArgs a, int r, int nchunk) {
  __shared__ unsigned seedb[kSR * kSC * 2];    // [row + halo][column + halo][word]: seed bits
  __shared__ unsigned hor[kSR * kCW * 2];      // [row + halo][column][word]: OR over the window's columns
  __shared__ unsigned red[256];
  const int tid = threadIdx.x, slab = blockIdx.y, n = blockIdx.z;
  const int band = blockIdx.x / nchunk, chunk = blockIdx.x - band * nchunk;
  const int H = a.H, W = a.W, C = a.C;
  const int h0 = band * kBH, w0 = chunk * kCW;
  const int bh = min(kBH, H - h0), cw = min(kCW, W - w0);
  const int rows = bh + 2 * r, cols = cw + 2 * r;
  const unsigned thr = *a.thr, offset = *a.offset;
  const unsigned long long site_base = (unsigned long long)a.site << 46;  // (site * 2^48) / 4

  // seed bits: 16 Philox calls per pixel of the slab, none outside the valid interior (no seed can lie there)
  const int items = rows * cols * 16;
  for (int base = 0; base < items; base += 256) {   // (uniform trip count: the wave shuffles below need every lane)
    const int i = base + tid, pix = i >> 4, quad = i & 15;
    const bool live = i < items;
    const int rr = pix / cols, cc = pix - rr * cols;
    const int h = h0 - r + rr, w = w0 - r + cc;
    unsigned nib = 0;
    if (live && h >= r && h < H - r && w >= r && w < W - r) {
      const unsigned long long e = (((unsigned long long)n * H + h) * W + w) * C + slab * kSlab + quad * 4;
      unsigned u[4];
      dbx::philox4x32_10(site_base + (e >> 2), a.seed, offset, u);
      nib = (u[0] < thr ? 1u : 0u) | (u[1] < thr ? 2u : 0u) | (u[2] < thr ? 4u : 0u) | (u[3] < thr ? 8u : 0u);
    }
    unsigned word = nib << (4 * (quad & 7));
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    word |= __shfl_xor(word, 4);
    if (live && (quad & 7) == 0) seedb[(rr * kSC + cc) * 2 + (quad >> 3)] = word;
  }
  __syncthreads();
  // OR over the bs columns of the window, for every staged row
  for (int i = tid; i < rows * cw * 2; i += 256) {
    const int k = i & 1, p = i >> 1, rr = p / cw, cc = p - rr * cw;
    unsigned v = 0;
    for (int d = 0; d <= 2 * r; ++d) v |= seedb[(rr * kSC + cc + d) * 2 + k];
    hor[(rr * kCW + cc) * 2 + k] = v;
  }
  __syncthreads();
  // OR over the bs rows, complement, store, count
  unsigned cnt = 0;
  unsigned* out = a.bits + (((size_t)n * H + h0) * W + w0) * (C / 32) + slab * 2;
  for (int i = tid; i < bh * cw * 2; i += 256) {
    const int k = i & 1, p = i >> 1, rr = p / cw, cc = p - rr * cw;
    unsigned v = 0;
    for (int d = 0; d <= 2 * r; ++d) v |= hor[((rr + d) * kCW + cc) * 2 + k];
    out[((size_t)rr * W + cc) * (C / 32) + k] = ~v;
    cnt += __popc(~v);
  }
  red[tid] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) atomicAdd(a.kept, (unsigned long long)red[0]);
}

__device__ __forceinline__ void load8f(const float* p, float* f) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}

enum { kFwd = 0, kReduce = 1, kApply = 2 };

// MODE kFwd   : out = relu(y*sc + sh) * keep * scale
//      kReduce: stats[shard] += [sum g, sum g * (y - c1) * c2]          (c1 = mean, c2 = invstd)
//      kApply : out = c1*g + c2*y + c3                                   (bn_bwd_coeff's k1, k2, k3)
template <int MODE>
__global__ __launch_bounds__(256) void dropblock_apply_kernel(const DropBlockArgs a, int M) {
  __shared__ float red[MODE == kReduce ? 2 * 256 * 8 : 1];
  const int tid = threadIdx.x, cg = tid & 7, px = tid >> 3;
  const int C = a.C, c0 = blockIdx.y * kSlab + cg * 8, wpp = C / 32;
  const unsigned long long kept = *a.kept;
  const float ks = (float)((double)((long long)M * C) / (double)(kept > 0 ? kept : 1ull));
  float s[8], h[8], k1[8], k2[8], k3[8];
  load8f(a.sc + c0, s); load8f(a.sh + c0, h);
  if (MODE != kFwd) { load8f(a.c1 + c0, k1); load8f(a.c2 + c0, k2); }
  if (MODE == kApply) load8f(a.c3 + c0, k3);
  float as[8] = {0, 0, 0, 0, 0, 0, 0, 0}, aq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int p0 = blockIdx.x * kPix;
#pragma unroll 2
  for (int it = 0; it < kPix / 32; ++it) {
    const int p = p0 + it * 32 + px;
    if (p >= M) break;
    const size_t e = (size_t)p * C + c0;
    const unsigned m8 = (a.bits[(size_t)p * wpp + blockIdx.y * 2 + (cg >> 2)] >> ((cg & 3) * 8)) & 0xffu;
    float yv[8], g[8];
    unpack8(*reinterpret_cast<const u32x4*>(a.y + e), yv);
    if (MODE == kFwd) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = fmaxf(yv[j] * s[j] + h[j], 0.f) * ((m8 >> j) & 1u ? ks : 0.f);
      *reinterpret_cast<u32x4*>(a.out + e) = pack8(g);
      continue;
    }
    unpack8(*reinterpret_cast<const u32x4*>(a.d + e), g);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      g[j] = (((m8 >> j) & 1u) && (yv[j] * s[j] + h[j]) > 0.f) ? g[j] * ks : 0.f;
    if (MODE == kApply) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = k1[j] * g[j] + k2[j] * yv[j] + k3[j];
      *reinterpret_cast<u32x4*>(a.out + e) = pack8(o);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) { as[j] += g[j]; aq[j] += g[j] * (yv[j] - k1[j]) * k2[j]; }
    }
  }
  if (MODE == kReduce) {
    // the block's 32 pixel lanes of a channel in a fixed order, then one fp64 add per channel and moment into the
    // block's shard: bn_bwd_reduce's scheme
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[tid * 8 + j] = as[j]; red[256 * 8 + tid * 8 + j] = aq[j]; }
    __syncthreads();
    const int bid = blockIdx.y * gridDim.x + blockIdx.x;
    double* st = a.stats + (size_t)(bid % a.nshard) * 2 * C + blockIdx.y * kSlab;
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

// op 1 dropblock_mask, 2 dropblock_fwd, 3 / 4 dropblock_bn_bwd reduce / apply on the fields of *args (a HOST struct,
// abi.h) that the op names; args->bs is the site's block size, clipped to the map and made odd here
extern "C" int dbx_dropblock_op(int op, const dbx::DropBlockArgs* args, hipStream_t st) {
  DropBlockArgs a = *args;
  if (a.N < 1 || a.H < 1 || a.W < 1 || a.C < kSlab || a.C % kSlab || a.bs < 1 || a.bs > 2 * kRMax + 1) return -1;
  if ((long long)a.N * a.H * a.W * a.C >= (1LL << 31) || a.N > 65535 || a.C / kSlab > 65535 || a.site < 0 ||
      a.site > 65535)
    return -3;
  int bs = min(a.bs, min(a.H, a.W));
  bs -= !(bs & 1);
  a.bs = bs;
  if (!a.bits || !a.kept) return -4;
  const int M = a.N * a.H * a.W;
  const dim3 block(256), agrid((M + kPix - 1) / kPix, a.C / kSlab);
  switch (op) {
    case 1: {
      if (!a.thr || !a.offset) return -4;
      const int nband = (a.H + kBH - 1) / kBH, nchunk = (a.W + kCW - 1) / kCW;
      hipLaunchKernelGGL(dropblock_mask_kernel, dim3(nband * nchunk, a.C / kSlab, a.N), block, 0, st, a, bs / 2,
                         nchunk);
      break;
    }
    case 2:
      if (!(a.y && a.sc && a.sh && a.out)) return -4;
      hipLaunchKernelGGL((dropblock_apply_kernel<kFwd>), agrid, block, 0, st, a, M);
      break;
    case 3:
      if (!(a.y && a.d && a.sc && a.sh && a.c1 && a.c2 && a.stats) || a.nshard < 1) return -4;
      hipLaunchKernelGGL((dropblock_apply_kernel<kReduce>), agrid, block, 0, st, a, M);
      break;
    case 4:
      if (!(a.y && a.d && a.sc && a.sh && a.c1 && a.c2 && a.c3 && a.out)) return -4;
      hipLaunchKernelGGL((dropblock_apply_kernel<kApply>), agrid, block, 0, st, a, M);
      break;
    default:
      return -5;
  }
  RET_LAST;
}
