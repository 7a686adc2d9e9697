// Squeeze-and-excitation kernels on CDNA4 (SE-ResNet / SE-ResNeXt blocks; Hu et al. 2018).
//
// The gate of an SE block is one factor per SAMPLE and channel, which none of the fused block tails can carry (they
// fold one number per channel into a BN's scale). So the block's tail runs here, around per-sample tables [N][C]:
//
//   forward   se_squeeze   zsum[n][c] = sum_hw y                                  (one read of y)
//             se_excite    z = scale * zsum / HW + shift -> bf16 zq ; h = relu(zq W1^T + b1) -> bf16 ;
//                          gate = sigmoid(h W2^T + b2)                            (MFMA, per 16-sample tile)
//             se_tail      out = relu(gate * (scale * y + shift) + r), mask bits  (one read of y and r)
//   backward  se_bwd_reduce   gm = g masked ; A = sum_hw gm ; B = sum_hw gm * xhat    (one read of g, y)
//             se_excite_bwd   dgate = gamma B + beta A ; dpre2 = dgate gate (1 - gate) -> bf16 ;
//                             dpre1 = (dpre2 W2) (h > 0) -> bf16 ; dz = dpre1 W1 ; then the BN's backward moments
//                             sum du, sum du xhat from the tables alone (du = gm gate + dz / HW)
//             se_bwd_apply    dy = k1 (gm gate + dz / HW) + k2 y + k3 ; gout = gm  (one read of g, y)
//
// Reductions (se_squeeze, se_bwd_reduce): a workgroup owns (sample, 64-channel slab, row range). 256 lanes =
// 8 channel lanes x 32 row lanes, a lane loads 16 bytes (8 channels) of every 32nd row and keeps fp32 partial sums;
// the 32 row lanes fold through LDS in a fixed binary tree. A map of more than 256 pixels is cut into nsplit row
// ranges (56x56: 13, 28x28: 4) whose partials a second kernel adds in range order -- at batch 8 a 56x56x256 map
// would otherwise run on 32 workgroups. No float atomics anywhere: every sum has one order.
//
// Excite (forward and backward share the two GEMM routines): a workgroup of 4 waves owns 16 samples, the M of
// v_mfma_f32_16x16x32_bf16. The [16][C] operand tile (zq / dpre2) is formed by all 256 lanes, stored (it is also
// the weight-gradient operand) and read back as MFMA fragments, 16 bytes per lane. GEMM 1 reduces over C into at
// most 256 squeezed channels: wave w owns the 16-wide output tiles w, w + 4, ... and keeps them in registers for
// one pass over K = C. Its result goes to LDS (bf16 [16][rd], zero-padded to the 32-deep MFMA k-step) and is GEMM
// 2's left operand; wave w then walks the C / 16 output tiles w, w + 4, ... of K = rd. Weight fragments are read
// straight from memory -- each element is used once per workgroup, so staging them in LDS would add a copy and no
// reuse. The forward's weights are [out][K] with K contiguous: a fragment is one 16-byte load. The backward
// multiplies by the same two matrices from the other side (TR): a lane gathers its 8 k with 2-byte loads, the 16
// lanes of a k covering 32 contiguous bytes -- weight_prep's transposed copies need 64-multiples, which rd is not.
#include "common.h"
#include "entry.h"

namespace dbx {

constexpr int kSeRdMax = 256;              // squeezed channels an excite workgroup holds
constexpr int kSeHld = kSeRdMax + 8;       // LDS row pitch of the [16][rd] tile: +16 bytes -> conflict-free b128 reads
constexpr int kSeMaxSplit = 16;

__device__ __forceinline__ void ld8f(const float* p, float* f) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}

// ---- reductions over a sample's pixels -------------------------------------------------------------------------
// grid (C / 64, nsplit, N). BWD = false: zsum = sum y. BWD = true: A = sum gm, B = sum gm * xhat.
template <bool BWD>
__global__ __launch_bounds__(256) void se_reduce_kernel(const SeArgs a) {
  __shared__ float red[BWD ? 2 : 1][32][64];
  const int tid = threadIdx.x, cl = tid & 7, rl = tid >> 3;
  const int c0 = blockIdx.x * 64 + cl * 8, sp = blockIdx.y, n = blockIdx.z;
  const int rps = (a.HW + a.nsplit - 1) / a.nsplit;
  const int rbeg = sp * rps, rend = min(a.HW, rbeg + rps);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float mu[8], is[8];
  if (BWD) { ld8f(a.mean + c0, mu); ld8f(a.invstd + c0, is); }
  for (int r = rbeg + rl; r < rend; r += 32) {
    const size_t e = ((size_t)n * a.HW + r) * a.C + c0;
    float yv[8];
    unpack8(*reinterpret_cast<const u32x4*>(a.y + e), yv);
    if (BWD) {
      float gv[8];
      unpack8(*reinterpret_cast<const u32x4*>(a.g + e), gv);
      const unsigned bits = a.mbits[e >> 3];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gm = (bits >> j) & 1u ? gv[j] : 0.f;
        s[j] += gm;
        q[j] += gm * ((yv[j] - mu[j]) * is[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += yv[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][rl][cl * 8 + j] = s[j];
    if (BWD) red[BWD ? 1 : 0][rl][cl * 8 + j] = q[j];
  }
  __syncthreads();
  // the fixed tree over the 32 row lanes: rows [0, h) += rows [h, 2h), h = 16, 8, 4, 2, 1
  for (int h = 16; h > 0; h >>= 1) {
    for (int i = tid; i < h * 64; i += 256) {
      const int r = i >> 6, c = i & 63;
      red[0][r][c] += red[0][r + h][c];
      if (BWD) red[BWD ? 1 : 0][r][c] += red[BWD ? 1 : 0][r + h][c];
    }
    __syncthreads();
  }
  if (tid < 64) {
    const int c = blockIdx.x * 64 + tid;
    const size_t o = (size_t)n * a.C + c;
    if (a.nsplit == 1) {
      if (BWD) { a.A[o] = red[0][0][tid]; a.B[o] = red[BWD ? 1 : 0][0][tid]; }
      else a.zsum[o] = red[0][0][tid];
    } else {  // part[split][which][N][C]
      const size_t plane = (size_t)a.N * a.C;
      a.part[((size_t)sp * 2) * plane + o] = red[0][0][tid];
      if (BWD) a.part[((size_t)sp * 2 + 1) * plane + o] = red[BWD ? 1 : 0][0][tid];
    }
  }
}

// second stage of a split reduction: the nsplit partials of every (n, c), added in range order
template <bool BWD>
__global__ __launch_bounds__(256) void se_reduce_fin_kernel(const SeArgs a) {
  const size_t plane = (size_t)a.N * a.C;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < plane; o += (size_t)gridDim.x * 256) {
    float s = 0.f, q = 0.f;
    for (int k = 0; k < a.nsplit; ++k) {
      s += a.part[((size_t)k * 2) * plane + o];
      if (BWD) q += a.part[((size_t)k * 2 + 1) * plane + o];
    }
    if (BWD) { a.A[o] = s; a.B[o] = q; }
    else a.zsum[o] = s;
  }
}

// ---- the two GEMMs of the excite kernels ------------------------------------------------------------------------
// out[16][rd] = X[16][C] W^T, W = [rd][C]. X: global bf16 rows m0 .. m0 + 15 of [N][C] (rows past N read as zero).
// Wave `wid` owns output tiles wid, wid + 4, ... (<= 4); acc[t][q] = out[m = lane & 15][16 (wid + 4 t) + 4 (lane >> 4) + q]
template <bool TR>
__device__ __forceinline__ void se_gemm_k_c(const bf16* X, const bf16* __restrict__ W, int N, int C, int rd,
                                            int m0, int wid, int lane, f32x4 (&acc)[4]) {
  const int ntile = (rd + 15) >> 4, lr = lane & 15, kq = (lane >> 4) * 8;
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (wid >= ntile) return;
  const bool xok = m0 + lr < N;
  const bf16* xp = X + (size_t)(xok ? m0 + lr : 0) * C + kq;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k0 = 0; k0 < C; k0 += 32) {
    const bf16x8 xf = xok ? *reinterpret_cast<const bf16x8*>(xp + k0) : zero;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = (wid + 4 * t) * 16 + lr;  // (wave-uniform tile test; rows past rd are the zero padding)
      if (wid + 4 * t < ntile) {
        bf16x8 wf = zero;
        if (row < rd) {
          if (!TR) wf = *reinterpret_cast<const bf16x8*>(W + (size_t)row * C + k0 + kq);
          else {
#pragma unroll
            for (int j = 0; j < 8; ++j) wf[j] = W[(size_t)(k0 + kq + j) * rd + row];
          }
        }
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[t], 0, 0, 0);
      }
    }
  }
}

// one 16-wide tile of out[16][C] = H[16][rd] W^T, W = [C][rd], H in LDS (pitch kSeHld, zero past rd):
// acc[q] = out[m = lane & 15][n0 + 4 (lane >> 4) + q]
template <bool TR>
__device__ __forceinline__ f32x4 se_gemm_k_rd(const bf16* hs, const bf16* __restrict__ W, int rd, int C, int n0,
                                              int lane) {
  const int lr = lane & 15, kq = (lane >> 4) * 8;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bf16* wp = TR ? W + n0 + lr : W + (size_t)(n0 + lr) * rd + kq;
  for (int k0 = 0; k0 < rd; k0 += 32) {
    const bf16x8 hf = *reinterpret_cast<const bf16x8*>(hs + lr * kSeHld + k0 + kq);
    bf16x8 wf = zero;
    if (k0 + kq < rd) {  // (rd % 8 == 0: a lane's 8 k are all inside or all padding)
      if (!TR) wf = *reinterpret_cast<const bf16x8*>(wp + k0);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) wf[j] = wp[(size_t)(k0 + kq + j) * C];
      }
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, hf, acc, 0, 0, 0);
  }
  return acc;
}

__device__ __forceinline__ void se_zero_h(bf16* hs, int tid) {
  for (int i = tid; i < 16 * kSeHld / 8; i += 256) reinterpret_cast<u32x4*>(hs)[i] = u32x4{0u, 0u, 0u, 0u};
}

// grid: ceil(N / 16) workgroups of 256
__global__ __launch_bounds__(256) void se_excite_kernel(const SeArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 hs[16 * kSeHld];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m0 = blockIdx.x * 16;
  const int C = a.C, rd = a.rd, rows = min(16, a.N - m0);
  const float inv_hw = 1.f / (float)a.HW;
  se_zero_h(hs, tid);
  // z = scale * zsum / HW + shift, rounded once to bf16: fc1's operand and its weight-gradient operand
  for (int i = tid; i < rows * (C >> 3); i += 256) {
    const int m = i / (C >> 3), c = (i - m * (C >> 3)) * 8;
    const size_t o = (size_t)(m0 + m) * C + c;
    float z[8], sc[8], sh[8];
    ld8f(a.zsum + o, z); ld8f(a.scale + c, sc); ld8f(a.shift + c, sh);
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = sc[j] * (z[j] * inv_hw) + sh[j];
    *reinterpret_cast<u32x4*>(a.zq + o) = pack8(z);
  }
  __syncthreads();  // (zq is read back by this workgroup only: the barrier orders its stores and loads)
  f32x4 acc[4];
  se_gemm_k_c<false>(a.zq, a.wa, a.N, C, rd, m0, wid, lane, acc);
  const int lr = lane & 15, nq = (lane >> 4) * 4;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = (wid + 4 * t) * 16 + nq + q;
      if (n < rd) {
        const bf16 hv = (bf16)fmaxf(acc[t][q] + a.ba[n], 0.f);
        hs[lr * kSeHld + n] = hv;
        if (lr < rows) a.h[(size_t)(m0 + lr) * rd + n] = hv;
      }
    }
  }
  __syncthreads();
  for (int tile = wid; tile < (C >> 4); tile += 4) {
    const f32x4 r = se_gemm_k_rd<false>(hs, a.wb, rd, C, tile * 16, lane);
    if (lr < rows) {
      const int c = tile * 16 + nq;
      const f32x4 b = *reinterpret_cast<const f32x4*>(a.bb + c);
      f32x4 gt;
#pragma unroll
      for (int q = 0; q < 4; ++q) gt[q] = 1.f / (1.f + __expf(-(r[q] + b[q])));
      *reinterpret_cast<f32x4*>(a.gate + (size_t)(m0 + lr) * C + c) = gt;
    }
  }
}

__global__ __launch_bounds__(256) void se_excite_bwd_kernel(const SeArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 hs[16 * kSeHld];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m0 = blockIdx.x * 16;
  const int C = a.C, rd = a.rd, rows = min(16, a.N - m0);
  se_zero_h(hs, tid);
  // dpre2 = (gamma B + beta A) gate (1 - gate) -> bf16 (a.zq): this GEMM's operand and fc2's weight-gradient operand
  for (int i = tid; i < rows * (C >> 3); i += 256) {
    const int m = i / (C >> 3), c = (i - m * (C >> 3)) * 8;
    const size_t o = (size_t)(m0 + m) * C + c;
    float A[8], B[8], gt[8], ga[8], be[8], d[8];
    ld8f(a.A + o, A); ld8f(a.B + o, B); ld8f(a.gate + o, gt); ld8f(a.gamma + c, ga); ld8f(a.beta + c, be);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = (ga[j] * B[j] + be[j] * A[j]) * gt[j] * (1.f - gt[j]);
    *reinterpret_cast<u32x4*>(a.zq + o) = pack8(d);
  }
  __syncthreads();
  f32x4 acc[4];
  se_gemm_k_c<true>(a.zq, a.wa, a.N, C, rd, m0, wid, lane, acc);  // dpre2 W2, W2 = [C][rd]: fragments gathered
  const int lr = lane & 15, nq = (lane >> 4) * 4;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = (wid + 4 * t) * 16 + nq + q;
      if (n < rd && lr < rows) {
        const size_t o = (size_t)(m0 + lr) * rd + n;
        const bf16 dv = (bf16)((float)a.h[o] > 0.f ? acc[t][q] : 0.f);
        hs[lr * kSeHld + n] = dv;
        a.dpre1[o] = dv;
      }
    }
  }
  __syncthreads();
  for (int tile = wid; tile < (C >> 4); tile += 4) {
    const f32x4 r = se_gemm_k_rd<true>(hs, a.wb, rd, C, tile * 16, lane);  // dpre1 W1, W1 = [rd][C]
    if (lr < rows) *reinterpret_cast<f32x4*>(a.dz + (size_t)(m0 + lr) * C + tile * 16 + nq) = r;
  }
}

// The last BN's backward moments from the tables alone: du = gm gate + dz / HW, so per channel
//   sum du      = sum_n (gate A + dz)
//   sum du xhat = sum_n (gate B + dz (zsum - HW mean) invstd / HW)
// in fp64, n in a fixed order (8 lanes take n = l, l + 8, ...; their sums are added in lane order). Written to shard 0
// of bstats ([nshard][2][C], what bn_bwd_coeff sums), the other shards zeroed. grid C / 32, 256 lanes = 32 c x 8 n.
__global__ __launch_bounds__(256) void se_moments_kernel(const SeArgs a) {
  __shared__ double red[2][8][32];
  const int cl = threadIdx.x & 31, nl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
  const double hw = (double)a.HW, mu = (double)a.mean[c], is = (double)a.invstd[c];
  double s = 0.0, q = 0.0;
  for (int n = nl; n < a.N; n += 8) {
    const size_t o = (size_t)n * a.C + c;
    const double gt = a.gate[o], dz = a.dz[o];
    s += gt * (double)a.A[o] + dz;
    q += gt * (double)a.B[o] + dz * (((double)a.zsum[o] - hw * mu) * is / hw);
  }
  red[0][nl][cl] = s;
  red[1][nl][cl] = q;
  __syncthreads();
  if (nl == 0) {
    double ss = 0.0, qq = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { ss += red[0][k][cl]; qq += red[1][k][cl]; }
    a.bstats[c] = ss;
    a.bstats[a.C + c] = qq;
    for (int k = 1; k < a.nshard; ++k) {
      a.bstats[(size_t)k * 2 * a.C + c] = 0.0;
      a.bstats[(size_t)k * 2 * a.C + a.C + c] = 0.0;
    }
  }
}

// ---- elementwise passes over the block's tensors -----------------------------------------------------------------
// out = relu(gate[n][c] * (scale_c y + shift_c) + r): one fp32 evaluation, one rounding; mask bits of the stored values
template <int RES>
__global__ __launch_bounds__(256) void se_tail_kernel(const SeArgs a) {
  const int cv = a.C >> 3;
  const long long per = (long long)a.HW * cv, total = per * a.N;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const int n = (int)(v / per), c = (int)(v % cv) * 8;
    const long long e = v * 8;
    float f[8], sc[8], sh[8], gt[8];
    unpack8(*reinterpret_cast<const u32x4*>(a.y + e), f);
    ld8f(a.scale + c, sc); ld8f(a.shift + c, sh); ld8f(a.gate + (size_t)n * a.C + c, gt);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = gt[j] * (sc[j] * f[j] + sh[j]);
    if (RES) {
      float r[8];
      unpack8(*reinterpret_cast<const u32x4*>(a.res + e), r);
      if (RES == 2) {
        float ra[8], rb[8];
        ld8f(a.rsc + c, ra); ld8f(a.rsh + c, rb);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] * ra[j] + rb[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += r[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = fmaxf(f[j], 0.f);
    const u32x4 o = pack8(f);
    *reinterpret_cast<u32x4*>(a.out + e) = o;
    if (a.mbits) {
      float qv[8];
      unpack8(o, qv);
      unsigned bits = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) bits |= (qv[j] > 0.f ? 1u : 0u) << j;
      a.mbits[v] = (unsigned char)bits;
    }
  }
}

// dy = k1 (gm gate + dz / HW) + k2 y + k3 (a.out) ; gout = gm
__global__ __launch_bounds__(256) void se_bwd_apply_kernel(const SeArgs a) {
  const int cv = a.C >> 3;
  const long long per = (long long)a.HW * cv, total = per * a.N;
  const float inv_hw = 1.f / (float)a.HW;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < total; v += (long long)gridDim.x * 256) {
    const int n = (int)(v / per), c = (int)(v % cv) * 8;
    const long long e = v * 8;
    float g[8], yv[8], gt[8], dz[8], k1[8], k2[8], k3[8], d[8];
    unpack8(*reinterpret_cast<const u32x4*>(a.g + e), g);
    unpack8(*reinterpret_cast<const u32x4*>(a.y + e), yv);
    const unsigned bits = a.mbits[v];
    ld8f(a.gate + (size_t)n * a.C + c, gt); ld8f(a.dz + (size_t)n * a.C + c, dz);
    ld8f(a.coeff + c, k1); ld8f(a.coeff + a.C + c, k2); ld8f(a.coeff + 2 * a.C + c, k3);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      g[j] = (bits >> j) & 1u ? g[j] : 0.f;
      d[j] = k1[j] * (g[j] * gt[j] + dz[j] * inv_hw) + k2[j] * yv[j] + k3[j];
    }
    *reinterpret_cast<u32x4*>(a.out + e) = pack8(d);
    *reinterpret_cast<u32x4*>(a.gout + e) = pack8(g);
  }
}

}  // namespace dbx

using namespace dbx;

// row ranges a sample's map is cut into by the reductions (ops/kernels.py se_nsplit is the same function)
static int se_nsplit(int HW) { return (HW + 255) / 256 < kSeMaxSplit ? (HW + 255) / 256 : kSeMaxSplit; }

// op: 1 se_squeeze, 2 se_excite, 3 se_tail, 4 se_bwd_reduce, 5 se_excite_bwd (+ the moments), 6 se_bwd_apply.
// -90: a shape outside the kernels' range; -91: a pointer the op needs is null; -92: an unknown op
extern "C" int dbx_se_op(int op, const dbx::SeArgs* args, hipStream_t st) {
  const SeArgs& a = *args;
  if (a.N <= 0 || a.HW <= 0 || a.C <= 0 || a.C % 64) return -90;
  if ((long long)a.N * a.HW * a.C >= (1ll << 31)) return -90;
  const long long vecs = (long long)a.N * a.HW * (a.C / 8);
  const int tiles = (a.N + 15) / 16;
  switch (op) {
    case 1:
    case 4: {
      const bool bwd = op == 4;
      if (a.nsplit != se_nsplit(a.HW) || a.N > 65535) return -90;
      if (!a.y || (a.nsplit > 1 && !a.part)) return -91;
      if (bwd ? !(a.g && a.mbits && a.mean && a.invstd && a.A && a.B) : !a.zsum) return -91;
      const dim3 grid(a.C / 64, a.nsplit, a.N);
      if (bwd) hipLaunchKernelGGL(se_reduce_kernel<true>, grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL(se_reduce_kernel<false>, grid, dim3(256), 0, st, a);
      if (a.nsplit > 1) {
        const int blocks = grid_for((long long)a.N * a.C, 256, 1024);
        if (bwd) hipLaunchKernelGGL(se_reduce_fin_kernel<true>, dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(se_reduce_fin_kernel<false>, dim3(blocks), dim3(256), 0, st, a);
      }
      RET_LAST;
    }
    case 2:
      if (a.rd < 8 || a.rd > kSeRdMax || a.rd % 8) return -90;
      if (!(a.zsum && a.scale && a.shift && a.zq && a.h && a.gate && a.wa && a.ba && a.wb && a.bb)) return -91;
      hipLaunchKernelGGL(se_excite_kernel, dim3(tiles), dim3(256), 0, st, a);
      RET_LAST;
    case 5:
      if (a.rd < 8 || a.rd > kSeRdMax || a.rd % 8 || a.nshard < 1 || a.nshard > 32) return -90;
      if (!(a.A && a.B && a.gate && a.gamma && a.beta && a.zq && a.h && a.dpre1 && a.dz && a.wa && a.wb && a.zsum &&
            a.mean && a.invstd && a.bstats))
        return -91;
      hipLaunchKernelGGL(se_excite_bwd_kernel, dim3(tiles), dim3(256), 0, st, a);
      hipLaunchKernelGGL(se_moments_kernel, dim3(a.C / 32), dim3(256), 0, st, a);
      RET_LAST;
    case 3: {
      if (!(a.y && a.scale && a.shift && a.gate && a.out)) return -91;
      if ((a.res_mode && !a.res) || (a.res_mode == 2 && !(a.rsc && a.rsh))) return -91;
      const dim3 grid(grid_for(vecs)), blk(256);
      if (a.res_mode == 0) hipLaunchKernelGGL(se_tail_kernel<0>, grid, blk, 0, st, a);
      else if (a.res_mode == 1) hipLaunchKernelGGL(se_tail_kernel<1>, grid, blk, 0, st, a);
      else if (a.res_mode == 2) hipLaunchKernelGGL(se_tail_kernel<2>, grid, blk, 0, st, a);
      else return -90;
      RET_LAST;
    }
    case 6:
      if (!(a.g && a.mbits && a.y && a.gate && a.dz && a.coeff && a.out && a.gout)) return -91;
      hipLaunchKernelGGL(se_bwd_apply_kernel, dim3(grid_for(vecs)), dim3(256), 0, st, a);
      RET_LAST;
  }
  return -92;
}
