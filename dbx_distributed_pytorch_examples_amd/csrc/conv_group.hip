// Grouped 3x3 convolutions (pad 1, stride 1 or 2, IC == OC == C, C % 64 == 0) for ResNeXt bottlenecks: forward,
// data gradient and weight gradient at cpg = C / groups in {4, 8, 16, 32, 64} channels per group. NHWC bf16
// activations, bf16 weights [C][9 * cpg] (KRSC inside the group: what weight_prep writes for IC = cpg), fp32
// accumulation.
//
// Channel slabs. CB = max(16, cpg) consecutive channels form one dense CB -> CB convolution whose per-tap weight
// matrix is block-diagonal (16 / cpg groups per slab at cpg = 4 / 8, one group above); the zeros are filled in
// once per workgroup, when the weights are expanded into register fragments, so every cpg runs on
// v_mfma_f32_16x16x32_bf16 and no tensor work is left to the VALU. At cpg = 4 three quarters of the MFMA work
// multiply zeros (cpg = 8: one half); the kernels read and write each activation once per launch (plus the
// tiles' halo rows, which neighbouring tiles find in L2).
//
// Forward and data gradient (gconv_kernel). A workgroup of four waves owns TH output rows of one image and 64
// channels. It stages the source rows it needs, halo included, once in LDS as [row][col + 2][64 + 8 pad] bf16
// (144-byte pixels: the 16-byte fragment reads of 16 consecutive pixels fall on 16 different bank groups); rows
// and columns outside the image are zeros (buffer loads past the range). Wave w owns output channels 16w..16w+15
// of the 64 and keeps their expanded weights stationary in registers: the K dimension of the MFMA is the flat
// list of (tap, 8-channel chunk) pairs of the wave's slab, 9 * CB / 8 chunks in fragments of four (5 / 9 / 18
// fragments at CB = 16 / 32 / 64; a chunk past the last tap is zero on both operands). The wave walks the tile's
// pixels sixteen at a time, two groups in flight: per fragment one ds_read_b128 at (pixel, tap) and one MFMA
// (weights = A, rows = output channels; pixels = B), then rounds to bf16 and stores four channels per lane. With
// `stats` it adds the per-channel sum and sum of squares of the ROUNDED outputs (fp32 per lane over the tile, a
// 16-lane butterfly, then one fp64 atomic pair per channel) into shard (tile % nshard) of the [nshard][2][C]
// slabs the other conv epilogues fill, so the existing finalize launches read them unchanged.
// The data gradient is the same kernel with the in-group transpose of the weights read straight from the KRSC
// copy (no transposed copy exists for grouped convs). Stride 1: the taps mirrored. Stride 2: ONE launch -- the
// dx pixels of a tile are walked in four parity classes (row parity x column parity); a class touches only the
// taps of its own parity (1, 2, 2 and 4 of the 9: every tap belongs to exactly one class, so the stationary
// fragments are again 5 / 9 / 18), gathered from the dy rows staged once for all four.
//
// Weight gradient (gconv_wgrad_kernel): dW[co][tap][ci] = sum over pixels dy[p][co] * x[p + tap][ci] per slab,
// pixels on the MFMA reduction dimension. A workgroup takes a contiguous range of (image, row tile) tiles and 64
// channels; per tile it stages the x rows (as above) and the dy rows in LDS and reads both operands with
// gfx950's transposing LDS reads (ds_read_b64_tr_b16: pixels along K out of a pixel-major image; the tap is a
// per-lane address offset). Wave w keeps the 9 x (CB / 16) fp32 accumulator blocks of its 16 output channels in
// registers over the whole range (36 / 72 / 144 VGPRs: at CB = 64 the 9 x 64 x 64 block is split over the four
// waves) and writes only the block-diagonal part, as its share of ONE fp32 slab [C][9 * cpg] per range;
// dbx_wgrad_reduce sums the slabs in fixed order (no float atomics: bit-reproducible).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any instantiation; LDS is
// dynamic, sized per launch to the tile (at most 64 KiB); the VGPR counts per cpg are in the README.
#include <type_traits>

#include "common.h"
#include "entry.h"

namespace dbx {

constexpr int kPix = 72;           // bf16 elements per staged pixel: 64 channels + 8 of padding
constexpr int kLdsMax = 64 << 10;  // dynamic LDS per workgroup

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// the parity classes of the stride-2 data gradient (SUB = 2; SUB = 1: one class with all nine taps): a dx row of
// parity ph takes the kernel rows r with (ph + 1 - r) even -- r = 1 for ph = 0, r = 0 and 2 for ph = 1
__host__ __device__ constexpr int cls_n(int sub, int par) { return sub == 1 ? 3 : (par == 0 ? 1 : 2); }
__host__ __device__ constexpr int cls_tap(int sub, int par, int j) { return sub == 1 ? j : (par == 0 ? 1 : 2 * j); }
__host__ __device__ constexpr int cls_frags(int sub, int cls, int ch) {  // MFMA K fragments (4 chunks) of a class
  return (cls_n(sub, cls / sub) * cls_n(sub, cls % sub) * ch + 3) / 4;
}
__host__ __device__ constexpr int cls_base(int sub, int cls, int ch) {  // fragments of the classes before it
  int n = 0;
  for (int c = 0; c < cls; ++c) n += cls_frags(sub, c, ch);
  return n;
}

// the source rows [row0, row0 + nrow) x columns [-1, SW] of one image, 64 channels from cb -> lds[(row, col + 1)]
__device__ __forceinline__ void stage_rows(bf16* lds, const bf16* img, int SH, int SW, int C, int cb, int row0,
                                           int nrow, int tid) {
  const rsrc_t sr = make_rsrc(img, 2ull * SH * SW * C);
  const int WP = SW + 2, total = nrow * WP * 8;
  for (int e0 = tid; e0 < total; e0 += 4 * 256) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + 256 * u, pix = e >> 3, pr = pix / WP, pc = pix - pr * WP;
      const int h = row0 + pr, w = pc - 1;
      const bool ok = e < total && (unsigned)h < (unsigned)SH && (unsigned)w < (unsigned)SW;
      v[u] = buf_load16(sr, ok ? 2u * (unsigned)((h * SW + w) * C + cb + (e & 7) * 8) : kOOB);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + 256 * u;
      if (e < total) *reinterpret_cast<u32x4*>(lds + (e >> 3) * kPix + (e & 7) * 8) = v[u];
    }
  }
}

// MODE 0: forward (y = conv(x), stride a.stride). MODE 1: data gradient (x = dy [N][OH][OW][C], y = dx
// [N][IH][IW][C]); SUB = the conv's stride. a.IC = cpg, a.OC = C, a.nr = TH (output rows per tile, a multiple of
// SUB), a.ns = row tiles per image.
template <int CPG, int MODE, int SUB, bool STATS>
__global__ __launch_bounds__(256) void gconv_kernel(const IGemmArgs a) {
  constexpr int CB = CPG < 16 ? 16 : CPG, CH = CB / 8, NCLS = SUB * SUB;
  constexpr int NF = cls_base(SUB, NCLS, CH);
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
  const int C = a.OC, TH = a.nr, ntile = a.ns;
  const int n = blockIdx.x / ntile, t0 = (blockIdx.x - n * ntile) * TH, cb = blockIdx.y * 64;
  const int OHo = MODE == 0 ? a.OH : a.IH, OWo = MODE == 0 ? a.OW : a.IW;  // the written tensor
  const int SH = MODE == 0 ? a.IH : a.OH, SW = MODE == 0 ? a.IW : a.OW;    // the staged tensor
  const int st = MODE == 0 ? a.stride : 1, WP = SW + 2;
  const int row0 = MODE == 0 ? t0 * st - 1 : (SUB == 1 ? t0 - 1 : t0 / 2);
  const int nrow = MODE == 0 ? (TH - 1) * st + 3 : (SUB == 1 ? TH + 2 : TH / 2 + 1);
  stage_rows(lds, a.x + (size_t)n * SH * SW * C, SH, SW, C, cb, row0, nrow, tid);

  // stationary weights: row = this lane's channel of the wave's 16, K = (tap, chunk) of the wave's slab
  const int slab = (16 * wid) / CB * CB;  // first channel of the slab, within the 64
  const int rowc = cb + 16 * wid + li;
  const unsigned short* wp = reinterpret_cast<const unsigned short*>(a.w);
  bf16x8 wf[NF];
  int dl[NF];
  bool live[NF];
  static_for<0, NCLS>([&](auto ic) {
    constexpr int c = decltype(ic)::value, ph = c / SUB, pw = c % SUB;
    constexpr int ns = cls_n(SUB, pw), ntap = cls_n(SUB, ph) * ns, f0 = cls_base(SUB, c, CH);
#pragma unroll
    for (int ks = 0; ks < cls_frags(SUB, c, CH); ++ks) {
      const int q = ks * 4 + g, j = q / CH, chunk = q - j * CH;
      const bool ok = j < ntap;
      const int jj = ok ? j : 0;
      const int r = cls_tap(SUB, ph, jj / ns), s = cls_tap(SUB, pw, jj % ns);
      const int kc = cb + slab + chunk * 8;  // first of the 8 channels on K
      unsigned short v[8];
      if constexpr (MODE == 0 && CPG >= 8) {  // 8 consecutive input channels of one group: one 16-byte load
        const bool same = rowc / CPG == kc / CPG;
        const u32x4 z = {0u, 0u, 0u, 0u};
        const u32x4 t = (ok && same) ? *reinterpret_cast<const u32x4*>(
                                           wp + (size_t)rowc * (9 * CPG) + (r * 3 + s) * CPG + kc % CPG)
                                     : z;
        wf[f0 + ks] = __builtin_bit_cast(bf16x8, t);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = kc + e;
          const bool same = ok && rowc / CPG == k / CPG;
          // forward: w[oc = row][tap][ci = k]; data gradient: w[co = k][tap][ci = row]
          const size_t off = MODE == 0 ? (size_t)rowc * (9 * CPG) + (r * 3 + s) * CPG + k % CPG
                                       : (size_t)k * (9 * CPG) + (r * 3 + s) * CPG + rowc % CPG;
          v[e] = same ? wp[off] : (unsigned short)0;
        }
        typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
        const u16x8 t = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
        wf[f0 + ks] = __builtin_bit_cast(bf16x8, t);
      }
      // LDS offset of the tap relative to the pixel's base (below), plus the chunk's channels
      int dr, dc;
      if constexpr (MODE == 0) { dr = r; dc = s; }
      else if constexpr (SUB == 1) { dr = 2 - r; dc = 2 - s; }
      else { dr = (ph + 1 - r) / 2; dc = (pw + 1 - s) / 2; }
      dl[f0 + ks] = ok ? (dr * WP + dc) * kPix + slab + chunk * 8 : slab;
      live[f0 + ks] = ok;
    }
  });
  __syncthreads();

  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
  const int oc0 = cb + 16 * wid + 4 * g;  // this lane's four output channels
  static_for<0, NCLS>([&](auto ic) {
    constexpr int c = decltype(ic)::value, ph = c / SUB, pw = c % SUB;
    constexpr int f0 = cls_base(SUB, c, CH), nf = cls_frags(SUB, c, CH);
    constexpr bool ragged = (cls_n(SUB, ph) * cls_n(SUB, pw) * CH) % 4 != 0;  // the last fragment has dead chunks
    const int OWc = (OWo - pw + SUB - 1) / SUB, npix = (TH / SUB) * OWc;
    if (OWc <= 0) return;
    const unsigned long long mag = ((1ull << 40) + OWc - 1) / OWc;
    for (int p0 = 0; p0 < npix; p0 += 32) {
      int base[2], orow[2], ocol[2];
      bool ok[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int p = p0 + 16 * u + li;
        const int pp = p < npix ? p : 0, i = mdiv(pp, mag), j = pp - i * OWc;
        orow[u] = t0 + ph + SUB * i;
        ocol[u] = pw + SUB * j;
        ok[u] = p < npix && orow[u] < OHo;
        base[u] = MODE == 0 ? (i * st * WP + j * st) * kPix : (SUB == 1 ? (i * WP + j) * kPix : (i * WP + j + 1) * kPix);
      }
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < nf; ++ks) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          bf16x8 b = *reinterpret_cast<const bf16x8*>(lds + base[u] + dl[f0 + ks]);
          if constexpr (ragged) {
            if (ks == nf - 1 && !live[f0 + ks]) b = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
          }
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[f0 + ks], b, acc[u], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!ok[u]) continue;
        const unsigned lo = pack2(acc[u][0], acc[u][1]), hi = pack2(acc[u][2], acc[u][3]);
        *reinterpret_cast<uint2*>(a.y + ((size_t)(n * OHo + orow[u]) * OWo + ocol[u]) * C + oc0) = uint2{lo, hi};
        if constexpr (STATS) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = bf2f(f2bf(acc[u][r]));
            ssum[r] += v;
            ssq[r] += v * v;
          }
        }
      }
    }
  });
  if constexpr (STATS) {
    double* sp = a.stats + (size_t)(blockIdx.x % a.nshard) * 2 * C;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = ssum[r], q = ssq[r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
      }
      if (li == 0) {
        atomicAdd(sp + oc0 + r, (double)s);
        atomicAdd(sp + C + oc0 + r, (double)q);
      }
    }
  }
}

// a.IC = cpg, a.OC = C, a.nsplit = slabs (blockIdx.x), a.m_per_split = tiles per slab, a.relu_in = TH, a.KTOT =
// 9 * cpg; x [N][IH][IW][C], dy [N][OH][OW][C]; ws [nsplit][C][9 * cpg]
template <int CPG>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(const WgradArgs a) {
  constexpr int CB = CPG < 16 ? 16 : CPG, NCI = CB / 16;
  extern __shared__ __attribute__((aligned(16))) bf16 lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, li = lane & 15;
  const int q4 = li >> 2, p4 = li & 3;
  const int C = a.OC, TH = a.relu_in, st = a.stride, WP = a.IW + 2;
  const int ntile = (a.OH + TH - 1) / TH, T = a.N * ntile, cb = blockIdx.y * 64;
  const int nrow = (TH - 1) * st + 3, P = TH * a.OW, PP = (P + 31) / 32 * 32;
  bf16* sx = lds;
  bf16* sdy = lds + nrow * WP * kPix;
  const int slab = (16 * wid) / CB * CB;
  const unsigned long long mag = ((1ull << 40) + a.OW - 1) / a.OW;

  f32x4 acc[9][NCI];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int c = 0; c < NCI; ++c) acc[tp][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int tbeg = blockIdx.x * a.m_per_split, tend = min(T, tbeg + a.m_per_split);
  for (int t = tbeg; t < tend; ++t) {
    const int n = t / ntile, t0 = (t - n * ntile) * TH;
    __syncthreads();  // the previous tile's fragments have been read
    stage_rows(sx, a.x + (size_t)n * a.IH * a.IW * C, a.IH, a.IW, C, cb, t0 * st - 1, nrow, tid);
    {  // dy rows t0 .. t0 + TH, pixel-major; pixels past the tile or the image are zeros
      const rsrc_t dr = make_rsrc(a.dy + (size_t)n * a.OH * a.OW * C, 2ull * a.OH * a.OW * C);
      const int live = min(TH, a.OH - t0) * a.OW;
      for (int e = tid; e < PP * 8; e += 256) {
        const int pix = e >> 3;
        const u32x4 v = buf_load16(dr, pix < live ? 2u * (unsigned)((t0 * a.OW + pix) * C + cb + (e & 7) * 8) : kOOB);
        *reinterpret_cast<u32x4*>(sdy + pix * kPix + (e & 7) * 8) = v;
      }
    }
    __syncthreads();
    for (int k0 = 0; k0 < PP; k0 += 32) {
      s16x4 va[2], vb[2][9][NCI];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int k = k0 + 8 * g + q4 + 4 * h2;  // this lane's pixel of the 32 on K
        const int kk = k < P ? k : 0, i = mdiv(kk, mag), j = kk - i * a.OW;
        va[h2] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DBX_LDS s16x4*)(sdy + k * kPix + 16 * wid + 4 * p4));
        const bf16* xb = sx + (i * st * WP + j * st) * kPix + slab + 4 * p4;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
#pragma unroll
          for (int c = 0; c < NCI; ++c)
            vb[h2][tp][c] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (DBX_LDS s16x4*)(xb + ((tp / 3) * WP + tp % 3) * kPix + 16 * c));
      }
      const bf16x8 af = __builtin_bit_cast(bf16x8, __builtin_shufflevector(va[0], va[1], 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int c = 0; c < NCI; ++c) {
          const bf16x8 bfr = __builtin_bit_cast(
              bf16x8, __builtin_shufflevector(vb[0][tp][c], vb[1][tp][c], 0, 1, 2, 3, 4, 5, 6, 7));
          acc[tp][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[tp][c], 0, 0, 0);
        }
    }
  }
  // D[row = co][col = ci]: lane holds co = 4g + r, ci = li of block c; only the block diagonal is stored
  float* out = a.ws + (size_t)blockIdx.x * C * (9 * CPG);
#pragma unroll
  for (int c = 0; c < NCI; ++c) {
    const int ci = cb + slab + 16 * c + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = cb + 16 * wid + 4 * g + r;
      if (co / CPG != ci / CPG) continue;
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) out[(size_t)co * (9 * CPG) + tp * CPG + ci % CPG] = acc[tp][c][r];
    }
  }
}

}  // namespace dbx

using namespace dbx;

static bool gconv_shape_ok(int IC, int OC, int R, int S, int stride, int pad, int IH, int IW, int OH, int OW) {
  const bool cpg = IC == 4 || IC == 8 || IC == 16 || IC == 32 || IC == 64;
  return cpg && OC % 64 == 0 && IC < OC && R == 3 && S == 3 && pad == 1 && (stride == 1 || stride == 2) &&
         OH == (IH - 1) / stride + 1 && OW == (IW - 1) / stride + 1 && IH > 0 && IW > 0;
}
// output rows per tile: the tallest tile (a multiple of `sub`) whose staged rows fit the LDS budget, then the
// image's rows spread evenly over that many tiles; rows(th) = staged source rows, extra(th) = further pixels
template <typename FR, typename FE>
static int gconv_tile_rows(int H, int WP, int sub, FR rows, FE extra) {
  int th = sub;
  while (th + sub <= H + sub - 1 && (rows(th + sub) * WP + extra(th + sub)) * kPix * 2 <= kLdsMax && th + sub <= 16)
    th += sub;
  if ((rows(th) * WP + extra(th)) * kPix * 2 > kLdsMax) return -1;
  const int nt = (H + th - 1) / th;
  return ((H + nt - 1) / nt + sub - 1) / sub * sub;
}

template <int CPG>
static int launch_gconv(int mode, IGemmArgs& a, int stats, dim3 grid, unsigned lds, hipStream_t st) {
#define L(...) hipLaunchKernelGGL((gconv_kernel<CPG, __VA_ARGS__>), grid, dim3(256), lds, st, a)
  if (mode == 0) {
    if (stats) L(0, 1, true); else L(0, 1, false);
  } else if (a.stride == 1) {
    L(1, 1, false);
  } else {
    L(1, 2, false);
  }
#undef L
  return (int)hipGetLastError();
}

// mode 0: y [N][OH][OW][C] = conv(x [N][IH][IW][C]) (+ stats); mode 1: y = dx [N][IH][IW][C] from x = dy
// [N][OH][OW][C]. args->IC = channels per group, args->OC = C. Reached through dbx_conv_igemm (modes 5 / 6).
int dbx_group_conv(int mode, const IGemmArgs* args, int stats, hipStream_t st) {
  IGemmArgs a = *args;
  if (mode != 0 && mode != 1) return -90;
  if (!gconv_shape_ok(a.IC, a.OC, a.R, a.S, a.stride, a.pad, a.IH, a.IW, a.OH, a.OW)) return -91;
  if (!a.x || !a.w || !a.y || a.N <= 0 || (stats && (!a.stats || mode != 0 || a.nshard < 1))) return -92;
  const int s = a.stride, dg2 = mode == 1 && s == 2;
  const int H = mode == 0 ? a.OH : a.IH, WP = (mode == 0 ? a.IW : a.OW) + 2;
  const int th = gconv_tile_rows(
      H, WP, dg2 ? 2 : 1, [&](int t) { return mode == 0 ? (t - 1) * s + 3 : (dg2 ? t / 2 + 1 : t + 2); },
      [](int) { return 0; });
  if (th < 1) return -93;
  a.nr = th;
  a.ns = (H + th - 1) / th;
  const int nrow = mode == 0 ? (th - 1) * s + 3 : (dg2 ? th / 2 + 1 : th + 2);
  const unsigned lds = (unsigned)(nrow * WP * kPix * 2);
  const dim3 grid((unsigned)(a.N * a.ns), (unsigned)(a.OC / 64));
  switch (a.IC) {
    case 4: return launch_gconv<4>(mode, a, stats, grid, lds, st);
    case 8: return launch_gconv<8>(mode, a, stats, grid, lds, st);
    case 16: return launch_gconv<16>(mode, a, stats, grid, lds, st);
    case 32: return launch_gconv<32>(mode, a, stats, grid, lds, st);
    case 64: return launch_gconv<64>(mode, a, stats, grid, lds, st);
  }
  return -91;
}

// Weight gradient: one fp32 slab [C][9 * cpg] per tile range into args->ws; returns the slab count (the caller
// reduces them with dbx_wgrad_reduce), < 0 on error. max_wg > 0: at most that many workgroups. Reached through
// dbx_wgrad_patch3 (args->IC < args->OC).
int dbx_group_conv_wgrad(const WgradArgs* args, long long ws_cap, hipStream_t st, int max_wg) {
  WgradArgs a = *args;
  if (!gconv_shape_ok(a.IC, a.OC, a.R, a.S, a.stride, a.pad, a.IH, a.IW, a.OH, a.OW)) return -94;
  if (!a.x || !a.dy || !a.ws || a.N <= 0) return -95;
  const int s = a.stride, WP = a.IW + 2, OW = a.OW;
  const int th = gconv_tile_rows(
      a.OH, WP, 1, [&](int t) { return (t - 1) * s + 3; }, [&](int t) { return (t * OW + 31) / 32 * 32; });
  if (th < 1) return -96;
  static const int cus = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  const int T = a.N * ((a.OH + th - 1) / th), nblk = a.OC / 64;
  const long long slab = (long long)a.OC * 9 * a.IC;
  // two workgroups per CU over the channel blocks, within the workspace (slabs + the reduction's partials)
  int want = (max_wg > 0 ? max_wg : 2 * cus) / nblk;
  if (want < 1) want = 1;
  if (want > T) want = T;
  while (want > 1 && (want + (want < 64 ? want : 64)) * slab > ws_cap) --want;
  if ((want + (want < 64 ? want : 64)) * slab > ws_cap) return -97;
  a.m_per_split = (T + want - 1) / want;
  a.nsplit = (T + a.m_per_split - 1) / a.m_per_split;  // every range non-empty
  a.relu_in = th;
  a.KTOT = 9 * a.IC;
  const unsigned lds = (unsigned)((((th - 1) * s + 3) * WP + (th * OW + 31) / 32 * 32) * kPix * 2);
  const dim3 grid((unsigned)a.nsplit, (unsigned)nblk);
#define L(CPG) hipLaunchKernelGGL((gconv_wgrad_kernel<CPG>), grid, dim3(256), lds, st, a)
  switch (a.IC) {
    case 4: L(4); break;
    case 8: L(8); break;
    case 16: L(16); break;
    case 32: L(32); break;
    case 64: L(64); break;
    default: return -94;
  }
#undef L
  const int e = (int)hipGetLastError();
  return e ? -e : a.nsplit;
}
