// The optimizer kernels of the native step (gfx950): everything that runs over the flat fp32 master buffer
// and its flat gradient, shared by every trainer.
//
//   sgd_kernel / adam_kernel<EMA, GROUPS>   the element-wise updates (+ bf16 compute copy, weight EMA, groups)
//   lars_norms_kernel / lars_apply_kernel   LARS pre-scaling of the gradient, per parameter tensor
//   lamb_moments_kernel / lamb_apply_kernel<EMA>   LAMB, per parameter tensor
//   grad_accum_kernel, ema_kernel, sumsq_kernel, clip_factor_kernel
//   gate_scale_kernel                       stochastic depth's per-block scalar over a table of rows
//
// Every piece the kernels share -- the EMA arguments, the group table in LDS and the lookup in it, the
// four-lane EMA lerp, the bf16x4 store, the per-(segment, block) norm slots and their fixed-order sum -- is
// one __forceinline__ function below; each optimizer has one C entry point that picks the instantiation from
// its nullable arguments.
#include "common.h"
#include "entry.h"

namespace dbx {

// ----------------------------------------------------------------------------------------
// Fused optimizers over the flat fp32 master buffer (+ optional bf16 compute copy).
//   SGD (PyTorch semantics): d = g + wd*p; v = mom*v + (1-damp)*d (v = d at step 1);
//                            d = nesterov ? d + mom*v : v; p -= lr*d
//   Adam/AdamW: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr * mhat/(sqrt(vhat)+eps)
//   grad_scale multiplies g first (DDP averaging / loss scaling / clipping factor), read
//   from device memory so it can be produced by a previous kernel (global-norm clip).
//   Weight EMA (compile-time variant EMA = true): e = fmaf(omd, p_new - e, e) from the parameter about
//   to be stored; omd = fl32(1 - decay), rounded once on the host (never 1 - d in fp32 here), read
//   from omd_ptr (device fp32[1], nullable) when given so a captured step follows a decay schedule.
//   Every EMA site goes through ema_lerp: fused and standalone updates give the same bits.
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ float ema_lerp(float e, float p, float omd) { return fmaf(omd, p - e, e); }
// the four consecutive elements of the average at e + k (16-byte aligned) towards the parameters pp (base and
// index apart, here and in store_bf16x4: the address is formed at the access, where the kernels formed it
// before these were functions -- with e + k as the caller's argument sgd_kernel and ema_kernel schedule differently)
__device__ __forceinline__ void ema_lerp4(float* e, size_t k, const f32x4 pp, float omd) {
  f32x4 ee = *reinterpret_cast<const f32x4*>(e + k);
  ee = f32x4{ema_lerp(ee[0], pp[0], omd), ema_lerp(ee[1], pp[1], omd), ema_lerp(ee[2], pp[2], omd),
             ema_lerp(ee[3], pp[3], omd)};
  *reinterpret_cast<f32x4*>(e + k) = ee;
}
// the EMA variant's extra kernel arguments; empty for the plain instantiation (same code as without)
template <bool EMA> struct EmaArgs { float* e; const float* omd_ptr; float omd; };
template <> struct EmaArgs<false> {};
// what a kernel works with: the average's slice and omd (unused, and gone, in the plain instantiation)
struct Ema { float* e; float omd; };
template <bool EMA>
__device__ __forceinline__ Ema ema_unpack(const EmaArgs<EMA>& ea) {
  if constexpr (EMA) return Ema{ea.e, ea.omd_ptr ? ea.omd_ptr[0] : ea.omd};
  else return Ema{nullptr, 0.f};
}

// the bf16 compute copy of the four consecutive parameters pp at p16 + e (8-byte aligned)
__device__ __forceinline__ void store_bf16x4(bf16* p16, size_t e, const f32x4 pp) {
  const bf16x4 b = {(bf16)pp[0], (bf16)pp[1], (bf16)pp[2], (bf16)pp[3]};
  *reinterpret_cast<bf16x4*>(p16 + e) = b;
}

// Parameter groups (compile-time variant GROUPS = true): weight decay and an LR multiplier per RUN of the
// flat buffer. tab (device int32, ops/kernels.py pack_opt_runs) = start[nruns + 1] | wd[nruns] | lr_mult[nruns]
// (the last two fp32 bits): run r covers flat indices [start[r], start[r + 1]), start[0] = 0, strictly
// increasing multiples of 4, so a 16-byte vector at a flat index that is a multiple of 4 lies in ONE run.
// run_base = the flat index of p[0] (a multiple of 4): a slice of the master uses the whole buffer's table.
// Every block copies start / wd / lr_mult into LDS once (12 KiB at the limit) and a lane finds its vector's
// run by a binary search there (neighbouring lanes read the same words: broadcasts); the per-element math is
// the plain kernel's with wd -> wd[r] and lr -> lr * lr_mult[r]. No HBM traffic per element is added. The host
// validates the table; the run index is clamped all the same: a bad table gives wrong numbers, never a
// read outside the LDS arrays.
constexpr int kOptMaxRuns = 1024;  // ops/kernels.py OPT_MAX_RUNS
template <bool GROUPS> struct GroupArgs { const int* tab; int nruns; int run_base; };
template <> struct GroupArgs<false> {};
struct OptRunsLds { int start[kOptMaxRuns]; float wd[kOptMaxRuns]; float lm[kOptMaxRuns]; };
// the staged table as a kernel's loops see it (empty in the plain instantiation)
template <bool GROUPS> struct OptRuns { const OptRunsLds* s; int nruns; int run_base; };
template <> struct OptRuns<false> {};

// stage the table into the block's LDS copy s (every thread of the block calls this: it holds a barrier)
__device__ __forceinline__ OptRuns<true> opt_runs_load(OptRunsLds& s, const GroupArgs<true>& ga) {
  const int* __restrict__ tab = ga.tab;
  const int nruns = ga.nruns < 1 ? 1 : (ga.nruns > kOptMaxRuns ? kOptMaxRuns : ga.nruns);
  for (int r = threadIdx.x; r < nruns; r += blockDim.x) {
    s.start[r] = tab[r];
    s.wd[r] = __int_as_float(tab[nruns + 1 + r]);
    s.lm[r] = __int_as_float(tab[2 * nruns + 1 + r]);
  }
  __syncthreads();
  return OptRuns<true>{&s, nruns, ga.run_base};
}
// the run of flat index idx: the largest r in [0, nruns) with start[r] <= idx (0 when there is none)
__device__ __forceinline__ int opt_run_of(const OptRunsLds& s, int nruns, int idx) {
  int lo = 0;
  for (int len = nruns; len > 1;) {  // (len is wave-uniform; lo + half < lo + len <= nruns)
    const int half = len >> 1;
    if (s.start[lo + half] <= idx) lo += half;
    len -= half;
  }
  return lo < 0 ? 0 : (lo >= nruns ? nruns - 1 : lo);
}
// wd, lr: the launch's scalars on entry; with GROUPS, on return those of the run that holds element k of the
// launch's slice (wd[r], lr * lr_mult[r])
template <bool GROUPS>
__device__ __forceinline__ void opt_run_wd_lr(const OptRuns<GROUPS>& runs, long long k, float& wd, float& lr) {
  if constexpr (GROUPS) {
    const int r = opt_run_of(*runs.s, runs.nruns, runs.run_base + (int)k);
    wd = runs.s->wd[r];
    lr = lr * runs.s->lm[r];
  }
}

template <bool EMA, bool GROUPS>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v,
                           bf16* __restrict__ p16, long long n, const float* __restrict__ hyper, float lr, float mom,
                           float damp, float wd, int nesterov, int first, const float* __restrict__ gscale_ptr,
                           float gscale, EmaArgs<EMA> ea, GroupArgs<GROUPS> ga) {
  // hyper (device, nullable): [lr] so a captured graph follows the LR schedule on replay
  if (hyper) lr = hyper[0];
  [[maybe_unused]] OptRuns<GROUPS> runs;
  if constexpr (GROUPS) {
    __shared__ OptRunsLds s_runs;
    runs = opt_runs_load(s_runs, ga);
  }
  [[maybe_unused]] const Ema ema = ema_unpack(ea);
  const float gs = gscale_ptr ? gscale * gscale_ptr[0] : gscale;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i * 4 < n; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 4;
    if (e + 4 <= n) {
      float wd_r = wd, lr_r = lr;  // this vector's run (GROUPS); the launch's scalars otherwise
      opt_run_wd_lr(runs, e, wd_r, lr_r);
      f32x4 pp = *reinterpret_cast<f32x4*>(p + e);
      f32x4 gg = *reinterpret_cast<const f32x4*>(g + e) * gs;
      gg += wd_r * pp;
      f32x4 d = gg;
      if (mom != 0.f) {
        f32x4 vv = first ? gg : (*reinterpret_cast<f32x4*>(v + e) * mom + (1.f - damp) * gg);
        *reinterpret_cast<f32x4*>(v + e) = vv;
        d = nesterov ? gg + mom * vv : vv;
      }
      pp -= lr_r * d;
      *reinterpret_cast<f32x4*>(p + e) = pp;
      if (p16) store_bf16x4(p16, e, pp);
      if constexpr (EMA) ema_lerp4(ema.e, e, pp, ema.omd);
    } else {
      for (long long k = e; k < n; ++k) {
        float wd_r = wd, lr_r = lr;  // (the tail resolves its run per element)
        opt_run_wd_lr(runs, k, wd_r, lr_r);
        float gg = g[k] * gs + wd_r * p[k];
        float d = gg;
        if (mom != 0.f) {
          const float vv = first ? gg : v[k] * mom + (1.f - damp) * gg;
          v[k] = vv;
          d = nesterov ? gg + mom * vv : vv;
        }
        p[k] -= lr_r * d;
        if (p16) p16[k] = (bf16)p[k];
        if constexpr (EMA) ema.e[k] = ema_lerp(ema.e[k], p[k], ema.omd);
      }
    }
  }
}

template <bool EMA, bool GROUPS>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, bf16* __restrict__ p16, long long n, const float* __restrict__ hyper,
                            float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2,
                            const float* __restrict__ gscale_ptr, float gscale, EmaArgs<EMA> ea,
                            GroupArgs<GROUPS> ga) {
  // hyper (device, nullable): [lr, 1-b1^t, 1-b2^t] so graph replays track the step count
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2 = hyper[2]; }
  [[maybe_unused]] OptRuns<GROUPS> runs;
  if constexpr (GROUPS) {
    __shared__ OptRunsLds s_runs;
    runs = opt_runs_load(s_runs, ga);
  }
  [[maybe_unused]] const Ema ema = ema_unpack(ea);
  const float gs = gscale_ptr ? gscale * gscale_ptr[0] : gscale;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
    float wd_r = wd, lr_r = lr;  // this element's run (GROUPS); the launch's scalars otherwise
    opt_run_wd_lr(runs, k, wd_r, lr_r);
    float gg = g[k] * gs;
    float pp = p[k];
    if (decoupled) pp -= lr_r * wd_r * pp;
    else gg += wd_r * pp;
    const float mm = b1 * m[k] + (1.f - b1) * gg;
    const float vv = b2 * v[k] + (1.f - b2) * gg * gg;
    m[k] = mm; v[k] = vv;
    pp -= lr_r * (mm / bc1) / (sqrtf(vv / bc2) + eps);
    p[k] = pp;
    if (p16) p16[k] = (bf16)pp;
    if constexpr (EMA) ema.e[k] = ema_lerp(ema.e[k], pp, ema.omd);
  }
}

// ----------------------------------------------------------------------------------------
// Per-segment norms of LARS and LAMB. grid = (chunks, nseg): blockIdx.y is the segment ("segment" = one
// parameter tensor), blocks stride over it. The first kernel of either reduces two fp32 lane sums per
// segment (wave shuffles, one LDS step over the 4 waves) into one fp64 pair per (segment, block) slot of
// ``norms`` ([nseg][kLarsMaxBlocks][2], every block writes its own) -- no atomics; the second, on the same
// grid, sums a segment's gridDim.x slots in block order (every block the same fixed order), so the trust
// ratios are bit-reproducible whatever order the blocks ran in.
// ----------------------------------------------------------------------------------------
constexpr int kLarsMaxBlocks = 64;  // blocks per segment (dbx_lars_scale / dbx_lamb clamp to this)
// a, b: every lane's wave sums. Every thread of the block calls this (it holds a barrier).
__device__ __forceinline__ void seg_norms_store(double* norms, int s, float a, float b) {
  __shared__ float red[2][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = norms + 2 * ((size_t)s * kLarsMaxBlocks + blockIdx.x);
    o[0] = (double)(red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    o[1] = (double)(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}
struct SegNorms { double a, b; };
__device__ __forceinline__ SegNorms seg_norms_sum(const double* norms, int s) {
  double a = 0.0, b = 0.0;
  const double* o = norms + 2 * (size_t)s * kLarsMaxBlocks;
  for (int k = 0; k < (int)gridDim.x; ++k) { a += o[2 * k]; b += o[2 * k + 1]; }
  return SegNorms{a, b};
}

// ----------------------------------------------------------------------------------------
// LARS (layer-wise adaptive rate scaling, large-batch SGD): per parameter tensor ("segment")
//   trust = eta * |w| / (|g| + wd * |w|)      (1 when either norm is 0)
//   g    <- adapt ? trust * (gs * g + wd * w) : gs * g
// followed by the plain SGD kernel with wd = 0. Phase 1 reduces |w|^2 and |gs*g|^2 per segment into the
// (segment, block) slots; phase 2 sums them in block order, then rescales in place.
// ----------------------------------------------------------------------------------------
__global__ void lars_norms_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                  const int* __restrict__ seg_off, const int* __restrict__ seg_len, float gs,
                                  double* __restrict__ norms) {
  const int s = blockIdx.y;
  const int off = seg_off[s], len = seg_len[s];
  float ww = 0.f, gg = 0.f;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) {
    const float w = p[off + i], d = g[off + i] * gs;
    ww += w * w;
    gg += d * d;
  }
  // (the two sums interleaved by hand: wave_sum twice, as in lamb_moments_kernel, is the same arithmetic but
  // another instruction schedule than this kernel has always had)
  for (int o = 32; o > 0; o >>= 1) {
    ww += __shfl_xor(ww, o, 64);
    gg += __shfl_xor(gg, o, 64);
  }
  seg_norms_store(norms, s, ww, gg);
}

__global__ void lars_apply_kernel(const float* __restrict__ p, float* __restrict__ g, const int* __restrict__ seg_off,
                                  const int* __restrict__ seg_len, const int* __restrict__ adapt,
                                  const double* __restrict__ norms, float gs, float eta, float wd) {
  const int s = blockIdx.y;
  const int off = seg_off[s], len = seg_len[s];
  float scale = gs, decay = 0.f;
  if (adapt[s]) {
    const SegNorms sq = seg_norms_sum(norms, s);
    const float wn = (float)sqrt(sq.a), gn = (float)sqrt(sq.b);
    const float trust = (wn > 0.f && gn > 0.f) ? eta * wn / (gn + wd * wn) : 1.f;
    scale = trust * gs;
    decay = trust * wd;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x)
    g[off + i] = scale * g[off + i] + decay * p[off + i];
}

// ----------------------------------------------------------------------------------------
// LAMB (layer-wise adaptive moments, the Adam-family large-batch optimizer): per parameter tensor
// ("segment" s, the LARS table), w the fp32 master, g the reduced flat gradient,
// gs = gscale * (gscale_ptr ? *gscale_ptr : 1), lr / bc1 / bc2 from hyper[0..2] when given:
//   gg = gs*g;  m = b1*m + (1-b1)*gg;  v = b2*v + (1-b2)*gg*gg
//   r  = (m/bc1) / (sqrt(v/bc2) + eps)
//   u  = adapt[s] ? r + wd*w : r                     (decay only where adapted)
//   t  = adapt[s] && |w|>0 && |u|>0 ? |w|/|u| : 1    (L2 norms over the tensor)
//   t  = clamp(t, trust_min, trust_max)              (only where adapted; a bound of 0 is no bound)
//   w -= lr * t * u
// Bias correction is always on. Two launches on the grid (blocks, nseg) of LARS, the same blocks for
// both: lamb_moments_kernel updates m and v, leaves u IN PLACE OVER g (the gradient is dead
// afterwards, as under LARS) and reduces |w|^2 and |u|^2 per block into the (segment, block) slots;
// lamb_apply_kernel sums a segment's slots in block order, forms t and updates w (+ the optional
// bf16 copy, + the weight EMA from the parameter it stores in the EMA variant). 16 B per lane: every
// segment offset is a multiple of 4 elements from 16-byte aligned bases (the wrapper checks); the
// len % 4 tail is scalar.
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ float lamb_u(float w, float gg, float& m, float& v, float b1, float b2, float eps, float wd,
                                        float bc1, float bc2) {
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  return (m / bc1) / (sqrtf(v / bc2) + eps) + wd * w;
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(
    const float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    const int* __restrict__ seg_off, const int* __restrict__ seg_len, const int* __restrict__ adapt,
    const float* __restrict__ hyper, float b1, float b2, float eps, float wd, float bc1, float bc2,
    const float* __restrict__ gscale_ptr, float gscale, double* __restrict__ norms) {
  if (hyper) { bc1 = hyper[1]; bc2 = hyper[2]; }
  const int s = blockIdx.y;
  const int off = seg_off[s], len = seg_len[s];
  if (!adapt[s]) wd = 0.f;  // (u = r + 0*w = r)
  const float gs = gscale_ptr ? gscale * gscale_ptr[0] : gscale;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  const int n4 = len / 4;
  float ww = 0.f, uu = 0.f;
  for (int i = tid; i < n4; i += nth) {
    const size_t e = (size_t)off + 4 * (size_t)i;
    const f32x4 pp = *reinterpret_cast<const f32x4*>(p + e);
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e) * gs;
    f32x4 mm = *reinterpret_cast<const f32x4*>(m + e);
    f32x4 vv = *reinterpret_cast<const f32x4*>(v + e);
    f32x4 u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = mm[j], vj = vv[j];
      u[j] = lamb_u(pp[j], gg[j], mj, vj, b1, b2, eps, wd, bc1, bc2);
      mm[j] = mj; vv[j] = vj;
      ww += pp[j] * pp[j];
      uu += u[j] * u[j];
    }
    *reinterpret_cast<f32x4*>(m + e) = mm;
    *reinterpret_cast<f32x4*>(v + e) = vv;
    *reinterpret_cast<f32x4*>(g + e) = u;
  }
  for (int k = n4 * 4 + tid; k < len; k += nth) {
    const size_t e = (size_t)off + k;
    const float w = p[e];
    float mj = m[e], vj = v[e];
    const float u = lamb_u(w, g[e] * gs, mj, vj, b1, b2, eps, wd, bc1, bc2);
    m[e] = mj; v[e] = vj; g[e] = u;
    ww += w * w;
    uu += u * u;
  }
  seg_norms_store(norms, s, wave_sum(ww), wave_sum(uu));
}

template <bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(
    float* __restrict__ p, const float* __restrict__ u, bf16* __restrict__ p16, const int* __restrict__ seg_off,
    const int* __restrict__ seg_len, const int* __restrict__ adapt, const double* __restrict__ norms,
    const float* __restrict__ hyper, float lr, float trust_min, float trust_max, EmaArgs<EMA> ea) {
  if (hyper) lr = hyper[0];
  [[maybe_unused]] const Ema ema = ema_unpack(ea);
  const int s = blockIdx.y;
  const int off = seg_off[s], len = seg_len[s];
  float t = 1.f;
  if (adapt[s]) {
    const SegNorms sq = seg_norms_sum(norms, s);
    const float wn = (float)sqrt(sq.a), un = (float)sqrt(sq.b);
    if (wn > 0.f && un > 0.f) t = wn / un;
    if (trust_min > 0.f) t = fmaxf(t, trust_min);
    if (trust_max > 0.f) t = fminf(t, trust_max);
  }
  const float step = lr * t;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  const int n4 = len / 4;
  for (int i = tid; i < n4; i += nth) {
    const size_t e = (size_t)off + 4 * (size_t)i;
    f32x4 pp = *reinterpret_cast<f32x4*>(p + e);
    pp -= step * *reinterpret_cast<const f32x4*>(u + e);
    *reinterpret_cast<f32x4*>(p + e) = pp;
    if (p16) store_bf16x4(p16, e, pp);
    if constexpr (EMA) ema_lerp4(ema.e, e, pp, ema.omd);
  }
  for (int k = n4 * 4 + tid; k < len; k += nth) {
    const size_t e = (size_t)off + k;
    const float pp = p[e] - step * u[e];
    p[e] = pp;
    if (p16) p16[e] = (bf16)pp;
    if constexpr (EMA) ema.e[e] = ema_lerp(ema.e[e], pp, ema.omd);
  }
}

// Gradient accumulation over the flat fp32 gradient: dst = first ? src : dst + src. ``flag`` (device,
// nullable) overrides ``first`` at run time (first = flag[0] != 0), so one captured micro-step serves
// every position of an accumulation window; in first mode dst is never read (stale NaN / Inf in the
// accumulator cannot leak, and no memset is needed). 16 B per lane when both pointers are 16-byte
// aligned; scalar otherwise (any 4-byte aligned slice is valid) and for the n % 4 tail.
__global__ void grad_accum_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n, int first,
                                  const float* __restrict__ flag) {
  if (flag) first = flag[0] != 0.f;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nth = (long long)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  for (long long i = tid; i < n4; i += nth) {
    f32x4 s = *reinterpret_cast<const f32x4*>(src + i * 4);
    if (!first) s = *reinterpret_cast<const f32x4*>(dst + i * 4) + s;
    *reinterpret_cast<f32x4*>(dst + i * 4) = s;
  }
  for (long long k = n4 * 4 + tid; k < n; k += nth) dst[k] = first ? src[k] : dst[k] + src[k];
}

// Standalone weight EMA, e = ema_lerp(e, p, omd), for what no optimizer kernel touches. One kernel,
// two launch shapes: desc == nullptr -- the flat slices (e, p, n), grid (blocks); desc != nullptr -- a
// device table of {dst address, src address, length} entries, grid (blocks, ntensors) with blockIdx.y
// the entry (the BatchNorm running statistics: separate module buffers, one launch for all of them).
// Alignment policy of grad_accum_kernel, per entry: 16 B per lane when both pointers are 16-byte
// aligned, scalar otherwise and for the n % 4 tail.
struct EmaDesc { long long dst, src, len; };
static_assert(sizeof(EmaDesc) == 24 && offsetof(EmaDesc, len) == 16, "EmaDesc layout (ops/kernels.py pack_ema_desc)");
__global__ void ema_kernel(const EmaDesc* __restrict__ desc, float* __restrict__ e, const float* __restrict__ p,
                           long long n, const float* __restrict__ omd_ptr, float omd) {
  if (desc) {
    const EmaDesc d = desc[blockIdx.y];
    e = reinterpret_cast<float*>(d.dst);
    p = reinterpret_cast<const float*>(d.src);
    n = d.len;
  }
  if (omd_ptr) omd = omd_ptr[0];
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nth = (long long)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  for (long long i = tid; i < n4; i += nth) ema_lerp4(e, i * 4, *reinterpret_cast<const f32x4*>(p + i * 4), omd);
  for (long long k = n4 * 4 + tid; k < n; k += nth) e[k] = ema_lerp(e[k], p[k], omd);
}

// Stochastic depth's per-block scalar: y[i] = gates[row.gate] * x[i] for every row of a device table of
// {dst address, src address, length, gate index} entries, grid (blocks, rows) as ema_kernel's table shape.
// The gates are fp32 in device memory, so a replayed graph follows the values the host copied in. dst == src
// is allowed (an element is read and written by one lane); partly overlapping rows are not. One fp32 multiply
// per element, in the vector and the scalar loop alike (a product by itself has nothing to contract with).
// Alignment policy of ema_kernel, per row. The host validates the gate index (ops/kernels.py pack_gate_desc).
struct GateDesc { long long dst, src, len, gate; };
static_assert(sizeof(GateDesc) == 32 && offsetof(GateDesc, gate) == 24, "GateDesc layout (ops/kernels.py pack_gate_desc)");
__global__ void gate_scale_kernel(const GateDesc* __restrict__ desc, const float* __restrict__ gates) {
  const GateDesc d = desc[blockIdx.y];
  float* y = reinterpret_cast<float*>(d.dst);
  const float* x = reinterpret_cast<const float*>(d.src);
  const long long n = d.len;
  const float m = gates[d.gate];
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long nth = (long long)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  for (long long i = tid; i < n4; i += nth) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
    *reinterpret_cast<f32x4*>(y + i * 4) = f32x4{m * v[0], m * v[1], m * v[2], m * v[3]};
  }
  for (long long k = n4 * 4 + tid; k < n; k += nth) y[k] = m * x[k];
}

// sum of squares over a flat fp32 buffer (global-norm clipping), one fp64 atomic per block. fp64
// sums of fp32 block partials are exact (hence independent of block order) while the partials'
// magnitudes span less than ~2^29; beyond that the last bits of the norm can depend on the order.
__global__ void sumsq_kernel(const float* __restrict__ x, long long n, double* out) {
  float s = 0.f;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) s += x[k] * x[k];
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, (double)(red[0] + red[1] + red[2] + red[3]));
}

// clip factor = min(1, max_norm / (sqrt(sumsq) + 1e-6)) written to out[0]
__global__ void clip_factor_kernel(const double* sumsq, float max_norm, float* out) {
  const float nrm = (float)sqrt(sumsq[0]);
  out[0] = fminf(1.f, max_norm / (nrm + 1e-6f));
  out[1] = nrm;
}

}  // namespace dbx

// ======================================================================================
// C ABI launchers
// ======================================================================================
using namespace dbx;

// SGD / Adam launches: <EMA, GROUPS> in all four combinations, deduced from the argument structs (the plain
// ones are what they were). The grouped kernels keep the plain grid (up to 8192 blocks): capped at the 2048
// blocks resident at once, so that each stages its table once for four times the trips, they ran 15-30 %
// slower (profiles/param_groups/).
template <bool EMA, bool GROUPS>
static int sgd_launch(float* p, const float* g, float* v, bf16* p16, long long n, const float* hyper, float lr,
                      float mom, float damp, float wd, int nesterov, int first, const float* gscale_ptr, float gscale,
                      EmaArgs<EMA> ea, GroupArgs<GROUPS> ga, hipStream_t st) {
  hipLaunchKernelGGL((sgd_kernel<EMA, GROUPS>), dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, p, g, v, p16, n, hyper,
                     lr, mom, damp, wd, nesterov, first, gscale_ptr, gscale, ea, ga);
  RET_LAST;
}
template <bool EMA, bool GROUPS>
static int adam_launch(float* p, const float* g, float* m, float* v, bf16* p16, long long n, const float* hyper,
                       float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2,
                       const float* gscale_ptr, float gscale, EmaArgs<EMA> ea, GroupArgs<GROUPS> ga, hipStream_t st) {
  hipLaunchKernelGGL((adam_kernel<EMA, GROUPS>), dim3(grid_for(n)), dim3(256), 0, st, p, g, m, v, p16, n, hyper, lr, b1,
                     b2, eps, wd, decoupled, bc1, bc2, gscale_ptr, gscale, ea, ga);
  RET_LAST;
}
// the run table's launch-side checks (its contents are validated by the Python wrapper, once per table);
// a table carries the decays, so the launch's scalar must stay 0
static bool opt_runs_ok(const int* tab, int nruns, long long run_base, long long n, float wd) {
  return tab && nruns >= 1 && nruns <= kOptMaxRuns && run_base >= 0 && run_base % 4 == 0 &&
         run_base + n <= 0x7fffffffLL && wd == 0.f;
}
// call launch(ea, ga) with the argument structs of the variant the nullable extras select: ema (+ omd_ptr /
// omd) the weight average, tab (+ nruns / run_base) the parameter groups (see EmaArgs, GroupArgs)
template <typename F>
static int opt_variant(float* ema, const float* omd_ptr, float omd, const int* tab, int nruns, long long run_base,
                       F launch) {
  const EmaArgs<true> ea{ema, omd_ptr, omd};
  const GroupArgs<true> ga{tab, nruns, (int)run_base};
  if (tab) return ema ? launch(ea, ga) : launch(EmaArgs<false>{}, ga);
  return ema ? launch(ea, GroupArgs<false>{}) : launch(EmaArgs<false>{}, GroupArgs<false>{});
}
extern "C" int dbx_sgd(float* p, const float* g, float* v, bf16* p16, long long n, const float* hyper, float lr,
                       float mom, float damp, float wd, int nesterov, int first, const float* gscale_ptr, float gscale,
                       float* ema, const float* omd_ptr, float omd, const int* tab, int nruns, long long run_base,
                       hipStream_t st) {
  if (tab && !opt_runs_ok(tab, nruns, run_base, n, wd)) return -1;
  return opt_variant(ema, omd_ptr, omd, tab, nruns, run_base, [&](auto ea, auto ga) {
    return sgd_launch(p, g, v, p16, n, hyper, lr, mom, damp, wd, nesterov, first, gscale_ptr, gscale, ea, ga, st);
  });
}
extern "C" int dbx_adam(float* p, const float* g, float* m, float* v, bf16* p16, long long n, const float* hyper,
                        float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2,
                        const float* gscale_ptr, float gscale, float* ema, const float* omd_ptr, float omd,
                        const int* tab, int nruns, long long run_base, hipStream_t st) {
  if (tab && !opt_runs_ok(tab, nruns, run_base, n, wd)) return -1;
  return opt_variant(ema, omd_ptr, omd, tab, nruns, run_base, [&](auto ea, auto ga) {
    return adam_launch(p, g, m, v, p16, n, hyper, lr, b1, b2, eps, wd, decoupled, bc1, bc2, gscale_ptr, gscale, ea,
                       ga, st);
  });
}
extern "C" int dbx_ema_update(float* e, const float* p, long long n, const float* omd_ptr, float omd,
                              hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, (const EmaDesc*)nullptr, e, p, n,
                     omd_ptr, omd);
  RET_LAST;
}
extern "C" int dbx_ema_update_multi(const void* desc, int ntensors, long long max_len, const float* omd_ptr, float omd,
                                    hipStream_t st, const float* gates) {
  if (gates) return dbx_gate_scale_multi(desc, ntensors, max_len, gates, st);
  if (ntensors <= 0 || max_len <= 0) return 0;
  if (!desc || ntensors > 65535) return -1;
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for((max_len + 3) / 4, 256, 64), ntensors), dim3(256), 0, st,
                     (const EmaDesc*)desc, (float*)nullptr, (const float*)nullptr, 0LL, omd_ptr, omd);
  RET_LAST;
}
extern "C" int dbx_gate_scale_multi(const void* desc, int nrows, long long max_len, const float* gates,
                                    hipStream_t st) {
  if (nrows <= 0 || max_len <= 0) return 0;
  if (!desc || !gates || nrows > 65535) return -1;
  hipLaunchKernelGGL(gate_scale_kernel, dim3(grid_for((max_len + 3) / 4, 256, 64), nrows), dim3(256), 0, st,
                     (const GateDesc*)desc, gates);
  RET_LAST;
}
// blocks per segment of the LARS / LAMB grids (the slots the second kernel reads are the ones the first wrote)
static inline int seg_blocks(int max_len) {
  const int bx = (int)((max_len + 255) / 256);
  return bx < 1 ? 1 : (bx > kLarsMaxBlocks ? kLarsMaxBlocks : bx);
}
extern "C" int dbx_lars_scale(const float* p, float* g, const int* seg_off, const int* seg_len, const int* adapt,
                              int nseg, int max_len, double* norms, float gs, float eta, float wd, hipStream_t st) {
  if (nseg <= 0) return 0;
  const int bx = seg_blocks(max_len);
  hipLaunchKernelGGL(lars_norms_kernel, dim3(bx, nseg), dim3(256), 0, st, p, g, seg_off, seg_len, gs, norms);
  hipLaunchKernelGGL(lars_apply_kernel, dim3(bx, nseg), dim3(256), 0, st, p, g, seg_off, seg_len, adapt, norms, gs,
                     eta, wd);
  RET_LAST;
}
// LAMB: both kernels on one grid
extern "C" int dbx_lamb(float* p, float* g, float* m, float* v, bf16* p16, const int* seg_off, const int* seg_len,
                        const int* adapt, int nseg, int max_len, double* norms, const float* hyper, float lr, float b1,
                        float b2, float eps, float wd, float bc1, float bc2, float trust_min, float trust_max,
                        const float* gscale_ptr, float gscale, float* ema, const float* omd_ptr, float omd,
                        hipStream_t st) {
  if (nseg <= 0) return 0;
  if (nseg > 65535 || !seg_off || !seg_len || !adapt || !norms) return -1;
  const dim3 grid(seg_blocks(max_len), nseg);
  hipLaunchKernelGGL(lamb_moments_kernel, grid, dim3(256), 0, st, p, g, m, v, seg_off, seg_len, adapt, hyper, b1, b2,
                     eps, wd, bc1, bc2, gscale_ptr, gscale, norms);
  if (ema)
    hipLaunchKernelGGL(lamb_apply_kernel<true>, grid, dim3(256), 0, st, p, g, p16, seg_off, seg_len, adapt, norms,
                       hyper, lr, trust_min, trust_max, EmaArgs<true>{ema, omd_ptr, omd});
  else
    hipLaunchKernelGGL(lamb_apply_kernel<false>, grid, dim3(256), 0, st, p, g, p16, seg_off, seg_len, adapt, norms,
                       hyper, lr, trust_min, trust_max, EmaArgs<false>{});
  RET_LAST;
}
extern "C" int dbx_grad_accum(float* dst, const float* src, long long n, int first, const float* flag,
                              hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(grad_accum_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, dst, src, n, first, flag);
  RET_LAST;
}
extern "C" int dbx_sumsq(const float* x, long long n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, st, x, n, out);
  RET_LAST;
}
extern "C" int dbx_clip_factor(const double* sumsq, float max_norm, float* out, hipStream_t st) {
  hipLaunchKernelGGL(clip_factor_kernel, dim3(1), dim3(1), 0, st, sumsq, max_norm, out);
  RET_LAST;
}
