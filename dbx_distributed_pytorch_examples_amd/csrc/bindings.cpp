// pybind11 bindings for the HIP kernels: a thin C ABI (raw device pointers + hipStream_t as
// integers). Deliberately independent of the libtorch C++ API so the extension builds in seconds
// with hipcc and never mixes ABIs with the bundled torch; the Python side (ops/kernels.py) checks
// dtype/shape/contiguity and passes tensor.data_ptr() + the current torch stream.
// The entry points are declared once, in entry.h. DBX_BIND derives a binding from that declaration;
// the entries that fill an argument struct (abi.h) are written out below with named arguments.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <stdint.h>

#include <stdexcept>
#include <string>

#include "entry.h"

namespace py = pybind11;
using namespace pybind11::literals;

static void check(int rc, const char* what) {
  if (rc != 0) {
    std::string msg = std::string("dbx kernel launch failed: ") + what + " rc=" + std::to_string(rc);
    if (rc > 0) msg += std::string(" (") + hipGetErrorString((hipError_t)rc) + ")";
    throw std::runtime_error(msg);
  }
}
// the entries that return their number of weight-gradient slabs
static int slabs(int n, const char* what) {
  if (n <= 0) check(n ? n : -1, what);
  return n;
}

// Bind<&dbx_f>::def(m, "f"): Python's f takes dbx_f's parameters in order -- a pointer of any kind (hipStream_t
// included) as an integer, everything else as it is -- and raises through check() unless dbx_f returns 0.
template <typename T> struct PyArg { using type = T; static T cast(T v) { return v; } };
template <typename T> struct PyArg<T*> {
  using type = uintptr_t;
  static T* cast(uintptr_t v) { return reinterpret_cast<T*>(v); }
};
template <auto F> struct Bind;
template <typename... A, int (*F)(A...)> struct Bind<F> {
  static void def(py::module& m, const char* name) {
    m.def(name, [name](typename PyArg<A>::type... a) { check(F(PyArg<A>::cast(a)...), name); });
  }
};
#define DBX_BIND(name) Bind<&dbx_##name>::def(m, #name)

// a struct's pointer field from the integer Python passed
template <typename T> static void ptr(T*& field, uintptr_t v) { field = reinterpret_cast<T*>(v); }
static hipStream_t stream(uintptr_t v) { return reinterpret_cast<hipStream_t>(v); }

void register_runtime(py::module& m);  // csrc/runtime/mds_loader.cpp
void register_comm(py::module& m);     // csrc/runtime/comm.cpp

PYBIND11_MODULE(_C, m) {
  register_runtime(m);
  register_comm(m);
  m.doc() = "dbx_distributed_pytorch_examples_amd native HIP kernels (gfx950)";

  // ---- entries that fill an argument struct: every argument named after the field it fills ----------------------
  m.def("conv_igemm", [](int mode, int bm, int bn, uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t in_scale,
                         uintptr_t in_shift, int relu_in, uintptr_t stats, int nshard, int N, int IH, int IW, int IC,
                         int OH, int OW, int OC, int R, int S, int stride, int pad, int accum, int nr, int ns, int r0,
                         int s0, int tstep, int dh0, int dw0, int osub, int oph, int opw, int FH, int FW,
                         uintptr_t addsrc, int add_sub, int epi, uintptr_t mbits, uintptr_t ybn, uintptr_t ybn2,
                         uintptr_t bsc, uintptr_t bsh, uintptr_t mean1, uintptr_t inv1, uintptr_t mean2,
                         uintptr_t inv2, uintptr_t bstats1, uintptr_t bstats2, uintptr_t a_out, uintptr_t res,
                         uintptr_t res_scale, uintptr_t res_shift, uintptr_t tail_out, uintptr_t tail_bits,
                         uintptr_t st, int dma, uintptr_t fin1, uintptr_t fin2, int fin_base, int fin_final,
                         uintptr_t fin_in, int ksplit, int kper, uintptr_t skws, uintptr_t skcnt) {
    dbx::IGemmArgs a{};
    ptr(a.x, x); ptr(a.w, w); ptr(a.y, y); ptr(a.in_scale, in_scale); ptr(a.in_shift, in_shift); ptr(a.stats, stats);
    a.N = N; a.IH = IH; a.IW = IW; a.IC = IC; a.OH = OH; a.OW = OW; a.OC = OC; a.R = R; a.S = S;
    a.stride = stride; a.pad = pad; a.M = N * OH * OW; a.nshard = nshard > 0 ? nshard : 1; a.relu_in = relu_in;
    a.nr = nr; a.ns = ns; a.r0 = r0; a.s0 = s0; a.tstep = tstep;
    a.dh0 = dh0; a.dw0 = dw0; a.osub = osub; a.oph = oph; a.opw = opw; a.FH = FH; a.FW = FW;
    ptr(a.addsrc, addsrc); a.add_sub = add_sub;
    ptr(a.mbits, mbits); ptr(a.ybn, ybn); ptr(a.ybn2, ybn2); ptr(a.bsc, bsc); ptr(a.bsh, bsh);
    ptr(a.mean1, mean1); ptr(a.inv1, inv1); ptr(a.mean2, mean2); ptr(a.inv2, inv2);
    ptr(a.bstats1, bstats1); ptr(a.bstats2, bstats2); ptr(a.a_out, a_out);
    ptr(a.res, res); ptr(a.res_scale, res_scale); ptr(a.res_shift, res_shift);
    ptr(a.tail_out, tail_out); ptr(a.tail_bits, tail_bits);
    ptr(a.fin1, fin1); ptr(a.fin2, fin2); a.fin_base = fin_base; a.fin_final = fin_final; ptr(a.fin_in, fin_in);
    ptr(a.skws, skws); ptr(a.skcnt, skcnt); a.ksplit = ksplit > 1 ? ksplit : 1; a.kper = kper;
    if (fin_in && !in_scale) throw std::invalid_argument("conv_igemm: input finalize without a BN prologue");
    if ((fin1 || fin2) && !(stats || bstats1)) throw std::invalid_argument("conv_igemm: BN finalize without statistics");
    if (fin2 && !bstats2) throw std::invalid_argument("conv_igemm: second BN finalize without its statistics");
    {  // magic divisors when exact: m < N*OH*OW, so m * OH*OW < 2^40 suffices
      const unsigned long long two40 = 1ull << 40, ohw = (unsigned long long)OH * OW;
      if (ohw > 0 && (unsigned long long)N * ohw * ohw < two40) {
        a.mag_ohw = (two40 + ohw - 1) / ohw;
        a.mag_ow = (two40 + OW - 1) / OW;
      }
    }
    check(dbx_conv_igemm(mode, bm, bn, &a, in_scale != 0, stats != 0, accum, epi, stream(st), dma), "conv_igemm");
  }, "mode"_a, "bm"_a, "bn"_a, "x"_a, "w"_a, "y"_a, "in_scale"_a = 0, "in_shift"_a = 0, "relu_in"_a = 0,
     "stats"_a = 0, "nshard"_a, "N"_a, "IH"_a, "IW"_a, "IC"_a, "OH"_a, "OW"_a, "OC"_a, "R"_a, "S"_a, "stride"_a,
     "pad"_a, "accum"_a = 0, "nr"_a, "ns"_a, "r0"_a, "s0"_a, "tstep"_a = 1, "dh0"_a = 0, "dw0"_a = 0, "osub"_a = 1,
     "oph"_a = 0, "opw"_a = 0, "FH"_a, "FW"_a, "addsrc"_a = 0, "add_sub"_a = 1, "epi"_a = 0, "mbits"_a = 0,
     "ybn"_a = 0, "ybn2"_a = 0, "bsc"_a = 0, "bsh"_a = 0, "mean1"_a = 0, "inv1"_a = 0, "mean2"_a = 0, "inv2"_a = 0,
     "bstats1"_a = 0, "bstats2"_a = 0, "a_out"_a = 0, "res"_a = 0, "res_scale"_a = 0, "res_shift"_a = 0,
     "tail_out"_a = 0, "tail_bits"_a = 0, "st"_a, "dma"_a, "fin1"_a = 0, "fin2"_a = 0, "fin_base"_a = 0,
     "fin_final"_a = 1, "fin_in"_a = 0, "ksplit"_a = 1, "kper"_a = 0, "skws"_a = 0, "skcnt"_a = 0);
  m.def("conv_wgrad", [](int mode, int bm, int bn, uintptr_t dy, uintptr_t x, uintptr_t ws, uintptr_t in_scale,
                         uintptr_t in_shift, int relu_in, int N, int IH, int IW, int IC, int OH, int OW, int OC, int R,
                         int S, int stride, int pad, int KTOT, int nsplit, int m_per_split, uintptr_t st,
                         unsigned lds_pad, int dma, uintptr_t dw, uintptr_t cnt, float scale, int accumulate) {
    const unsigned long long two40 = 1ull << 40;
    const unsigned long long ohw = (unsigned long long)OH * OW;
    if ((unsigned long long)N * ohw * ohw >= two40) throw std::runtime_error("conv_wgrad: batch too large for mdiv");
    dbx::WgradArgs a{};
    ptr(a.dy, dy); ptr(a.x, x); ptr(a.ws, ws); ptr(a.in_scale, in_scale); ptr(a.in_shift, in_shift);
    a.N = N; a.IH = IH; a.IW = IW; a.IC = IC; a.OH = OH; a.OW = OW; a.OC = OC; a.R = R; a.S = S;
    a.stride = stride; a.pad = pad; a.M = N * OH * OW; a.KTOT = KTOT; a.nsplit = nsplit;
    a.m_per_split = m_per_split; a.relu_in = relu_in;
    a.mag_ow = (two40 + OW - 1) / OW; a.mag_ohw = (two40 + ohw - 1) / ohw;
    ptr(a.dw, dw); ptr(a.cnt, cnt); a.scale = scale; a.accumulate = accumulate;
    if (dw && nsplit > 1 && !cnt) throw std::invalid_argument("conv_wgrad: fused split-K reduction needs tile counters");
    check(dbx_conv_wgrad(mode, bm, bn, &a, in_scale != 0, stream(st), lds_pad, dma), "conv_wgrad");
  }, "mode"_a, "bm"_a, "bn"_a, "dy"_a, "x"_a, "ws"_a, "in_scale"_a, "in_shift"_a, "relu_in"_a, "N"_a,
     "IH"_a, "IW"_a, "IC"_a, "OH"_a, "OW"_a, "OC"_a, "R"_a, "S"_a, "stride"_a, "pad"_a, "KTOT"_a, "nsplit"_a,
     "m_per_split"_a, "st"_a, "lds_pad"_a, "dma"_a, "dw"_a = 0, "cnt"_a = 0, "scale"_a, "accumulate"_a);
  m.def("wgrad_patch3", [](uintptr_t dy, uintptr_t x, uintptr_t ws, long long ws_cap, int N, int IH, int IW, int IC,
                           int OH, int OW, int OC, int R, int S, int stride, int pad, uintptr_t st, int max_wg) {
    // 3x3 patch weight gradient (conv_patch3.hip): one fp32 slab per workgroup; returns the count
    dbx::WgradArgs a{};
    ptr(a.dy, dy); ptr(a.x, x); ptr(a.ws, ws);
    a.N = N; a.IH = IH; a.IW = IW; a.IC = IC; a.OH = OH; a.OW = OW; a.OC = OC; a.R = R; a.S = S;
    a.stride = stride; a.pad = pad; a.M = N * OH * OW; a.KTOT = R * S * IC;
    return slabs(dbx_wgrad_patch3(&a, ws_cap, stream(st), max_wg), "wgrad_patch3");
  }, "dy"_a, "x"_a, "ws"_a, "ws_cap"_a, "N"_a, "IH"_a, "IW"_a, "IC"_a, "OH"_a, "OW"_a, "OC"_a, "R"_a, "S"_a,
     "stride"_a, "pad"_a, "st"_a, "max_wg"_a = 0);
  m.def("conv_dwfused", [](uintptr_t g, uintptr_t y3, uintptr_t coeff, uintptr_t wt, uintptr_t y2, uintptr_t bsc,
                           uintptr_t bsh, uintptr_t mean2, uintptr_t inv2, uintptr_t da, uintptr_t bstats, uintptr_t ws,
                           long long ws_cap, int M, int K, int C, int nshard, uintptr_t st, int max_cus) {
    // fused bottleneck-conv3 backward (conv_dwfused.hip): returns the number of dW partial slabs
    dbx::DwFusedArgs a{};
    ptr(a.g, g); ptr(a.y3, y3); ptr(a.coeff, coeff); ptr(a.wt, wt); ptr(a.y2, y2); ptr(a.bsc, bsc); ptr(a.bsh, bsh);
    ptr(a.mean2, mean2); ptr(a.inv2, inv2); ptr(a.da, da); ptr(a.bstats, bstats); ptr(a.ws, ws);
    a.M = M; a.K = K; a.C = C; a.nshard = nshard > 0 ? nshard : 1;
    return slabs(dbx_conv_dwfused(&a, ws_cap, stream(st), max_cus), "conv_dwfused");
  }, "g"_a, "y3"_a, "coeff"_a, "wt"_a, "y2"_a, "bsc"_a, "bsh"_a, "mean2"_a, "inv2"_a, "da"_a, "bstats"_a, "ws"_a,
     "ws_cap"_a, "M"_a, "K"_a, "C"_a, "nshard"_a, "st"_a, "max_cus"_a);
  m.def("stem_bwd", [](uintptr_t dpool, uintptr_t arg, uintptr_t y, uintptr_t sc, uintptr_t sh, uintptr_t coeff,
                       uintptr_t x4, uintptr_t ws, long long ws_cap, int N, int H, int W, int C, int P, int Q, int PK,
                       int pstride, int ppad, int IH, int IW, int R, int S, int stride, int pad, int fused,
                       uintptr_t st) {
    // stem backward / stem weight gradient (stem_bwd.hip): returns the number of dW partial slabs
    const unsigned long long two40 = 1ull << 40, hw = (unsigned long long)H * W;
    if ((unsigned long long)N * hw * hw >= two40) throw std::runtime_error("stem_bwd: batch too large for mdiv");
    dbx::StemBwdArgs a{};
    ptr(a.dpool, dpool); ptr(a.arg, arg); ptr(a.y, y); ptr(a.sc, sc); ptr(a.sh, sh); ptr(a.coeff, coeff);
    ptr(a.x4, x4); ptr(a.ws, ws);
    a.N = N; a.H = H; a.W = W; a.C = C; a.P = P; a.Q = Q; a.PK = PK; a.pstride = pstride; a.ppad = ppad;
    a.IH = IH; a.IW = IW; a.R = R; a.S = S; a.stride = stride; a.pad = pad; a.M = N * H * W;
    a.mag_hw = (two40 + hw - 1) / hw; a.mag_w = (two40 + W - 1) / W;
    return slabs(dbx_stem_bwd(&a, ws_cap, fused, stream(st)), "stem_bwd");
  }, "dpool"_a = 0, "arg"_a = 0, "y"_a, "sc"_a = 0, "sh"_a = 0, "coeff"_a = 0, "x4"_a, "ws"_a, "ws_cap"_a, "N"_a,
     "H"_a, "W"_a, "C"_a, "P"_a, "Q"_a, "PK"_a, "pstride"_a, "ppad"_a, "IH"_a, "IW"_a, "R"_a, "S"_a, "stride"_a, "pad"_a,
     "fused"_a = 0, "st"_a);
  m.def("small_gemm", [](int ta, int tb, int out_f32, int drop, uintptr_t A, uintptr_t B, uintptr_t C, uintptr_t bias_f,
                         uintptr_t bias_h, int M, int N, int K, int lda, int ldb, int ldc, float alpha, int accumulate,
                         unsigned long long seed, unsigned offset, unsigned thresh, float inv_keep, uintptr_t offset_dev,
                         uintptr_t st, uintptr_t ws, int splitk) {
    // classifier-head GEMM (head_ops.hip); splitk > 1: K split over workgroups, partials in ws
    dbx::GemmArgs g{};
    ptr(g.A, A); ptr(g.B, B); ptr(g.C, C); ptr(g.bias_f, bias_f); ptr(g.bias_h, bias_h);
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.alpha = alpha; g.accumulate = accumulate;
    g.seed = seed; g.offset = offset; g.thresh = thresh; g.inv_keep = inv_keep; ptr(g.offset_dev, offset_dev);
    ptr(g.ws, ws); g.splitk = splitk;
    check(dbx_small_gemm(ta, tb, out_f32, drop, &g, stream(st)), "small_gemm");
  }, "ta"_a, "tb"_a, "out_f32"_a, "drop"_a, "A"_a, "B"_a, "C"_a, "bias_f"_a, "bias_h"_a, "M"_a, "N"_a, "K"_a, "lda"_a,
     "ldb"_a, "ldc"_a, "alpha"_a, "accumulate"_a, "seed"_a, "offset"_a, "thresh"_a, "inv_keep"_a, "offset_dev"_a,
     "st"_a, "ws"_a = 0, "splitk"_a = 1);

  // ---- entries that return a value or take lists ------------------------------------------------------------
  m.def("wgrad_reduce_multi_plan", [](std::vector<uintptr_t> ws, std::vector<uintptr_t> dw, std::vector<long long> n,
                                       std::vector<int> nsplit, std::vector<float> scale, std::vector<int> acc,
                                       uintptr_t table) {
    const size_t nj = ws.size();
    if (dw.size() != nj || n.size() != nj || nsplit.size() != nj || scale.size() != nj || acc.size() != nj)
      throw std::invalid_argument("wgrad_reduce_multi_plan: job lists of different lengths");
    std::vector<const float*> w(nj);
    std::vector<float*> d(nj);
    for (size_t q = 0; q < nj; ++q) { ptr(w[q], ws[q]); ptr(d[q], dw[q]); }
    int ga = 0, gb = 0;
    check(dbx_wgrad_reduce_multi_plan(w.data(), d.data(), n.data(), nsplit.data(), scale.data(), acc.data(), (int)nj,
                                      reinterpret_cast<void*>(table), &ga, &gb),
          "wgrad_reduce_multi_plan");
    return std::make_pair(ga, gb);
  });
  m.def("wgrad_reduce_job_bytes", []() { return dbx_wgrad_reduce_job_bytes(); });
  m.def("mnist_saved_bytes", []() { return dbx_mnist_saved_bytes(); });

  // ---- everything else: the declaration's parameters, in its order ------------------------------------------
  DBX_BIND(wgrad_reduce_multi_run);
  DBX_BIND(wgrad_reduce_gather);
  DBX_BIND(wgrad_reduce);
  DBX_BIND(bn_finalize);
  DBX_BIND(bn_eval_coeff);
  DBX_BIND(bn_eval_coeff_multi);
  DBX_BIND(ce_eval);
  DBX_BIND(channel_stats);
  DBX_BIND(bn_apply);
  DBX_BIND(bn_bwd_reduce);
  DBX_BIND(bn_bwd_coeff);
  DBX_BIND(bn_bwd_apply);
  DBX_BIND(bn_bwd_apply2);
  DBX_BIND(maxpool_fwd);
  DBX_BIND(maxpool_bwd);
  DBX_BIND(pool_bn_bwd);
  DBX_BIND(avgpool_fwd);
  DBX_BIND(avgpool_bwd);
  DBX_BIND(softmax_ce);
  DBX_BIND(weight_prep);
  DBX_BIND(weight_prep16);
  DBX_BIND(cast_f32_bf16);
  DBX_BIND(sgd);
  DBX_BIND(adam);
  DBX_BIND(lars_scale);
  DBX_BIND(lamb);
  DBX_BIND(ema_update);
  DBX_BIND(ema_update_multi);
  DBX_BIND(grad_accum);
  DBX_BIND(sumsq);
  DBX_BIND(clip_factor);
  DBX_BIND(normalize_u8);
  DBX_BIND(augment_u8);
  DBX_BIND(augment_mix_u8);
  DBX_BIND(crop_resize_u8);
  DBX_BIND(ta_prepare);
  DBX_BIND(ta_apply_u8);  // (with T_out: dbx_ta_stage_u8 -- the module exports the names it exported)
  DBX_BIND(mnist_fwd);
  DBX_BIND(mnist_bwd);
  DBX_BIND(colsum);
  DBX_BIND(dropout);
  m.attr("arch") = "gfx950";
}
