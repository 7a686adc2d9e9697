// Every host entry point of the extension, declared once. The .hip file that defines one, the files that call one
// (conv_igemm.hip, runtime/comm.cpp) and bindings.cpp, which derives the Python binding from the declaration, all
// include this header, so a definition or a call that disagrees with it does not compile. Pointers are device
// pointers unless noted; an entry returns 0, a hipError_t (> 0) or a negative code of its own.
#pragma once
#include <hip/hip_runtime.h>

#include "abi.h"

extern "C" {
// ---- convolutions (conv_igemm.hip; the struct-filling bindings of bindings.cpp) ---------------------------------
// pro / stats / accum / epi select the kernel instantiation; dma: the tile's operand path (ops/kernels.py _tile_dma)
int dbx_conv_igemm(int mode, int bm, int bn, const dbx::IGemmArgs* args, int pro, int stats, int accum, int epi,
                   hipStream_t st, int dma);
int dbx_conv_wgrad(int mode, int bm, int bn, const dbx::WgradArgs* args, int pro, hipStream_t st, unsigned lds_pad,
                   int dma_req);
// what dbx_conv_igemm forwards to: conv_patch3.hip, conv_fast.hip, conv_sweep.hip
int dbx_conv_patch3(int mode, const dbx::IGemmArgs* args, int pro, int stats, int epi, hipStream_t st, int streamed);
int dbx_stem_patch(const dbx::IGemmArgs* args, int stats, hipStream_t st);
int dbx_conv_fast(int mode, int bn, const dbx::IGemmArgs* args, int stats, int accum, int epi, hipStream_t st);
int dbx_conv_sweep(int mode, const dbx::IGemmArgs* args, int pro, int stats, int accum, int epi, hipStream_t st);
// these three return the number of fp32 weight-gradient slabs they wrote to args->ws (<= 0: failure)
int dbx_wgrad_patch3(const dbx::WgradArgs* args, long long ws_cap, hipStream_t st, int max_wg);      // conv_patch3.hip
int dbx_conv_dwfused(const dbx::DwFusedArgs* args, long long ws_cap, hipStream_t st, int max_cus);  // conv_dwfused.hip
int dbx_stem_bwd(dbx::StemBwdArgs* args, long long ws_cap, int fused, hipStream_t st);              // stem_bwd.hip
// split reductions of the weight-gradient slabs: dw = scale * sum of nsplit slabs (+ dw)
int dbx_wgrad_reduce(const float* ws, float* dw, long long n, int nsplit, float scale, int accumulate, hipStream_t st);
int dbx_wgrad_reduce_gather(const float* ws, float* dw, int OC, int R, int S, int IC, int nsplit, float scale,
                            int accumulate, hipStream_t st);
// several reductions in two launches: plan fills a HOST table (host arrays in, njobs * job_bytes out), run takes its
// device copy
int dbx_wgrad_reduce_multi_plan(const float* const* ws, float* const* dw, const long long* n, const int* nsplit,
                                const float* scale, const int* accumulate, int njobs, void* table, int* grid_a,
                                int* grid_b);
int dbx_wgrad_reduce_multi_run(const void* table_dev, int njobs, int grid_a, int grid_b, hipStream_t st);
int dbx_wgrad_reduce_job_bytes();

// ---- batch norm, pooling, loss, weight preparation (nn_ops.hip) -------------------------------------------------
int dbx_bn_finalize(const double* stats, int nshard, int C, float count, const float* gamma, const float* beta,
                    float eps, float momentum, float* rm, float* rv, float* scale, float* shift, float* save_mean,
                    float* save_invstd, hipStream_t st);
int dbx_bn_eval_coeff(int C, const float* gamma, const float* beta, float eps, const float* rm, const float* rv,
                      float* scale, float* shift, hipStream_t st);
int dbx_bn_eval_coeff_multi(const void* desc, int nbn, int max_c, hipStream_t st);  // desc: BnEvalDesc[nbn]
int dbx_channel_stats(const bf16* y, long long M, int C, double* stats, int nshard, hipStream_t st);
int dbx_bn_apply(const bf16* y, const float* sc, const float* sh, const bf16* res, const float* rsc, const float* rsh,
                 bf16* out, long long n, int C, int res_mode, int relu, unsigned char* mbits, hipStream_t st,
                 const dbx::BnFin* fin, const dbx::BnFin* rfin);
int dbx_bn_bwd_reduce(const bf16* dout, const bf16* mref, const bf16* y, const float* sc, const float* sh,
                      const float* mean, const float* invstd, long long M, int C, double* stats, int nshard,
                      int mask_mode, hipStream_t st);
int dbx_bn_bwd_coeff(const double* stats, int nshard, int C, float count, const float* gamma, const float* mean,
                     const float* invstd, float* coeff, float* dgamma, float* dbeta, int accumulate, hipStream_t st);
int dbx_bn_bwd_apply(const bf16* dout, const bf16* mref, const bf16* y, const float* sc, const float* sh,
                     const float* coeff, bf16* dy, bf16* gout, long long n, int C, int mask_mode, hipStream_t st,
                     const dbx::BnFin* fin);
int dbx_bn_bwd_apply2(const bf16* g, const bf16* y1, const float* c1, bf16* dy1, const bf16* y2, const float* c2,
                      bf16* dy2, long long n, int C, hipStream_t st, const dbx::BnFin* fin1, const dbx::BnFin* fin2);
int dbx_maxpool_fwd(const bf16* x, const float* sc, const float* sh, bf16* out, unsigned char* arg, bf16* ymax, int N,
                    int H, int W, int C, int P, int Q, int K, int stride, int pad, int relu, hipStream_t st,
                    const dbx::BnFin* fin);
int dbx_maxpool_bwd(const bf16* dout, const unsigned char* arg, bf16* dx, int N, int H, int W, int C, int P, int Q,
                    int K, int stride, int pad, hipStream_t st);
int dbx_pool_bn_bwd(const bf16* dpool, const unsigned char* arg, const bf16* y, const float* sc, const float* sh,
                    const float* c1, const float* c2, const float* c3, bf16* dy, double* stats, int nshard, int N,
                    int H, int W, int C, int P, int Q, int K, int stride, int pad, int apply, hipStream_t st);
int dbx_avgpool_fwd(const bf16* x, bf16* out, int N, int HW, int C, hipStream_t st);
int dbx_avgpool_bwd(const bf16* dout, bf16* dx, int N, int HW, int C, hipStream_t st);
// the training loss: kind 0 = softmax cross-entropy, 1 = binary cross-entropy on the logits (target_thresh >= 0
// binarises the targets, negative = none; sum_classes: the row loss is summed over the classes, not averaged)
int dbx_softmax_ce(const void* logits, int is_bf16, const long long* labels, void* dlogits, float* loss_out,
                   double* stats, int B, int C, float smoothing, float gscale, const long long* labels2,
                   const float* lam, hipStream_t st, int kind, float target_thresh, int sum_classes);
int dbx_ce_eval(const void* logits, int is_bf16, const long long* labels, double* stats, int B, int C, int k,
                const int* nvalid, float* loss_out, int* rank_out, hipStream_t st);
int dbx_weight_prep(const float* master, bf16* wbuf, const void* desc_dev, int nlayers, hipStream_t st);  // WDesc[]
int dbx_weight_prep16(const bf16* src, bf16* wbuf, const void* desc_dev, int nlayers, hipStream_t st);
int dbx_cast_f32_bf16(const float* x, bf16* y, long long n, hipStream_t st);

// ---- optimizers (optim_ops.hip) ---------------------------------------------------------------------------------
int dbx_sgd(float* p, const float* g, float* v, bf16* p16, long long n, const float* hyper, float lr, float mom,
            float damp, float wd, int nesterov, int first, const float* gscale_ptr, float gscale, float* ema,
            const float* omd_ptr, float omd, const int* tab, int nruns, long long run_base, hipStream_t st);
int dbx_adam(float* p, const float* g, float* m, float* v, bf16* p16, long long n, const float* hyper, float lr,
             float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2, const float* gscale_ptr,
             float gscale, float* ema, const float* omd_ptr, float omd, const int* tab, int nruns, long long run_base,
             hipStream_t st);
int dbx_ema_update(float* e, const float* p, long long n, const float* omd_ptr, float omd, hipStream_t st);
int dbx_ema_update_multi(const void* desc, int ntensors, long long max_len, const float* omd_ptr, float omd,
                         hipStream_t st, const float* gates);  // desc: EmaDesc[ntensors]
// stochastic depth: y = gates[row.gate] * x per row of desc (GateDesc[nrows]; gates: device fp32). Python reaches it
// through ema_update_multi's binding: non-null gates there forward here (desc a GateDesc table, omd unread)
int dbx_gate_scale_multi(const void* desc, int nrows, long long max_len, const float* gates, hipStream_t st);
int dbx_lars_scale(const float* p, float* g, const int* seg_off, const int* seg_len, const int* adapt, int nseg,
                   int max_len, double* norms, float gs, float eta, float wd, hipStream_t st);
int dbx_lamb(float* p, float* g, float* m, float* v, bf16* p16, const int* seg_off, const int* seg_len,
             const int* adapt, int nseg, int max_len, double* norms, const float* hyper, float lr, float b1, float b2,
             float eps, float wd, float bc1, float bc2, float trust_min, float trust_max, const float* gscale_ptr,
             float gscale, float* ema, const float* omd_ptr, float omd, hipStream_t st);
int dbx_grad_accum(float* dst, const float* src, long long n, int first, const float* flag, hipStream_t st);
int dbx_sumsq(const float* x, long long n, double* out, hipStream_t st);
int dbx_clip_factor(const double* sumsq, float max_norm, float* out, hipStream_t st);

// ---- input pipeline (input_ops.hip) -----------------------------------------------------------------------------
// augment_u8, augment_mix_u8 and crop_resize_u8 read a dense batch [N][Hin][Win][Cin], or -- with src_tab, an int32
// [N][4] table (offset / 16, H, W, stride) -- images of different sizes packed in the byte arena `in` of arena16
// 16-byte units (Hin / Win are then unread)
int dbx_normalize_u8(const unsigned char* in, bf16* out, const unsigned char* flip, int N, int H, int W, int Cin,
                     float m0, float m1, float m2, float s0, float s1, float s2, hipStream_t st);
int dbx_augment_u8(const unsigned char* in, bf16* out, const float* boxes, const unsigned char* flip, int N, int Hin,
                   int Win, int Cin, int Ho, int Wo, float m0, float m1, float m2, float s0, float s1, float s2,
                   const int* perm, const int* mixbox, hipStream_t st, const int* src_tab = nullptr,
                   long long arena16 = 0);
// the augment kernel with a MixUp blend and / or random erasing
int dbx_augment_mix_u8(const unsigned char* in, bf16* out, const float* boxes, const unsigned char* flip, int N,
                       int Hin, int Win, int Cin, int Ho, int Wo, float m0, float m1, float m2, float s0, float s1,
                       float s2, const int* perm, const int* mixbox, const float* blend, const int* erase, int pixel,
                       unsigned long long seed, const int* rng_offset, hipStream_t st, const int* src_tab = nullptr,
                       long long arena16 = 0);
// TrivialAugmentWide: source uint8 -> T (R, G, B, L) + histograms; LUTs and gray means; the mixing kernel on T
int dbx_crop_resize_u8(const unsigned char* in, unsigned char* T, int* hist, const float* boxes,
                       const unsigned char* flip, int N, int Hin, int Win, int Ho, int Wo, hipStream_t st,
                       const int* src_tab = nullptr, long long arena16 = 0);
int dbx_ta_prepare(const int* hist, const int* ops, unsigned char* lut, int* tmean, int N, hipStream_t st);
int dbx_ta_apply_u8(const unsigned char* T, bf16* out, const int* ops, const unsigned char* lut, const int* tmean,
                    int N, int Ho, int Wo, float m0, float m1, float m2, float s0, float s1, float s2, const int* perm,
                    const int* mixbox, const float* blend, const int* erase, int pixel, unsigned long long seed,
                    const int* rng_offset, hipStream_t st, unsigned char* T_out, int* hist_out);
// one operation of a chain: T_in -> T_out (R, G, B, L; not aliased) by ops, T_out's histograms added to hist. Python
// reaches it through ta_apply_u8's binding: a non-null T_out there forwards here (out and the mixing arguments unread)
int dbx_ta_stage_u8(const unsigned char* T_in, unsigned char* T_out, int* hist, const int* ops,
                    const unsigned char* lut, const int* tmean, int N, int Ho, int Wo, hipStream_t st);

// ---- classifier head (head_ops.hip) -----------------------------------------------------------------------------
int dbx_small_gemm(int ta, int tb, int out_f32, int drop, const dbx::GemmArgs* args, hipStream_t st);
int dbx_colsum(const bf16* X, float* out, int M, int N, int accumulate, hipStream_t st);
int dbx_dropout(const bf16* x, bf16* y, long long n, unsigned long long seed, unsigned offset, unsigned thresh,
                float inv_keep, const unsigned* offset_dev, hipStream_t st);

// ---- fused MNIST Net, one workgroup per image (mnist_ops.hip) -----------------------------------------------------
long long dbx_mnist_saved_bytes();
int dbx_mnist_fwd(const float* x, const float* params, void* saved, float* logp, int N, unsigned long long seed,
                  unsigned offset, int train, hipStream_t st);
int dbx_mnist_bwd(const float* x, const float* params, const void* saved, const float* dlogp, float* gws, float* grad,
                  int N, unsigned long long seed, unsigned offset, hipStream_t st);

// ---- direct all-reduce over peer-mapped buffers (direct_ar.hip; bound by runtime/comm.cpp) ------------------------
// bufs / flags / gens / errs: HOST arrays of one device pointer per rank
int dbx_dar_launch(float* const* bufs, unsigned* const* flags, unsigned* gen, int* err, int* err_host, long long n,
                   int rank, int world, int grid, double timeout_s, hipStream_t st);
int dbx_dar_alloc(int grid, void** flags, void** gen, void** err, void** err_host, void** err_host_dev);
int dbx_dar_free(void* flags, void* gen, void* err, void* err_host);
int dbx_dar_max_ranks();
int dbx_dar_launch_multi(float* const* bufs, unsigned* const* flags, unsigned* const* gens, int* const* errs,
                         long long n, int world, int grid, double timeout_s, hipStream_t st);
}

// conv_dgrad.hip: the data-gradient instantiations of the implicit-GEMM kernel (C++ linkage)
int dbx_dispatch_dgrad(int bm, int bn, const dbx::IGemmArgs& a, bool accum, int epi, int dma, hipStream_t st);
