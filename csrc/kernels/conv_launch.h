// Host entry points of the conv-VAE kernels, declared once: included by the
// .hip file that defines each launcher and by the bindings that call it
// (csrc/runtime/conv_ops.cpp), so a parameter list changed on one side only is
// a compile error (the names have C linkage: the linker would not see it).
// Host-clean: g++ and hipcc include it. Every launcher returns 0 or an error
// code; `st` / `hp` are a TrainState / HParams device buffer (vae_mlp.h).
// An op whose first parameter is a JobBlob* has ONE builder for both forms: null launches its
// stand-alone kernel, non-null records the same arguments as a job of a fused launch (conv_jobs.hip).
#pragma once
#include "conv_igemm.h"
#include "vae_mlp.h"

extern "C" {

// conv_plan.hip: the planners (1: unsupported geometry)
int mdt_igemm_plan(int mode, mdt::ConvDesc d, int allow_split, int fwd, mdt::FwdPlan* q);
int mdt_wgrad_plan(mdt::ConvDesc d, mdt::WgradPlan* q);

// conv_igemm.hip: implicit-GEMM convolutions and weight gradients
int mdt_igemm(mdt::JobBlob* g, mdt::JobBlob* c, int mode, const void* A, int a_is_f32, const void* B16,
              mdt::ConvDesc d, const float* bias, int relu, void* y16, float* y32, const void* omask, float* colsum,
              float* ws, int skip_combine, hipStream_t s, const mdt::APro* pro, int fwd);
int mdt_wgrad(mdt::JobBlob* j, const void* G16, const void* X, int x_is_f32, mdt::ConvDesc d, float* out,
              hipStream_t s);
int mdt_job_wgrad_adam(mdt::JobBlob* j, const void* G16, const void* X, int x_is_f32, mdt::ConvDesc d, float* P,
                       float* Mo, float* Vo, void* w16, const float* adamc);
void mdt_dconv_stamps(unsigned long long* p);
int mdt_colsum(mdt::JobBlob* j, const void* G16, int M, int N, int rows_per, float* slab, hipStream_t s);

// conv_thin.hip: the single-channel edge layers
int mdt_thin_conv(mdt::JobBlob* j, const void* X, int x_is_f32, const float* Wf, mdt::ConvDesc d, const float* bias,
                  int relu, void* y16, const void* omask, float* colsum, const int* idx, void* st, const void* hp,
                  int B, float* xb, hipStream_t s);
int mdt_thin_blocks(int tconv, mdt::ConvDesc d);
int mdt_thin_tconv(const void* G16, const float* Wf, mdt::ConvDesc d, const float* bias, float* y32, const float* X,
                   void* dlog16, float* recon, float* part, float* gpart, hipStream_t s);

// conv_bf16.hip: the step's small kernels
int mdt_reparam(const float* mulv, float* eps, void* z16, float* z32, int B, int Z, const void* st, const void* hp,
                unsigned stream, float* kld_part, hipStream_t s);
int mdt_reparam_bwd(const float* dz, const float* mulv, const float* eps, float* dmulv, void* dmulv16, int B, int Z,
                    const float* klw, const float* fbw, hipStream_t s);
int mdt_gather_rows(const float* X, const int* idx, const void* st, int B, int M, int P, float* xb, hipStream_t s);
int mdt_bce_logits(const float* logits, const float* X, const int* rows, int B, int P, void* dlog16, float* recon,
                   float* part, float* gpart, hipStream_t s);
int mdt_conv_loss_finalize(mdt::JobBlob* j, const float* bce_part, int nb, const float* kld_part, int nk, void* st,
                           const void* hp, int advance_cursor, hipStream_t s);
int mdt_step_begin(void* st, const void* hp, hipStream_t s);
int mdt_adam_cast(float* P, const float* G, float* Mo, float* Vo, void* w16, const void* segs, int nseg,
                  long long total, const void* st, const void* hp, int do_adam, hipStream_t s);
int mdt_grad_finalize(mdt::JobBlob* j, float* P, float* G, float* Mo, float* Vo, void* w16, const void* segs,
                      const void* units, int nunits, const void* st, const void* hp, int do_adam, const float* gX,
                      const int* gidx, float* xn, unsigned* xtag, int gB, hipStream_t s);
int mdt_job_comm(mdt::JobBlob* j, float* P, float* G, float* Mo, float* Vo, void* w16, const void* segs,
                 const void* units, int nunits, const void* st, const void* hp, int do_adam, const void* ctx, int mode);
int mdt_wtrans(mdt::JobBlob* j, const void* w16, void* w16t, const void* segs, const void* units, int nunits,
               hipStream_t s);
int mdt_combine_reparam(const float* slab, int ks, const float* bias, float* mulv, float* eps, void* z16, float* z32,
                        int B, int Z, const void* st, const void* hp, unsigned stream, float* kld_part, hipStream_t s);
int mdt_combine_reparam_bwd(const float* slab, int ks, const float* mulv, const float* eps, float* dmulv,
                            void* dmulv16, float* dz, int B, int Z, const float* klw, const float* fbw,
                            hipStream_t s);
int mdt_combine_reparam_blocks(int ks, int B, int Z);

// conv_jobs.hip: the horizontally fused launches over recorded jobs
int mdt_launch_jobs(const mdt::JobBlob* jobs, int n, hipStream_t s);
int mdt_launch_job1(const mdt::JobBlob* j, hipStream_t s);
int mdt_jobs_multi_bytes();
int mdt_pack_jobs_multi(const mdt::JobBlob* jobs, int n, void* dst);
int mdt_pack_jobs_multi_stamps(void* img, void* stamps);
int mdt_launch_jobs_multi(const void* dev_pack, int grid, hipStream_t s);

// conv28_fused.hip: the fused 28x28 step. p / pf, pb, pp: the forward, backward and pair tables of
// conv28_slots.h as device addresses, validated by the caller
int mdt_f28_forward(const long long* p, int B, int M, unsigned stream, int train, hipStream_t s);
int mdt_f28_forward_pair(const long long* p, const long long* pp, int B, int M, unsigned stream, hipStream_t s);
int mdt_f28_backward(const long long* p, int M, const void* st, hipStream_t s);
int mdt_f28_step(const long long* pf, const long long* pb, const long long* pp, int B, int M, unsigned stream,
                 int pair, int delay_us, float* adamc, hipStream_t s);
int mdt_f28_pair_words();

}  // extern "C"
