// Internal (non-exported) functions of the mel-cepstral kernel families that one translation unit defines and another calls.  Every
// unit that defines or calls one of them sees THIS declaration (common.h includes the file), so a signature that changes on one
// side only is a compile error; default arguments are written here and nowhere else.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsa {

// ---- csrc/mcep_mfma.hip: tuned forward, float32, fft_length 512, cep_order 24 (kernels: mcep_mfma_f16.h)
struct StftIn;   // the waveform side of the fused launch (mcep_mfma_f16.h)
int mcep_mfma_supported(int nfft, int M, int dtype);
int64_t mcep_mfma_images_bytes();
int mcep_mfma_prepare(const void* G, const void* D, const void* E, void* images, hipStream_t st);
int mcep_mfma_fwd(const void* X, int64_t F, int n_iter, const void* G, const void* D, const void* E, const void* av,
                  const void* images, void* scratch, void* mc, void* hist, hipStream_t st, bool scratch_clean = false,
                  const StftIn* sti = nullptr, bool hist_has_rt = false, bool overlapped = false, int reserve_cus = 0,
                  bool fixed_steps = false, bool full_chains = false);
int stft_mcep_fused_fwd(const void* x, int64_t B, int64_t T, int P, int center, const void* window, const void* twiddle, double eps,
                        int n_iter, const void* G, const void* D, const void* E, const void* av, const void* images, void* scratch,
                        void* mc, void* hist, void* X_out, hipStream_t st, bool scratch_clean, bool hist_has_rt, bool overlapped, int pad_mode,
                        int zmean, float floor_lin, int reserve_cus, bool fixed_steps, bool full_chains);

// ---- csrc/mcep_mfma_bwd.hip: its backward (mcep_mfma_bwd_f16.h, mcep_mfma_bwd2_f16.h)
int mcep_mfma_bwd(const void* gmc, const void* X, const void* hist, int64_t F, int n_iter, const void* av,
                  const void* images, void* scratch, void* gX, hipStream_t st, bool has_workspace = false, bool hist_has_rt = false);
// the backward's half of mcep_mfma_prepare: launches mcep_hb_prep_kernel, the caller checks the launch
void mcep_mfma_bwd_prepare_launch(const void* G, const void* D, const void* E, void* images, hipStream_t st);

// ---- csrc/mgcep_step.hip: the whole Newton step of mgcep (gamma != 0, fft_length 512, cep_order 24, float32) in one launch (mgcep_step_f16.h)
int mgcep_step_solve_fwd(const void* x, const void* b1, int64_t F, double gamma, const void* images, void* b1_out, void* r_out, hipStream_t st,
                         void* pt_out = nullptr, void* qt_out = nullptr, int n_steps = 1, void* b1_prev_out = nullptr);
int mgcep_step_bwd_h(const void* x, const void* b1, const void* gpt, const void* gqt, const void* gr, int64_t F, double gamma,
                     const void* images, const void* gx_in, void* gx, void* gb1, hipStream_t st);
// the step's solve alone: 24 x 24 Toeplitz-plus-Hankel systems, float32, 16 per wave in the quad layout
int thsolve_quad24_fwd(const void* p, const void* q, const void* r, int64_t F, void* g, hipStream_t st, int r_stride = 24,
                       int r_off = 0, const void* add = nullptr);

// ---- csrc/mcep_resid.hip: the spectral half of a Newton step of the untuned mel-cepstral analysis on binary16-split chains
// (mcep_resid_f16.h), its adjoint (mcep_resid_bwd_f16.h) and the one-pass glogx (mcep_glogx_f16.h)
int64_t mcep_resid_h_images_bytes(int K, int M1);
int mcep_resid_h_prepare(const void* D, int ldd, const void* E, int lde, int K, int M1, void* images, hipStream_t st);
int mcep_resid_h_fwd(const void* logx, int64_t F, int K, const void* mc, int M1, const void* images, void* out, int ldo, hipStream_t st);
int64_t mcep_resid_bwd_images_bytes(int K, int M1);
int mcep_resid_bwd_prepare(const void* D, int ldd, const void* E, int lde, int K, int M1, void* images, hipStream_t st);
int mcep_glogx_h(const void* logx, int64_t F, int K, const void* mcs, int M1, const void* grts, int n_iter, const void* images, void* glogx,
                 hipStream_t st);
int mcep_resid_bwd_h(const void* logx, int64_t F, int K, const void* mc, int M1, const void* grt, const void* images, void* glogx, void* gmc,
                     hipStream_t st);

// ---- csrc/mcep_big.hip: all Newton steps of the 48 kHz set-ups in one persistent launch (mcep_big_f16.h, mcep_big4_f16.h)
int mcep_big_newton(const void* logx, int64_t F, int K, const void* mc_in, int M1, const void* images, const void* av, int n_iter,
                    void* mc_out, hipStream_t st);

// ---- csrc/thsolve_quad.hip: Toeplitz-plus-Hankel systems of orders 2 .. 55, float32, strided operands, in the quad / octet layout
int thsolve_quadn_fwd(const void* p, int ldp, const void* q, int ldq, const void* r, int ldr, const void* sub, const void* add, int64_t F,
                      int n, void* g, hipStream_t st);

}  // namespace dsa
