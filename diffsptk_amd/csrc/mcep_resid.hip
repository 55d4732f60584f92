// The mel-cepstral analysis at the geometries the tuned tile kernels do not cover (the 48 kHz set-ups: fft_length 1024 / 2048,
// orders 32 .. 54), one launch per piece of a Newton step: its spectral half rt = exp(logx - 2 mc D) E (mcep_resid_f16.h), that half's
// adjoint (mcep_resid_bwd_f16.h) and glogx summed over the steps in one pass (mcep_glogx_f16.h).  This unit: the kernels, the
// operand-image preparation and the launches (callers: rows_gemm.hip).  The one-launch iteration on the same images: mcep_big.hip.
#include "mcep_glogx_f16.h"
#include "mcep_resid_bwd_f16.h"
#include "mcep_resid_f16.h"

namespace dsa {

int64_t mcep_resid_h_images_bytes(int K, int M1)
{
    const int ks1 = (M1 + 31) / 32, nt = (2 * M1 - 1 + 15) / 16;
    return (int64_t)((K + 31) / 32) * mrh::stage_halves(ks1, nt) * 2;
}

int mcep_resid_h_prepare(const void* D, int ldd, const void* E, int lde, int K, int M1, void* images, hipStream_t st)
{
    const int ks1 = (M1 + 31) / 32, nt = (2 * M1 - 1 + 15) / 16;
    const long pairs = (long)((K + 31) / 32) * mrh::stage_halves(ks1, nt) / 2;
    hipLaunchKernelGGL(mcep_resid_h_prep_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, (const float*)D, ldd, (const float*)E, lde,
                       K, M1, 2 * M1 - 1, ks1, nt, (_Float16*)images);
    return check_launch("mcep_resid_prepare");
}

int mcep_resid_h_fwd(const void* logx, int64_t F, int K, const void* mc, int M1, const void* images, void* out, int ldo, hipStream_t st)
{
    const int ks1 = (M1 + 31) / 32, nt = (2 * M1 - 1 + 15) / 16, N = 2 * M1 - 1;
    const dim3 grid((unsigned)((F + 63) / 64));
#define DSA_RESID_H(KS, NTV)                                                                                                           \
    hipLaunchKernelGGL((mcep_resid_h_kernel<KS, NTV>), grid, dim3(256), 0, st, (const float*)logx, (long)F, K, (const float*)mc, M1, \
                       (const _Float16*)images, N, (float*)out, ldo)
    if (ks1 == 1) {
        switch (nt) {
            case 1: DSA_RESID_H(1, 1); break;
            case 2: DSA_RESID_H(1, 2); break;
            case 3: DSA_RESID_H(1, 3); break;
            default: DSA_RESID_H(1, 4); break;
        }
    } else {
        switch (nt) {
            case 5: DSA_RESID_H(2, 5); break;
            case 6: DSA_RESID_H(2, 6); break;
            default: DSA_RESID_H(2, 7); break;
        }
    }
#undef DSA_RESID_H
    return check_launch("mcep_resid_h");
}

int64_t mcep_resid_bwd_images_bytes(int K, int M1)
{
    const int ks1 = (M1 + 31) / 32;
    return (int64_t)((K + 31) / 32) * mrb::stage_halves_b(ks1, mrb::kse_of(M1), mrb::nt3_of(M1)) * 2;
}

int mcep_resid_bwd_prepare(const void* D, int ldd, const void* E, int lde, int K, int M1, void* images, hipStream_t st)
{
    const int ks1 = (M1 + 31) / 32, kse = mrb::kse_of(M1), nt3 = mrb::nt3_of(M1);
    const long pairs = (long)((K + 31) / 32) * mrb::stage_halves_b(ks1, kse, nt3) / 2;
    hipLaunchKernelGGL(mcep_resid_bwd_prep_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, (const float*)D, ldd, (const float*)E,
                       lde, K, M1, 2 * M1 - 1, ks1, kse, nt3, (_Float16*)images);
    return check_launch("mcep_resid_bwd_prepare");
}

// orders 32 .. 54 (M1 33 .. 55: two k-steps of coefficients); DSA_ERR_UNSUPPORTED otherwise -- the caller keeps the composed gradient
int mcep_resid_bwd_h(const void* logx, int64_t F, int K, const void* mc, int M1, const void* grt, const void* images, void* glogx, void* gmc,
                     hipStream_t st)
{
    const int ks1 = (M1 + 31) / 32, kse = mrb::kse_of(M1), nt3 = mrb::nt3_of(M1), N = 2 * M1 - 1;
    if (!(ks1 == 2 && M1 >= 33 && M1 <= 55 && K >= 4)) return DSA_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((F + 63) / 64));
    auto launch = [&](auto kse_, auto with_glogx) {   // (the kernel's NT3 is its KSE at every order served; without glogx: a null pointer)
        constexpr int KSEV = decltype(kse_)::value;
        constexpr int lds_b = 2 * mrb::stage_halves_b(2, KSEV, KSEV) * 2;
        return launch_lds<mcep_resid_bwd_h_kernel<2, KSEV, KSEV, decltype(with_glogx)::value>>(
            lds_b, "mcep_resid_bwd_h: cannot reserve LDS%s", grid, dim3(256), lds_b, st, (const float*)logx, (long)F, K, (const float*)mc, M1,
            (const float*)grt, N, (const _Float16*)images, (float*)glogx, (float*)gmc);
    };
    auto by_glogx = [&](auto kse_) { return glogx ? launch(kse_, std::true_type{}) : launch(kse_, std::false_type{}); };
    (void)nt3;
    // M1 33 .. 48: N = 2 M1 - 1 <= 95 columns of rt, three tiles of coefficients; M1 49 .. 55: four
    if (int rc = kse == 3 ? by_glogx(int_c<3>{}) : by_glogx(int_c<4>{})) return rc;
    return check_launch("mcep_resid_bwd_h");
}

// glogx = sum over the steps of (grt_s E^T) * exp(logx - 2 mc_s D): mcs (n_iter, F, M1) the iterates the steps started from, grts
// (n_iter, F, 2 M1 - 1) the cotangents dsa_mcep_newton_update_bwd produced for them; `images` of mcep_resid_bwd_prepare.
// DSA_ERR_UNSUPPORTED (no error text): orders outside 32 .. 54 or more steps than one workgroup's LDS holds -- the caller keeps the
// in-place accumulation of dsa_mcep_newton_resid_h_bwd.
int mcep_glogx_h(const void* logx, int64_t F, int K, const void* mcs, int M1, const void* grts, int n_iter, const void* images, void* glogx,
                 hipStream_t st)
{
    const int ks1 = (M1 + 31) / 32, kse = mrb::kse_of(M1), N = 2 * M1 - 1;
    if (!(ks1 == 2 && M1 >= 33 && M1 <= 55 && K >= 4 && n_iter >= 1)) return DSA_ERR_UNSUPPORTED;
    if ((long)n_iter * mgx::step_bytes(2, kse) > mgx::kMaxLds) return DSA_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((F + 15) / 16));
    const int lds_b = n_iter * mgx::step_bytes(2, kse);
    auto launch = [&](auto kse_) {
        constexpr int KSEV = decltype(kse_)::value;
        return launch_lds<mcep_glogx_h_kernel<2, KSEV, KSEV>>(mgx::kMaxLds, "mcep_glogx_h: cannot reserve LDS%s", grid, dim3(512), lds_b, st,
                                                              (const float*)logx, (long)F, K, (const float*)mcs, M1, (const float*)grts, N, n_iter,
                                                              (const _Float16*)images, (float*)glogx);
    };
    if (int rc = kse == 3 ? launch(int_c<3>{}) : launch(int_c<4>{})) return rc;
    return check_launch("mcep_glogx_h");
}

}  // namespace dsa
