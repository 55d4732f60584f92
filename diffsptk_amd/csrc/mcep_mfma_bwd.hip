// Backward of the tuned mel-cepstral analysis for gfx950 (float32, fft_length 512, cep_order 24): the reverse sweep over the
// unrolled Newton iteration from the iterates the forward (mcep_mfma.hip) saved.  This unit: the kernels (mcep_mfma_bwd_f16.h, one
// wave per SIMD; mcep_mfma_bwd2_f16.h, two, when the forward also saved its rt rows), their launch, and the launch that writes the
// backward's operand images behind the forward's (mcep_mfma_prepare calls it).
#include <stdlib.h>

#include <type_traits>

#include "mcep_mfma_bwd2_f16.h"
#include "mcep_mfma_bwd_f16.h"

namespace dsa {

void mcep_mfma_bwd_prepare_launch(const void* G, const void* D, const void* E, void* images, hipStream_t st)
{
    hipLaunchKernelGGL(mcep_hb_prep_kernel, dim3((mhb::IMG_EB + mhb::IMG_DB + mhb::IMG_GB + 255) / 256), dim3(256), 0, st,
                       (const float*)G, (const float*)D, (const float*)E, (_Float16*)images);
}

int mcep_mfma_bwd(const void* gmc, const void* X, const void* hist, int64_t F, int n_iter, const void* av,
                  const void* images, void* scratch, void* gX, hipStream_t st, bool has_workspace, bool hist_has_rt)
{
    const float* hist_rt = hist_has_rt ? (const float*)hist + (size_t)(n_iter + 1) * (size_t)F * mm::M1 : nullptr;
    // With the forward's rt rows at hand the sweep runs on the two-waves-per-SIMD kernel (mcep_mfma_bwd2_f16.h); DSA_MCEP_BWD2=0: A/B
    const bool two = hist_rt && env_int("DSA_MCEP_BWD2", 1) != 0;
    const int waves = two ? mh2::WAVES_2 : mhb::WAVES_B;
    const int lds_bytes = (two ? mh2::C_LDS_FLOATS : mhb::B_LDS_FLOATS) * 4;
    unsigned int* queue = reset_queue(scratch, st, 13);
    if (!queue) return fail(DSA_ERR_LAUNCH, "mcep_mfma_bwd: cannot reset the tile queue%s");
    long ntiles16 = (long)((F + 15) / 16);
    long blocks = (ntiles16 + waves - 1) / waves;
    long grid = blocks < 256 ? blocks : 256;
    // A last round that fills at most half of the wave slots is cut into pieces of Newton steps (see the kernel) when the caller's
    // scratch carries the hand-over workspace behind the counters (DSA_ALGO_SCRATCH_HAS_WORKSPACE)
    const long slots = grid * waves, rounds = ntiles16 / slots, rest = ntiles16 - rounds * slots;
    int split_tiles = 0, split_pieces = 0;
    if (!two && has_workspace && rounds >= 1 && rest > 0 && rest <= slots / 2 && rest <= 512 && n_iter >= 2) {
        long pieces = slots / rest;
        if (pieces > n_iter) pieces = n_iter;
        if (pieces > rounds + 1) pieces = rounds + 1;
        if (pieces > 9) pieces = 9;   // one counter word of the scratch per piece level
        split_tiles = (int)rest;
        split_pieces = (int)pieces;
    }
    const char* lds_error = "mcep_mfma_bwd: cannot reserve the LDS operand images%s";
    if (two) {
        if (int rc = launch_lds<mcep_mfma_bwd2_kernel_h>(lds_bytes, lds_error, dim3((unsigned)grid), dim3(waves * 64), lds_bytes, st, (const float*)gmc,
                                                         (const float*)X, (const float*)hist, (long)F, n_iter, (const float*)av, (float*)gX, ntiles16,
                                                         queue, (const _Float16*)images, hist_rt))
            return rc;
        return check_launch("mcep_mfma_bwd2");
    }
    auto launch = [&](auto saved_rt) {   // the one-wave-per-SIMD kernel, with or without the forward's rt rows
        return launch_lds<mcep_mfma_bwd_kernel_h<saved_rt()>>(lds_bytes, lds_error, dim3((unsigned)grid), dim3(256), lds_bytes, st, (const float*)gmc,
                                                              (const float*)X, (const float*)hist, (long)F, n_iter, (const float*)av, (float*)gX,
                                                              ntiles16, queue, (const _Float16*)images, split_tiles, split_pieces,
                                                              reinterpret_cast<float*>(static_cast<char*>(scratch) + DSA_SCRATCH_BYTES), hist_rt);
    };
    if (int rc = hist_rt ? launch(std::true_type{}) : launch(std::false_type{})) return rc;
    return check_launch("mcep_mfma_bwd");
}

}  // namespace dsa
