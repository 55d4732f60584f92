// Tuned mel-cepstral analysis for gfx950: float32, fft_length 512, cep_order 24.
// (MelCepstralAnalysis._forward, diffsptk/modules/mcep.py:189-224, in the composed-matrix form
//  described in mcep.hip.)  tools/proto_mcep_mfma.py is a lane-level numpy model of the data flow.
//
// This unit is the forward: its kernels (mcep_mfma_f16.h) and the host side -- operand-image preparation and the launches.  What
// the forward shares with the backward (mcep_mfma_bwd.hip) and the other mel-cepstral units -- the LDS carve-up constants, the
// quad-layout elimination of the 25 x 25 system, the binary16 splits -- is in mcep_solve.h and f16_split.h; the functions other
// units call are declared in mcep_units.h.  The library keeps NO device memory of its own: the binary16
// operand images of (G, D, E) are written once per configuration into a caller-owned buffer
// (dsa_mcep_images_bytes / dsa_mcep_prepare) and the tile-queue counters of a launch live in a caller-owned
// scratch (DSA_SCRATCH_BYTES), so launches on any number of streams / devices never share mutable state.
// (Earlier kernel generations -- float32-MFMA chains, row-cyclic elimination, role-split waves -- are in the
// git history; DESIGN.md section 3.2 keeps their measurements.)
//
// Mapping.  One wave64 owns 16 frames for the whole Newton iteration; lane l = (n = l & 15: frame, g = l >> 4:
// lane group).  The frames are the N (column) dimension of the MFMAs, so products come out TRANSPOSED:
//     d^T (256 x 16) = D^T mc^T,   rt^T (48 x 16) = E^T e^T.
// In the C/D layout lane (n, g) register r of tile mt holds bin 16 mt + 4 g + r of frame n -- exactly a B operand
// if the k-steps of the second product are enumerated in that order (the E^T image is laid out for it), so
// e = exp(log X - 2 d) feeds the second chain straight from the accumulator registers: no transpose, no LDS
// round trip, log X stays in 64 VGPRs for all iterations.  Bin 256 (Nyquist) and output rt[48] are one extra
// k-step / one VALU dot product instead of padded tiles.
#include <type_traits>

#include "mcep_mfma_f16.h"

namespace dsa {

int mcep_mfma_supported(int nfft, int M, int dtype) { return dtype == DSA_F32 && nfft == 512 && M == 24; }

// bytes of the prepared operand images (forward + backward) of one configuration
int64_t mcep_mfma_images_bytes() { return ((int64_t)mhb::IMG_B_BYTES + 255) & ~(int64_t)255; }

// Splits (G, D, E) into the binary16 hi / lo operand images, in MFMA lane order, that both kernels consume
// (two tiny launches; done once per configuration by the caller, not per analysis call).
int mcep_mfma_prepare(const void* G, const void* D, const void* E, void* images, hipStream_t st)
{
    hipLaunchKernelGGL(mcep_h_prep_kernel, dim3((mh::IMG_D + mh::IMG_E + mh::IMG_G + 255) / 256), dim3(256), 0, st,
                       (const float*)G, (const float*)D, (const float*)E, (_Float16*)images);
    mcep_mfma_bwd_prepare_launch(G, D, E, images, st);
    return check_launch("mcep_prepare");
}

// `sti`: NULL (spectra in X) or the waveform side of the fused STFT -> mel-cepstrum launch (X is then unused)
int mcep_mfma_fwd(const void* X, int64_t F, int n_iter, const void* G, const void* D, const void* E, const void* av,
                  const void* images, void* scratch, void* mc, void* hist, hipStream_t st, bool scratch_clean, const StftIn* sti,
                  bool hist_has_rt, bool overlapped, int reserve_cus, bool fixed_steps, bool full_chains)
{
    // DSA_ALGO_HIST_HAS_RT: the caller's history buffer continues behind the (n_iter + 1, F, 25) iterates with (n_iter, F, 49) rows of rt
    float* hist_rt = (hist && hist_has_rt) ? (float*)hist + (size_t)(n_iter + 1) * (size_t)F * mm::M1 : nullptr;
    constexpr int WAVES = 8;
    const int lds_bytes = (sti ? mh::h_lds_floats_fused(WAVES) : mh::h_lds_floats(WAVES)) * 4;
    const bool rt = hist_rt != nullptr;
    const bool padm = sti && (sti->pad_mode != (int)DSA_PAD_CONSTANT || sti->zmean || sti->floor_lin >= 0.f);
    long ntiles16 = (long)((F + 15) / 16);
    long blocks = (ntiles16 + WAVES - 1) / WAVES;
    long grid = blocks < 256 ? blocks : 256;  // one persistent workgroup per CU
    // DSA_ALGO_RESERVE_CUS(n): n CUs stay free for a kernel of ANOTHER stream that has to run beside this launch (a collective's: a
    // persistent workgroup fills its CU's LDS and registers, so nothing else starts on a CU before the launch's tail)
    if (reserve_cus > 0 && grid == 256 && !overlapped) {
        // at least reserve_cus, and up to twice as many where they cost no further round of tiles: a launch is rounds of (8 grid) tiles, a
        // short last round (at most half full) goes to one wave per SIMD pair and takes 0.8 of a round (below).  A side kernel whose
        // workgroup count EQUALS the free CUs was measured to start late now and then (profiles/r06_reserve_cus_ab.txt): slack is cheap
        auto rounds = [&](long g) {
            const long s = g * WAVES, full = ntiles16 / s, rest = ntiles16 - full * s;
            return (double)full + (rest == 0 ? 0.0 : (full > 0 && rest <= s / 2) ? 0.8 : 1.0);
        };
        const long g_hi = 256 - (reserve_cus < 63 ? reserve_cus : 63), g_lo = 256 - 2 * (reserve_cus < 63 ? reserve_cus : 63) < 128 ? 128 : 256 - 2 * (reserve_cus < 63 ? reserve_cus : 63);
        grid = g_hi;
        for (long g = g_hi - 1; g >= g_lo; --g)
            if (rounds(g) <= rounds(g_hi) + 1e-9) grid = g;
    }
    // the kernel zeroes the counters again when its last wave retires: a caller that vouches for a clean scratch
    // (DSA_ALGO_SCRATCH_IS_CLEAN) saves the fill launch
    unsigned int* queue = scratch_clean ? (unsigned int*)scratch : reset_queue(scratch, st, 3);
    if (!queue) return fail(DSA_ERR_LAUNCH, "mcep_mfma: cannot reset the tile queue%s");
    // see the ticket comment in the kernel: a short last round goes to one wave per SIMD pair
    const long slots = grid * WAVES, full = ntiles16 / slots * slots, rest = ntiles16 - full;
    // (sized for tiles that all take the same time.  With the stopping rule a tile takes mostly 5, sometimes 6 to 8 steps (round 9;
    //  5 to 8 in round 8), and the plan still wins: the bench step at 0.3769 - 0.3774 ms against 0.3925 - 0.3929 with every tile in
    //  the shared queue, three alternating runs each, profiles/r09_quadratic_stop_ab.txt; round 8: 0.390 against 0.405,
    //  profiles/r08_early_stop_ab.txt)
    long tiles_shared = (full > 0 && rest > 0 && rest <= slots / 2) ? full : ntiles16;
    // DSA_ALGO_OVERLAPPED_LAUNCHES: the short round packed onto the first tail_wgs workgroups at two waves per SIMD; everyone else
    // exits and leaves its CU to the next launch on the caller's other stream (include/diffsptk_amd.h)
    int tail_wgs = 0;
    if (overlapped && full > 0 && rest > 0 && grid == 256) {
        tiles_shared = full;
        tail_wgs = (int)((rest + WAVES - 1) / WAVES);
    }
    // DSA_ALGO_FIXED_STEPS: a threshold no update compares below -- every step runs and every update is applied
    const float tau = fixed_steps ? -1.f : mh::STOP_TAU;
    // Round 11: the first n_coarse steps run their chains on the hi pieces alone (one product for three), each with at least six full
    // steps behind it.  A static schedule of (step, n_iter), whatever the stopping rule does.  DSA_ALGO_FULL_CHAINS, or
    // DSA_MCEP_FULL_CHAINS=1 in the environment: none -- every step on three-term chains, the arithmetic of versions before 0.3.8.
    const bool three_terms = full_chains || env_int("DSA_MCEP_FULL_CHAINS", 0) != 0;
    const int n_coarse = three_terms ? 0 : (n_iter - 6 < 0 ? 0 : n_iter - 6 > 2 ? 2 : n_iter - 6);
    // HIST_RT and PADM (reflect / replicate / circular padding, zmean, relative floor) are instantiations of their own
    auto launch = [&](auto fused, auto with_rt, auto options) {
        if (int rc = launch_lds<mcep_mfma_fwd_kernel_h<WAVES, fused(), with_rt(), options()>>(
                lds_bytes, "mcep_mfma: cannot reserve the LDS operand images%s", dim3((unsigned)grid), dim3(WAVES * 64), lds_bytes, st,
                sti ? nullptr : (const float*)X, (long)F, n_iter, (const float*)G, (const float*)D, (const float*)E, (const float*)av, (float*)mc,
                (float*)hist, ntiles16, tiles_shared, queue, (const _Float16*)images, sti ? *sti : StftIn{}, hist_rt, tail_wgs, tau, n_coarse))
            return rc;
        return check_launch(fused() ? "stft512_mcep_fused_fwd" : "mcep_mfma_fwd");
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (padm) return rt ? launch(yes, yes, yes) : launch(yes, no, yes);
    if (sti) return rt ? launch(yes, yes, no) : launch(yes, no, no);
    return rt ? launch(no, yes, no) : launch(no, no, no);
}

// STFT (frame length 400, fft_length 512, power format, constant padding) -> MelCepstralAnalysis (cep_order 24) in one launch
int stft_mcep_fused_fwd(const void* x, int64_t B, int64_t T, int P, int center, const void* window, const void* twiddle, double eps,
                        int n_iter, const void* G, const void* D, const void* E, const void* av, const void* images, void* scratch,
                        void* mc, void* hist, void* X_out, hipStream_t st, bool scratch_clean, bool hist_has_rt, bool overlapped, int pad_mode,
                        int zmean, float floor_lin, int reserve_cus, bool fixed_steps, bool full_chains)
{
    const int64_t N = T <= 0 ? 0 : (T - 1) / P + 1;
    StftIn sti;
    sti.x = (const float*)x;
    sti.Tlen = (long)T;
    sti.N = (long)N;
    sti.P = P;
    sti.left = center ? mh::FU_LC / 2 : 0;
    sti.w = (const float*)window;
    sti.twiddle = (const float*)twiddle;
    sti.eps = (float)eps;
    sti.X_out = (float*)X_out;
    sti.pad_mode = pad_mode;
    sti.zmean = zmean;
    sti.floor_lin = floor_lin;
    return mcep_mfma_fwd(nullptr, B * N, n_iter, G, D, E, av, images, scratch, mc, hist, st, scratch_clean, &sti, hist_has_rt, overlapped, reserve_cus, fixed_steps, full_chains);
}

}  // namespace dsa
