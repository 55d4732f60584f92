// All Newton steps of the mel-cepstral analysis at the 48 kHz set-ups in one persistent launch: the kernels (mcep_big_f16.h: eight
// waves per workgroup, narrow and wide tiles; mcep_big4_f16.h: twin four-wave workgroups) and the plan that picks among them.  The
// kernels read the operand images of mcep_resid.hip and run the solver templates of thsolve_tq.h.  (Caller: rows_gemm.hip.)
#include "mcep_big4_f16.h"
#include "mcep_big_f16.h"

namespace dsa {

// mcep.py:208-222, all n_iter steps in one persistent launch, for orders 32 .. 54 (the 48 kHz set-ups fft_length 2048 / order 49 and
// 1024 / order 34 among them); DSA_ERR_UNSUPPORTED (no error text) otherwise --
// the caller then runs the step as two launches.  `images`: dsa_mcep_resid_prepare's.
int mcep_big_newton(const void* logx, int64_t F, int K, const void* mc_in, int M1, const void* images, const void* av, int n_iter,
                    void* mc_out, hipStream_t st)
{
    const int ks1 = (M1 + 31) / 32, nt = (2 * M1 - 1 + 15) / 16;
    // the orders of the octet-layout solver, 35 .. 54, and -- quad layout -- 32 .. 34 (the 48 kHz set-up fft_length 1024 / order 34)
    if (!(ks1 == 2 && M1 >= 33 && M1 <= 55 && K >= 4)) return DSA_ERR_UNSUPPORTED;
    if (env_int("DSA_MCEP_BIG", 1) == 0) return DSA_ERR_UNSUPPORTED;   // A/B: the two-launch step
    // The kernel's INSTANTIATION is chosen by the order alone; its tile shape by the batch.  A persistent launch is rounds of 256 tiles
    // (one eight-wave workgroup per CU) and a round takes a tile's time however few tiles it has.  Narrow tiles (64 frames, two
    // waves per 16-frame group: the shortest step) for up to one round; beyond it a PLAN: W rounds of wide tiles (128 frames, a wave per
    // group: 1.6 x a narrow round's time for twice the frames) over the first W x 32 768 frames, narrow rounds over the rest -- the W
    // that minimises the sum, two launches on the caller's stream over disjoint frames.  Both shapes -- and the two launches per
    // step -- give the same bits (mcep_resid_f16.h sums the even and the odd stages separately, as the two waves of a narrow group /
    // the one wave of a wide group do), so a frame's result does not depend on the plan (tests/test_gpu_configs.py).
    // Measured, us per analysis, fft_length 2048 / order 49, 10 steps (profiles/r06_mcep_big_newton.txt, two launches per step ->
    // narrow): 200 frames 696 -> 593, 3 200 724 -> 630, 12 800 920 -> 672, 20 000 1 250 -> 1 300, 40 000 2 027 -> 2 008, 102 400
    // 4 813 -> 4 720; with the plan: profiles/r06_mcep_big_wide.txt.
    const int wide_env = env_int("DSA_MCEP_BIG_WIDE", -1);   // A/B and tests: 0 never, 1 always
    const bool quad = M1 <= 35;
    // Quad-layout orders: the rounds of 32 768 frames run as TWIN workgroups (mcep_big4_f16.h: two four-wave workgroups per CU, the
    // second half a step late: 1024 / 34 at 122 880 frames 2.15 -> 1.99 ms, profiles/r06_mcep_big_twin.txt) instead of eight-wave wide
    // tiles (DSA_MCEP_BIG_TWIN=0, A/B); the same bits either way.  At the octet-layout orders the twin shape measured no faster than
    // the plan (each workgroup streams the images itself: twice the bytes from L2 per frame) and is not instantiated.
    const bool twin = quad && env_int("DSA_MCEP_BIG_TWIN", 1) != 0;
    const long FN = 256L * 64, FW = 256L * 128;          // frames a full round of narrow / wide (or twin) tiles takes
    long wide_rounds = 0;
    if (wide_env > 0 || (wide_env < 0 && twin && F > FN)) {
        // (twin workgroups take 64-frame tiles like the narrow shape: beyond one narrow round every frame goes to them -- measured
        //  against twin rounds + narrow rounds for the rest, 1024 / 34: 79 200 frames 1.28 / 1.34 ms, 245 760 3.62 / 3.88)
        wide_rounds = (long)((F + FW - 1) / FW);
    } else if (wide_env < 0 && F > FN) {
        // a wide round's time in units of a narrow round's (measured: 1.09 / 0.67 ms at 2048 / 49, 0.48 / 0.34 ms at 1024 / 34)
        const double tw = quad ? 1.42 : 1.63;
        double best = (double)((F + FN - 1) / FN);
        for (long w = 1; w <= (long)((F + FW - 1) / FW); ++w) {
            const long rest = F - w * FW;
            const double c = w * tw + (rest > 0 ? (double)((rest + FN - 1) / FN) : 0.0);
            if (c < best - 1e-9) {
                best = c;
                wide_rounds = w;
            }
        }
    }
    const long F_wide = wide_rounds * FW < F ? wide_rounds * FW : (wide_rounds > 0 ? (long)F : 0);
    const int stagger = env_int("DSA_MCEP_BIG_STAGGER", 5);   // x ~8 k cycles (measured 4 .. 6 best: profiles/r06_mcep_big_twin.txt)
#define DSA_BIG_NEWTON_1(NTV, NGV, NMINV, QUADV, WIDEV, F0, FC)                                                                         \
    do {                                                                                                                                \
        constexpr int lds_b = mbg::lds_floats<2, NTV, NGV, QUADV, WIDEV>() * 4;                                                         \
        static_assert(lds_b <= 160 * 1024, "mcep_big_newton: LDS");                                                                     \
        static std::atomic<uint64_t> attr{0};                                                                                           \
        if (!ensure_dynamic_lds((const void*)mcep_big_newton_kernel<2, NTV, NGV, NMINV, QUADV, WIDEV>, lds_b, attr))                    \
            return fail(DSA_ERR_LAUNCH, "mcep_big_newton: cannot reserve LDS%s");                                                       \
        const long tiles_ = ((FC) + (WIDEV ? 127 : 63)) / (WIDEV ? 128 : 64);                                                           \
        const long grid_ = tiles_ < 256 ? tiles_ : 256;   /* persistent: one eight-wave workgroup per CU (105 / 148 KB of LDS) */        \
        hipLaunchKernelGGL((mcep_big_newton_kernel<2, NTV, NGV, NMINV, QUADV, WIDEV>), dim3((unsigned)grid_), dim3(512), lds_b, st,     \
                           (const float*)logx + (F0) * (long)K, (long)(FC), K, (const float*)mc_in + (F0) * (long)M1, M1,               \
                           (const _Float16*)images, (const float*)av, n_iter, (float*)mc_out + (F0) * (long)M1);                        \
    } while (0)
#define DSA_BIG_NEWTON4_1(NTV, NGV, NMINV, QUADV, F0, FC)                                                                               \
    do {                                                                                                                                \
        constexpr int lds_b = mbg4::lds_floats<2, NTV, NGV, QUADV>() * 4;                                                               \
        static_assert(lds_b <= 80 * 1024, "mcep_big_newton: two workgroups per CU");                                                    \
        static std::atomic<uint64_t> attr{0};                                                                                           \
        if (!ensure_dynamic_lds((const void*)mcep_big_newton4_kernel<2, NTV, NGV, NMINV, QUADV>, lds_b, attr))                          \
            return fail(DSA_ERR_LAUNCH, "mcep_big_newton: cannot reserve LDS%s");                                                       \
        const long tiles_ = ((FC) + 63) / 64;                                                                                           \
        const long grid_ = tiles_ < 512 ? tiles_ : 512;   /* persistent: two four-wave workgroups per CU */                             \
        hipLaunchKernelGGL((mcep_big_newton4_kernel<2, NTV, NGV, NMINV, QUADV>), dim3((unsigned)grid_), dim3(256), lds_b, st,           \
                           (const float*)logx + (F0) * (long)K, (long)(FC), K, (const float*)mc_in + (F0) * (long)M1, M1,               \
                           (const _Float16*)images, (const float*)av, n_iter, (float*)mc_out + (F0) * (long)M1, stagger);               \
    } while (0)
#define DSA_BIG_NEWTON_Q(NTV, NGV, NMINV)                                                                                               \
    do {                                                                                                                                \
        if (F_wide > 0 && twin) DSA_BIG_NEWTON4_1(NTV, NGV, NMINV, true, 0L, F_wide);                                                   \
        else if (F_wide > 0) DSA_BIG_NEWTON_1(NTV, NGV, NMINV, true, true, 0L, F_wide);                                                 \
        if (F_wide < (long)F) DSA_BIG_NEWTON_1(NTV, NGV, NMINV, true, false, F_wide, (long)F - F_wide);                                 \
    } while (0)
#define DSA_BIG_NEWTON(NTV, NGV, NMINV, QUADV)                                                                                          \
    do {                                                                                                                                \
        if (F_wide > 0) DSA_BIG_NEWTON_1(NTV, NGV, NMINV, QUADV, true, 0L, F_wide);                                                     \
        if (F_wide < (long)F) DSA_BIG_NEWTON_1(NTV, NGV, NMINV, QUADV, false, F_wide, (long)F - F_wide);                                \
    } while (0)
    // (M1 = order + 1; the solver's instantiations as thsolve_quadn_fwd picks them: quad <9,28> up to 35, <11,36> up to 43, <13,44> up to
    //  51, <14,52>)
    if (quad) {
        DSA_BIG_NEWTON_Q(5, 9, 28);
    } else if (M1 <= 43) {
        if (nt == 5) DSA_BIG_NEWTON(5, 11, 36, false);
        else DSA_BIG_NEWTON(6, 11, 36, false);
    } else if (M1 <= 51) {
        if (nt == 6) DSA_BIG_NEWTON(6, 13, 44, false);
        else DSA_BIG_NEWTON(7, 13, 44, false);
    } else {
        DSA_BIG_NEWTON(7, 14, 52, false);
    }
#undef DSA_BIG_NEWTON
#undef DSA_BIG_NEWTON_Q
#undef DSA_BIG_NEWTON_1
#undef DSA_BIG_NEWTON4_1
    return check_launch("mcep_big_newton");
}

}  // namespace dsa
