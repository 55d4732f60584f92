// All Newton steps of the mel-cepstral analysis at the 48 kHz set-ups in one persistent launch: the kernels (mcep_big_f16.h: eight
// waves per workgroup, narrow and wide tiles; mcep_big4_f16.h: twin four-wave workgroups) and the plan that picks among them.  The
// kernels read the operand images of mcep_resid.hip and run the solver templates of thsolve_tq.h.  (Caller: rows_gemm.hip.)
#include "mcep_big4_f16.h"
#include "mcep_big_f16.h"

namespace dsa {

namespace {

// what every launch of mcep_big_newton passes on
struct BigNewtonCall {
    const float *logx, *mc_in, *av;
    const _Float16* images;
    float* mc_out;
    int K, M1, n_iter, stagger;
    hipStream_t st;
};

// the eight-wave kernel over the frames [f0, f0 + fc)
template <int NTV, int NGV, int NMINV, bool QUADV, bool WIDEV>
int big_newton_launch(const BigNewtonCall& c, long f0, long fc)
{
    constexpr int lds_b = mbg::lds_floats<2, NTV, NGV, QUADV, WIDEV>() * 4;
    static_assert(lds_b <= 160 * 1024, "mcep_big_newton: LDS");
    const long tiles = (fc + (WIDEV ? 127 : 63)) / (WIDEV ? 128 : 64);
    const long grid = tiles < 256 ? tiles : 256;   // persistent: one eight-wave workgroup per CU (105 / 148 KB of LDS)
    return launch_lds<mcep_big_newton_kernel<2, NTV, NGV, NMINV, QUADV, WIDEV>>(
        lds_b, "mcep_big_newton: cannot reserve LDS%s", dim3((unsigned)grid), dim3(512), lds_b, c.st, c.logx + f0 * (long)c.K, fc, c.K,
        c.mc_in + f0 * (long)c.M1, c.M1, c.images, c.av, c.n_iter, c.mc_out + f0 * (long)c.M1);
}

// the twin four-wave kernel over the frames [f0, f0 + fc)
template <int NTV, int NGV, int NMINV, bool QUADV>
int big_newton4_launch(const BigNewtonCall& c, long f0, long fc)
{
    constexpr int lds_b = mbg4::lds_floats<2, NTV, NGV, QUADV>() * 4;
    static_assert(lds_b <= 80 * 1024, "mcep_big_newton: two workgroups per CU");
    const long tiles = (fc + 63) / 64;
    const long grid = tiles < 512 ? tiles : 512;   // persistent: two four-wave workgroups per CU
    return launch_lds<mcep_big_newton4_kernel<2, NTV, NGV, NMINV, QUADV>>(
        lds_b, "mcep_big_newton: cannot reserve LDS%s", dim3((unsigned)grid), dim3(256), lds_b, c.st, c.logx + f0 * (long)c.K, fc, c.K,
        c.mc_in + f0 * (long)c.M1, c.M1, c.images, c.av, c.n_iter, c.mc_out + f0 * (long)c.M1, c.stagger);
}

// the plan's launches of one instantiation: wide tiles (quad layout: twin workgroups, when asked for) over the first F_wide frames, narrow
// tiles over the rest
template <int NTV, int NGV, int NMINV, bool QUADV>
int big_newton_plan(const BigNewtonCall& c, long F_wide, long F, bool twin)
{
    int rc = DSA_OK;
    if constexpr (QUADV) {
        if (F_wide > 0 && twin) rc = big_newton4_launch<NTV, NGV, NMINV, true>(c, 0L, F_wide);
        else if (F_wide > 0) rc = big_newton_launch<NTV, NGV, NMINV, true, true>(c, 0L, F_wide);
    } else if (F_wide > 0) {
        rc = big_newton_launch<NTV, NGV, NMINV, false, true>(c, 0L, F_wide);
    }
    if (rc == DSA_OK && F_wide < F) rc = big_newton_launch<NTV, NGV, NMINV, QUADV, false>(c, F_wide, F - F_wide);
    return rc;
}

}  // namespace

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
    const BigNewtonCall call{(const float*)logx, (const float*)mc_in, (const float*)av, (const _Float16*)images, (float*)mc_out, K, M1, n_iter, stagger,
                             st};
    // (M1 = order + 1; the solver's instantiations as thsolve_quadn_fwd picks them: quad <9,28> up to 35, <11,36> up to 43, <13,44> up to
    //  51, <14,52>)
    const long Fn = (long)F;
    int rc;
    if (quad) rc = big_newton_plan<5, 9, 28, true>(call, F_wide, Fn, twin);
    else if (M1 <= 43 && nt == 5) rc = big_newton_plan<5, 11, 36, false>(call, F_wide, Fn, false);
    else if (M1 <= 43) rc = big_newton_plan<6, 11, 36, false>(call, F_wide, Fn, false);
    else if (M1 <= 51 && nt == 6) rc = big_newton_plan<6, 13, 44, false>(call, F_wide, Fn, false);
    else if (M1 <= 51) rc = big_newton_plan<7, 13, 44, false>(call, F_wide, Fn, false);
    else rc = big_newton_plan<7, 14, 52, false>(call, F_wide, Fn, false);
    if (rc) return rc;
    return check_launch("mcep_big_newton");
}

}  // namespace dsa
