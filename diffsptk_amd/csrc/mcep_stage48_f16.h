// The stage arithmetic of the 48 kHz mel-cepstral family, written ONCE: what a wave does with a stage of 32 bins of its 16 frames in
//   rt = exp(logx - 2 mc D) E   (mcep.py:210-215)
// on three-term binary16 splits, and the per-bin expression of that product's adjoint.  Every route of the family -- two launches per
// step (mcep_resid_f16.h), the one-launch kernels with narrow tiles, wide tiles (straight and software-pipelined) and the plan that
// mixes them (mcep_big_f16.h), twin workgroups (mcep_big4_f16.h) -- calls these functions, and the gradient pair (mcep_resid_bwd_f16.h
// in the sweep, mcep_glogx_f16.h in one pass) calls mfma_h3 and z_bin: that a frame's result has the SAME BITS whichever route runs
// (tests/test_gpu_configs.py, tests/test_gpu_48k_grad.py) rests on this file -- scale constants, the order of the three products, the
// dead-bin mask, the ceil of the stage maximum and the ldexp exponents have one definition.  All forceinline: the callers' code is the
// code of the text written out in place (profiles/mcep48_share_isa.txt).
#pragma once

#include "common.h"
#include "f16_split.h"   // the splits; namespace mrh: the stage geometry and scales

namespace dsa {

// a b accumulated into c with a = ah + al, b = bh + bl: lo . hi, then hi . lo, then hi . hi (the small terms first; lo . lo is
// left out: csrc/mcep_mfma_f16.h explains the scheme)
__device__ __forceinline__ f32x4 mfma_h3(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x4 c)
{
    c = mfma_h(al, bh, c);
    c = mfma_h(ah, bl, c);
    return mfma_h(ah, bh, c);
}

namespace mrh {

constexpr int MC_LOG2 = 12;   // scaled mc stays below 2^12

// a frame's row (mc: top = MC_LOG2; a cotangent: mrb::VMAX_LOG2) as a B operand: `bv` holds the lane's values of it (k-slot (g, i)
// of k-step ks <-> element 32 ks + 8 g + i, zero past the row's end) and `bmax` their largest magnitude, which the caller's load loop
// forms as it goes; the frame's four lanes g = 0 .. 3 together hold the row.  The row is scaled by the power of two 2^s that puts its
// largest magnitude just below 2^top, and split; the chain's accumulators x 2^-s are then the product with the row.  Returns s.
// (The loads stay with the caller, and so does the running maximum: formed here, in a loop of its own, every kernel's code changed.
//  Three sites keep this text written out, because the call changed their kernels' instruction order: the mc rows of
//  mcep_resid_bwd_h_kernel and both rows of mcep_glogx_h_kernel -- a change here is a change there.)
template <int KS>
__device__ __forceinline__ int scale_split(const float (&bv)[KS][8], float bmax, int top, f16x8 (&h)[KS], f16x8 (&l)[KS])
{
    bmax = rows_max4(bmax);
    const int s = top - __builtin_amdgcn_frexp_expf(bmax);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        float ms[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ms[i] = __builtin_ldexpf(bv[ks][i], s);
        split8(ms, h[ks], l[ks]);
    }
    return s;
}

// first chain: s[t] += (-2 log2(e) D)^T mc of the stage's two 16-bin tiles, KS1 k-steps of 32 coefficients.  `c1`: this lane's view
// of the stage's image ([2 t][KS1 ks][2 (hi, lo)][64 lane] f16x8, mcep_resid_h_prep_kernel); (bh, bl): the frame's mc, scaled by a
// power of two per frame and split -- the accumulators x 2^k1 are the product
template <int KS1>
__device__ __forceinline__ void chain1(const f16x8* c1, const f16x8 (&bh)[KS1], const f16x8 (&bl)[KS1], f32x4 (&s)[2])
{
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f16x8 dh = c1[((t * KS1 + ks) * 2 + 0) * 64], dl = c1[((t * KS1 + ks) * 2 + 1) * 64];
            s[t] = mfma_h3(dh, dl, bh[ks], bl[ks], s[t]);
        }
}

// t = log2(e) logx - 2 log2(e) (mc D) of the lane's eight bins 32 j + 16 t + 4 g + r (`xv`: their log-spectrum values; bins past K
// are dead: masked to -huge, exp2 gives 0); the stage's shift ceil(max t) over the frame's 32 bins; e = exp2(t - shift) scaled to
// 2^EMAX_LOG2 and split: the first chain's C/D tiles ARE the k-slots of the second chain's B operand.  Returns k2: the second chain's
// accumulators x 2^k2 are the stage's share of rt
__device__ __forceinline__ int exp_split(int j, int g, int K, int k1, const f32x4 (&xv)[2], const f32x4 (&s)[2], f16x8& eh, f16x8& el)
{
    float tv[8];
    float tmax = -3.0e38f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool live = 32 * j + 16 * t + 4 * g + r < K;
            const float v = __builtin_fmaf(xv[t][r], 1.4426950408889634f, __builtin_ldexpf(s[t][r], k1));
            tv[4 * t + r] = live ? v : -3.0e38f;
            tmax = __builtin_fmaxf(tmax, tv[4 * t + r]);
        }
    tmax = rows_max4(tmax);
    const float mi = __builtin_ceilf(tmax);
    const float shf = (float)EMAX_LOG2 - mi;
    float ev[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ev[i] = __builtin_amdgcn_exp2f(tv[i] + shf);   // (dead bins: exp2(-huge) = 0)
    split8(ev, eh, el);
    return (int)mi - EMAX_LOG2 - LOG2_SE;
}

// second chain: acc[tc] += 2^k2 (W e) over NT column tiles, fresh accumulators per stage (the
// stages' scales differ), added into the float32 sums with the stage's scale.  `w2`: this lane's view of the image
// ([NT tc][2 (hi, lo)][64 lane] f16x8)
template <int NT>
__device__ __forceinline__ void chain2(const f16x8* w2, const f16x8& eh, const f16x8& el, int k2, f32x4* acc)
{
#pragma unroll
    for (int tc = 0; tc < NT; ++tc) {
        const f16x8 wh = w2[(tc * 2 + 0) * 64], wlo = w2[(tc * 2 + 1) * 64];
        const f32x4 a_ = mfma_h3(wh, wlo, eh, el, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[tc][r] += __builtin_ldexpf(a_[r], k2);
    }
}

// the adjoint's per-bin value z = ebar e: e = exp(tau) recomputed from the first chain's accumulator `s` (x 2^k1) and the bin's
// log-spectrum value `x` exactly as the forward forms it (a dead bin: 0), `eb` the ebar chain's accumulator (x 2^ke)
__device__ __forceinline__ float z_bin(bool live, float x, float s, int k1, float eb, int ke)
{
    const float tv = __builtin_fmaf(x, 1.4426950408889634f, __builtin_ldexpf(s, k1));
    const float e_ = live ? __builtin_amdgcn_exp2f(tv) : 0.f;
    return __builtin_ldexpf(eb * e_, ke);
}

}  // namespace mrh

}  // namespace dsa
