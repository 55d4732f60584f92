// The row-pivoted Toeplitz-plus-Hankel solve of ONE system by ONE wave, rows in registers (shared by csrc/thsolve.hip -- the general
// kernel -- and the quad-layout kernels of csrc/mgcep_step_f16.h / csrc/mcep_big_f16.h / csrc/thsolve_quad.hip, which fall back to it
// for the systems their unpivoted elimination gives up on).
#pragma once

#include "common.h"

namespace dsa {

// Register version for n <= NMAX (NMAX = 24 or 32: cep_order 24 is the usual size): lane i holds row i of the system and
// its right-hand side in registers, the pivot row reaches the other lanes through v_readlane (the pivot lane is uniform),
// everything is statically indexed (both loops unrolled).  Same pivot rule as the LDS version below, which remains for
// larger systems: that one spends ~80 cycles per element on dependent LDS round trips (0.53 ms per 51 200 frames of 24 x 24,
// 43 % of a mel-generalized analysis), this one ~6 k cycles per frame.
// Returns in (col, sol): lane i < n was the pivot row of column `col`, and x[col] = sol.
template <typename T, int NMAX>
__device__ __forceinline__ void th_solve_reg(const T* ps, const T* qs, T rhs, int n, int lane, int& col, T& sol)
{
    T row[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) {
        const int d = lane > j ? lane - j : j - lane;
        row[j] = (lane < n && j < n) ? ps[d] + qs[lane + j] : T(0);
    }
    if (lane >= n) rhs = T(0);
    bool used = lane >= n;
    T piv = T(1);
    col = 0;
#pragma unroll
    for (int k = 0; k < NMAX; ++k) {
        if (k < n) {   // uniform
            // pivot = the unused row with the largest |a_ik|: one unsigned key per lane (magnitude bits with the lane in the
            // low 6 bits: ties and near-ties go to the lowest lane), maximum over the wave by DPP shifts -- cross-lane
            // shuffles through the LDS crossbar cost 12 dependent round trips per step here
            const float magf = (float)(row[k] < T(0) ? -row[k] : row[k]);
            unsigned key = used ? 0u : ((__builtin_bit_cast(unsigned, magf) & 0xffffffc0u) | (unsigned)(63 - lane));
#define DSA_TH_MAX(CTRL, RM)                                                                                            \
    {                                                                                                                  \
        const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)key, CTRL, RM, 0xf, false);                   \
        key = o > key ? o : key;                                                                                       \
    }
            DSA_TH_MAX(0x111, 0xf) DSA_TH_MAX(0x112, 0xf) DSA_TH_MAX(0x114, 0xf) DSA_TH_MAX(0x118, 0xf)   // row_shr:1, 2, 4, 8
            DSA_TH_MAX(0x142, 0xa) DSA_TH_MAX(0x143, 0xc)                                                 // row_bcast:15, :31
#undef DSA_TH_MAX
            // (the builtin itself: through wave_readlane the compiler swaps operands of scalar ORs in 25 kernels that inline this)
            const int p = 63 - (int)(__builtin_amdgcn_readlane((int)key, 63) & 63);
            const T pk = wave_readlane(row[k], p);
            const T fac = (lane != p) ? row[k] / pk : T(0);
            if (lane == p) {
                used = true;
                col = k;
                piv = row[k];
            }
#pragma unroll
            for (int j = k + 1; j < NMAX; ++j) row[j] -= fac * wave_readlane(row[j], p);
            rhs -= fac * wave_readlane(rhs, p);
        }
    }
    sol = rhs / piv;
}

}  // namespace dsa
