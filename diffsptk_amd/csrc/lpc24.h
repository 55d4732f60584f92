// What the tuned order-24 LPC kernels share: the forward pair (lpc24.hip) and the backward pair (lpc24_bwd.hip).  Device side: the
// steps of the lag sums (row sums by DPP, the 625-FMA block; of the two-frame round on the matrix pipe: maximum and shift, binary16
// split, the nine products, scatter, float64 row sums) and the unrolled Levinson-Durbin recursion.  Host side: frames per work item,
// and the launch of a kernel with large dynamic LDS.
// What of a round is NOT here stands in each kernel, forward and backward line for line: the window products, the per-lane wa / addr,
// the operand shifts, the fetch; and of the float64 pass its loop.  As forceinline helpers each of them made the kernels compile to
// other instructions, and timed one at a time none stayed inside the parent's spread (profiles/lpc_split_isa.txt, lpc_split_bench.txt).
// A fix there is made in BOTH units; tools/dump_lpc.py compares the outputs of two builds bit for bit.
#pragma once

#include <atomic>
#include <type_traits>
#include <utility>

#include "common.h"

namespace dsa {

constexpr int kLpcM1 = 25;

// Sum over the 16 lanes of a DPP row, left in every lane: four rotate-and-add steps (row_ror 8, 4, 2, 1) on the
// vector ALU.  (`__shfl_xor` on a double is two ds_bpermute_b32: 200 LDS-crossbar instructions per pass for the 25
// lag sums, which kept the LDS pipe busier than the float64 FMAs kept the ALU.)  Addition is commutative, so every
// lane of the row ends with the bit-identical sum.
template <int SH>
__device__ __forceinline__ double row_ror_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x120 + SH, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x120 + SH, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row16_allsum(double v)
{
    v += row_ror_f64<8>(v);
    v += row_ror_f64<4>(v);
    v += row_ror_f64<2>(v);
    v += row_ror_f64<1>(v);
    return v;
}

template <int... Is>
__device__ __forceinline__ void lag_block(double (&acc)[kLpcM1], const double (&xw)[2 * kLpcM1 - 1],
                                          std::integer_sequence<int, Is...>)
{
    // acc[m] += xw[i] * xw[i + m] for i, m in 0..24, flattened (Is = 25 i + m)
    ((acc[Is % kLpcM1] = __builtin_fma(xw[Is / kLpcM1], xw[Is / kLpcM1 + Is % kLpcM1], acc[Is % kLpcM1])), ...);
}

// One order update of the Levinson-Durbin recursion (levdur.py:113-127 as a recursion), float64 in registers: from
// s = r[m] + sum_q a[q] r[m - q] and the order-(m - 1) error to the order-m predictor and its error.
__device__ __forceinline__ void levinson24_step(double (&a)[kLpcM1], int m, double s, double& Ecur)
{
    const double kk = -s / Ecur;
#pragma unroll
    for (int q = 1; 2 * q <= m; ++q) {
        const double aq = a[q], amq = a[m - q];
        a[q] = __builtin_fma(kk, amq, aq);
        if (q != m - q) a[m - q] = __builtin_fma(kk, aq, amq);
    }
    a[m] = kk;
    Ecur *= (1.0 - kk * kk);
}

// The whole recursion of one frame, fully unrolled (no cross-lane traffic at all): a[1..24] from the lag sums r[0..24] and eps;
// returns the gain's square r0 + sum_m r[m] a[m].
__device__ __forceinline__ double levinson24(const double (&r)[kLpcM1], double eps, double (&a)[kLpcM1])
{
#pragma unroll
    for (int m = 0; m < kLpcM1; ++m) a[m] = 0.0;
    double Ecur = r[0] + eps;
#pragma unroll
    for (int m = 1; m < kLpcM1; ++m) {
        double s = r[m];
#pragma unroll
        for (int q = 1; q < m; ++q) s = __builtin_fma(a[q], r[m - q], s);
        levinson24_step(a, m, s, Ecur);
    }
    double gsum = r[0];  // un-regularised r0 (levdur.py:124)
#pragma unroll
    for (int m = 1; m < kLpcM1; ++m) gsum = __builtin_fma(r[m], a[m], gsum);
    return gsum;
}

// The end of the recursion's adjoint, from the gain's square to the cotangent of the lag sums: with u = (R + eps I)^{-1} abar from
// the order updates, sbar = Kbar / (2K) and v = u - sbar a (because R a = -r_1),
//   rbar[m] = -sum_{|i-j|=m} v_i a_j  (+ sbar a_m - v_m for m >= 1;  + sbar for m = 0),   handed to put(m, rbar[m]) in order.
// (Where the lag sums are read from -- registers or the frame's LDS row -- is the caller's: it forms gsum.)
template <typename Put>
__device__ __forceinline__ void levinson24_adjoint_tail(double kbar, double gsum, const double (&a)[kLpcM1], double (&u)[kLpcM1], Put&& put)
{
    const double sbar = kbar / (2.0 * sqrt(gsum));
#pragma unroll
    for (int m = 1; m < kLpcM1; ++m) u[m] = __builtin_fma(-sbar, a[m], u[m]);  // v
#pragma unroll
    for (int m = 0; m < kLpcM1; ++m) {
        double acc = (m == 0) ? sbar : __builtin_fma(sbar, a[m], -u[m]);
#pragma unroll
        for (int i = 1; i + m < kLpcM1; ++i) {
            if (m < kLpcM1 - 1) {
                acc = __builtin_fma(-u[i], a[i + m], acc);
                if (m > 0) acc = __builtin_fma(-u[i + m], a[i], acc);
            }
        }
        put(m, acc);
    }
}

// x = hi + lo in binary16 (round to nearest), two values at a time: one packed conversion, then lo = binary16(x - float(hi)) as ONE
// v_fma_mixlo_f16 / v_fma_mixhi_f16 per value (binary16 operand from its half register, float32 multiply-add, result rounded into
// the low / high half).  The wait state after each half-register write is what gfx950 wants before the register is touched again
// (same helper as csrc/mcep_mfma_f16.h:split2).
typedef _Float16 lp_h2 __attribute__((ext_vector_type(2)));
typedef float lp_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void lp_split2(float x0, float x1, lp_h2& hi, lp_h2& lo)
{
    hi = __builtin_convertvector(lp_f2{x0, x1}, lp_h2);
    const unsigned hb = __builtin_bit_cast(unsigned, hi);
    unsigned lb;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\ts_nop 0\n\t"
        "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\ts_nop 0"
        : "=&v"(lb) : "v"(hb), "v"(x0), "v"(x1));
    lo = __builtin_bit_cast(lp_h2, lb);
}

// The scatter area of a frame: lag rows kLsDS floats apart + a dump row.  kLsDS = 23: with lag = 16 s + j - (4 g + r) and slot
// i = 4 g + r the 64 lanes of a store hit bank (23 j + 8 g + const) mod 32 -- two lanes per bank, the floor for 256 bytes -- where
// the 16-byte aligned stride 20 of round 4 put (j + g) mod 8 classes, i.e. eight lanes, on one bank; entries whose lag is outside
// [0, 24] go to a per-lane dump slot instead of all onto row 25's four addresses (sixteen lanes on one address).  Rows are read
// back as 16-byte accesses at 4-byte alignment.  (round-4 review: lds_conflict_frac 0.49 in this kernel)
constexpr int kLsDS = 23;
constexpr int kLsArea = ((26 * kLsDS + 3) & ~3) + 64;   // floats per frame of a round: 26 rows (25 = never written, read by idle lanes) + dump
typedef float lp_f4a4 __attribute__((ext_vector_type(4), aligned(4)));

// ---- steps of one two-frame round on the matrix pipe (frame u of the round uses scatter area u of dm), in the round's order ----
typedef float lp_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 lp_h8 __attribute__((ext_vector_type(8)));
// the maximum over the wave of each frame's |sample|, left in lane 63: DPP steps within the rows, then across them
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void lp_dpp_fmax2(float (&fmx)[2])
{
#pragma unroll
    for (int u = 0; u < 2; ++u)
        fmx[u] = __builtin_fmaxf(fmx[u], __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(fmx[u]), CTRL, ROW_MASK, 0xf, false)));
}
__device__ __forceinline__ void lp_wave_fmax2(float (&fmx)[2])
{
    lp_dpp_fmax2<0x111, 0xf>(fmx); lp_dpp_fmax2<0x112, 0xf>(fmx); lp_dpp_fmax2<0x114, 0xf>(fmx); lp_dpp_fmax2<0x118, 0xf>(fmx);   // row_shr 1, 2, 4, 8
    lp_dpp_fmax2<0x142, 0xa>(fmx); lp_dpp_fmax2<0x143, 0xc>(fmx);                                                                 // row_bcast 15, 31
}
// the power of two that puts the frame's largest sample in [2^13, 2^14)
__device__ __forceinline__ int lp_frame_shift(float fmx)
{
    const float fmax_all = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fmx), 63));
    int fe = __builtin_amdgcn_frexp_expf(fmax_all);            // fmax_all = m 2^fe, m in [0.5, 1)
    fe = fe < -100 ? -100 : (fe > 100 ? 100 : fe);             // silent frames / denormals: any scale will do
    return 14 - fe;                                            // scaled maximum in [2^13, 2^14)
}
// lane (m, h) = (lane & 31, lane >> 5) adds slots 8 h .. 8 h + 7 of lag m in float64 (rows 25 .. 31 read the spare row) ...
__device__ __forceinline__ double lp_lag_halfsum(const float* dm, int lane)
{
    const int m_ = lane & 31, h_ = lane >> 5;
    const lp_f4a4* row = reinterpret_cast<const lp_f4a4*>(dm + (m_ < kLpcM1 ? m_ : kLpcM1) * kLsDS + 8 * h_);
    const lp_f4 q0 = row[0], q1 = row[1];
    double sm = ((double)q0[0] + (double)q0[1]) + ((double)q0[2] + (double)q0[3]);
    sm += ((double)q1[0] + (double)q1[1]) + ((double)q1[2] + (double)q1[3]);
    return sm;
}
// ... and the halves meet through one cross-half exchange
__device__ __forceinline__ double lp_lag_total(double sm, int lane)
{
    const int lo = __builtin_amdgcn_ds_bpermute(4 * (lane ^ 32), __double2loint(sm));
    const int hi = __builtin_amdgcn_ds_bpermute(4 * (lane ^ 32), __double2hiint(sm));
    const double other = __hiloint2double(hi, lo);
    // the same association on both halves: (slots 0..7) + (slots 8..15)
    return (lane >> 5) == 0 ? sm + other : other + sm;
}
// the 12 matrix entries of each frame to the lane's scatter addresses
__device__ __forceinline__ void lp_round_scatter(float* dm, const int (&addr)[3][4], const lp_f4 (&c1)[2], const lp_f4 (&c2)[2], const lp_f4 (&c3)[2])
{
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dm[u * kLsArea + addr[0][r]] = c1[u][r];
            dm[u * kLsArea + addr[1][r]] = c2[u][r];
            dm[u * kLsArea + addr[2][r]] = c3[u][r];
        }
}
// The nine matrix products of one round's frames: hi hi + hi lo + lo hi of C1, C2, C3, the frames interleaved
__device__ __forceinline__ void lp_round_products(const lp_h8 (&ah)[2], const lp_h8 (&al)[2], const lp_h8 (&bh)[2], const lp_h8 (&bl)[2],
                                                  const lp_h8 (&ch)[2], const lp_h8 (&cl)[2], lp_f4 (&c1)[2], lp_f4 (&c2)[2], lp_f4 (&c3)[2])
{
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        c1[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u], ah[u], c1[u], 0, 0, 0);
        c2[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u], bh[u], c2[u], 0, 0, 0);
        c3[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u], ch[u], c3[u], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        c1[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], al[u], c1[u], 0, 0, 0);
        c2[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], bl[u], c2[u], 0, 0, 0);
        c3[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], cl[u], c3[u], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        c1[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], ah[u], c1[u], 0, 0, 0);
        c2[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], bh[u], c2[u], 0, 0, 0);
        c3[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], ch[u], c3[u], 0, 0, 0);
    }
}

// Frames per work item of a launch that deals items of up to 64 consecutive frames to `grid` waves: 64 fills the lanes of the
// one-frame-per-lane recursion, but e.g. 204 800 frames / 64 = 3200 items are 3.125 per wave of 1024 -- four rounds with the last one
// an eighth full.  Pick the multiple of 4 (<= 64) that makes the item count a whole number of rounds (there 52 frames: 3939 items,
// 3.85 rounds of 13 passes instead of 4 of 16).
inline int lpc24_frames_per_item(long F, long grid)
{
    int fpi = 64;
    if (F > grid * 64) {
        const long rounds = (F + grid * 64 - 1) / (grid * 64);
        long f = (F + rounds * grid - 1) / (rounds * grid);
        f = (f + 3) & ~3L;
        if (f >= 16 && f <= 64) fpi = (int)f;
    }
    return fpi;
}

}  // namespace dsa
