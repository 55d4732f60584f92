// What the kernels of the tuned mel-cepstral family (fft_length 512, cep_order 24, float32) share, whichever unit they are compiled
// in (mcep_mfma.hip, mcep_mfma_bwd.hip, mgcep_step.hip; through f16_split.h the 48 kHz units take the typedefs): the LDS
// carve-up constants of the float32 layout, the quad-layout column-cyclic and 4 x 4 block elimination of the 25 x 25 system with
// their back substitutions, the timing stamps of measurement builds, and the host-side reset of a launch's tile queue.
#pragma once

#include <utility>

#include "common.h"

namespace dsa {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4_u4 __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte access at dword alignment

namespace mm {
constexpr int H = 256, K = 257;   // nfft = 512
constexpr int M1 = 25, M2 = 49;   // cep_order 24
constexpr int KS = 7;             // k-steps of the first product (28 >= M1 coefficients)
constexpr int NR = 7;             // local rows per lane group (ceil(M1 / 4))
constexpr int RS = 68;            // per-frame stride of the rt / rr windows in LDS (floats; 68 % 32 = 4:
                                  // the quad-layout reads of 8 frames x 4 lanes hit 32 distinct banks)
// LDS carve-up (floats)
constexpr int DT_OFF = 0;                       // [16 mt][2 half][64 lane][4]
constexpr int ET_OFF = DT_OFF + 16 * 2 * 64 * 4;  // [3 it][16 mt][64 lane][4 r]
constexpr int E48_OFF = ET_OFF + 3 * 16 * 64 * 4; // [16 mt][4 g][4 r]
constexpr int E256_OFF = E48_OFF + 256;         // [48] + [1] = E[256][0..48]
constexpr int D256_OFF = E256_OFF + 52;         // [28]
constexpr int AV_OFF = D256_OFF + 28;           // [28]
constexpr int WAVE_OFF = AV_OFF + 28;           // per wave: rt [16][RS], rr [16][RS]
constexpr int WAVE_FLOATS = 2 * 16 * RS;
constexpr int LDS_FLOATS = WAVE_OFF + 4 * WAVE_FLOATS;
}  // namespace mm

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

#ifdef DSA_MCEP_TIMING
// Phase stamps of a Newton step (tools/bench_mcep.cpp): the cycle counter goes into SCALAR registers, without a branch (a
// conditional store at every stamp split the step's basic block and with it the instruction schedule being measured); the
// stamps of one (tile, step) are written out by DSA_STAMPS_FLUSH at the end of the step.
__device__ unsigned long long g_mcep_stamps[64];
__device__ unsigned long long g_mcep_slotlog[2048 * 3];   // per wave slot: entry, exit (100 MHz ticks), tiles run
#define DSA_STAMPS_DECL unsigned dsa_st_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define DSA_STAMP(i) dsa_st_[i] = (unsigned)__builtin_readcyclecounter()
#define DSA_STAMPS_FLUSH                                                                \
    do {                                                                               \
        if (blockIdx.x == 0 && threadIdx.x == 0 && tile == 0 && iter == 1)             \
            for (int i_ = 0; i_ < 12; ++i_) g_mcep_stamps[i_] = dsa_st_[i_];            \
    } while (0)
#else
#define DSA_STAMPS_DECL
#define DSA_STAMP(i)
#define DSA_STAMPS_FLUSH
#endif

// Branch-free per-lane selection by lane group: gm[i] is all-ones where g == i (hipcc turns
// nested ?: on lane-dependent conditions into exec-mask control flow; the bit form stays VALU).
struct GroupMask {
    unsigned m[4];
    unsigned gt[4];  // gt[i]: all-ones where g > i
};
__device__ __forceinline__ GroupMask make_group_mask(int g)
{
    GroupMask q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        q.m[i] = g == i ? 0xffffffffu : 0u;
        q.gt[i] = g > i ? 0xffffffffu : 0u;
    }
    return q;
}
__device__ __forceinline__ float sel4(const GroupMask& q, float c0, float c1, float c2, float c3)
{
    unsigned r = (__float_as_uint(c0) & q.m[0]) | (__float_as_uint(c1) & q.m[1]) | (__float_as_uint(c2) & q.m[2]) |
                 (__float_as_uint(c3) & q.m[3]);
    return __uint_as_float(r);
}
__device__ __forceinline__ float keep_if(unsigned mask, float v) { return __uint_as_float(__float_as_uint(v) & mask); }
// 1/x: v_rcp_f32 (1 ulp) + one Newton step
__device__ __forceinline__ float rcp_nr(float x)
{
    float r = __builtin_amdgcn_rcpf(x);
    return r * __builtin_fmaf(-x, r, 2.f);
}

// Reductions over the four lane groups g = lane >> 4 of a frame (lanes n, n + 16, n + 32, n + 48) without the LDS crossbar:
// v_permlane16_swap / v_permlane32_swap (gfx950) exchange the odd 16-lane rows of one register with the even rows of another
// (resp. the upper half of one with the lower half of the other); with both operands holding x the two results are
// (x of the even row | x of the odd row) on both rows of a pair, so one add / max of the pair is x (op) x[lane ^ 16] -- three
// vector instructions and no memory latency, where __shfl_xor is a ds_bpermute_b32 round trip (~100+ cycles on the wave's
// in-order critical path, six of them per Newton step).
__device__ __forceinline__ float rows_sum4(float x)
{
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float rows_max4(float x)
{
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __builtin_fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __builtin_fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
// the same on unsigned values (the bit patterns of non-negative floats order like the floats, with every NaN above them)
__device__ __forceinline__ unsigned rows_maxu4(unsigned x)
{
    auto a = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    x = a[0] > a[1] ? a[0] : a[1];
    auto b = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return b[0] > b[1] ? b[0] : b[1];
}

// value of lane Q of this lane's quad (DPP quad_perm broadcast: a plain VALU move, no LDS)
template <int Q>
__device__ __forceinline__ float quad_bcast(float v)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), Q * 0x55, 0xf, 0xf, true));
}

// ---------------------------------------------------------------------------------------------
// Column-cyclic symmetric elimination in the quad layout.  Lane gs of a quad owns COLUMNS
// j = gs + 4c (c = 0..6) of every row; row i keeps its entries c >= i >> 2 (upper triangle plus at
// most three harmless sub-diagonal ones): 109 registers.  At step k the pivot row's own-column
// entries are already local; only the 24 - k multipliers a[k][i] / a[k][k] (by symmetry elements of
// the pivot ROW) are broadcast, each from the lane that owns column i -- no lane-dependent
// selection anywhere.  Column 25 (lane 1, slot c = 6) carries the right-hand side and column 26
// (lane 2, slot c = 6) an optional second one, so they ride along the row updates for free.
// ---------------------------------------------------------------------------------------------
namespace colm {
using namespace mm;
constexpr int row_len(int i) { return 7 - (i >> 2); }
constexpr int row_off(int i)
{
    int o = 0;
    for (int q = 0; q < i; ++q) o += row_len(q);
    return o;
}
constexpr int TOTAL = row_off(M1);  // 109
}  // namespace colm
#define COL_AT(a, i, c) (a)[colm::row_off(i) + (c) - ((i) >> 2)]

// rt0 / rr0: un-shifted windows of this lane's frame; rhs2: second right-hand side (or nullptr)
template <int i>
__device__ __forceinline__ void col_build_rows(float (&a)[colm::TOTAL], const float* rt0, const float* rr0,
                                               const float* avs, const float* rhs2, int gs, const GroupMask& gq)
{
    using namespace mm;
    if constexpr (i < M1) {
        const float* rt_g = rt0 + gs;
        const float* rr_g = rr0 + 27 - gs;
        // entry (i, j = gs + 4c): R[i][j] + Q[i][j] = rr[27 + i - j] + rt[i + j]  (mcep.py:219-221)
#pragma unroll
        for (int c = i >> 2; c < 6; ++c) COL_AT(a, i, c) = rt_g[i + 4 * c] + rr_g[i - 4 * c];
        const float v24 = rt_g[i + 24] + rr_g[i - 24];   // column 24 exists on lane 0 only
        const float r1 = rt0[i] - avs[i];                // mcep.py:216-217
        const float r2 = rhs2 ? rhs2[i] : 0.f;
        COL_AT(a, i, 6) = sel4(gq, v24, r1, r2, 0.f);
        col_build_rows<i + 1>(a, rt0, rr0, avs, rhs2, gs, gq);
    }
}

// The same rows with slot c = 6 read through two per-lane pointers instead of computed three ways and selected:
// lane 0 of a quad: rt[24 + i] + rr[3 + i] (column 24), lane 1: rt[i] + (-alpha_vec[i]) (the right-hand side), lanes 2, 3:
// 0 + 0 (pa6 / pb6 point at this frame's windows, at the negated alpha table, or at a row of zeros).  Bit-identical to
// col_build_rows with rhs2 = nullptr; 6 instructions fewer per row (the forward kernel is bound by vector issue).
template <int i>
__device__ __forceinline__ void col_build_rows_p(float (&a)[colm::TOTAL], const float* rt0, const float* rr0,
                                                 const float* pa6, const float* pb6, int gs)
{
    using namespace mm;
    if constexpr (i < M1) {
        const float* rt_g = rt0 + gs;
        const float* rr_g = rr0 + 27 - gs;
#pragma unroll
        for (int c = i >> 2; c < 6; ++c) COL_AT(a, i, c) = rt_g[i + 4 * c] + rr_g[i - 4 * c];
        COL_AT(a, i, 6) = pa6[i] + pb6[i];
        col_build_rows_p<i + 1>(a, rt0, rr0, pa6, pb6, gs);
    }
}

// acc += quad_bcast<Q>(s0) * s1 in ONE instruction: the DPP quad_perm broadcast is the src0 modifier
// of v_fmac_f32 (hipcc CSEs builtin DPP moves into separate v_mov_b32_dpp instead of fusing them)
template <int Q>
__device__ __forceinline__ void fmac_quad_bcast(float& acc, float s0, float s1)
{
    if constexpr (Q == 0)
        asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(s0), "v"(s1));
    else if constexpr (Q == 1)
        asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(s0), "v"(s1));
    else if constexpr (Q == 2)
        asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(s0), "v"(s1));
    else
        asm volatile("v_fmac_f32_dpp %0, %1, %2 quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(s0), "v"(s1));
}

template <int k, int i>
__device__ __forceinline__ void col_update_rows(float (&a)[colm::TOTAL], const float (&pneg)[7])
{
    using namespace mm;
    if constexpr (i < M1) {
        // row_i -= (a[k][i] / a[k][k]) row_k.  The multiplier is element i of the pre-scaled pivot row
        // (pneg = -row_k / a[k][k]), which lives on lane i & 3 of the quad
#pragma unroll
        for (int c = i >> 2; c < 7; ++c) fmac_quad_bcast<(i & 3)>(COL_AT(a, i, c), pneg[(i >> 2) - (k >> 2)], COL_AT(a, k, c));
        col_update_rows<k, i + 1>(a, pneg);
    }
}
template <int k>
__device__ __forceinline__ void col_elim_step(float (&a)[colm::TOTAL])
{
    // v_rcp_f32 (1 ulp) without a Newton step: the error of the pivot reciprocal enters the solution like one more rounding
    // of the elimination, and the outer Newton iteration only ever uses the solve for an UPDATE
    const float ninv = -__builtin_amdgcn_rcpf(quad_bcast<(k & 3)>(COL_AT(a, k, k >> 2)));
    float pneg[7];
    constexpr int NP = 7 - (k >> 2);   // entries of the pivot row this lane owns
#pragma unroll
    for (int c = 0; c < 7; ++c) pneg[c] = c < NP ? COL_AT(a, k, (c < NP ? c : 0) + (k >> 2)) * ninv : 0.f;
    // VALU write -> DPP read of pneg needs 2 wait states, which hipcc cannot see inside inline asm; the
    // dummy in/out operands pin the nop after the multiplies.  Only the NP live entries are operands: naming all
    // seven made the compiler materialise the unused tail (a v_mov 0 each: 66 instructions per 25 x 25 system).
    if constexpr (NP == 7)
        asm volatile("s_nop 1" : "+v"(pneg[0]), "+v"(pneg[1]), "+v"(pneg[2]), "+v"(pneg[3]), "+v"(pneg[4]), "+v"(pneg[5]), "+v"(pneg[6]));
    else if constexpr (NP == 6)
        asm volatile("s_nop 1" : "+v"(pneg[0]), "+v"(pneg[1]), "+v"(pneg[2]), "+v"(pneg[3]), "+v"(pneg[4]), "+v"(pneg[5]));
    else if constexpr (NP == 5)
        asm volatile("s_nop 1" : "+v"(pneg[0]), "+v"(pneg[1]), "+v"(pneg[2]), "+v"(pneg[3]), "+v"(pneg[4]));
    else if constexpr (NP == 4)
        asm volatile("s_nop 1" : "+v"(pneg[0]), "+v"(pneg[1]), "+v"(pneg[2]), "+v"(pneg[3]));
    else if constexpr (NP == 3)
        asm volatile("s_nop 1" : "+v"(pneg[0]), "+v"(pneg[1]), "+v"(pneg[2]));
    else if constexpr (NP == 2)
        asm volatile("s_nop 1" : "+v"(pneg[0]), "+v"(pneg[1]));
    else
        asm volatile("s_nop 1" : "+v"(pneg[0]));
    col_update_rows<k, k + 1>(a, pneg);
    // the pivot row stays behind NORMALISED and negated (-row_k / a_kk: a register renaming, no instruction): the back
    // substitution then needs neither the reciprocal nor its broadcast again
#pragma unroll
    for (int c = 0; c < NP; ++c) COL_AT(a, k, c + (k >> 2)) = pneg[c];
}
template <int... Ks>
__device__ __forceinline__ void col_elim_all(float (&a)[colm::TOTAL], std::integer_sequence<int, Ks...>)
{
    (col_elim_step<Ks>(a), ...);
}

// back substitution of right-hand side RHS (1 or 2): xq[c] accumulates x[gs + 4c]; the slot of the
// right-hand-side column is preset to -1 on its owner lane, so  sum_j U[k][j] x_j - b_k  is one dot product
// (the rows arrive as -U[k][.] / U[k][k] from col_elim_step: the dot product is x_k itself)
template <int k>
__device__ __forceinline__ float col_backsub_step(const float (&a)[colm::TOTAL], float (&xq)[mm::KS],
                                                  const GroupMask& gq)
{
    float sl = 0.f;
#pragma unroll
    for (int c = k >> 2; c < 7; ++c) sl = __builtin_fmaf(COL_AT(a, k, c), xq[c], sl);
    sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
    sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0x4E, 0xf, 0xf, true));  // quad_perm [2,3,0,1]
    // rows are normalised and negated by the elimination: sum_j (-U_kj / U_kk) x_j with x_rhs = -1 IS x_k
    const float xk = sl;
    // the owner lane of column k takes xk, the others keep their slot: one v_cndmask_b32 (the slot is still 0 on the owner)
    xq[k >> 2] = gq.m[k & 3] ? xk : xq[k >> 2];
    return xk;
}
template <int... Ks>
__device__ __forceinline__ void col_backsub_all(const float (&a)[colm::TOTAL], float (&xq)[mm::KS],
                                                const GroupMask& gq, std::integer_sequence<int, Ks...>)
{
    ((void)col_backsub_step<mm::M1 - 1 - Ks>(a, xq, gq), ...);
}


// ---------------------------------------------------------------------------------------------
// The same elimination with its rank-1 updates on v_mfma_f32_4x4x1_16b_f32 (round 3).
// One instruction is 16 independent 4 x 4 outer products D_b += A_b (x) B_b, block b = the lanes 4b .. 4b + 3: exactly the
// quad layout -- 16 systems per wave, lane gs of a quad owning the columns gs + 4c.  The matrix is kept as 4 x 4 BLOCKS,
// block (rg, cg) = rows 4 rg .. 4 rg + 3 x columns 4 cg .. 4 cg + 3 as one register quadruple (register i = row 4 rg + i, the
// lane = the column within the group): the C / D operand.  With the pivot row scaled to m = -row_k / a_kk, the update of
// block (rg, cg) is ONE instruction with A = slot rg of m (lane i: the multiplier of row 4 rg + i -- by symmetry that is
// where it already is) and B = slot cg of the unscaled pivot row (lane j: column 4 cg + j): no broadcast, no DPP, no
// wait states, 305 matrix instructions per 25 x 25 system (+ right-hand sides in column group 6) instead of 986
// v_fmac_f32_dpp.  tools/bench_issue.cpp (profiles/r03_issue_calibration*.txt) has the prices: a v_fmac_f32(_dpp) occupies a
// SIMD for 4 cycles (64 multiply-adds), the 4 x 4 x 1 product for 8 (256): twice the multiply-adds per cycle, on the same
// datapath (the float32 products and the vector ALU do NOT overlap, neither within a wave nor across the waves of a SIMD).
// The elimination's arithmetic is the same fmaf(multiplier, pivot-row entry, entry) per element as in the column-cyclic code
// above (rows <= k of the pivot's own row group are kept by zeroing their lanes of A); the back substitution divides by the
// pivot at the end of each row instead of reading pre-scaled rows.
// ---------------------------------------------------------------------------------------------
namespace blk {
constexpr int NG = 7;                                     // row / column groups (28 >= 25 rows, + right-hand sides)
constexpr int NBLK = NG * (NG + 1) / 2;                   // upper-triangular blocks: 28 quadruples = 112 registers
constexpr int at(int rg, int cg) { return rg * NG - rg * (rg - 1) / 2 + (cg - rg); }
}  // namespace blk

__device__ __forceinline__ f32x4 mfma441(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

// rows of R + Q in block layout; slot 6 through the two per-lane pointers of col_build_rows_p (column 24 | right-hand side
// | second right-hand side or zero | zero).  Rows 25 .. 27 are padding: never pivots, never read.  (A set of N = NBLK - 1
// quadruples leaves out block (6, 6): the forward kernels keep row 24 in one register of its own, blk_elim_all_r24.)
template <int rg, int N>
__device__ __forceinline__ void blk_build_rows(f32x4 (&a)[N], const float* rt0, const float* rr0, const float* pa6,
                                               const float* pb6, int gs)
{
    using namespace mm;
    if constexpr (rg < blk::NG && blk::at(rg, rg) < N) {
        const float* rt_g = rt0 + gs;
        const float* rr_g = rr0 + 27 - gs;
#ifndef DSA_BLK_BUILD_SCALAR   // the four rows of a block as ONE 16-byte read per window (dword-aligned) and two packed additions
        // (round 5: half the LDS instructions of the build, the same sums; the forward kernels' last 28 bytes of scratch go with it)
        if constexpr (4 * rg + 3 < M1) {
#pragma unroll
            for (int c = rg; c < 6; ++c)
                a[blk::at(rg, c)] = *reinterpret_cast<const f32x4_u4*>(rt_g + 4 * rg + 4 * c) + *reinterpret_cast<const f32x4_u4*>(rr_g + 4 * rg - 4 * c);
            a[blk::at(rg, 6)] = *reinterpret_cast<const f32x4_u4*>(pa6 + 4 * rg) + *reinterpret_cast<const f32x4_u4*>(pb6 + 4 * rg);
        } else
#endif
        {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * rg + i;
                if (row < M1) {
#pragma unroll
                    for (int c = rg; c < 6; ++c) a[blk::at(rg, c)][i] = rt_g[row + 4 * c] + rr_g[row - 4 * c];
                    a[blk::at(rg, 6)][i] = pa6[row] + pb6[row];
                } else {
                    a[blk::at(rg, 6)][i] = 0.f;
                }
            }
        }
        blk_build_rows<rg + 1>(a, rt0, rr0, pa6, pb6, gs);
    }
}

template <int k, int rg, int N>
__device__ __forceinline__ void blk_update_groups(f32x4 (&a)[N], const float (&m)[blk::NG])
{
    if constexpr (rg < blk::NG && blk::at(rg, rg) < N) {
        // A = the multipliers of rows 4 rg .. 4 rg + 3 (slot rg of the scaled pivot row), B = the pivot row where it stands
#pragma unroll
        for (int c = rg; c < blk::NG; ++c) a[blk::at(rg, c)] = mfma441(m[rg], a[blk::at(k >> 2, c)][k & 3], a[blk::at(rg, c)]);
        blk_update_groups<k, rg + 1>(a, m);
    }
}

// One step.  The pivot row stays in place UNSCALED (writing single elements of the register quadruples makes the compiler
// copy whole quadruples); its scaled copy m = -row_k / a_kk lives for this step only, and the back substitution divides by
// the pivot again (one v_rcp_f32_dpp per row).
template <int k>
__device__ __forceinline__ void blk_elim_step(f32x4 (&a)[blk::NBLK], const GroupMask& gq, float (&ninvs)[mm::M1])
{
    using namespace blk;
    constexpr int c0 = k >> 2, q = k & 3;
    if constexpr (k == mm::M1 - 1) ninvs[k] = -__builtin_amdgcn_rcpf(quad_bcast<q>(a[at(c0, c0)][q]));
    if constexpr (k < mm::M1 - 1) {
        // The vector instructions of a step in ONE run ahead of its matrix instructions: a vector instruction between two
        // 4 x 4 x 1 products costs ~9 cycles on top of its own issue (tools/bench_issue.cpp, "mix" rows), and left alone the
        // scheduler sprinkles the multiplies between the products.
        const float ninv = -__builtin_amdgcn_rcpf(quad_bcast<q>(a[at(c0, c0)][q]));
        ninvs[k] = ninv;
        float m[NG];
#pragma unroll
        for (int c = 0; c < NG; ++c) m[c] = c >= c0 ? a[at(c0, c >= c0 ? c : c0)][q] * ninv : 0.f;
        // the pivot's own row group: rows <= k keep their values (their lanes of A are zero)
        const float m0 = keep_if(gq.gt[q], m[c0]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (q < 3) {
#pragma unroll
            for (int c = c0; c < NG; ++c) a[at(c0, c)] = mfma441(m0, a[at(c0, c)][q], a[at(c0, c)]);
        }
        blk_update_groups<k, c0 + 1>(a, m);
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int... Ks>
__device__ __forceinline__ void blk_elim_all(f32x4 (&a)[blk::NBLK], const GroupMask& gq, float (&ninvs)[mm::M1],
                                             std::integer_sequence<int, Ks...>)
{
    (blk_elim_step<Ks>(a, gq, ninvs), ...);
}

// back substitution over the unscaled rows: x_k = -(sum_{j > k} U_kj x_j - b_k) / U_kk with the right-hand-side slot of xq
// preset to -1 on its owner lane (the diagonal and the sub-diagonal lanes of slot k >> 2 still hold 0 in xq).
// Row group by row group: the sums over the FINISHED column groups (c > rg) of the group's four rows are packed two rows to
// an instruction (a register pair of the quadruple times the broadcast x slot); only the row's own column group, the quad
// reduction and the division are serial.
template <int rg, int N>
__device__ __forceinline__ void blk_backsub_group(const f32x4 (&a)[N], float (&xq)[mm::KS], const GroupMask& gq,
                                                  const float (&ninvs)[mm::M1])
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 p01 = {0.f, 0.f}, p23 = {0.f, 0.f};
#pragma unroll
    for (int c = rg + 1; c < blk::NG; ++c) {
        const f32x4 v = a[blk::at(rg, c)];
        const f2 x = {xq[c], xq[c]};
        p01 = __builtin_shufflevector(v, v, 0, 1) * x + p01;
        if constexpr (4 * rg + 2 < mm::M1) p23 = __builtin_shufflevector(v, v, 2, 3) * x + p23;
    }
    const float part[4] = {p01[0], p01[1], p23[0], p23[1]};
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const int k = 4 * rg + i;
        if (k < mm::M1) {
            float sl = __builtin_fmaf(a[blk::at(rg, rg)][i], xq[rg], part[i]);
            sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
            sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0x4E, 0xf, 0xf, true));  // quad_perm [2,3,0,1]
            const float xk = sl * ninvs[k];   // the negated pivot reciprocals of the elimination (quad-uniform)
            xq[rg] = gq.m[i] ? xk : xq[rg];
        }
    }
}
template <int... Gs>
__device__ __forceinline__ void blk_backsub_all(const f32x4 (&a)[blk::NBLK], float (&xq)[mm::KS], const GroupMask& gq,
                                                const float (&ninvs)[mm::M1], std::integer_sequence<int, Gs...>)
{
    (blk_backsub_group<blk::NG - 1 - Gs>(a, xq, gq, ninvs), ...);
}

// The forward kernels' elimination (one right-hand side).  Bit-identical to blk_elim_all + blk_backsub_all: every element
// still takes the same fmaf(multiplier, pivot-row entry, entry) in the same order, only work on dead lanes goes.
//  - Row 24 is one register r24 (lane 0: column 24, lane 1: the right-hand side, lanes 2, 3: zero -- slot 6 of the row as in
//    the block set) instead of block (6, 6), whose rows 25 .. 27 are padding: its update in each of the steps 0 .. 23 is one
//    vector multiply-add with the multiplier of lane 0 of m[6] instead of a 4 x 4 x 1 product (8 cycles of the float32
//    datapath for 4 + 2 of the broadcast), and the quadruple's three dead registers go.
//  - At q == 2 the only live row of the pivot's own row group is 4 c0 + 3: 7 - c0 vector multiply-adds on element 3 of the
//    group's blocks (the multiplier broadcast from lane 3) instead of 7 - c0 products with three quarters of A zero.
// Both stay in the step's vector run, ahead of its products (a vector instruction between two products costs ~9 cycles).
template <int k>
__device__ __forceinline__ void blk_elim_step_r24(f32x4 (&a)[blk::NBLK - 1], float& r24, const GroupMask& gq,
                                                  float (&ninvs)[mm::M1])
{
    using namespace blk;
    constexpr int c0 = k >> 2, q = k & 3;
    if constexpr (k == mm::M1 - 1) ninvs[k] = -__builtin_amdgcn_rcpf(quad_bcast<0>(r24));
    if constexpr (k < mm::M1 - 1) {
        const float ninv = -__builtin_amdgcn_rcpf(quad_bcast<q>(a[at(c0, c0)][q]));
        ninvs[k] = ninv;
        float m[NG];
#pragma unroll
        for (int c = 0; c < NG; ++c) m[c] = c >= c0 ? a[at(c0, c >= c0 ? c : c0)][q] * ninv : 0.f;
        r24 = __builtin_fmaf(quad_bcast<0>(m[6]), a[at(c0, 6)][q], r24);
        if constexpr (q == 2) {
            const float m3 = quad_bcast<3>(m[c0]);
#pragma unroll
            for (int c = c0; c < NG; ++c) a[at(c0, c)][3] = __builtin_fmaf(m3, a[at(c0, c)][2], a[at(c0, c)][3]);
        }
        const float m0 = keep_if(gq.gt[q], m[c0]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (q < 2) {
#pragma unroll
            for (int c = c0; c < NG; ++c) a[at(c0, c)] = mfma441(m0, a[at(c0, c)][q], a[at(c0, c)]);
        }
        blk_update_groups<k, c0 + 1>(a, m);
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int... Ks>
__device__ __forceinline__ void blk_elim_all_r24(f32x4 (&a)[blk::NBLK - 1], float& r24, const GroupMask& gq,
                                                 float (&ninvs)[mm::M1], std::integer_sequence<int, Ks...>)
{
    (blk_elim_step_r24<Ks>(a, r24, gq, ninvs), ...);
}

// back substitution of blk_elim_all_r24: row 24 (blk_backsub_group<6> with its one live row read from r24), then groups 5 .. 0
template <int... Gs>
__device__ __forceinline__ void blk_backsub_all_r24(const f32x4 (&a)[blk::NBLK - 1], float r24, float (&xq)[mm::KS],
                                                    const GroupMask& gq, const float (&ninvs)[mm::M1],
                                                    std::integer_sequence<int, Gs...>)
{
    float sl = __builtin_fmaf(r24, xq[6], 0.f);
    sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
    sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0x4E, 0xf, 0xf, true));  // quad_perm [2,3,0,1]
    const float x24 = sl * ninvs[mm::M1 - 1];
    xq[6] = gq.m[0] ? x24 : xq[6];
    (blk_backsub_group<blk::NG - 2 - Gs>(a, xq, gq, ninvs), ...);
}

// The same back substitution taking the pivots' reciprocals again instead of reading the 25 kept by the elimination (the
// two-wave backward: 25 registers fewer across the elimination are worth 25 v_rcp_f32 per right-hand side there).
template <int rg>
__device__ __forceinline__ void blk_backsub_group_r(const f32x4 (&a)[blk::NBLK], float (&xq)[mm::KS], const GroupMask& gq)
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 p01 = {0.f, 0.f}, p23 = {0.f, 0.f};
#pragma unroll
    for (int c = rg + 1; c < blk::NG; ++c) {
        const f32x4 v = a[blk::at(rg, c)];
        const f2 x = {xq[c], xq[c]};
        p01 = __builtin_shufflevector(v, v, 0, 1) * x + p01;
        if constexpr (4 * rg + 2 < mm::M1) p23 = __builtin_shufflevector(v, v, 2, 3) * x + p23;
    }
    const float part[4] = {p01[0], p01[1], p23[0], p23[1]};
    const f32x4 d = a[blk::at(rg, rg)];
    const float ninv[4] = {-__builtin_amdgcn_rcpf(quad_bcast<0>(d[0])), -__builtin_amdgcn_rcpf(quad_bcast<1>(d[1])),
                           -__builtin_amdgcn_rcpf(quad_bcast<2>(d[2])), -__builtin_amdgcn_rcpf(quad_bcast<3>(d[3]))};
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        const int k = 4 * rg + i;
        if (k < mm::M1) {
            float sl = __builtin_fmaf(d[i], xq[rg], part[i]);
            sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
            sl += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(sl), 0x4E, 0xf, 0xf, true));  // quad_perm [2,3,0,1]
            const float xk = sl * ninv[i];
            xq[rg] = gq.m[i] ? xk : xq[rg];
        }
    }
}
template <int... Gs>
__device__ __forceinline__ void blk_backsub_all_r(const f32x4 (&a)[blk::NBLK], float (&xq)[mm::KS], const GroupMask& gq,
                                                  std::integer_sequence<int, Gs...>)
{
    (blk_backsub_group_r<blk::NG - 1 - Gs>(a, xq, gq), ...);
}

// `scratch`: DSA_SCRATCH_BYTES of caller-owned device memory; the first two words are this launch's tile counters.
inline unsigned int* reset_queue(void* scratch, hipStream_t st, int words = 2)
{
    if (hipMemsetAsync(scratch, 0, words * sizeof(unsigned int), st) != hipSuccess) return nullptr;
    return (unsigned int*)scratch;
}

}  // namespace dsa
