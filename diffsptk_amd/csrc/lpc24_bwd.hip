// Tuned backward of the order-24 LPC branch for float32, 25 <= frame_length <= 512: lpc24_bwd_kernel on framed rows with its
// launcher (which dsa_lpc_bwd in lpc.hip calls), and the one-launch backward of Frame -> Window -> LPC with its entry
// dsa_frame_window_lpc_bwd.  Phase A of both recomputes the forward's lag sums: the steps in lpc24.h, the rest line for line.
#include "lpc24.h"
#include "lpc_units.h"

namespace dsa {

// ---------------------------------------------------------------------------------------------
// Tuned backward of LinearPredictiveCodingAnalysis for float32 frames, lpc_order 24, 25 <= L <= 512
// (the adjoint of acorr.py:110-120 + levdur.py:113-127 in one launch).  One wave64 per workgroup
// owns 64 consecutive frames:
//   A. lag sums r[0..24] recomputed 4 frames per pass (16 lanes each) exactly as in the forward;
//   B. one frame per LANE, float64, fully unrolled: the Levinson recursion is re-run and carries a
//      general right-hand side along (u = (R + eps I)^{-1} abar, by the order-update with the
//      reversed predictor), then with sbar = Kbar / (2K), v = u - sbar a (because R a = -r_1):
//        rbar[m] = -sum_{|i-j|=m} v_i a_j  (+ sbar a_m - v_m for m >= 1;  + sbar for m = 0);
//   C. xbar[l] = sum_m rbar[m] (x[l+m] + x[l-m]), 4 frames per pass, each lane a contiguous run of
//      samples with the 49-sample window in registers (2 x 625 float64 FMAs per 25 samples), the
//      result staged through LDS and written back as whole rows.
// dynamic LDS: in_buf[4][S] floats (24 zeros | frame | zeros) | out_buf[4][16 C] floats |
//              rbuf[64][25] doubles (r, then rbar) | gbuf[64 * 25] floats (cotangent rows)
template <int... Is>
__device__ __forceinline__ void corr_block_fwd(double (&acc)[kLpcM1], const double (&g)[kLpcM1],
                                               const double (&xw)[2 * kLpcM1 - 1], std::integer_sequence<int, Is...>)
{
    // acc[i] += g[m] * xw[i + m]   (Is = 25 i + m)
    ((acc[Is / kLpcM1] = __builtin_fma(g[Is % kLpcM1], xw[Is / kLpcM1 + Is % kLpcM1], acc[Is / kLpcM1])), ...);
}

template <int... Is>
__device__ __forceinline__ void corr_block_rev(double (&acc)[kLpcM1], const double (&g)[kLpcM1],
                                               const double (&xw)[2 * kLpcM1 - 1], std::integer_sequence<int, Is...>)
{
    // acc[i] += g[m] * xw[24 + i - m]   (xw[24 + i] is the lane's sample i)
    ((acc[Is / kLpcM1] =
          __builtin_fma(g[Is % kLpcM1], xw[kLpcM1 - 1 + Is / kLpcM1 - Is % kLpcM1], acc[Is / kLpcM1])),
     ...);
}

__global__ __launch_bounds__(64, 1) void lpc24_bwd_kernel(const float* __restrict__ gout,
                                                          const float* __restrict__ x, long F, int L, double eps,
                                                          float* __restrict__ gx, long total_sc, int S, int So, int fpi)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* in_buf = reinterpret_cast<float*>(smem_raw);
    float* out_buf = in_buf + 4 * S;
    double* rbuf = reinterpret_cast<double*>(out_buf + 4 * So);
    // the cotangent rows are dead before the output staging starts: they share its buffer when it is large enough
    float* gbuf = 4 * So >= 64 * kLpcM1 ? out_buf : reinterpret_cast<float*>(rbuf + 64 * kLpcM1);
    const int lane = threadIdx.x;
    const int j = lane & 15, fl = lane >> 4;
    const int C = (L + 15) >> 4;
    const int nblk = (C + kLpcM1 - 1) / kLpcM1;
    const bool vec4 = (L & 3) == 0 && ((((size_t)x) | ((size_t)gx)) & 15) == 0;
    for (int l = lane; l < 4 * S; l += 64) in_buf[l] = 0.f;  // the pads stay zero for the whole kernel

    auto stage = [&](long frame0, int nvalid) {
        __syncthreads();
        for (int fr = 0; fr < nvalid; ++fr) {
            const float* src = x + (frame0 + fr) * (long)L;
            float* dst = in_buf + fr * S + (kLpcM1 - 1);
            if (vec4) {
                for (int q = lane; q < (L >> 2); q += 64)
                    reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
            } else {
                for (int t = lane; t < L; t += 64) dst[t] = src[t];
            }
        }
        __syncthreads();
    };

    for (long sc = blockIdx.x; sc < total_sc; sc += gridDim.x) {
        const long fbase = sc * fpi;   // fpi <= 64 frames per work item (see the launcher)
        const int nfr = (int)((F - fbase) < fpi ? (F - fbase) : fpi);
        const int npass = (nfr + 3) >> 2;
        __syncthreads();
        for (int q = lane; q < nfr * kLpcM1; q += 64) gbuf[q] = gout[fbase * kLpcM1 + q];
        // ---- A: lag sums ----
        for (int p = 0; p < npass; ++p) {
            const int nvalid = (nfr - 4 * p) < 4 ? (nfr - 4 * p) : 4;
            stage(fbase + 4 * p, nvalid);
            double acc[kLpcM1];
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) acc[m] = 0.0;
            const float* fsrc = in_buf + fl * S + (kLpcM1 - 1);
            for (int blk = 0; blk < nblk; ++blk) {
                const int t0 = j * C + blk * kLpcM1;
                const int own = C - blk * kLpcM1;
                double xw[2 * kLpcM1 - 1];
#pragma unroll
                for (int i = 0; i < 2 * kLpcM1 - 1; ++i) xw[i] = (double)fsrc[t0 + i];
                if (own >= kLpcM1) {
                    lag_block(acc, xw, std::make_integer_sequence<int, kLpcM1 * kLpcM1>{});
                } else {
#pragma unroll
                    for (int i = 0; i < kLpcM1; ++i) {
                        const double li = i < own ? xw[i] : 0.0;
#pragma unroll
                        for (int m = 0; m < kLpcM1; ++m) acc[m] = __builtin_fma(li, xw[i + m], acc[m]);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) {
                acc[m] = row16_allsum(acc[m]);
            }
            if (fl < nvalid) {
                double* rrow = rbuf + (size_t)(4 * p + fl) * kLpcM1;
#pragma unroll
                for (int m = 0; m < kLpcM1; ++m)
                    if ((m & 15) == j) rrow[m] = acc[m];
            }
        }
        __syncthreads();
        // ---- B: adjoint of the Yule-Walker solve, one frame per lane ----
        if (lane < nfr) {
            double r[kLpcM1], a[kLpcM1], u[kLpcM1];
            double* row = rbuf + (size_t)lane * kLpcM1;
            const float* go = gbuf + lane * kLpcM1;
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) {
                r[m] = row[m];
                a[m] = 0.0;
                u[m] = 0.0;
            }
            double Ecur = r[0] + eps;
#pragma unroll
            for (int m = 1; m < kLpcM1; ++m) {
                // order update of the general solve with the order-(m-1) predictor and its error
                double d = (double)go[m];
#pragma unroll
                for (int q = 1; q < m; ++q) d = __builtin_fma(-r[m - q], u[q], d);
                const double mu = d / Ecur;
#pragma unroll
                for (int q = 1; q < m; ++q) u[q] = __builtin_fma(mu, a[m - q], u[q]);
                u[m] = mu;
                // Levinson step (as in the forward kernels)
                double s = r[m];
#pragma unroll
                for (int q = 1; q < m; ++q) s = __builtin_fma(a[q], r[m - q], s);
                levinson24_step(a, m, s, Ecur);
            }
            double gsum = r[0];
#pragma unroll
            for (int m = 1; m < kLpcM1; ++m) gsum = __builtin_fma(r[m], a[m], gsum);
            levinson24_adjoint_tail((double)go[0], gsum, a, u, [&](int m, double rbar) __attribute__((always_inline)) { row[m] = rbar; });
        }
        __syncthreads();
        // ---- C: adjoint of the lag sums ----
        for (int p = 0; p < npass; ++p) {
            const int nvalid = (nfr - 4 * p) < 4 ? (nfr - 4 * p) : 4;
            stage(fbase + 4 * p, nvalid);
            double g[kLpcM1];
            {
                const double* grow = rbuf + (size_t)(4 * p + (fl < nvalid ? fl : 0)) * kLpcM1;
#pragma unroll
                for (int m = 0; m < kLpcM1; ++m) g[m] = grow[m];
            }
            const float* fsrc = in_buf + fl * S + (kLpcM1 - 1);
            float* odst = out_buf + fl * So;
            for (int blk = 0; blk < nblk; ++blk) {
                const int t0 = j * C + blk * kLpcM1;
                const int own = C - blk * kLpcM1;
                double acc[kLpcM1];
#pragma unroll
                for (int i = 0; i < kLpcM1; ++i) acc[i] = 0.0;
                {
                    double xw[2 * kLpcM1 - 1];
#pragma unroll
                    for (int i = 0; i < 2 * kLpcM1 - 1; ++i) xw[i] = (double)fsrc[t0 + i];
                    corr_block_fwd(acc, g, xw, std::make_integer_sequence<int, kLpcM1 * kLpcM1>{});
                }
                {
                    double xw[2 * kLpcM1 - 1];
#pragma unroll
                    for (int i = 0; i < 2 * kLpcM1 - 1; ++i) xw[i] = (double)fsrc[t0 - (kLpcM1 - 1) + i];
                    corr_block_rev(acc, g, xw, std::make_integer_sequence<int, kLpcM1 * kLpcM1>{});
                }
                if (own >= kLpcM1) {
#pragma unroll
                    for (int i = 0; i < kLpcM1; ++i) odst[t0 + i] = (float)acc[i];
                } else {
#pragma unroll
                    for (int i = 0; i < kLpcM1; ++i)
                        if (i < own) odst[t0 + i] = (float)acc[i];
                }
            }
            __syncthreads();
            for (int fr = 0; fr < nvalid; ++fr) {
                float* dst = gx + (fbase + 4 * p + fr) * (long)L;
                const float* src = out_buf + fr * So;
                if (vec4) {
                    for (int q = lane; q < (L >> 2); q += 64)
                        reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
                } else {
                    for (int t = lane; t < L; t += 64) dst[t] = src[t];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Round 5: backward of the fused Frame -> Window -> LPC launch in ONE launch (the adjoint of frame.py:120-141, window.py:185-193,
// acorr.py:110-120 and levdur.py:113-127 composed; README.md:198-201 of the reference with a gradient).  The module chain ran it as
// lpc24_bwd (0.71 ms per 204 800 frames: 1875 v_fma_f64 per four frames at one wave per SIMD behind synchronous stagings) + window
// and frame backward over two materialised (F, 400) tensors.  Here a wave owns a run of Hc hops of one utterance -- the output
// samples [h0 P, (h0 + Hc) P) -- and every frame that touches them (Hc + 4..5 frames at L = 400, P = 80: the halo is recomputed,
// nothing is exchanged between waves, and every sample's sum runs over its frames in increasing order whatever the partition:
// bit-identical for every Hc):
//   A. lag sums of every frame as the forward kernel forms them (banded Gram product of binary16 splits on the matrix pipe, the
//      16 entries of a lag added in float64) -> rbuf;
//   B. one frame per LANE, float64, fully unrolled: the Levinson recursion re-run with a general right-hand side riding along
//      (as lpc24_bwd_kernel) -> the cotangent of the lag sums rbar[0..24], left in the frame's row as float32 scaled by a power of
//      two (its largest entry in [2^13, 2^14));
//   C. the adjoint of the lag sums  xwbar[l] = sum_m rbar[m] (xw[l + m] + xw[l - m])  -- a 49-tap symmetric filter per frame -- as a
//      banded matrix product on the binary16 matrix pipe: with u_c the c-th block of 16 windowed samples and E[q] = ext[q - 32]
//      (ext[m] = rbar[|m|], doubled at 0), block c of xwbar is  sum_{s=-2..2} T_s u_{c+s},  (T_s)[i][j] = E[16 s + 32 + j - i]:
//      A operand (16 x 96) = the Toeplitz band, row i = 8 consecutive taps from E[k - i] (a 16-byte LDS read at a 2-byte
//      aligned address: gfx950 takes unaligned DS accesses), B operand (96 x 16) = column c = samples 16 c - 32 + k (aligned),
//      3 k-steps x 2 column tiles x 3 split terms = 18 v_mfma_f32_16x16x32_f16 per frame instead of 1250 v_fma_f64 per 25
//      samples and lane.  The result layout gives lane (c, g) the four consecutive samples 16 c + 4 g .. + 3: times the window,
//      scale undone, added into the wave's overlap-add stretch in LDS (one 16-byte read-modify-write per tile and lane; frames in
//      increasing order); the own range of the stretch goes to gx as whole rows at the end.
// dynamic LDS per workgroup (one wave): rbuf[nfr_max][26] doubles | stretch[(nfr_max - 1) P + 512] floats |
//   area shared by phase A (scatter rows dm[2][26][23] floats) and phase C (XH[640] XL[640] EH[128] EL[128] binary16)
typedef _Float16 lp_h8u __attribute__((ext_vector_type(8), aligned(2)));
typedef float lp_f4u __attribute__((ext_vector_type(4), aligned(4)));
constexpr int kLbRow = 26;          // doubles per frame row of rbuf: 25 lag sums (then: 25 scaled taps as floats, their shift) | the samples' shift
constexpr int kLbRing = 1024;       // floats of the overlap-add ring (frame_length + frame_period <= 1024)
constexpr int kLbOps = 2 * 640 + 2 * 128;   // binary16 values of one operand set of phase C: XH | XL | EH | EL
constexpr int kLbAreaBytes = 2 * kLbOps * 2 > 2 * kLsArea * 4 ? 2 * kLbOps * 2 : 2 * kLsArea * 4;
__host__ __device__ inline long lb_floordiv(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

template <int LC>
__global__ __launch_bounds__(64, 2) void frame_window_lpc24_bwd_mfma_kernel(
    const float* __restrict__ gout, const float* __restrict__ x, long Tlen, long N, int L_rt, int P, int left,
    const float* __restrict__ w, double eps, float* __restrict__ gx, long total_items, int items_per_utt, int Hc, int nfr_max)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef unsigned lp_u4 __attribute__((ext_vector_type(4)));
    constexpr int DS = kLsDS;
    extern __shared__ __attribute__((aligned(16))) unsigned char lb_smem[];
    const int L = LC ? LC : L_rt;
    const int lane = threadIdx.x;
    double* rbuf = reinterpret_cast<double*>(lb_smem);
    float* ring = reinterpret_cast<float*>(rbuf + nfr_max * kLbRow);
    float* dm = ring + kLbRing;
    // phase C operand arrays, one set per frame of a round (u), over phase A's scatter rows: per set XH | XL [32 zeros | 512 samples |
    // 96 zeros] and EH | EL (E[q] at q + 16, q in [-16, 112)), set stride kLbOps halves
    _Float16* XH = reinterpret_cast<_Float16*>(dm);
    _Float16* XL = XH + 640;
    _Float16* EH = XL + 640;
    _Float16* EL = EH + 128;
    const int j = lane & 15, g = lane >> 4;
    // ---- per-lane constants ----
    float wa[8];    // phase A: element e of lane (j, g) is sample 128 g + 16 e + j
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int la = 128 * g + 16 * e + j;
        wa[e] = la < L ? (w ? w[la] : 1.f) : 0.f;
    }
    float wc[8];    // phase C input: samples 8 lane .. 8 lane + 7
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int la = 8 * lane + e;
        wc[e] = la < L ? (w ? w[la] : 1.f) : 0.f;
    }
    float wo[2][4]; // phase C output: samples 16 (16 nt + j) + 4 g + r
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int la = 16 * (16 * nt + j) + 4 * g + r;
            wo[nt][r] = la < L ? (w ? w[la] : 1.f) : 0.f;
        }
    int addr[3][4];
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * g + r, lag = 16 * s_ + j - i;
            addr[s_][r] = (lag >= 0 && lag < kLpcM1) ? lag * DS + i : kLsArea - 64 + lane;
        }

    for (int q = lane; q < kLbRing / 4; q += 64) reinterpret_cast<f4*>(ring)[q] = f4{0.f, 0.f, 0.f, 0.f};   // (every flush leaves its slots zero)
    for (long item = blockIdx.x; item < total_items; item += gridDim.x) {
        const long b = item / items_per_utt;
        const long h0 = (item - b * items_per_utt) * Hc;
        const long s0 = h0 * P;
        long s1 = s0 + (long)Hc * P;
        if (s1 > Tlen) s1 = Tlen;
        if (s0 >= s1) continue;
        long n_lo = lb_floordiv(s0 + left - L, P) + 1;
        long n_hi = lb_floordiv(s1 - 1 + left, P);
        if (n_lo < 0) n_lo = 0;
        if (n_hi > N - 1) n_hi = N - 1;
        const int nfr = (int)(n_hi - n_lo + 1);       // <= nfr_max (host); may be <= 0 when no frame reaches the range (L < P)
        const float* xb = x + b * Tlen;
        __builtin_amdgcn_wave_barrier();
#ifndef LPB_ABL
#define LPB_ABL 0   // measurement builds only: 1 no lag sums, 2 no recursion, 4 no filter / overlap-add, 8 taps read at an aligned address,
                    // 16 no ring update / flush, 32 no matrix products
#endif
        // ================= A: lag sums (the forward kernel's rounds of two frames) =================
        if (nfr > 0 && !(LPB_ABL & 1)) {
            constexpr int U = 2;
            float a[U][8];
            const int soff = 128 * g + j;
            auto fetch = [&](int u, int fi) __attribute__((always_inline)) {
                const long start = (n_lo + fi) * P - left;
                if (start >= 0 && start + 512 <= Tlen) {
                    const float* src = xb + start + soff;
#pragma unroll
                    for (int e = 0; e < 8; ++e) a[u][e] = src[16 * e];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const long si = start + soff + 16 * e;
                        a[u][e] = (soff + 16 * e < L && si >= 0 && si < Tlen) ? xb[si] : 0.f;
                    }
                }
            };
            fetch(0, 0);
            fetch(1, 1 < nfr ? 1 : 0);
            for (int fi = 0; fi < nfr; fi += U) {
                float va[U][8];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int e = 0; e < 8; ++e) va[u][e] = soff + 16 * e < L ? a[u][e] * wa[e] : 0.f;
                if (fi + U < nfr) {
                    fetch(0, fi + U);
                    fetch(1, fi + U + 1 < nfr ? fi + U + 1 : fi + U);
                }
                float fmx[U];
                int sh[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    fmx[u] = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) fmx[u] = __builtin_fmaxf(fmx[u], __builtin_fabsf(va[u][e]));
                }
                lp_wave_fmax2(fmx);
#pragma unroll
                for (int u = 0; u < U; ++u) sh[u] = lp_frame_shift(fmx[u]);
                lp_h8 ah[U], al[U], bh[U], bl[U], ch[U], cl[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    lp_u4 hr, lr;
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        lp_h2 h, l;
                        lp_split2(__builtin_ldexpf(va[u][e], sh[u]), __builtin_ldexpf(va[u][e + 1], sh[u]), h, l);
                        hr[e >> 1] = __builtin_bit_cast(unsigned, h);
                        lr[e >> 1] = __builtin_bit_cast(unsigned, l);
                    }
                    unsigned nh = (unsigned)__builtin_amdgcn_ds_bpermute(4 * ((lane + 16) & 63), (int)hr[0]);
                    unsigned nl = (unsigned)__builtin_amdgcn_ds_bpermute(4 * ((lane + 16) & 63), (int)lr[0]);
                    nh = g == 3 ? 0u : nh;
                    nl = g == 3 ? 0u : nl;
                    const lp_u4 bhr = {__builtin_amdgcn_alignbit(hr[1], hr[0], 16), __builtin_amdgcn_alignbit(hr[2], hr[1], 16),
                                       __builtin_amdgcn_alignbit(hr[3], hr[2], 16), __builtin_amdgcn_alignbit(nh, hr[3], 16)};
                    const lp_u4 blr = {__builtin_amdgcn_alignbit(lr[1], lr[0], 16), __builtin_amdgcn_alignbit(lr[2], lr[1], 16),
                                       __builtin_amdgcn_alignbit(lr[3], lr[2], 16), __builtin_amdgcn_alignbit(nl, lr[3], 16)};
                    const lp_u4 chr = {hr[1], hr[2], hr[3], nh}, clr = {lr[1], lr[2], lr[3], nl};
                    ah[u] = __builtin_bit_cast(lp_h8, hr);
                    al[u] = __builtin_bit_cast(lp_h8, lr);
                    bh[u] = __builtin_bit_cast(lp_h8, bhr);
                    bl[u] = __builtin_bit_cast(lp_h8, blr);
                    ch[u] = __builtin_bit_cast(lp_h8, chr);
                    cl[u] = __builtin_bit_cast(lp_h8, clr);
                }
                f4 c1[U], c2[U], c3[U];
#pragma unroll
                for (int u = 0; u < U; ++u) c1[u] = c2[u] = c3[u] = f4{0.f, 0.f, 0.f, 0.f};
                lp_round_products(ah, al, bh, bl, ch, cl, c1, c2, c3);
                __builtin_amdgcn_wave_barrier();
                lp_round_scatter(dm, addr, c1, c2, c3);
                __builtin_amdgcn_wave_barrier();
                {
                    double sm[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) sm[u] = lp_lag_halfsum(dm + u * kLsArea, lane);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double tot = lp_lag_total(sm[u], lane);
                        if (lane < kLpcM1 && fi + u < nfr) rbuf[(fi + u) * kLbRow + lane] = ldexp(tot, -2 * sh[u]);
                        if (lane == kLpcM1 && fi + u < nfr) rbuf[(fi + u) * kLbRow + kLpcM1] = (double)sh[u];   // the samples' shift, for phase C
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ================= B: adjoint of the Yule-Walker solve, one frame per lane (as lpc24_bwd_kernel) =================
        // (the lag sums stay in the frame's LDS row and are read where the recursion wants them: a, u in registers are 100 of them
        //  instead of 150, and three waves share a SIMD)
        if (lane < nfr && !(LPB_ABL & 2)) {
            double a[kLpcM1], u[kLpcM1];
            double* row = rbuf + (size_t)lane * kLbRow;
            const float* go = gout + (b * N + n_lo + lane) * (long)kLpcM1;
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) {
                a[m] = 0.0;
                u[m] = 0.0;
            }
            const double r0 = row[0];
            double Ecur = r0 + eps;
#pragma unroll
            for (int m = 1; m < kLpcM1; ++m) {
                double d = (double)go[m];
                double s = row[m];
#pragma unroll
                for (int q = 1; q < m; ++q) {
                    const double rv = row[m - q];
                    d = __builtin_fma(-rv, u[q], d);
                    s = __builtin_fma(a[q], rv, s);
                }
                const double mu = d / Ecur;
#pragma unroll
                for (int q = 1; q < m; ++q) u[q] = __builtin_fma(mu, a[m - q], u[q]);
                u[m] = mu;
                levinson24_step(a, m, s, Ecur);
            }
            double gsum = r0;
#pragma unroll
            for (int m = 1; m < kLpcM1; ++m) gsum = __builtin_fma(row[m], a[m], gsum);
            // the taps ext[m] = rbar[m] (doubled at 0: the lag-0 sum's adjoint is 2 rbar[0] xw[l]) over the dead lag sums, as float64
            double mx = 0.0;
            levinson24_adjoint_tail((double)go[0], gsum, a, u, [&](int m, double rbar) __attribute__((always_inline)) {
                if (m == 0) rbar += rbar;
                row[m] = rbar;
                mx = fmax(mx, fabs(rbar));
            });
            // ... then in place as float32 scaled by 2^she (largest in [2^13, 2^14)): float m lies inside doubles <= m / 2, all read by
            // then.  A non-finite cotangent keeps the shift 0 and poisons its own frame only.
            int fe = 0;
            const bool okmx = mx > 0.0 && mx < 1e300;
            if (okmx) (void)frexp(mx, &fe);
            const int she = okmx ? 14 - fe : 0;
            float* frow = reinterpret_cast<float*>(row);
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) {
                const double tv = row[m];
                asm volatile("" ::: "memory");
                frow[m] = (float)ldexp(tv, she);
            }
            reinterpret_cast<int*>(frow)[kLpcM1] = she;
        }
        __builtin_amdgcn_wave_barrier();
        // ================= C: the 49-tap filter of every frame on the matrix pipe, overlap-add in a ring in LDS =================
        // Two frames per round (their chains share nothing and interleave).  The overlap-add runs in a ring of kLbRing floats:
        // position q of the item's stretch (sample n_lo P - left + q) lives at q mod kLbRing; after frame fi's contribution the
        // P positions [fi P, (fi + 1) P) are final -- no later frame reaches them -- and go to gx (own range only), their slots back to zero.
        for (int q = lane; q < 2 * kLbOps * 2 / 16; q += 64) reinterpret_cast<f4*>(dm)[q] = f4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_wave_barrier();
        {
            const long base = n_lo * P - left;        // sample of stretch position 0
            float* gxb = gx + b * Tlen;
            const bool vec = (P & 3) == 0;
            auto flush = [&](long q0, int cnt) __attribute__((always_inline)) {   // positions [q0, q0 + cnt) -> gx, slots zeroed
                if (vec && (((size_t)(gxb + base + q0)) & 15) == 0 && (cnt & 3) == 0) {
                    for (int t = 4 * lane; t < cnt; t += 256) {
                        f4* slot = reinterpret_cast<f4*>(ring + ((q0 + t) & (kLbRing - 1)));
                        const f4 v = *slot;
                        *slot = f4{0.f, 0.f, 0.f, 0.f};
                        const long sidx = base + q0 + t;
                        if (sidx >= s0 && sidx + 3 < s1) *reinterpret_cast<f4*>(gxb + sidx) = v;
                        else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (sidx + r >= s0 && sidx + r < s1) gxb[sidx + r] = v[r];
                        }
                    }
                } else {
                    for (int t = lane; t < cnt; t += 64) {
                        float* slot = ring + ((q0 + t) & (kLbRing - 1));
                        const float v = *slot;
                        *slot = 0.f;
                        const long sidx = base + q0 + t;
                        if (sidx >= s0 && sidx < s1) gxb[sidx] = v;
                    }
                }
            };
            constexpr int U = 2;
            float c8[U][8];
            // this lane's band offset into the taps (lane-constant), as the dword that holds its first tap + a funnel shift
            typedef unsigned lp_u4a4 __attribute__((ext_vector_type(4), aligned(4)));
            const int eoff = 16 + 8 * g - j;                 // >= 1
            const unsigned* etap = reinterpret_cast<const unsigned*>(EH) + (eoff >> 1);
            const unsigned esh = (eoff & 1) ? 16u : 0u;
            auto fetchc = [&](int u, int fi) __attribute__((always_inline)) {
                const long start = (n_lo + fi) * P - left;
                if (start >= 0 && start + 512 <= Tlen) {
                    const lp_f4u* src = reinterpret_cast<const lp_f4u*>(xb + start + 8 * lane);
                    const lp_f4u q0 = src[0], q1 = src[1];
                    c8[u][0] = q0[0]; c8[u][1] = q0[1]; c8[u][2] = q0[2]; c8[u][3] = q0[3];
                    c8[u][4] = q1[0]; c8[u][5] = q1[1]; c8[u][6] = q1[2]; c8[u][7] = q1[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const long si = start + 8 * lane + e;
                        c8[u][e] = (8 * lane + e < L && si >= 0 && si < Tlen) ? xb[si] : 0.f;
                    }
                }
            };
            const int nfr_c = (LPB_ABL & 4) ? 0 : nfr;
            if (nfr_c > 0) {
                fetchc(0, 0);
                fetchc(1, 1 < nfr_c ? 1 : 0);
            }
            for (int fi = 0; fi < nfr_c; fi += U) {
                int back[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int fu = fi + u < nfr_c ? fi + u : fi;    // (an odd count: the round's second frame is its first again, never added)
                    const double* row = rbuf + (size_t)fu * kLbRow;
                    const float* frow = reinterpret_cast<const float*>(row);
                    const int shx = (int)row[kLpcM1];
                    const int she = reinterpret_cast<const int*>(frow)[kLpcM1];
                    back[u] = -(shx + she);
                    // windowed samples 8 lane .. 8 lane + 7, scaled and split, one 16-byte store per half
                    lp_u4 hr, lr;
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        const float v0 = 8 * lane + e < L ? c8[u][e] * wc[e] : 0.f, v1 = 8 * lane + e + 1 < L ? c8[u][e + 1] * wc[e + 1] : 0.f;
                        lp_h2 h, l;
                        lp_split2(__builtin_ldexpf(v0, shx), __builtin_ldexpf(v1, shx), h, l);
                        hr[e >> 1] = __builtin_bit_cast(unsigned, h);
                        lr[e >> 1] = __builtin_bit_cast(unsigned, l);
                    }
                    *reinterpret_cast<lp_u4*>(XH + u * kLbOps + 32 + 8 * lane) = hr;
                    *reinterpret_cast<lp_u4*>(XL + u * kLbOps + 32 + 8 * lane) = lr;
                    // taps: E[q], q = 8 + lane (lanes 0 .. 48) = ext[lane - 24] = the row's entry |lane - 24|
                    if (lane < 2 * kLpcM1 - 1) {
                        const int m = lane < kLpcM1 - 1 ? kLpcM1 - 1 - lane : lane - (kLpcM1 - 1);
                        const float tv = frow[m];
                        const _Float16 th = (_Float16)tv;
                        EH[u * kLbOps + 16 + 8 + lane] = th;
                        EL[u * kLbOps + 16 + 8 + lane] = (_Float16)(tv - (float)th);
                    }
                }
                if (fi + U < nfr_c) {
                    fetchc(0, fi + U);
                    fetchc(1, fi + U + 1 < nfr_c ? fi + U + 1 : fi + U);
                }
                __builtin_amdgcn_wave_barrier();
                lp_h8 eh[U][3], el[U][3];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        // eight taps from band offset 32 t + 8 g - j: read as FIVE aligned dwords from the dword that holds the first one
                        // and funnel-shifted by 0 / 16 bits (lanes j, j + 1 then read the same dwords -- a broadcast -- where the
                        // 2-byte aligned 16-byte read of the first version cost the launch 0.07 of 0.34 ms: ablations LPB_ABL 8 / 64 / 128)
                        const unsigned* eph = etap + (u * kLbOps + 32 * t) / 2;
                        const unsigned* epl = eph + 64;
                        const lp_u4a4 hq = *reinterpret_cast<const lp_u4a4*>(eph), lq = *reinterpret_cast<const lp_u4a4*>(epl);
                        const unsigned h4 = eph[4], l4 = epl[4];
                        const lp_u4 hs = {__builtin_amdgcn_alignbit(hq[1], hq[0], esh), __builtin_amdgcn_alignbit(hq[2], hq[1], esh),
                                          __builtin_amdgcn_alignbit(hq[3], hq[2], esh), __builtin_amdgcn_alignbit(h4, hq[3], esh)};
                        const lp_u4 ls = {__builtin_amdgcn_alignbit(lq[1], lq[0], esh), __builtin_amdgcn_alignbit(lq[2], lq[1], esh),
                                          __builtin_amdgcn_alignbit(lq[3], lq[2], esh), __builtin_amdgcn_alignbit(l4, lq[3], esh)};
                        eh[u][t] = __builtin_bit_cast(lp_h8, hs);
                        el[u][t] = __builtin_bit_cast(lp_h8, ls);
                    }
                f4 acc[U][2];
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u][0] = acc[u][1] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    lp_h8 xh[U][2], xl[U][2];
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) {
                            const int off = u * kLbOps + 16 * (16 * nt + j) + 32 * t + 8 * g;   // (+ 32 of padding, - 32 of the band's reach)
                            xh[u][nt] = *reinterpret_cast<const lp_h8*>(XH + off);
                            xl[u][nt] = *reinterpret_cast<const lp_h8*>(XL + off);
                        }
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) acc[u][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(el[u][t], xh[u][nt], acc[u][nt], 0, 0, 0);
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) acc[u][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(eh[u][t], xl[u][nt], acc[u][nt], 0, 0, 0);
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) acc[u][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(eh[u][t], xh[u][nt], acc[u][nt], 0, 0, 0);
                }
                // lane (c, g): samples 16 c + 4 g + r of the frame; times the window (zero past the frame), scale undone; frames in order
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (fi + u < nfr_c && !(LPB_ABL & 16)) {
                        const long q0 = (long)(fi + u) * P;
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) {
                            const int l0 = 16 * (16 * nt + j) + 4 * g;
                            if (vec) {
                                f4* slot = reinterpret_cast<f4*>(ring + ((q0 + l0) & (kLbRing - 1)));
                                f4 cur = *slot;
#pragma unroll
                                for (int r = 0; r < 4; ++r)   // (selected, not multiplied, past the frame: a non-finite frame stays inside its own samples)
                                    cur[r] += wo[nt][r] != 0.f ? __builtin_ldexpf(acc[u][nt][r], back[u]) * wo[nt][r] : 0.f;
                                *slot = cur;
                            } else {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    ring[(q0 + l0 + r) & (kLbRing - 1)] += wo[nt][r] != 0.f ? __builtin_ldexpf(acc[u][nt][r], back[u]) * wo[nt][r] : 0.f;
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                        flush(q0, P);
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
            // what the last frame left beyond its first P positions (all zeros when there was no frame)
            if (nfr_c > 0) flush((long)nfr_c * P, 512 > P ? 512 - P : 0);
            // samples of the own range that no frame reaches (frame_period > frame_length, or no frame at all): zero gradient
            {
                const long covered_lo = nfr_c > 0 ? base : s1, covered_hi = nfr_c > 0 ? base + (long)(nfr_c - 1) * P + 512 : s1;
                for (long sidx = s0 + lane; sidx < s1; sidx += 64)
                    if (sidx < covered_lo || sidx >= covered_hi) gxb[sidx] = 0.f;
            }
        }
    }
}

// launcher of lpc24_bwd_kernel
int lpc24_bwd(const void* gout, const void* x, int64_t F, int L, double eps, void* gx, hipStream_t st)
{
    const int C = (L + 15) >> 4, nblk = (C + kLpcM1 - 1) / kLpcM1;
    const int S = (2 * (kLpcM1 - 1) + 15 * C + kLpcM1 * nblk + 4 + 3) & ~3;  // 24 | reach of the last lane | 24
    const int So = (16 * C + 3) & ~3;
    size_t lds_t = (size_t)(4 * S + 4 * So) * 4 + 64 * kLpcM1 * sizeof(double) +
                   (4 * So >= 64 * kLpcM1 ? 0 : 64 * kLpcM1 * sizeof(float));
    long grid = 256L * 4;   // 280 registers: one wave per SIMD (a 256-register build spills and is slower)
    const int fpi = lpc24_frames_per_item((long)F, grid);   // 64 fills phase B's lanes
    long total_sc = (long)((F + fpi - 1) / fpi);
    if (grid > total_sc) grid = total_sc;
    hipLaunchKernelGGL(lpc24_bwd_kernel, dim3((unsigned)grid), dim3(64), lds_t, st,
                       (const float*)gout, (const float*)x, (long)F, L, eps, (float*)gx, total_sc, S, So, fpi);
    return check_launch("lpc24_bwd");
}

}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_frame_window_lpc_bwd(const void* gout, const void* x, int64_t B, int64_t T, int32_t L, int32_t P, const void* w,
                                        int32_t center, int32_t pad_mode, int32_t M, double eps, int32_t dtype, void* gx, void* stream)
{
    DSA_REQUIRE(L > 0 && P > 0 && T > 0 && B >= 0 && M >= 0 && M < L && eps >= 0, "frame_window_lpc_bwd: invalid sizes");
    const int64_t N = dsa_num_frames(T, P);
    if (B * N == 0) return DSA_OK;
    DSA_REQUIRE(gout && x && gx, "frame_window_lpc_bwd: null pointer");
    if (!(dtype == DSA_F32 && M == 24 && L >= 25 && L <= 512 && pad_mode == DSA_PAD_CONSTANT))
        return fail(DSA_ERR_UNSUPPORTED, "frame_window_lpc_bwd: the one-launch backward covers float32, lpc_order 24, 25 <= frame_length <= 512, constant padding%s");
    const int left = center ? L / 2 : 0;
    // frames that touch a run of Hc hops: Hc + halo, each a lane of phase B; the overlap-add ring holds frame_length + frame_period
    if (L + P > kLbRing) return fail(DSA_ERR_UNSUPPORTED, "frame_window_lpc_bwd: frame_length + frame_period above 1024%s");
    const long halo = lb_floordiv(left - 1, P) - lb_floordiv(left - L, P);
    long Hc = 64 - halo;
    if (Hc > N) Hc = N;
    if (Hc < 1 || halo > 48)
        return fail(DSA_ERR_UNSUPPORTED, "frame_window_lpc_bwd: this frame_length / frame_period pair does not fit the one-launch backward%s");
    // runs of about 40 hops: LDS for nine waves per CU (the lag-sum rows are 208 bytes per frame) against 5 halo frames per run
    if (Hc > 40 && halo <= 8) Hc = 40;
    long ipu = (N + Hc - 1) / Hc;
    Hc = (N + ipu - 1) / ipu;                      // equal runs per utterance
    const int nfr_max = (int)(Hc + halo);
    const size_t lds = (size_t)nfr_max * kLbRow * sizeof(double) + (size_t)kLbRing * 4 + kLbAreaBytes;
    const long total = (long)B * ipu;
    long per_cu = (long)(160 * 1024 / lds);
    if (per_cu > 8) per_cu = 8;                    // two waves per SIMD (256 registers)
    long grid = 256L * per_cu;
    if (grid > total) grid = total;
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](auto lc) {
        return launch_lds<frame_window_lpc24_bwd_mfma_kernel<lc()>>(lds > 48 * 1024 ? (int)lds : 0, "frame_window_lpc_bwd: cannot reserve LDS%s",
                                                                    dim3((unsigned)grid), dim3(64), lds, st, (const float*)gout, (const float*)x, (long)T,
                                                                    (long)N, L, P, left, (const float*)w, eps, (float*)gx, total, (int)ipu, (int)Hc,
                                                                    nfr_max);
    };
    if (int rc = L == 400 ? launch(int_c<400>{}) : launch(int_c<0>{})) return rc;
    return check_launch("frame_window_lpc24_bwd_mfma");
}
