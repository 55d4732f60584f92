// The two tuned forward kernels of the LPC branch (float64 lag sums; lag sums on the binary16 matrix pipe, the default) and their
// launcher, which dsa_frame_window_lpc_fwd (lpc.hip) calls.  What they share with the backward pair (lpc24_bwd.hip): lpc24.h.
#include <stdlib.h>

#include "lpc24.h"
#include "lpc_units.h"

namespace dsa {

// ---------------------------------------------------------------------------------------------
// Tuned fused Frame -> Window -> autocorrelation -> Levinson for float32 input, lpc_order 24,
// frame_length <= 512 (README.md:198-201 of the reference; BASELINE configs[3]).
//   * one wave64 per workgroup owns up to 64 consecutive frames of one utterance;
//   * autocorrelation: 4 frames per pass (16 lanes each) out of one LDS-resident stretch of
//     3P + L samples (each sample read from HBM once); lane j of a frame owns a contiguous run of
//     samples, keeps 25 + 24 windowed samples in registers (as float64: products of float32 are
//     exact) and accumulates its 25 lag sums with 625 statically indexed float64 FMAs per 25-sample
//     block; the 16 partials are added by rotate-and-add inside the DPP row (row16_allsum; first: an xor butterfly);
//   * Levinson-Durbin: one frame per LANE for all 64 frames at once, float64, fully unrolled in
//     registers (no cross-lane traffic at all), then [K, a_1..a_24] is written out.
// dynamic LDS: in_buf[(3P + L) rounded] floats | wtab[L + 64] floats | rbuf[64][25] doubles
__global__ __launch_bounds__(64, 2) void frame_window_lpc24_kernel(
    const float* __restrict__ x, long Tlen, long N, int L, int P, int left, int mode,
    const float* __restrict__ w, double eps, float* __restrict__ out, long total_sc, int sc_per_utt,
    int in_floats, int wtab_floats, unsigned* __restrict__ queue, int fpi)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* in_buf = reinterpret_cast<float*>(smem_raw);
    float* wtab = in_buf + in_floats;
    double* rbuf = reinterpret_cast<double*>(wtab + wtab_floats);
    const int lane = threadIdx.x;
    const int j = lane & 15, fl = lane >> 4;
    const int C = (L + 15) >> 4;                       // samples per lane
    const int nblk = (C + kLpcM1 - 1) / kLpcM1;        // 25-sample blocks per lane
    for (int l = lane; l < wtab_floats; l += 64) wtab[l] = l < L ? (w ? w[l] : 1.f) : 0.f;   // w == NULL: a window of ones

    // Work items are chunks of fpi <= 64 consecutive frames of one utterance (the launcher sizes them so that the
    // utterances split evenly and the item count is close to a whole number of rounds: 200 frames = 4 x 52 instead
    // of 64 + 64 + 64 + 8), handed out by a ticket counter.
    for (;;) {
        unsigned ticket = 0;
        if (lane == 0) ticket = atomicAdd(queue, 1u);
        const long tk = (long)__builtin_amdgcn_readfirstlane(ticket);
        if (tk >= total_sc) {
            // Every wave draws exactly one ticket past the end, so the counter stops at total_sc + (number of waves): the wave that
            // drew the last of those hands it back zeroed (DSA_LPC_SCRATCH_IS_CLEAN: no fill launch before the next call) -- no
            // second counter.  (A separate "waves done" counter put 3072 more atomics on one address at the very end: + 0.03 ms.)
            if (lane == 0 && tk == total_sc + (long)(gridDim.x * (blockDim.x >> 6)) - 1)
                __hip_atomic_store(queue, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        const long b = tk / sc_per_utt;
        const long ci = tk - b * sc_per_utt;
        const long fbase = ci * fpi;
        const int nfr = (int)((N - fbase) < fpi ? (N - fbase) : fpi);
        const float* xb = x + b * Tlen;
        const int npass = (nfr + 3) >> 2;
        for (int p = 0; p < npass; ++p) {
            const long frame0 = fbase + 4 * p;
            const int nvalid = (int)((N - frame0) < 4 ? (N - frame0) : 4);
            __syncthreads();
            {   // stage the shared stretch; zero-fill what the lanes may read beyond it
                const long g0 = frame0 * P - left;
                const int need = (nvalid - 1) * P + L;
                const bool interior = g0 >= 0 && g0 + need <= Tlen;
                if (interior && (((size_t)(xb + g0)) & 15) == 0 && (need & 3) == 0) {
                    const float4* src4 = reinterpret_cast<const float4*>(xb + g0);
                    float4* dst4 = reinterpret_cast<float4*>(in_buf);
                    for (int sidx = lane; sidx < (need >> 2); sidx += 64) dst4[sidx] = src4[sidx];
                } else {
                    for (int sidx = lane; sidx < need; sidx += 64) in_buf[sidx] = load_padded(xb, g0 + sidx, Tlen, mode);
                }
                for (int sidx = need + lane; sidx < in_floats; sidx += 64) in_buf[sidx] = 0.f;
            }
            __syncthreads();
            double acc[kLpcM1];
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) acc[m] = 0.0;
            const float* fsrc = in_buf + fl * P;
            for (int blk = 0; blk < nblk; ++blk) {
                const int t0 = j * C + blk * kLpcM1;  // this lane's block start within the frame
                const int own = C - blk * kLpcM1;     // samples of the block that belong to the lane
                double xw[2 * kLpcM1 - 1];
#pragma unroll
                for (int i = 0; i < 2 * kLpcM1 - 1; ++i) {
                    const int t = t0 + i;
                    // window.py:190 in float32 (as the reference), then exact promotion; zero past the
                    // frame, and zero for "own" positions that belong to the next lane (i >= own)
                    const float v = (t < L) ? fsrc[t] * wtab[t] : 0.f;
                    xw[i] = (double)v;
                }
                if (own >= kLpcM1) {
                    lag_block(acc, xw, std::make_integer_sequence<int, kLpcM1 * kLpcM1>{});
                } else {
                    // partial last block: the leading factor stops at the end of the lane's own run
#pragma unroll
                    for (int i = 0; i < kLpcM1; ++i) {
                        const double li = i < own ? xw[i] : 0.0;
#pragma unroll
                        for (int m = 0; m < kLpcM1; ++m) acc[m] = __builtin_fma(li, xw[i + m], acc[m]);
                    }
                }
            }
            // add the 16 lanes of the frame (rotate-and-add inside the DPP row: row16_allsum)
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) {
                acc[m] = row16_allsum(acc[m]);
            }
            if (fl < nvalid) {
                double* rrow = rbuf + (size_t)(4 * p + fl) * kLpcM1;
#pragma unroll
                for (int m = 0; m < kLpcM1; ++m)
                    if ((m & 15) == j) rrow[m] = acc[m];  // lane j stores lags j and j + 16
            }
        }
        __syncthreads();
        // ---- Levinson-Durbin, one frame per lane (levdur.py:113-127 as a recursion) ----
        if (lane < nfr) {
            double r[kLpcM1], a[kLpcM1];
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) r[m] = rbuf[(size_t)lane * kLpcM1 + m];
            const double gsum = levinson24(r, eps, a);
            float* o = out + ((b * N + fbase + lane) * (long)kLpcM1);
            o[0] = (float)sqrt(gsum);
#pragma unroll
            for (int m = 1; m < kLpcM1; ++m) o[m] = (float)a[m];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Round 4: the same fused Frame -> Window -> autocorrelation -> Levinson with the lag sums on the float32 MATRIX instruction.
// The float64 vector unit was the whole kernel above (625 v_fma_f64 per 25 samples and lane: 0.24 ms per 204 800 frames).  Here a
// wave takes its frames one at a time (since then: two per round, see the loop) and forms its lag sums as a banded Gram product: with u_b = the b-th block of 16 windowed samples,
//     C1 = sum_b u_b u_b^T,   C2 = sum_b u_b u_{b+1}^T,   C3 = sum_b u_b u_{b+2}^T        (16 x 16 each)
// hold every product xw[l] xw[l + m], m <= 24, exactly once: entry (i, j) of C_s is lag 16 (s - 1) + j - i summed over the
// positions l = i (mod 16).  Operands need no staging at all: lane = i + 16 k of v_mfma_f32_16x16x4_f32 is sample 64 e + lane of
// the frame -- a coalesced load times the window -- and the B operand of C2 / C3 is the same load 16 / 32 samples further on
// (L1 hits).  The products run as 3-term binary16 splits on the matrix pipe (9 instructions per frame, see the loop); the 16 entries of a lag are added in FLOAT64 (scattered through LDS so that a lane reads its lag's
// 16 slots as four 16-byte reads), then Levinson-Durbin in float64, one frame per lane, as above.
// Accuracy: the lag sums are ~1e-7 r[0] from the exact ones (what the reference's own float32 FFT route has); the exact kernel
// stays selectable (DSA_LPC_LAGSUMS=f64) and is what float64 input runs.
#ifndef LPC_ABL
#define LPC_ABL 0   // measurement builds only (tools/build_variant.sh): 1 no recursion, 2 no scatter / sums, 4 no products, 8 no maximum / scale
#endif
template <int NE, int LC>   // NE = 8: operand elements per lane (512 samples); LC: the frame length at compile time (0: run time)
__global__ __launch_bounds__(256, 3) void frame_window_lpc24_mfma_kernel(
    const float* __restrict__ x, long Tlen, long N, int L_rt, int P, int left, int mode, const float* __restrict__ w, double eps,
    float* __restrict__ out, long total_sc, int sc_per_utt, int fpi)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    constexpr int DS = kLsDS;                      // floats per lag row of the scatter area (see kLsDS)
    // dynamic LDS, per wave: rbuf[fpi][25] doubles | dm[2][26][DS] floats (a scatter area per frame of a round)  (fpi = 40 at the bench
    // geometry: three workgroups per CU)
    extern __shared__ __attribute__((aligned(16))) unsigned char lpc_smem[];
    const int L = LC ? LC : L_rt;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wave_bytes = fpi * kLpcM1 * (int)sizeof(double) + 2 * kLsArea * (int)sizeof(float);
    double* rbuf = reinterpret_cast<double*>(lpc_smem + (size_t)wave * wave_bytes);
    float* dm = reinterpret_cast<float*>(rbuf + fpi * kLpcM1);
    const int j = lane & 15, g = lane >> 4;
    // Operand element e of lane (j, g) is sample 16 (8 g + e) + j: the lane's eight elements are eight CONSECUTIVE blocks of 16
    // samples (k-slot (g, e) <-> block 8 g + e; any bijection serves, A and B use the same one).  The operands of C2 / C3 -- the same
    // samples one / two blocks on -- are then the lane's own elements one / two places on, i.e. (packed two to a register) one
    // v_alignbit per register resp. the next register, plus element 0 of the lane 16 further on for the last place(s): one
    // ds_bpermute per frame and half.  (With k-slot <-> block 4 e + g the three operand sets were three loads, window products,
    // scalings and splits of the same samples: 0.107 of the kernel's 0.145 ms were operand preparation.)
    // window values (w == NULL: ones); samples past the frame are selected away
    float wa[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int la = 128 * g + 16 * e + j;
        wa[e] = la < L ? (w ? w[la] : 1.f) : 0.f;
    }
    // scatter addresses of this lane's 12 matrix entries: entry (tile s, register r) = C_s[4 g + r][j], lag = 16 s + j - (4 g + r);
    // lags outside [0, 24] go to the spare row 25
    int addr[3][4];
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * g + r, lag = 16 * s_ + j - i;
            addr[s_][r] = (lag >= 0 && lag < kLpcM1) ? lag * DS + i : kLsArea - 64 + lane;
        }
    // Items are dealt out statically, item = wave + k (number of waves).  (A ticket counter put an atomic on ONE address behind every
    // item and every wave's exit -- 5120 + 3072 of them per launch at the bench size, about one per 16 ns: the counter's throughput,
    // not the arithmetic, set the launch time: 0.135 against 0.087 ms.)
    const long nwaves_g = (long)gridDim.x * (blockDim.x >> 6);
    for (long tk = (long)blockIdx.x * (blockDim.x >> 6) + wave; tk < total_sc; tk += nwaves_g) {
        const long b = tk / sc_per_utt;
        const long ci = tk - b * sc_per_utt;
        const long fbase = ci * fpi;
        const int nfr = (int)((N - fbase) < fpi ? (N - fbase) : fpi);
        const float* xb = x + b * Tlen;
        // TWO frames per round (frame fi + u uses scatter area u): loads -> maximum -> split -> products -> scatter -> sums is one
        // dependent chain per frame, and at three waves per SIMD a wave that walks its frames one at a time leaves the vector unit
        // idle half the time (46 % busy, 0.150 ms); the two chains of a round share no data and interleave.  The samples of the
        // next round are requested while this one is in the matrix pipeline.
        constexpr int U = 2;
        float a[U][8];
        const int soff = 128 * g + j;   // this lane's first sample inside a frame
        auto fetch = [&](int u, int fi) __attribute__((always_inline)) {
            const long start = (fbase + fi) * P - left;
            if (start >= 0 && start + 512 <= Tlen) {   // uniform: every sample any lane touches exists
                const float* src = xb + start + soff;
#pragma unroll
                for (int e = 0; e < 8; ++e) a[u][e] = src[16 * e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) a[u][e] = soff + 16 * e < L ? load_padded(xb, start + soff + 16 * e, Tlen, mode) : 0.f;
            }
        };
        // (an odd count: the last round's second frame is the first one again, computed and not stored)
        // (Tried twice: the samples of two rounds in flight, two register sets and the round loop unrolled by two -- with the ticket counter
        // 0.135 -> 0.145 ms, without it 0.087 -> 0.093 ms.)
        fetch(0, 0);
        fetch(1, 1 < nfr ? 1 : 0);
        for (int fi = 0; fi < nfr; fi += U) {
            float va[U][8];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e)   // window.py:190 in float32 (as the reference); samples past the frame are selected away, never multiplied
                    va[u][e] = soff + 16 * e < L ? a[u][e] * wa[e] : 0.f;
            if (fi + U < nfr) {
                fetch(0, fi + U);
                fetch(1, fi + U + 1 < nfr ? fi + U + 1 : fi + U);
            }
            // The Gram products on the BINARY16 matrix pipe (separate from the float32 datapath the float64 sums and the recursion
            // need).  Every value is split hi + lo into two binary16 numbers after scaling the frame by a power of two that puts its
            // largest sample in [2^13, 2^14) (lo stays a normal number down to 2^-17 of the maximum); a product is three
            // instructions, hi hi + hi lo + lo hi (the dropped lo lo is 2^-22 of the product), exact binary16 products accumulated
            // in float32 over the whole frame at once (K = 32 blocks of 16 samples cover 512).  9 matrix instructions per frame
            // instead of 19 float32 ones (round 4, first version: 608 cycles of the float32 datapath per frame).
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
            for (int u = 0; u < U; ++u) sh[u] = (LPC_ABL & 8) ? 3 : lp_frame_shift(fmx[u]);
            lp_h8 ah[U], al[U], bh[U], bl[U], ch[U], cl[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                typedef unsigned lp_u4 __attribute__((ext_vector_type(4)));
                lp_u4 hr, lr;   // the packed halves: register k = elements (2 k, 2 k + 1)
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    lp_h2 h, l;
                    lp_split2(__builtin_ldexpf(va[u][e], sh[u]), __builtin_ldexpf(va[u][e + 1], sh[u]), h, l);
                    hr[e >> 1] = __builtin_bit_cast(unsigned, h);
                    lr[e >> 1] = __builtin_bit_cast(unsigned, l);
                }
                // elements (0, 1) of the lane 16 further on (blocks 8 (g + 1), 8 (g + 1) + 1); past the last row: zeros
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
            if (!(LPC_ABL & 4)) {
                lp_round_products(ah, al, bh, bl, ch, cl, c1, c2, c3);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) { c1[u][0] = va[u][0]; c2[u][0] = va[u][1]; c3[u][0] = va[u][2]; }
            }
            if (LPC_ABL & 2) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (lane < kLpcM1 && fi + u < nfr) rbuf[(fi + u) * kLpcM1 + lane] = c1[u][0] + c2[u][1] + c3[u][2] + (lane == 0 ? 1.0 : 0.0);
                continue;
            }
            __builtin_amdgcn_wave_barrier();   // the previous round's row reads are done (LDS operations of a wave run in order)
            lp_round_scatter(dm, addr, c1, c2, c3);
            __builtin_amdgcn_wave_barrier();
            {
                // lane (m, h) = (lane & 31, lane >> 5) adds slots 8 h .. 8 h + 7 of lag m in float64; the halves meet through one
                // cross-half exchange (rows 25 .. 31 read the spare row: finite or not, their sums are never stored)
                double sm[U];
#pragma unroll
                for (int u = 0; u < U; ++u) sm[u] = lp_lag_halfsum(dm + u * kLsArea, lane);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double tot = lp_lag_total(sm[u], lane);
                    if (lane < kLpcM1 && fi + u < nfr) rbuf[(fi + u) * kLpcM1 + lane] = ldexp(tot, -2 * sh[u]);   // the frame's scale, undone exactly
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        // ---- Levinson-Durbin, one frame per lane (levdur.py:113-127 as a recursion), as in frame_window_lpc24_kernel ----
        if ((LPC_ABL & 1) && lane < nfr) {
            float* o = out + ((b * N + fbase + lane) * (long)kLpcM1);
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) o[m] = (float)rbuf[(size_t)lane * kLpcM1 + m];
        } else if (lane < nfr) {
            double r[kLpcM1], al[kLpcM1];
#pragma unroll
            for (int m = 0; m < kLpcM1; ++m) r[m] = rbuf[(size_t)lane * kLpcM1 + m];
            const double gsum = levinson24(r, eps, al);
            float* o = out + ((b * N + fbase + lane) * (long)kLpcM1);
            o[0] = (float)sqrt(gsum);
#pragma unroll
            for (int m = 1; m < kLpcM1; ++m) o[m] = (float)al[m];
        }
        __builtin_amdgcn_wave_barrier();   // rbuf is rewritten by the next chunk
    }
}

// the float64 kernel's LDS carve-up (see its head comment)
static int lpc24_in_floats(int L, int P) { return ((3 * P + L + 64 + kLpcM1 * 2) + 3) & ~3; }
static int lpc24_wtab_floats(int L) { return (L + 64 + 3) & ~3; }
static size_t lpc24_f64_lds(int L, int P) { return (size_t)(lpc24_in_floats(L, P) + lpc24_wtab_floats(L)) * 4 + 64 * kLpcM1 * sizeof(double); }
bool lpc24_fwd_fits(int L, int P) { return lpc24_f64_lds(L, P) <= 60 * 1024; }

int lpc24_fwd(const void* x, int64_t B, int64_t T, int64_t N, int L, int P, int left, int pad_mode, const void* w, double eps,
              bool exact_flag, bool scratch_clean, void* scratch, void* out, hipStream_t st)
{
    const int64_t F = B * N;
    const size_t lds_t = lpc24_f64_lds(L, P);
    int waves_per_cu = (int)(144 * 1024 / lds_t);
    if (waves_per_cu > 8) waves_per_cu = 8;
    long grid = 256L * waves_per_cu;
    // frames per work item: close to a whole number of items per wave, utterances split evenly
    int fpi = lpc24_frames_per_item((long)F, grid);
    {
        const long cpu = (N + fpi - 1) / fpi;            // chunks per utterance
        long f = ((N + cpu - 1) / cpu + 3) & ~3L;        // ... of equal size
        if (f >= 4 && f <= 64) fpi = (int)f;
    }
    int sc_per_utt = (int)((N + fpi - 1) / fpi);
    long total_sc = (long)B * sc_per_utt;
    if (grid > total_sc) grid = total_sc;
    // lag sums: float32 matrix instruction (default) or the float64 vector unit (DSA_LPC_LAGSUMS=f64: exact sums)
    const bool exact = exact_flag || strcmp(env_text("DSA_LPC_LAGSUMS"), "f64") == 0;
    // ticket counter (the float64 kernel; the default kernel deals its items out statically and needs none): the first word of
    // the caller's scratch, zeroed in stream order before the launch unless the caller says it is
    unsigned* queue = (unsigned*)scratch;
    if (exact && !scratch_clean && hipMemsetAsync(queue, 0, sizeof(unsigned), st) != hipSuccess)
        return fail(DSA_ERR_LAUNCH, "frame_window_lpc: cannot reset the ticket counter%s");
    if (!exact) {
        // three workgroups per CU need 4 (200 fpi + 5312) <= 53 KB: at most 41 frames per item, utterances split evenly.
        // (Tried: frames per item chosen so that every one of the 3072 resident waves gets the same number of items -- 34
        // frames, 6144 items at the bench size instead of 40 / 5120: 0.135 -> 0.140 ms; more recursion phases on fewer lanes.)
        if (fpi > 41) {
            const long cpu = (N + 40) / 41;
            long f = ((N + cpu - 1) / cpu + 3) & ~3L;
            if (f > 41) f = 40;
            fpi = (int)f;
            sc_per_utt = (int)((N + fpi - 1) / fpi);
            total_sc = (long)B * sc_per_utt;
        }
        const int lds_m = 4 * (fpi * kLpcM1 * (int)sizeof(double) + 2 * kLsArea * (int)sizeof(float));
        long wgs = (total_sc + 3) / 4;
        const long wg_cap = 256L * (lds_m <= 53 * 1024 ? 3 : 2);   // workgroups of four waves per CU
        if (wgs > wg_cap) wgs = wg_cap;
        auto launch = [&](auto lc) {
            return launch_lds<frame_window_lpc24_mfma_kernel<8, lc()>>(lds_m > 48 * 1024 ? lds_m : 0, "frame_window_lpc: cannot reserve LDS%s",
                                                                       dim3((unsigned)wgs), dim3(256), lds_m, st, (const float*)x, (long)T, (long)N, L, P,
                                                                       left, pad_mode, (const float*)w, eps, (float*)out, total_sc, sc_per_utt, fpi);
        };
        if (int rc = L == 400 ? launch(int_c<400>{}) : launch(int_c<0>{})) return rc;   // (400: the 25 ms window at 16 kHz)
        return check_launch("frame_window_lpc24_mfma_fwd");
    }
    hipLaunchKernelGGL(frame_window_lpc24_kernel, dim3((unsigned)grid), dim3(64), lds_t, st, (const float*)x,
                       (long)T, (long)N, L, P, left, pad_mode, (const float*)w, eps, (float*)out, total_sc,
                       sc_per_utt, lpc24_in_floats(L, P), lpc24_wtab_floats(L), queue, fpi);
    return check_launch("frame_window_lpc24_fwd");
}

}  // namespace dsa
