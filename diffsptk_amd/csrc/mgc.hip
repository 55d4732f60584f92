// Mel-generalized cepstra: the spectrum arithmetic of the Newton step of the mel-generalized cepstral analysis (mgcep_spectra,
// mgcep_step, mgcep_step_bwd; the step's solve is thsolve.hip / thsolve_quad.hip), gain normalisation (gnorm, mgcep_gain) and the
// generalized cepstral transformation gc2gc.
#include "common.h"
#include "lds_fft.h"

namespace dsa {

// ---------------------------------------------------------------------------------------------
// The spectrum arithmetic of one Newton step of MelGeneralizedCepstralAnalysis (mgcep.py:199-209), gamma not in {0, -1},
// in ONE pass over the (F, K) spectra (as stock element-wise operators it is ~20 passes and dominated the step):
//   C = b1 (Cr[1:], Ci[1:])   (b[0] = 0),  X = 1 + gamma Re C,  Y = gamma Im C,  D = X^2 + Y^2,
//   pp = x D^(-1/gamma - 1),  qq = pp / D,
//   out[0] = pp   out[1] = qq (X^2 - Y^2)   out[2] = qq 2 X Y   out[3] = pp X   out[4] = pp Y      (each (F, K))
// -- the inputs of the five row products against Pr, Qr, Qi, Rr, Ri.  A thread owns one bin: its 2 M matrix entries stay
// in registers for the workgroup's tile of frames, the frames' coefficients are broadcast from LDS.
constexpr int kMsFrames = 32, kMsMaxM = 64;
template <typename T, int MT>   // MT: compile-time bound on M (register-resident matrix columns)
__global__ __launch_bounds__(320) void mgcep_spectra_kernel(const T* __restrict__ x, const T* __restrict__ b1, long F, int K, int M,
                                                            const T* __restrict__ Cr, const T* __restrict__ Ci, T gamma,
                                                            T* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) T bs[kMsFrames * MT];   // row stride MT, zero-padded: static offsets, 16-byte reads
    const long f0 = (long)blockIdx.x * kMsFrames;
    const int nf = (int)((F - f0) < kMsFrames ? (F - f0) : kMsFrames);
    for (int i = threadIdx.x; i < kMsFrames * MT; i += blockDim.x) {
        const int fi = i / MT, m = i - fi * MT;
        bs[i] = (fi < nf && m < M) ? b1[(f0 + fi) * M + m] : T(0);
    }
    __syncthreads();
    const T ex = T(-1) / gamma - T(1);
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        T cr[MT], ci[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            cr[m] = m < M ? Cr[(long)(m + 1) * K + k] : T(0);
            ci[m] = m < M ? Ci[(long)(m + 1) * K + k] : T(0);
        }
        for (int fb = 0; fb < nf; fb += 8) {
        // (the eight spectrum values of a round are fetched together, ahead of the arithmetic: one round trip, not eight)
        T xv8[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) xv8[q] = x[(f0 + (fb + q < nf ? fb + q : nf - 1)) * K + k];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int fi = fb + q;
            if (fi >= nf) break;
            T re = 0, im = 0;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const T b = bs[fi * MT + m];
                re += b * cr[m];
                im += b * ci[m];
            }
            const T X = T(1) + gamma * re, Y = gamma * im;
            const T XX = X * X, YY = Y * Y, D = XX + YY;
            T dp;
            if constexpr (sizeof(T) == 4) dp = __builtin_amdgcn_exp2f(ex * __builtin_amdgcn_logf(D));   // D > 0; 1 ulp each
            else dp = dsa_pow(D, ex);
            const T pp = xv8[q] * dp;
            const T qq = pp / D;
            const long o = (f0 + fi) * K + k, S = F * (long)K;
            out[o] = pp;
            out[S + o] = qq * (XX - YY);
            out[2 * S + o] = qq * (T(2) * X * Y);
            out[3 * S + o] = pp * X;
            out[4 * S + o] = pp * Y;
        }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// One Newton step's spectrum arithmetic AND its five row products in ONE launch (float32, fft_length 512, cep_order <= 24):
//   (re, im) = b1 (Cr, Ci)            first chain: 24 coefficients -> 257 bins, real and imaginary part   (mgcep.py:191-193, 199-201)
//   X = 1 + g re, Y = g im, D = X^2 + Y^2, pp = x D^(-1/g - 1), qq = pp / D                                 (mgcep.py:202-209)
//   pt = pp Pr,  qt = (1 + g) (qq (X^2 - Y^2) Qr + qq 2XY Qi),  r = pp X Rr + pp Y Ri                         (mgcep.py:212-220)
// on v_mfma_f32_16x16x4_f32 with the FRAMES as the N dimension, as in the mel-cepstral kernels: the first chain's result comes out
// with lane (n, g) register r holding bin 16 mt + 4 g + r of frame n -- exactly a B operand of the second chain if its k-steps are
// enumerated as (mt, r) with k-slot g <-> bin 16 mt + 4 g + r, so the five spectra feed the second chain from registers and never
// exist in memory (round 2: dsa_mgcep_spectra wrote them, 263 MB per step at 51 200 frames, and five launches of the matrix-core
// row product read them back: 0.14 + 5 x 0.05 ms per step).  One wave = 16 frames; the four waves of a workgroup share the
// operand images of a 16-bin tile through LDS (15 KB per tile, double-buffered, one barrier per tile).  Float32 products with
// float32 accumulation: nothing given up.  Bins 256 .. 271 are a seventeenth tile whose images are zero past bin 256.
// `images` (built by the caller once per configuration, tables.mgcep_step_images): per bin tile mt = 0 .. 16
//   [2 (Cr, Ci)][6 ks][64 l]      A of the first chain:  C[1 + 4 ks + (l >> 4)][16 mt + (l & 15)]                    (768 floats)
//   [12 c][64 l][4 r]             A of the second chain: W_c[16 mt + 4 (l >> 4) + r][16 tile_c + (l & 15)]           (3072 floats)
//   chains c: 0-1 Pr (input pp), 2-4 Qr (qq (X^2 - Y^2)), 5-7 Qi (qq 2XY), 8-9 Rr (pp X), 10-11 Ri (pp Y); 16-column tiles of each matrix.
// ---------------------------------------------------------------------------------------------------------------------------
typedef float ms_f4 __attribute__((ext_vector_type(4)));
typedef float ms_f4u __attribute__((ext_vector_type(4), aligned(4)));   // rows of 257 floats: 4-byte aligned only
constexpr int kMsTileFloats = 768 + 3072, kMsTiles = 17;
__global__ __launch_bounds__(256) void mgcep_step_kernel(const float* __restrict__ x, const float* __restrict__ b1, long F, int M, float gamma,
                                                        const float* __restrict__ img, float* __restrict__ pt, float* __restrict__ qt,
                                                        float* __restrict__ rr)
{
    __shared__ __attribute__((aligned(16))) float tile[2][kMsTileFloats];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    const long f_raw = ((long)blockIdx.x * 4 + wave) * 16 + n;
    const bool f_ok = f_raw < F;
    const long f = f_ok ? f_raw : F - 1;
    // B operand of the first chain: b1[4 ks + g] of this lane's frame
    float bv[6];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) bv[ks] = 4 * ks + g < M ? b1[f * M + 4 * ks + g] : 0.f;
    const float ex = -1.f / gamma - 1.f;
    ms_f4 acc[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) acc[t] = ms_f4{0.f, 0.f, 0.f, 0.f};
    // staging: 3840 floats = 960 float4 per tile, 256 threads x 4 (threads 240 .. 255 idle on the last one)
    const ms_f4* img4 = reinterpret_cast<const ms_f4*>(img);
    ms_f4 st[4];
    auto fetch = [&](int mt) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q;
            st[q] = i < kMsTileFloats / 4 ? img4[(long)mt * (kMsTileFloats / 4) + i] : ms_f4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stage = [&](int buf) __attribute__((always_inline)) {
        ms_f4* d = reinterpret_cast<ms_f4*>(tile[buf]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q;
            if (i < kMsTileFloats / 4) d[i] = st[q];
        }
    };
    fetch(0);
    stage(0);
    __syncthreads();
    for (int mt = 0; mt < kMsTiles; ++mt) {
        const int buf = mt & 1;
        if (mt + 1 < kMsTiles) fetch(mt + 1);
        // this lane's four spectrum values of the tile: bins 16 mt + 4 g + r (only bin 256 exists in the last tile)
        ms_f4 xv = {0.f, 0.f, 0.f, 0.f};
        if (mt < 16) xv = *reinterpret_cast<const ms_f4u*>(x + f * 257 + 16 * mt + 4 * g);
        else if (g == 0) xv[0] = x[f * 257 + 256];
        const float* t1 = tile[buf];
        const ms_f4* t2 = reinterpret_cast<const ms_f4*>(tile[buf] + 768);
        ms_f4 re = {0.f, 0.f, 0.f, 0.f}, im = re;
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(t1[ks * 64 + lane], bv[ks], re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(t1[384 + ks * 64 + lane], bv[ks], im, 0, 0, 0);
        }
        float s[5][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float X = 1.f + gamma * re[r], Y = gamma * im[r];
            const float XX = X * X, YY = Y * Y, D = XX + YY;
            const float dp = __builtin_amdgcn_exp2f(ex * __builtin_amdgcn_logf(D));   // D > 0; 1 ulp each (as dsa_mgcep_spectra)
            const float pp = xv[r] * dp;
            const float qq = pp / D;
            s[0][r] = pp;
            s[1][r] = qq * (XX - YY);
            s[2][r] = qq * (2.f * X * Y);
            s[3][r] = pp * X;
            s[4][r] = pp * Y;
        }
        // second chain: k-step (mt, r), k-slot g <-> bin 16 mt + 4 g + r: the values above ARE the B operands
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            const ms_f4 a = t2[c * 64 + lane];
            const int in = c < 2 ? 0 : (c < 5 ? 1 : (c < 8 ? 2 : (c < 10 ? 3 : 4)));
            const int t = c < 2 ? c : (c < 5 ? c : (c < 8 ? c - 3 : (c < 10 ? c - 3 : c - 5)));   // accumulators: 0-1 pt | 2-4 qt | 5-6 r
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], s[in][r], acc[t], 0, 0, 0);
        }
        if (mt + 1 < kMsTiles) {
            stage(buf ^ 1);      // the other buffer: its readers finished before the barrier that ended tile mt - 1
            __syncthreads();
        }
    }
    if (!f_ok) return;
    // C/D layout: lane (n, g) register r of tile t <-> column 16 t + 4 g + r of frame n
    const float og = 1.f + gamma;
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (t < 2) {
                const int col = 16 * t + 4 * g + r;
                if (col < M) pt[f * M + col] = acc[t][r];
            } else if (t < 5) {
                const int col = 16 * (t - 2) + 4 * g + r;
                if (col < 2 * M - 1) qt[f * (2 * M - 1) + col] = og * acc[t][r];
            } else {
                const int col = 16 * (t - 5) + 4 * g + r;
                if (col < M + 1) rr[f * (M + 1) + col] = acc[t][r];
            }
        }
}

// Backward of one Newton step's (pt, qt, r) = mgcep_step(x, b1) (above) in ONE launch, same tiling: a wave = 16 frames, a pass =
// 16 bins.  Per pass: re / im recomputed (first chain as above), the cotangents of the five spectra at these bins as row products
// of (gpt | (1 + gamma) gqt | gr) with the TRANSPOSED second-chain matrices (44 k-steps: the cotangent vectors are the B
// operands, held in registers for the whole launch), the element-wise chain rule, gx written, and the cotangent of (re, im)
// accumulated into gb1 = gamma (gX Cr^T + gY Ci^T) (16 k-steps).  72 products per pass (forward: 60).
// Image per tile (tables.mgcep_step_bwd_images): [0, 768) the forward's first-chain operands | [768, 3584) the 44 k-steps
// A[i = bin 16 mt + (lane & 15)][k = column 4 ks + (lane >> 4)] of Pr (6) | Qr (12) | Qi (12) | Rr (7) | Ri (7) |
// [3584, 4608) A[i = coefficient 1 + 16 t + (lane & 15)][k = bin 16 mt + 4 (lane >> 4) + r] of Cr (t, r) | Ci (t, r).
constexpr int kMbTileFloats = 768 + 44 * 64 + 16 * 64;
__global__ __launch_bounds__(256) void mgcep_step_bwd_kernel(const float* __restrict__ x, const float* __restrict__ b1,
                                                            const float* __restrict__ gpt, const float* __restrict__ gqt,
                                                            const float* __restrict__ grr, long F, int M, float gamma,
                                                            const float* __restrict__ img, const float* __restrict__ gx_in,
                                                            float* __restrict__ gx, float* __restrict__ gb1)
{
    __shared__ __attribute__((aligned(16))) float tile[2][kMbTileFloats];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, g = lane >> 4;
    const long f_raw = ((long)blockIdx.x * 4 + wave) * 16 + n;
    const bool f_ok = f_raw < F;
    const long f = f_ok ? f_raw : F - 1;
    const float og = 1.f + gamma;
    // B operands held for the whole launch: coefficient / column 4 ks + g of this lane's frame
    float bv[6], vp[6], vq[12], vr[7];
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
        bv[ks] = 4 * ks + g < M ? b1[f * M + 4 * ks + g] : 0.f;
        vp[ks] = 4 * ks + g < M ? gpt[f * M + 4 * ks + g] : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 12; ++ks) vq[ks] = 4 * ks + g < 2 * M - 1 ? og * gqt[f * (2 * M - 1) + 4 * ks + g] : 0.f;
#pragma unroll
    for (int ks = 0; ks < 7; ++ks) vr[ks] = 4 * ks + g < M + 1 ? grr[f * (M + 1) + 4 * ks + g] : 0.f;
    const float ex = -1.f / gamma - 1.f;
    ms_f4 accb[2] = {ms_f4{0.f, 0.f, 0.f, 0.f}, ms_f4{0.f, 0.f, 0.f, 0.f}};
    const ms_f4* img4 = reinterpret_cast<const ms_f4*>(img);
    constexpr int kQ = (kMbTileFloats / 4 + 255) / 256;   // float4 per thread and tile
    ms_f4 st[kQ];
    auto fetch = [&](int mt) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const int i = tid + 256 * q;
            st[q] = i < kMbTileFloats / 4 ? img4[(long)mt * (kMbTileFloats / 4) + i] : ms_f4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stage = [&](int buf) __attribute__((always_inline)) {
        ms_f4* d = reinterpret_cast<ms_f4*>(tile[buf]);
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const int i = tid + 256 * q;
            if (i < kMbTileFloats / 4) d[i] = st[q];
        }
    };
    fetch(0);
    stage(0);
    __syncthreads();
    for (int mt = 0; mt < kMsTiles; ++mt) {
        const int buf = mt & 1;
        if (mt + 1 < kMsTiles) fetch(mt + 1);
        ms_f4 xv = {0.f, 0.f, 0.f, 0.f};
        if (mt < 16) xv = *reinterpret_cast<const ms_f4u*>(x + f * 257 + 16 * mt + 4 * g);
        else if (g == 0) xv[0] = x[f * 257 + 256];
        const float* t1 = tile[buf];
        const float* t2 = tile[buf] + 768;
        const float* t3 = tile[buf] + 768 + 44 * 64;
        ms_f4 re = {0.f, 0.f, 0.f, 0.f}, im = re;
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(t1[ks * 64 + lane], bv[ks], re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(t1[384 + ks * 64 + lane], bv[ks], im, 0, 0, 0);
        }
        // cotangents of the five spectra at bins 16 mt + 4 g + r
        ms_f4 gs[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) gs[i] = ms_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) gs[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(t2[ks * 64 + lane], vp[ks], gs[0], 0, 0, 0);
#pragma unroll
        for (int ks = 0; ks < 12; ++ks) {
            gs[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(t2[(6 + ks) * 64 + lane], vq[ks], gs[1], 0, 0, 0);
            gs[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(t2[(18 + ks) * 64 + lane], vq[ks], gs[2], 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 7; ++ks) {
            gs[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(t2[(30 + ks) * 64 + lane], vr[ks], gs[3], 0, 0, 0);
            gs[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(t2[(37 + ks) * 64 + lane], vr[ks], gs[4], 0, 0, 0);
        }
        float gre[4], gim[4], gxv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float X = 1.f + gamma * re[r], Y = gamma * im[r];
            const float XX = X * X, YY = Y * Y, D = XX + YY;
            const float dp = __builtin_amdgcn_exp2f(ex * __builtin_amdgcn_logf(D));
            const float pp = xv[r] * dp;
            const float rD = 1.f / D;
            const float qq = pp * rD;
            const float g_qq = gs[1][r] * (XX - YY) + gs[2][r] * (2.f * X * Y);
            const float g_pp = gs[0][r] + gs[3][r] * X + gs[4][r] * Y + g_qq * rD;
            const float g_D = (g_pp * ex * pp - g_qq * qq) * rD;
            const float gX = 2.f * qq * (gs[1][r] * X + gs[2][r] * Y) + gs[3][r] * pp + 2.f * X * g_D;
            const float gY = 2.f * qq * (gs[2][r] * X - gs[1][r] * Y) + gs[4][r] * pp + 2.f * Y * g_D;
            gre[r] = gamma * gX;
            gim[r] = gamma * gY;
            gxv[r] = g_pp * dp;
        }
        if (f_ok) {
            if (mt < 16) {
                float* dst = gx + f * 257 + 16 * mt + 4 * g;
                ms_f4 o = {gxv[0], gxv[1], gxv[2], gxv[3]};
                if (gx_in) o += *reinterpret_cast<const ms_f4u*>(gx_in + f * 257 + 16 * mt + 4 * g);
                *reinterpret_cast<ms_f4u*>(dst) = o;
            } else if (g == 0) {
                gx[f * 257 + 256] = gxv[0] + (gx_in ? gx_in[f * 257 + 256] : 0.f);
            }
        }
        // gb1[16 t + 4 g + r'] += sum over the tile's bins: k-step r, k-slot g <-> bin 16 mt + 4 g + r
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                accb[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(t3[(t * 4 + r) * 64 + lane], gre[r], accb[t], 0, 0, 0);
                accb[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(t3[(8 + t * 4 + r) * 64 + lane], gim[r], accb[t], 0, 0, 0);
            }
        if (mt + 1 < kMsTiles) {
            stage(buf ^ 1);
            __syncthreads();
        }
    }
    if (!f_ok) return;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = 16 * t + 4 * g + r;
            if (col < M) gb1[f * M + col] = accb[t][r];
        }
}

template <typename T>
static int mgcep_spectra_launch(const void* x, const void* b1, int64_t F, int K, int M, const void* Cr, const void* Ci, double gamma,
                                void* out, hipStream_t st)
{
    const unsigned grid = (unsigned)((F + kMsFrames - 1) / kMsFrames);
#define DSA_MS_LAUNCH(MT)                                                                                                  \
    hipLaunchKernelGGL((mgcep_spectra_kernel<T, MT>), dim3(grid), dim3(K > 256 ? 320 : 256), 0, st, (const T*)x, (const T*)b1,  \
                       (long)F, K, M, (const T*)Cr, (const T*)Ci, (T)gamma, (T*)out)
    if (M <= 16) DSA_MS_LAUNCH(16);
    else if (M <= 32) DSA_MS_LAUNCH(32);
    else DSA_MS_LAUNCH(64);
#undef DSA_MS_LAUNCH
    return check_launch("mgcep_spectra");
}

// ---------------------------------------------------------------------------------------------
// Generalized cepstral transformation in ONE launch (GeneralizedCepstrumToGeneralizedCepstrum._forward, mgc2mgc.py:333-361):
//   c01 = (0, c1[1:]) -> C1 = fft(c01, n) -> s = (1 + g1 C1)^(1/g1) (g1 = 0: exp C1) -> C2 = (|s|^g2 cos(g2 angle(s)) - 1) / g2
//   (g2 = 0: log |s|) -> c02 = ifft(C2).real[: M2 + 1] -> c2 = (c1[0], 2 c02[1:]).
// One workgroup per row, the n complex points in LDS; both transforms are the radix-2 LDS transform of lds_fft.h: c01 is real, so C1 is
// Hermitian and C2 is real and even -- its inverse transform IS its forward transform / n, and only the real parts leave.
// As separate launches (row transform -> five element-wise operators -> adjoint row transform, modules/mgc2mgc.py) the
// 4096-point spectra of the MLSA filter's impulse responses went through memory seven times (profiles/r02_mlsa_single_stage_trace.txt:
// 7.2 of the 8.3 ms of the single-stage mode).  Forward only (the module composes the differentiable operators when a gradient is
// wanted).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gc2gc_fused_kernel(const T* __restrict__ c1, int n_in, int out_order, T g1, T g2, int nfft,
                                                         const T* __restrict__ tw, int flags, T* __restrict__ c2)
{
    // Both transforms act on REAL data (c01, and the real even C2), so each runs as a complex transform of HALF the length on
    // the packed sequence z[n] = x[2n] + i x[2n+1], followed by the split  X[k] = (Z[k] + conj Z[H-k]) / 2 - i W^k (Z[k] - conj Z[H-k]) / 2
    // (H = n / 2): half the butterflies and half the LDS traffic of the full-length version (2.59 -> see DESIGN ms per 51 200 rows
    // of 4096 points).  LDS: re[H] | im[H] | cb[H + 1] (the mapped half spectrum, natural order).
    extern __shared__ unsigned char smem_raw[];
    const int H = nfft >> 1;
    T* re = reinterpret_cast<T*>(smem_raw);
    T* im = re + H;
    T* cb = im + H;
    const long f = blockIdx.x;
    const T* row = c1 + f * n_in;
    const int lgh = 30 - __clz(nfft);   // log2(H)
    // flags: the per-row scalar steps mgc2mgc.py:217-300 wraps around the transformation, folded in (each was a pass over the
    // row in memory): 1 gnorm(in_gamma) before, 2 ignorm(out_gamma) after, 4 tail times out_gamma, 8 zeroth coefficient * out_gamma + 1
    T k0 = row[0], tin = T(1);
    if (flags & 1) {   // gnorm.py:99-109
        if (g1 == T(0)) k0 = dsa_exp(row[0]);
        else {
            const T z = T(1) + g1 * row[0];
            k0 = dsa_pow(z, T(1) / g1);
            tin = T(1) / z;
        }
    }
    for (int n = threadIdx.x; n < H; n += blockDim.x) {   // fft(c01, n): longer rows are cropped, c01[0] = 0
        const int i0 = 2 * n, i1 = 2 * n + 1;
        re[n] = (i0 >= 1 && i0 < n_in) ? row[i0] * tin : T(0);
        im[n] = i1 < n_in ? row[i1] * tin : T(0);
    }
    __syncthreads();
    lds_fft_pow2(re, im, H, lgh, tw, 2);   // Z[k] at position brev(k)
    constexpr T pi = T(kPi);
    auto gmap = [&](T cr, T ci) -> T {
        T lmag, ang;   // log |s|, angle(s) (wrapped to (-pi, pi] as .angle() of the reference's polar(r, theta) is)
        if (g1 == T(0)) {
            lmag = cr;
            ang = ci;
        } else {
            const T zr = T(1) + g1 * cr, zi = g1 * ci;
            lmag = T(0.5) * dsa_log(zr * zr + zi * zi) / g1;
            ang = atan2(zi, zr) / g1;
        }
        if (g2 == T(0)) return lmag;
        ang -= T(2) * pi * rint(ang / (T(2) * pi));
        return (dsa_exp(g2 * lmag) * cos(ang * g2) - T(1)) / g2;
    };
    // split into X[k], X[H - k] and map both (C2 is real and even: cb[k], k = 0 .. H, carries it all)
    for (int k = threadIdx.x; k <= (H >> 1); k += blockDim.x) {
        if (k == 0) {
            const T zr = re[0], zi = im[0];
            cb[0] = gmap(zr + zi, T(0));
            cb[H] = gmap(zr - zi, T(0));
        } else {
            const int pa = fft_brev(k, lgh), pb = fft_brev(H - k, lgh);
            const T ar = re[pa], ai = im[pa], br = re[pb], bi = -im[pb];          // A = Z[k], B = conj Z[H - k]
            const T sr = T(0.5) * (ar + br), si = T(0.5) * (ai + bi), dr = T(0.5) * (ar - br), di = T(0.5) * (ai - bi);
            const T wr = tw[2 * k], wi = tw[2 * k + 1];                            // W_n^k = (cos, -sin)(2 pi k / n)
            const T pr = wr * dr - wi * di, pi_ = wr * di + wi * dr;              // W D
            cb[k] = gmap(sr + pi_, si - pr);                                       // X[k]     = S - i W D
            cb[H - k] = gmap(sr - pi_, -si - pr);                                  // X[H - k] = conj(S + i W D)
        }
    }
    __syncthreads();
    for (int m = threadIdx.x; m < H; m += blockDim.x) {   // pack the even sequence C2[0 .. n - 1]: C2[j] = cb[j <= H ? j : n - j]
        const int j0 = 2 * m, j1 = 2 * m + 1;
        re[m] = cb[j0 <= H ? j0 : nfft - j0];
        im[m] = cb[j1 <= H ? j1 : nfft - j1];
    }
    __syncthreads();
    lds_fft_pow2(re, im, H, lgh, tw, 2);
    T* out = c2 + f * (long)(out_order + 1);
    T sc = T(2) / T(nfft), o0 = k0;
    if (flags & 2) {   // ignorm.py:99-109
        if (g2 == T(0)) o0 = dsa_log(k0);
        else {
            const T zz = dsa_pow(k0, g2);
            o0 = (zz - T(1)) / g2;
            sc *= zz;
        }
    }
    if (flags & 4) sc *= g2;
    if (flags & 8) o0 = o0 * g2 + T(1);
    for (int m = threadIdx.x; m <= out_order; m += blockDim.x) {
        T v;
        if (m == 0) {
            v = o0;
        } else {
            const int n = m <= H ? m : nfft - m;   // the inverse transform of a real even spectrum is even
            T y;                                   // Re of the length-n transform of C2 at index n
            if (n == H) {
                y = re[0] - im[0];
            } else {
                const int pa = fft_brev(n, lgh), pb = fft_brev(H - n, lgh);
                const T ar = re[pa], ai = im[pa], br = re[pb], bi = -im[pb];
                const T dr = T(0.5) * (ar - br), di = T(0.5) * (ai - bi);
                y = T(0.5) * (ar + br) + tw[2 * n] * di + tw[2 * n + 1] * dr;
            }
            v = sc * y;
        }
        out[m] = v;
    }
}

// Backward of gc2gc_fused_kernel (flags = 0) in ONE launch per row: gc1 from the row c1 and the cotangent g2 of c2.
//   c2[0] = c1[0];  c2[m] = 2 c02[m],  c02 = Re ifft(C2),  C2[k] = f(X[k]) for the half spectrum k = 0 .. H of X = fft(c01).
// Three half-length transforms in LDS: X is recomputed from c01; the cotangent of the even spectrum is a cosine transform of
// g2, gcb[k] = (2 / n) w_k Re fft(g)[k] (w = 1 at k = 0, H, else 2: cb[k] is read for j = k and j = n - k); the element-wise
// chain rule gives (gXr, gXi)[k]; and gc01[m] = sum_{k=0}^{H} gXr[k] cos(2 pi k m / n) - gXi[k] sin(2 pi k m / n) is the
// unnormalised inverse real transform of the Hermitian spectrum Y (Y[0] = gXr[0], Y[H] = gXr[H], Y[k] = (gXr + i gXi)[k] / 2),
// run as the conjugate of a forward half-length transform of Z[k] = E[k] + i O[k], E = (Y[k] + conj Y[H-k]) / 2,
// O = conj(W)^k (Y[k] - conj Y[H-k]) / 2.  LDS: re[H] | im[H] | xr[H+1] | xi[H+1] | gcb[H+1].
template <typename T>
__global__ __launch_bounds__(256) void gc2gc_fused_bwd_kernel(const T* __restrict__ c1, const T* __restrict__ g2row, int n_in,
                                                             int out_order, T g1, T g2, int nfft, const T* __restrict__ tw,
                                                             T* __restrict__ gc1)
{
    extern __shared__ unsigned char smem_raw[];
    const int H = nfft >> 1;
    T* re = reinterpret_cast<T*>(smem_raw);
    T* im = re + H;
    T* xr = im + H;
    T* xi = xr + (H + 1);
    T* gcb = xi + (H + 1);
    const long f = blockIdx.x;
    const T* row = c1 + f * n_in;
    const T* grow = g2row + f * (long)(out_order + 1);
    const int lgh = 30 - __clz(nfft);
    constexpr T pi = T(kPi);
    // half-length transform of a packed real sequence, then the split into the half spectrum (dr, di)[0 .. H]
    auto split_to = [&](T* dr, T* di) {
        for (int k = threadIdx.x; k <= (H >> 1); k += blockDim.x) {
            if (k == 0) {
                const T zr = re[0], zi = im[0];
                dr[0] = zr + zi;
                dr[H] = zr - zi;
                if (di) {
                    di[0] = T(0);
                    di[H] = T(0);
                }
            } else {
                const int pa = fft_brev(k, lgh), pb = fft_brev(H - k, lgh);
                const T ar = re[pa], ai = im[pa], br = re[pb], bi = -im[pb];
                const T sr = T(0.5) * (ar + br), si = T(0.5) * (ai + bi), dr_ = T(0.5) * (ar - br), di_ = T(0.5) * (ai - bi);
                const T wr = tw[2 * k], wi = tw[2 * k + 1];
                const T pr = wr * dr_ - wi * di_, pi_ = wr * di_ + wi * dr_;
                dr[k] = sr + pi_;
                dr[H - k] = sr - pi_;
                if (di) {
                    di[k] = si - pr;
                    di[H - k] = -si - pr;
                }
            }
        }
    };
    // ---- X = fft(c01) ----
    for (int n = threadIdx.x; n < H; n += blockDim.x) {
        const int i0 = 2 * n, i1 = 2 * n + 1;
        re[n] = (i0 >= 1 && i0 < n_in) ? row[i0] : T(0);
        im[n] = i1 < n_in ? row[i1] : T(0);
    }
    __syncthreads();
    lds_fft_pow2(re, im, H, lgh, tw, 2);
    split_to(xr, xi);
    __syncthreads();
    // ---- cosine transform of the cotangent: g[0] = 0, g[m] = g2[m] ----
    for (int n = threadIdx.x; n < H; n += blockDim.x) {
        const int i0 = 2 * n, i1 = 2 * n + 1;
        re[n] = (i0 >= 1 && i0 <= out_order) ? grow[i0] : T(0);
        im[n] = i1 <= out_order ? grow[i1] : T(0);
    }
    __syncthreads();
    lds_fft_pow2(re, im, H, lgh, tw, 2);
    split_to(gcb, static_cast<T*>(nullptr));
    __syncthreads();
    // ---- element-wise chain rule: (xr, xi)[k] <- (gXr, gXi)[k] ----
    for (int k = threadIdx.x; k <= H; k += blockDim.x) {
        const T cr = xr[k], ci = xi[k];
        const T gc = gcb[k] * ((k == 0 || k == H) ? T(2) : T(4)) / T(nfft);
        T lmag, ang, l_r, l_i, a_r, a_i;   // log |s|, angle(s) and their partial derivatives with respect to (cr, ci)
        if (g1 == T(0)) {
            lmag = cr; ang = ci;
            l_r = T(1); l_i = T(0); a_r = T(0); a_i = T(1);
        } else {
            const T zr = T(1) + g1 * cr, zi = g1 * ci, r2 = zr * zr + zi * zi;
            lmag = T(0.5) * dsa_log(r2) / g1;
            ang = atan2(zi, zr) / g1;
            l_r = zr / r2; l_i = zi / r2; a_r = -zi / r2; a_i = zr / r2;
        }
        T f_l, f_a;
        if (g2 == T(0)) {
            f_l = T(1); f_a = T(0);
        } else {
            ang -= T(2) * pi * rint(ang / (T(2) * pi));
            const T e = dsa_exp(g2 * lmag);
            f_l = e * cos(ang * g2);
            f_a = -e * sin(ang * g2);
        }
        xr[k] = gc * (f_l * l_r + f_a * a_r);
        xi[k] = gc * (f_l * l_i + f_a * a_i);
    }
    __syncthreads();
    // ---- gc01 = 2 * conj(fft_H(conj Z)) unpacked ----
    for (int k = threadIdx.x; k < H; k += blockDim.x) {
        T yr, yi, br, bi;                      // Y[k], conj Y[H - k]
        if (k == 0) {
            yr = xr[0]; yi = T(0);
            br = xr[H]; bi = T(0);
        } else {
            yr = T(0.5) * xr[k]; yi = T(0.5) * xi[k];
            br = T(0.5) * xr[H - k]; bi = -T(0.5) * xi[H - k];
        }
        const T er = T(0.5) * (yr + br), ei = T(0.5) * (yi + bi), dr = T(0.5) * (yr - br), di = T(0.5) * (yi - bi);
        const T wr = tw[2 * k], wi = -tw[2 * k + 1];            // conj(W)^k = (cos, +sin)(2 pi k / n)
        const T or_ = wr * dr - wi * di, oi = wr * di + wi * dr;  // O[k]
        // Z = E + i O = (er - oi) + i (ei + or); the transform runs on conj Z
        re[k] = er - oi;
        im[k] = -(ei + or_);
    }
    __syncthreads();
    lds_fft_pow2(re, im, H, lgh, tw, 2);
    T* out = gc1 + f * n_in;
    for (int m = threadIdx.x; m < n_in; m += blockDim.x) {
        T v;
        if (m == 0) {
            v = grow[0];
        } else if (m >= nfft) {
            v = T(0);                          // (rows longer than the transform are cropped by the forward)
        } else {
            const int pos = fft_brev(m >> 1, lgh);
            v = T(2) * ((m & 1) ? -im[pos] : re[pos]);
        }
        out[m] = v;
    }
}

template <typename T>
static int gc2gc_launch(const void* c1, int64_t F, int n_in, int out_order, double g1, double g2, int nfft, const void* tw, int flags,
                        void* c2, hipStream_t st)
{
    const size_t lds = sizeof(T) * (3 * (size_t)(nfft / 2) + 1);
    // short transforms: one wave per row (two butterflies per lane and pass, the passes' barriers are single-wave barriers)
    const int block = nfft <= 1024 ? 64 : 256;
    if (int rc = launch_lds<gc2gc_fused_kernel<T>>(lds > 48 * 1024 ? 150 * 1024 : 0, "gc2gc: cannot raise the dynamic LDS limit%s", dim3((unsigned)F),
                                                   dim3(block), lds, st, (const T*)c1, n_in, out_order, (T)g1, (T)g2, nfft, (const T*)tw, flags,
                                                   (T*)c2))
        return rc;
    return check_launch("gc2gc_fused");
}

}  // namespace dsa

using namespace dsa;

// ---- gain normalisation of generalized cepstra and its inverse as ONE launch each (gnorm.py:102-112, ignorm.py:99-109), forward only ----
//   forward:  (K, x1 / z),  z = 1 + gamma x0,  K = z^(1/gamma)      (gamma = 0: (exp x0, x1))
//   inverse:  ((z - 1) / gamma, y1 z),  z = K^gamma                   (gamma = 0: (log K, y1))
// As stock tensor operations (split, multiply-add, pow, divide, cat) a call was five to six launches of ~5 us; the mel-generalized
// analysis makes three such calls around its Newton steps.  (With a gradient wanted the modules keep the stock composition.)
namespace dsa {
template <typename T>
__global__ __launch_bounds__(256) void gnorm_rows_kernel(const T* __restrict__ x, long F, int n, T gamma, int inverse, T* __restrict__ out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= F * n) return;
    // (32-bit division where the element count allows it; the launch is ~10 us per 1.3 M elements either way: its own latency)
    const long f = F * n < (1L << 31) ? (long)((unsigned)i / (unsigned)n) : i / n;
    const int m = (int)(i - f * n);
    const T x0 = x[f * n];
    T scale, head;
    if (!inverse) {
        if (gamma == T(0)) {
            head = dsa_exp(x0);
            scale = T(1);
        } else {
            const T z = T(1) + gamma * x0;
            head = dsa_pow(z, T(1) / gamma);
            scale = T(1) / z;
        }
    } else {
        if (gamma == T(0)) {
            head = dsa_log(x0);
            scale = T(1);
        } else {
            const T z = dsa_pow(x0, gamma);
            head = (z - T(1)) / gamma;
            scale = z;
        }
    }
    out[i] = m == 0 ? head : (!inverse && gamma != T(0) ? x[i] / (T(1) + gamma * x0) : x[i] * scale);
}
// b = (sqrt(r_0 + gamma sum_m r_{m+1} b_eps_m), b_join): the gain of a Newton step of the mel-generalized analysis joined to its
// coefficients (mgcep.py:213-215, 221, 231-233).  A row per wave (coalesced reads, the sum over the wave by DPP; one thread per row
// read 25 scattered words per lane: 19 us per 51 200 rows); orders above 64 loop.
template <typename T>
__global__ __launch_bounds__(256) void mgcep_gain_kernel(const T* __restrict__ r, const T* __restrict__ b_eps, const T* __restrict__ b_join,
                                                        long F, int M, T gamma, T* __restrict__ b)
{
    const int lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= F) return;
    T acc = T(0);
    for (int m = lane; m < M; m += 64) {
        acc += r[f * (M + 1) + m + 1] * b_eps[f * M + m];
        b[f * (M + 1) + m + 1] = b_join[f * M + m];
    }
    acc = wave_sum(acc);
    if (lane == 0) b[f * (M + 1)] = sqrt(r[f * (M + 1)] + gamma * acc);
}
}  // namespace dsa

DSA_EXPORT int dsa_gnorm_fwd(const void* x, int64_t F, int32_t n, double gamma, int32_t inverse, int32_t dtype, void* out, void* stream)
{
    DSA_REQUIRE(F >= 0 && n >= 1 && (F == 0 || (x && out)), "gnorm: invalid arguments");
    DSA_REQUIRE(gamma >= -1 && gamma <= 1, "gnorm: gamma must be in [-1, 1]");
    if (F == 0) return DSA_OK;
    const dim3 grid((unsigned)((F * n + 255) / 256));
    return with_dtype(dtype, "gnorm", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dsa::gnorm_rows_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, (long)F, (int)n, (T)gamma, (int)inverse,
                           (T*)out);
        return check_launch(inverse ? "ignorm_fwd" : "gnorm_fwd");
    });
}

DSA_EXPORT int dsa_mgcep_gain(const void* r, const void* b_eps, const void* b_join, int64_t F, int32_t M, double gamma, int32_t dtype,
                              void* b, void* stream)
{
    DSA_REQUIRE(F >= 0 && M >= 1 && (F == 0 || (r && b_eps && b_join && b)), "mgcep_gain: invalid arguments");
    if (F == 0) return DSA_OK;
    const dim3 grid((unsigned)((F + 3) / 4));
    return with_dtype(dtype, "mgcep_gain", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(dsa::mgcep_gain_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)r, (const T*)b_eps, (const T*)b_join, (long)F,
                           (int)M, (T)gamma, (T*)b);
        return check_launch("mgcep_gain");
    });
}

DSA_EXPORT int dsa_mgcep_step(const void* x, const void* b1, int64_t F, int32_t fft_length, int32_t M, double gamma, const void* images,
                              int32_t dtype, void* pt, void* qt, void* r, void* stream)
{
    DSA_REQUIRE(F >= 0 && M >= 1, "mgcep_step: sizes must be positive");
    DSA_REQUIRE(gamma != 0.0 && gamma >= -1.0 && gamma < 0.0, "mgcep_step: gamma must be in [-1, 0)");
    if (dtype != DSA_F32 || fft_length != 512 || M > 24) return fail(DSA_ERR_UNSUPPORTED, "mgcep_step: needs float32, fft_length 512, cep_order <= 24%s");
    if (F == 0) return DSA_OK;
    hipLaunchKernelGGL(mgcep_step_kernel, dim3((unsigned)((F + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)x, (const float*)b1,
                       (long)F, (int)M, (float)gamma, (const float*)images, (float*)pt, (float*)qt, (float*)r);
    return check_launch("mgcep_step");
}

DSA_EXPORT int dsa_mgcep_step_bwd_h(const void* x, const void* b1, const void* gpt, const void* gqt, const void* gr, int64_t F,
                                    int32_t fft_length, int32_t M, double gamma, const void* images_bwd_h, int32_t dtype, const void* gx_in,
                                    void* gx, void* gb1, void* stream)
{
    DSA_REQUIRE(F >= 0, "mgcep_step_bwd_h: sizes must be positive");
    DSA_REQUIRE(F == 0 || (x && b1 && gpt && gqt && gr && images_bwd_h && gx && gb1), "mgcep_step_bwd_h: null pointer");
    DSA_REQUIRE(gamma != 0.0 && gamma >= -1.0 && gamma < 0.0, "mgcep_step_bwd_h: gamma must be in [-1, 0)");
    if (dtype != DSA_F32 || fft_length != 512 || M != 24)
        return fail(DSA_ERR_UNSUPPORTED, "mgcep_step_bwd_h: needs float32, fft_length 512, cep_order 24%s");
    if (F == 0) return DSA_OK;
    return mgcep_step_bwd_h(x, b1, gpt, gqt, gr, F, gamma, images_bwd_h, gx_in, gx, gb1, (hipStream_t)stream);
}

DSA_EXPORT int dsa_mgcep_step_solve(const void* x, const void* b1, int64_t F, int32_t fft_length, int32_t M, double gamma,
                                    const void* images_h, int32_t dtype, void* b1_out, void* r, void* pt, void* qt, int32_t n_steps,
                                    void* b1_prev, void* stream)
{
    DSA_REQUIRE(F >= 0 && n_steps >= 1, "mgcep_step_solve: sizes must be positive");
    DSA_REQUIRE(F == 0 || (x && b1 && images_h && b1_out && r), "mgcep_step_solve: null pointer");
    DSA_REQUIRE(gamma != 0.0 && gamma > -1.0 && gamma < 0.0, "mgcep_step_solve: gamma must be in (-1, 0)");
    if (dtype != DSA_F32 || fft_length != 512 || M != 24)
        return fail(DSA_ERR_UNSUPPORTED, "mgcep_step_solve: needs float32, fft_length 512, cep_order 24%s");
    if (F == 0) return DSA_OK;
    return mgcep_step_solve_fwd(x, b1, F, gamma, images_h, b1_out, r, (hipStream_t)stream, pt, qt, n_steps, b1_prev);
}

DSA_EXPORT int dsa_mgcep_step_bwd(const void* x, const void* b1, const void* gpt, const void* gqt, const void* gr, int64_t F,
                                  int32_t fft_length, int32_t M, double gamma, const void* images_bwd, int32_t dtype, const void* gx_in,
                                  void* gx, void* gb1, void* stream)
{
    DSA_REQUIRE(F >= 0 && M >= 1, "mgcep_step_bwd: sizes must be positive");
    DSA_REQUIRE(gamma != 0.0 && gamma >= -1.0 && gamma < 0.0, "mgcep_step_bwd: gamma must be in [-1, 0)");
    if (dtype != DSA_F32 || fft_length != 512 || M > 24)
        return fail(DSA_ERR_UNSUPPORTED, "mgcep_step_bwd: needs float32, fft_length 512, cep_order <= 24%s");
    if (F == 0) return DSA_OK;
    hipLaunchKernelGGL(mgcep_step_bwd_kernel, dim3((unsigned)((F + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                       (const float*)b1, (const float*)gpt, (const float*)gqt, (const float*)gr, (long)F, (int)M, (float)gamma,
                       (const float*)images_bwd, (const float*)gx_in, (float*)gx, (float*)gb1);
    return check_launch("mgcep_step_bwd");
}

DSA_EXPORT int dsa_mgcep_spectra(const void* x, const void* b1, int64_t F, int32_t fft_length, int32_t M, const void* Cr,
                                 const void* Ci, double gamma, int32_t dtype, void* out, void* stream)
{
    DSA_REQUIRE(F >= 0 && fft_length > 1 && fft_length % 2 == 0 && M >= 1, "mgcep_spectra: sizes must be positive");
    DSA_REQUIRE(gamma != 0.0 && gamma >= -1.0 && gamma < 0.0, "mgcep_spectra: gamma must be in [-1, 0)");
    if (M > kMsMaxM) return fail(DSA_ERR_UNSUPPORTED, "mgcep_spectra: cep_order above 64%s");
    if (F == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    const int K = fft_length / 2 + 1;
    return with_dtype(dtype, "mgcep_spectra", [&](auto tag) { return mgcep_spectra_launch<decltype(tag)>(x, b1, F, K, M, Cr, Ci, gamma, out, st); });
}

DSA_EXPORT int dsa_gc2gc_fwd(const void* c1, int64_t F, int32_t n_in, int32_t out_order, double in_gamma, double out_gamma,
                             int32_t nfft, const void* twiddle, int32_t flags, int32_t dtype, void* c2, void* stream)
{
    DSA_REQUIRE(F >= 0 && n_in >= 1 && out_order >= 0, "gc2gc: sizes must be positive");
    DSA_REQUIRE(nfft >= 4 && (nfft & (nfft - 1)) == 0, "gc2gc: n_fft must be a power of two");
    DSA_REQUIRE(flags >= 0 && flags < 16, "gc2gc: unknown flags");
    if (out_order + 1 > nfft || F > 0x7fffffffLL) return fail(DSA_ERR_UNSUPPORTED, "gc2gc: out_order + 1 must not exceed n_fft%s");
    if (F == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DSA_F32 && (size_t)nfft * 8 <= 150 * 1024) return gc2gc_launch<float>(c1, F, n_in, out_order, in_gamma, out_gamma, nfft, twiddle, flags, c2, st);
    if (dtype == DSA_F64 && (size_t)nfft * 16 <= 150 * 1024) return gc2gc_launch<double>(c1, F, n_in, out_order, in_gamma, out_gamma, nfft, twiddle, flags, c2, st);
    return fail(DSA_ERR_UNSUPPORTED, "gc2gc: unsupported dtype or n_fft too long for LDS%s");
}

DSA_EXPORT int dsa_gc2gc_bwd(const void* c1, const void* g2, int64_t F, int32_t n_in, int32_t out_order, double in_gamma,
                             double out_gamma, int32_t nfft, const void* twiddle, int32_t dtype, void* gc1, void* stream)
{
    DSA_REQUIRE(F >= 0 && n_in >= 1 && out_order >= 0, "gc2gc_bwd: sizes must be positive");
    DSA_REQUIRE(nfft >= 4 && (nfft & (nfft - 1)) == 0, "gc2gc_bwd: n_fft must be a power of two (>= 4)");
    DSA_REQUIRE(out_order + 1 <= nfft, "gc2gc_bwd: out_order + 1 must not exceed n_fft");
    if (F == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    const int block = nfft <= 1024 ? 64 : 256;
    auto launch = [&](auto tag) {
        using T = decltype(tag);
        const size_t lds = sizeof(T) * (5 * (size_t)(nfft / 2) + 3);
        if (int rc = launch_lds<gc2gc_fused_bwd_kernel<T>>(lds > 48 * 1024 ? 150 * 1024 : 0, "gc2gc_bwd: cannot raise the dynamic LDS limit%s",
                                                           dim3((unsigned)F), dim3(block), lds, st, (const T*)c1, (const T*)g2, n_in, out_order,
                                                           (T)in_gamma, (T)out_gamma, nfft, (const T*)twiddle, (T*)gc1))
            return rc;
        return check_launch("gc2gc_fused_bwd");
    };
    if (dtype == DSA_F32 && (size_t)nfft * 10 + 64 <= 150 * 1024) return launch(float{});
    if (dtype == DSA_F64 && (size_t)nfft * 20 + 64 <= 150 * 1024) return launch(double{});
    return fail(DSA_ERR_UNSUPPORTED, "gc2gc_bwd: unsupported dtype or n_fft too long for LDS%s");
}
