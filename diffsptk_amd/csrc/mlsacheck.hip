// MLSA filter stability check (include/diffsptk_amd.h, section a16):
//   mlsacheck  MLSADigitalFilterStabilityCheck._forward, mlsacheck.py:181-230   (about a dozen stock operators there, in the FFT modes
//              three complex (F, n_fft/2+1) temporaries kept for the backward, and a host read of torch.any)
// forward and adjoint in one launch each, float64 arithmetic whatever the data's dtype, one rounding at the store, no workspace: the
// adjoint recomputes everything from the input mel-cepstrum.
//
// Per frame, with av_m = (-alpha)^m and thr the threshold:  gain = sum_m mc_m av_m,  c = mc with c_0 -= gain  (mlsacheck.py:191, 198).
//   fast   a = max(sum_m c_m, 1e-16), s = min(1, thr / a), out = s c, out_0 += gain                                 (:196, 202, 217-226)
//   scale  C_k = sum_m c_m e^{-j 2 pi k m / n_fft}, k < K = n_fft / 2 + 1;  a = max(max_k |C_k|, 1e-16), s = min(1, thr / a)   (:199-202)
//   clip   s_k = min(1, thr / |C_k|) per bin                                                                           (:215)
// and then out_m = (1 / N') sum_k w_k Re(s_k C_k e^{+j 2 pi k m / N'}), m <= M, N' = 2 (K - 1) -- torch's default irfft length, n_fft
// only when that is even --, w = 2 except w_0 = w_{K-1} = 1 whose imaginary parts the inverse ignores; out_0 += gain (:228-229).
// No FFT: M + 1 inputs are non-zero and M + 1 outputs are kept, so both transforms are (M + 1) x K sums.  The complex exponentials come
// from the rotation recurrence z <- z w in float64, seeded by sincospi of an exactly representable argument per bin (or per output).
//
// For EVEN n_fft the two transforms invert each other on the first M + 1 samples (N' = n_fft >= M + 1), hence
//   * a frame that nothing clips (a <= thr) leaves with the INPUT'S BITS, and its gradient with the cotangent's -- a departure: the
//     reference re-rounds c_0 through (c_0 - gain) * 1 + gain and the others through its FFT pair;
//   * scale mode is out = s c;
//   * the tuned kernel's clip mode subtracts what the clipped bins lose, c_m - (1 / N) sum_{k clipped} w_k (1 - s_k) Re(C_k e^{..}).
// For ODD n_fft, N' = n_fft - 1 and irfft(rfft(c)) is another vector than c even when nothing is clipped: the frame goes through both
// transforms as in the reference.
//
// The adjoint.  h = the gradient with respect to c of <g, T(c)>; then gmc = h + (g_0 - h_0) av (c_0 = mc_0 - gain, out_0 += gain).
//   fast   h = s g - (s / a) <g, c> 1                       scale  h = s P^T g - (s / a) <P^T g, c> d|C_k*| / dc, k* the bin of the maximum
//   clip   the adjoint of the inverse gives G_k; a clipped bin keeps s_k times the part of G_k at right angles to C_k; the adjoint of the
//          forward transform takes it back to m.
// torch.clip passes the gradient on its bound: a frame with a == thr (a bin with |C_k| == thr) leaves unchanged in value but its
// gradient goes through thr / a.
//
// TUNED (float32, M <= 63, n_fft = 256 or fast mode): one wave per frame.  Lane m holds sample m; lane l owns the bins l and l + 64, bin
// 128 is a wave sum with alternating signs; the maximum is a wave reduction.  Everything that depends on the lane alone -- av_m, the
// bins' rotation steps, the inverse's seeds -- is computed once per wave, which walks a grid-stride loop of frames.  The inverse over the
// clipped bins splits the bins over 64 / pow2ceil(M + 1) lane groups that are summed by shuffles.
// GENERIC (everything else: float64, M > 63, any n_fft, odd ones included): one wave per frame too, the row and the K bins in dynamic
// LDS, lanes over the bins for the forward transform and over m for the inverse; the powers of -alpha in LDS, once per workgroup.
#include "common.h"

namespace dsa {
namespace {

constexpr int MC_TUNED_MAX_ORDER = 63;
constexpr int MC_TUNED_NFFT = 256;
constexpr int MC_MAX_LDS = 144 * 1024;
constexpr double kMcFloor = 1e-16;   // mlsacheck.py:202

// (-alpha)^m as (-alpha) ** arange(M + 1) gives it in float64 (mlsacheck.py:165): 0^0 = 1
__device__ __forceinline__ double mc_alpha_pow(double alpha, int m)
{
    if (m == 0) return 1.0;
    const double p = pow(fabs(alpha), (double)m);
    return ((m & 1) && alpha > 0.0) ? -p : p;
}
// z <- z w
__device__ __forceinline__ void mc_rot(double& zr, double& zi, double wr, double wi)
{
    const double r = fma(zr, wr, -zi * wi), i = fma(zr, wi, zi * wr);
    zr = r;
    zi = i;
}
__device__ __forceinline__ double mc_abs(double r, double i) { return sqrt(fma(r, r, i * i)); }

// the largest amplitude of the wave with its bin and its spectrum value; among equals the lowest bin
__device__ __forceinline__ void mc_wave_argmax(double& A, int& k, double& cr, double& ci)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double A2 = __shfl_xor(A, o, 64), r2 = __shfl_xor(cr, o, 64), i2 = __shfl_xor(ci, o, 64);
        const int k2 = __shfl_xor(k, o, 64);
        if (A2 > A || (A2 == A && k2 < k)) {
            A = A2;
            k = k2;
            cr = r2;
            ci = i2;
        }
    }
}
__device__ __forceinline__ void mc_take_larger(double& A, int& k, double& cr, double& ci, double A2, int k2, double r2, double i2)
{
    if (A2 > A) {
        A = A2;
        k = k2;
        cr = r2;
        ci = i2;
    }
}

// ---------------------------------------------------------------------------------------------- tuned: float32, M <= 63, n_fft = 256
template <bool BWD>
__global__ __launch_bounds__(64) void mlsacheck_tuned_kernel(const float* __restrict__ gout, const float* __restrict__ mc, long F, int M,
                                                             double alpha, double thr, int mode, float* __restrict__ out,
                                                             int* __restrict__ unstable)
{
    __shared__ double c[64], g[64];
    __shared__ double Er[MC_TUNED_NFFT / 2 + 1], Ei[MC_TUNED_NFFT / 2 + 1];   // what the clipped bins lose (forward) / do not pass (backward)
    constexpr int K = MC_TUNED_NFFT / 2 + 1;
    constexpr double inv_n = 1.0 / MC_TUNED_NFFT;
    const int lane = threadIdx.x, M1 = M + 1;
    const bool live = lane <= M;
    const double av = live ? mc_alpha_pow(alpha, lane) : 0.0;
    const double sgn = (lane & 1) ? -1.0 : 1.0;
    double w0r, w0i, w1r, w1i;   // e^{j 2 pi k / 256} of the bins k = lane and lane + 64
    sincospi((double)lane * (2.0 * inv_n), &w0i, &w0r);
    sincospi((double)(lane + 64) * (2.0 * inv_n), &w1i, &w1r);
    // the inverse over the bins: 64 / P2 groups of P2 lanes, group q takes the bins [k0, k1) for the samples m = lane mod P2
    int P2 = 1;
    while (P2 < M1) P2 <<= 1;
    const int mm = lane & (P2 - 1), per = (K + 64 / P2 - 1) / (64 / P2);
    const int k0 = (lane / P2) * per, k1 = k0 + per < K ? k0 + per : K;
    double s0r, s0i, str, sti;   // e^{j 2 pi m k0 / 256} and the step e^{j 2 pi m / 256}
    sincospi((double)((mm * k0) & (MC_TUNED_NFFT - 1)) * (2.0 * inv_n), &s0i, &s0r);
    sincospi((double)mm * (2.0 * inv_n), &sti, &str);

    for (long f = blockIdx.x; f < F; f += gridDim.x) {
        const long at = f * M1 + lane;
        const float xin = live ? mc[at] : 0.f;
        const float gin = (BWD && live) ? gout[at] : 0.f;
        const double x = (double)xin, gd = (double)gin;
        const double gain = wave_sum(x * av);
        const double cm = lane == 0 ? x - gain : x;   // c of this lane's sample; 0 beyond M
        const double g0 = BWD ? __shfl(gd, 0, 64) : 0.0;

        if (mode == DSA_MLSACHECK_FAST) {
            const double a_raw = wave_sum(cm), a = a_raw > kMcFloor ? a_raw : kMcFloor;
            const double s = thr / a;
            if (!BWD) {
                const bool moved = a > thr;
                if (moved && unstable && lane == 0) *unstable = 1;
                if (live) out[at] = moved ? (float)fma(s, cm, lane == 0 ? gain : 0.0) : xin;
            } else {
                const bool active = a >= thr;
                const double dot = wave_sum(gd * cm);
                const double h = fma(s, gd, a_raw >= kMcFloor ? -(s / a) * dot : 0.0);
                const double h0 = __shfl(h, 0, 64);
                if (live) out[at] = active ? (float)fma(g0 - h0, av, h) : gin;
            }
            continue;
        }

        __syncthreads();   // the frame before this one has been read out of c, g and E
        c[lane] = cm;
        if (BWD) g[lane] = gd;
        __syncthreads();
        double z0r = 1.0, z0i = 0.0, z1r = 1.0, z1i = 0.0;
        double c0r = 0.0, c0i = 0.0, c1r = 0.0, c1i = 0.0, g0r = 0.0, g0i = 0.0, g1r = 0.0, g1i = 0.0;
        for (int m = 0; m <= M; ++m) {
            const double v = c[m];
            c0r = fma(v, z0r, c0r);
            c0i = fma(-v, z0i, c0i);
            c1r = fma(v, z1r, c1r);
            c1i = fma(-v, z1i, c1i);
            if (BWD) {
                const double u = g[m];
                g0r = fma(u, z0r, g0r);
                g0i = fma(-u, z0i, g0i);
                g1r = fma(u, z1r, g1r);
                g1i = fma(-u, z1i, g1i);
            }
            mc_rot(z0r, z0i, w0r, w0i);
            mc_rot(z1r, z1i, w1r, w1i);
        }
        const double cn = wave_sum(cm * sgn);   // bin 128: real
        const double A0 = mc_abs(c0r, c0i), A1 = mc_abs(c1r, c1i), An = fabs(cn);
        const double wt0 = (lane == 0 ? 1.0 : 2.0) * inv_n, wt1 = 2.0 * inv_n, wtn = inv_n;   // w_k / N

        if (!BWD) {
            double amax = wave_max(A0 > A1 ? A0 : A1);
            amax = An > amax ? An : amax;
            const double a = amax > kMcFloor ? amax : kMcFloor;
            const bool moved = a > thr;   // the same in every lane
            if (moved && unstable && lane == 0) *unstable = 1;
            if (!moved) {
                if (live) out[at] = xin;
            } else if (mode == DSA_MLSACHECK_SCALE) {
                if (live) out[at] = (float)fma(thr / a, cm, lane == 0 ? gain : 0.0);
            } else {
                const double l0 = A0 > thr ? wt0 * (1.0 - thr / A0) : 0.0, l1 = A1 > thr ? wt1 * (1.0 - thr / A1) : 0.0;
                Er[lane] = l0 * c0r;
                Ei[lane] = l0 * c0i;
                Er[lane + 64] = l1 * c1r;
                Ei[lane + 64] = l1 * c1i;
                if (lane == 0) {
                    Er[K - 1] = An > thr ? wtn * (1.0 - thr / An) * cn : 0.0;
                    Ei[K - 1] = 0.0;
                }
                __syncthreads();
                double zr = s0r, zi = s0i, acc = 0.0;
                for (int k = k0; k < k1; ++k) {
                    acc = fma(Er[k], zr, acc);
                    acc = fma(-Ei[k], zi, acc);
                    mc_rot(zr, zi, str, sti);
                }
                for (int o = P2; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
                if (live) out[at] = (float)(cm - acc + (lane == 0 ? gain : 0.0));
            }
        } else if (mode == DSA_MLSACHECK_SCALE) {
            double A = A0, kr = c0r, ki = c0i;
            int kk = lane;
            mc_take_larger(A, kk, kr, ki, A1, lane + 64, c1r, c1i);
            mc_wave_argmax(A, kk, kr, ki);
            mc_take_larger(A, kk, kr, ki, An, K - 1, cn, 0.0);
            const double a = A > kMcFloor ? A : kMcFloor;
            if (!(a >= thr)) {
                if (live) out[at] = gin;
            } else {
                const double s = thr / a, dot = wave_sum(gd * cm);
                const double coef = A >= kMcFloor ? -(s / a) * dot / A : 0.0;
                double sn, cs;
                sincospi((double)((kk * lane) & (MC_TUNED_NFFT - 1)) * (2.0 * inv_n), &sn, &cs);
                const double h = fma(s, gd, coef * fma(kr, cs, -ki * sn));
                const double h0 = __shfl(h, 0, 64);
                if (live) out[at] = (float)fma(g0 - h0, av, h);
            }
        } else {
            const double gn = wave_sum(gd * sgn) * wtn;
            g0r *= wt0;
            g0i *= wt0;
            g1r *= wt1;
            g1i *= wt1;
            const bool cl0 = A0 >= thr && A0 > 0.0, cl1 = A1 >= thr && A1 > 0.0, cln = An >= thr && An > 0.0;
            if (!__ballot(cl0 || cl1 || cln)) {
                if (live) out[at] = gin;
            } else {
                // what a clipped bin does not pass: G - s (G - C <G, C> / A^2)
                double d0r = 0.0, d0i = 0.0, d1r = 0.0, d1i = 0.0;
                if (cl0) {
                    const double s = thr / A0, rad = fma(g0r, c0r, g0i * c0i) / (A0 * A0);
                    d0r = g0r - s * (g0r - c0r * rad);
                    d0i = g0i - s * (g0i - c0i * rad);
                }
                if (cl1) {
                    const double s = thr / A1, rad = fma(g1r, c1r, g1i * c1i) / (A1 * A1);
                    d1r = g1r - s * (g1r - c1r * rad);
                    d1i = g1i - s * (g1i - c1i * rad);
                }
                Er[lane] = d0r;
                Ei[lane] = d0i;
                Er[lane + 64] = d1r;
                Ei[lane + 64] = d1i;
                if (lane == 0) {
                    Er[K - 1] = cln ? gn : 0.0;   // a real bin: all of G is along C, none of it passes
                    Ei[K - 1] = 0.0;
                }
                __syncthreads();
                double zr = s0r, zi = s0i, acc = 0.0;
                for (int k = k0; k < k1; ++k) {
                    acc = fma(Er[k], zr, acc);
                    acc = fma(-Ei[k], zi, acc);
                    mc_rot(zr, zi, str, sti);
                }
                for (int o = P2; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
                const double h = gd - acc;
                const double h0 = __shfl(h, 0, 64);
                if (live) out[at] = (float)fma(g0 - h0, av, h);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- generic: one wave per frame, LDS
// in0: gout (BWD) or unused; LDS: av[M1] (the powers of -alpha, once per workgroup), c[M1], g[M1] (BWD), Pr[K], Pi[K]
template <typename T, bool BWD>
__global__ __launch_bounds__(64) void mlsacheck_generic_kernel(const T* __restrict__ gout, const T* __restrict__ mc, long F, int M, double alpha,
                                                               double thr, int mode, int n_fft, T* __restrict__ out, int* __restrict__ unstable)
{
    extern __shared__ double mc_smem[];
    const int lane = threadIdx.x, M1 = M + 1;
    const bool fft = mode != DSA_MLSACHECK_FAST;
    const int K = fft ? n_fft / 2 + 1 : 1, N2 = fft ? 2 * (K - 1) : 2;
    const bool even = N2 == n_fft;
    double* av = mc_smem;
    double* c = av + M1;
    double* g = c + M1;
    double* Pr = g + (BWD ? M1 : 0);
    double* Pi = Pr + K;
    const double inv_n2 = 1.0 / (double)N2;
    for (int m = lane; m <= M; m += 64) av[m] = mc_alpha_pow(alpha, m);   // (each lane reads back only what it wrote)

    for (long f = blockIdx.x; f < F; f += gridDim.x) {
        const long base = f * M1;
        __syncthreads();
        double part = 0.0;
        for (int m = lane; m <= M; m += 64) {
            const double v = (double)mc[base + m];
            c[m] = v;
            part = fma(v, av[m], part);
            if (BWD) g[m] = (double)gout[base + m];
        }
        const double gain = wave_sum(part);
        __syncthreads();
        if (lane == 0) c[0] -= gain;
        __syncthreads();
        bool pass;        // the frame leaves with the input's (the cotangent's) bits
        double s = 1.0;   // the one factor of fast and scale mode

        if (!fft) {
            double ps = 0.0, pd = 0.0;
            for (int m = lane; m <= M; m += 64) {
                ps += c[m];
                if (BWD) pd = fma(g[m], c[m], pd);
            }
            const double a_raw = wave_sum(ps), a = a_raw > kMcFloor ? a_raw : kMcFloor;
            s = thr / a;
            if (!BWD) {
                pass = !(a > thr);
                if (!pass && unstable && lane == 0) *unstable = 1;
                for (int m = lane; m <= M && !pass; m += 64) out[base + m] = (T)fma(s, c[m], m == 0 ? gain : 0.0);
            } else {
                pass = !(a >= thr);
                const double coef = a_raw >= kMcFloor ? -(s / a) * wave_sum(pd) : 0.0;
                __syncthreads();
                for (int m = lane; m <= M && !pass; m += 64) c[m] = fma(s, g[m], coef);   // h
            }
        } else if (!BWD) {
            double amax = 0.0;
            for (int k = lane; k < K; k += 64) {
                double wr, wi;
                sincospi((double)(2 * k) / (double)n_fft, &wi, &wr);
                double zr = 1.0, zi = 0.0, cr = 0.0, ci = 0.0;
                for (int m = 0; m <= M; ++m) {
                    const double v = c[m];
                    cr = fma(v, zr, cr);
                    ci = fma(-v, zi, ci);
                    mc_rot(zr, zi, wr, wi);
                }
                const double A = mc_abs(cr, ci);
                const bool edge = k == 0 || k == K - 1;
                double sc = (edge ? 1.0 : 2.0) * inv_n2;
                if (mode == DSA_MLSACHECK_CLIP && A > thr) sc *= thr / A;
                Pr[k] = sc * cr;
                Pi[k] = edge ? 0.0 : sc * ci;   // the inverse ignores the imaginary parts of its first and last bin
                amax = A > amax ? A : amax;
            }
            amax = wave_max(amax);
            const double a = amax > kMcFloor ? amax : kMcFloor;
            const bool moved = a > thr;
            if (moved && unstable && lane == 0) *unstable = 1;
            if (mode == DSA_MLSACHECK_SCALE && moved) s = thr / a;
            pass = even && !moved;
            __syncthreads();
            if (!pass && even && mode == DSA_MLSACHECK_SCALE) {
                for (int m = lane; m <= M; m += 64) out[base + m] = (T)fma(s, c[m], m == 0 ? gain : 0.0);
            } else if (!pass) {
                for (int m = lane; m <= M; m += 64) {
                    double wr, wi;
                    sincospi((double)(2 * m) * inv_n2, &wi, &wr);
                    double zr = 1.0, zi = 0.0, acc = 0.0;
                    for (int k = 0; k < K; ++k) {
                        if ((k & 63) == 0 && k) sincospi((double)(2 * (((long)k * m) % N2)) * inv_n2, &zi, &zr);   // (anew every 64 bins: its rounding grows with the steps, 1e-13 at 9 000 bins)
                        acc = fma(Pr[k], zr, acc);
                        acc = fma(-Pi[k], zi, acc);
                        mc_rot(zr, zi, wr, wi);
                    }
                    out[base + m] = (T)fma(s, acc, m == 0 ? gain : 0.0);
                }
            }
        } else {
            // lanes over the bins: C_k, and G_k = the adjoint of the inverse applied to g
            double A = -1.0, kr = 0.0, ki = 0.0, dotp = 0.0;
            int kk = 0;
            bool clipped = false;
            for (int k = lane; k < K; k += 64) {
                double wr, wi, vr, vi;
                sincospi((double)(2 * k) / (double)n_fft, &wi, &wr);
                sincospi((double)(2 * k) * inv_n2, &vi, &vr);
                double zr = 1.0, zi = 0.0, yr = 1.0, yi = 0.0, cr = 0.0, ci = 0.0, gr = 0.0, gi = 0.0;
                for (int m = 0; m <= M; ++m) {
                    const double v = c[m], u = g[m];
                    cr = fma(v, zr, cr);
                    ci = fma(-v, zi, ci);
                    gr = fma(u, yr, gr);
                    gi = fma(-u, yi, gi);
                    mc_rot(zr, zi, wr, wi);
                    mc_rot(yr, yi, vr, vi);
                }
                const bool edge = k == 0 || k == K - 1;
                const double wt = (edge ? 1.0 : 2.0) * inv_n2;
                gr *= wt;
                gi = edge ? 0.0 : gi * wt;
                const double Ak = mc_abs(cr, ci);
                dotp += fma(gr, cr, gi * ci);   // <g, inverse(C)> = <G, C>
                if (mode == DSA_MLSACHECK_CLIP && Ak >= thr && Ak > 0.0) {
                    const double sk = thr / Ak, rad = fma(gr, cr, gi * ci) / (Ak * Ak);
                    gr = sk * (gr - cr * rad);
                    gi = sk * (gi - ci * rad);
                    clipped = true;
                }
                Pr[k] = gr;
                Pi[k] = gi;
                mc_take_larger(A, kk, kr, ki, Ak, k, cr, ci);
            }
            mc_wave_argmax(A, kk, kr, ki);
            double coef = 0.0;
            if (mode == DSA_MLSACHECK_SCALE) {
                const double a = A > kMcFloor ? A : kMcFloor;
                const bool active = a >= thr;
                const double dot = wave_sum(dotp);
                if (active) {
                    s = thr / a;
                    if (A >= kMcFloor) coef = -(s / a) * dot / A;
                }
                pass = even && !active;
            } else {
                pass = even && !__ballot(clipped);
            }
            __syncthreads();
            if (!pass) {
                for (int m = lane; m <= M; m += 64) {
                    double h;
                    if (even && mode == DSA_MLSACHECK_SCALE) {
                        h = s * g[m];
                    } else {
                        double wr, wi;
                        sincospi((double)(2 * m) / (double)n_fft, &wi, &wr);
                        double zr = 1.0, zi = 0.0, acc = 0.0;
                        for (int k = 0; k < K; ++k) {
                            if ((k & 63) == 0 && k) sincospi((double)(2 * (((long)k * m) % n_fft)) / (double)n_fft, &zi, &zr);   // (as the forward)
                            acc = fma(Pr[k], zr, acc);
                            acc = fma(-Pi[k], zi, acc);
                            mc_rot(zr, zi, wr, wi);
                        }
                        h = s * acc;
                    }
                    if (coef != 0.0) {
                        double sn, cs;
                        sincospi((double)(2 * (((long)kk * m) % n_fft)) / (double)n_fft, &sn, &cs);
                        h = fma(coef, fma(kr, cs, -ki * sn), h);
                    }
                    c[m] = h;
                }
            }
        }

        if (pass) {
            const T* from = BWD ? gout : mc;
            for (int m = lane; m <= M; m += 64) out[base + m] = from[base + m];
        } else if (BWD) {
            __syncthreads();
            const double lift = g[0] - c[0];
            for (int m = lane; m <= M; m += 64) out[base + m] = (T)fma(lift, av[m], c[m]);
        }
    }
}

template <typename T, bool BWD>
int mlsacheck_generic_launch(const void* gout, const void* mc, int64_t F, int M, double alpha, double thr, int mode, int n_fft, void* out,
                             void* unstable, hipStream_t st)
{
    const char* name = BWD ? "mlsacheck_generic_bwd" : "mlsacheck_generic_fwd";
    const int64_t K = mode == DSA_MLSACHECK_FAST ? 1 : n_fft / 2 + 1;
    const int64_t lds = (((int64_t)M + 1) * (BWD ? 3 : 2) + 2 * K) * (int64_t)sizeof(double);
    if (lds > MC_MAX_LDS) return fail(DSA_ERR_UNSUPPORTED, "%s: the row and the bins do not fit the LDS", name);
    const dim3 grid((unsigned)(F < (1 << 16) ? F : (1 << 16)));
    if (launch_lds<mlsacheck_generic_kernel<T, BWD>>(MC_MAX_LDS, "%s: cannot reserve LDS", grid, dim3(64), (size_t)lds, st, (const T*)gout, (const T*)mc,
                                                     (long)F, M, alpha, thr, mode, n_fft, (T*)out, (int*)unstable))
        return fail(DSA_ERR_LAUNCH, "%s: cannot reserve LDS", name);   // (the message again, with the name in it)
    return check_launch(name);
}

template <bool BWD>
int mlsacheck_launch(const void* gout, const void* mc, int64_t F, int32_t M, double alpha, double thr, int32_t mode, int32_t n_fft,
                     int32_t dtype, void* out, void* unstable, void* stream)
{
    const char* what = BWD ? "mlsacheck_vjp" : "mlsacheck";
    const bool fft = mode != DSA_MLSACHECK_FAST;
    if (!(F >= 0 && M >= 0 && M < INT32_MAX)) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: invalid sizes", what);
    if (mode != DSA_MLSACHECK_FAST && mode != DSA_MLSACHECK_SCALE && mode != DSA_MLSACHECK_CLIP)
        return fail(DSA_ERR_INVALID_ARGUMENT, "%s: unknown mode", what);
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: unknown dtype", what);
    if (fft && !(n_fft > 0 && 2 * ((int64_t)n_fft / 2) >= (int64_t)M + 1))
        return fail(DSA_ERR_INVALID_ARGUMENT, "%s: n_fft must be positive and 2 (n_fft / 2) at least M + 1", what);
    if (F == 0) return DSA_OK;
    if (!(mc && out && (!BWD || gout))) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DSA_F32 && M <= MC_TUNED_MAX_ORDER && (!fft || n_fft == MC_TUNED_NFFT)) {
        const dim3 grid((unsigned)(F < (1 << 14) ? F : (1 << 14)));
        hipLaunchKernelGGL((mlsacheck_tuned_kernel<BWD>), grid, dim3(64), 0, st, (const float*)gout, (const float*)mc, (long)F, M, alpha, thr,
                           mode, (float*)out, (int*)unstable);
        return check_launch(BWD ? "mlsacheck_tuned_bwd" : "mlsacheck_tuned_fwd");
    }
    return with_dtype(dtype, what, [&](auto tag) {
        return mlsacheck_generic_launch<decltype(tag), BWD>(gout, mc, F, M, alpha, thr, mode, n_fft, out, unstable, st);
    });
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_mlsacheck(const void* mc, int64_t F, int32_t M, double alpha, double threshold, int32_t mode, int32_t n_fft, int32_t dtype,
                             void* out, int32_t* unstable, void* stream)
{
    return mlsacheck_launch<false>(nullptr, mc, F, M, alpha, threshold, mode, n_fft, dtype, out, unstable, stream);
}

DSA_EXPORT int dsa_mlsacheck_vjp(const void* gout, const void* mc, int64_t F, int32_t M, double alpha, double threshold, int32_t mode,
                                 int32_t n_fft, int32_t dtype, void* gmc, void* stream)
{
    return mlsacheck_launch<true>(gout, mc, F, M, alpha, threshold, mode, n_fft, dtype, gmc, nullptr, stream);
}
