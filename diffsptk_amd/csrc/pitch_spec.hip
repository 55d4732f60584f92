// The pitch-adaptive spectral envelope of CheapTrick (include/diffsptk_amd.h, section a26): SpectrumExtractionByCheapTrick.forward,
// pitch_spec.py:257-304, with the formatter of pitch_spec.py:158-168.  (There: about forty torch operators over (B, N, L) tensors, a host
// read of the batch's widest smoothing boundary, and a smoothing that is the difference of two running sums in the data's dtype.)
//
//   frames      one workgroup per (utterance, frame), everything in float64 in LDS and registers whatever the data's dtype: the window of
//               2 h + 1 samples and its two sums, the replicate-padded frame with its noise and its weighted mean removed, |FFT|^2 + eps with
//               the relative floor, the DC correction, the spectrum mirrored by the frame's own boundary b and summed from ITS first element
//               in ascending order by one thread (the sum's rounding sequence is the result's last bits), the two linear reads and their
//               difference, the floor noise, the logarithm, the cepstrum through a second L-point transform, the two lifters, the third
//               transform, the output format.  The positions the reads truncate to are the frame's: f / rate = Bd + fd for the DC correction,
//               b - 1/2 -/+ f / (3 rate) = Bl + fl, Bh + fh for the smoothing -- bin k reads at k + Bl and k + Bh with the same fractions,
//               which is the reference's trunc(k + c) in exact arithmetic and continuous across its truncations.
//   frames vjp  the same workgroup again, keeping the spectrum X and the smoothed spectrum, then the transposes in reverse order: the format,
//               two cosine transforms (hfft and irfft of K real values; the inner bins count twice), 1 / smoothed, the smoothing as a
//               difference of prefix sums of the cotangent folded back over the mirror, the DC correction, the floor (a floored bin sends its
//               cotangent to the bin of the maximum), 2 X g through a fourth ... sixth transform, the mean removal and the window.  The frame's
//               cotangent, L float64 values that are zero outside |j| <= h, goes to the caller's scratch.
//   gather      one thread per waveform sample adds, in ascending frame order, the frames that cover it; two more workgroups sum what the
//               replicate padding sent to the first and the last sample (with one sample, the first of the two sums all L columns).  No atomics.
//
// LDS, in float64 words: the transform's two arrays of L, the kept spectrum (2 K), the smoothed spectrum (K) and 32 words for the reductions:
// DSA_PITCH_SPEC_LDS_BYTES(L) = 28 L + 280.
#include "common.h"
#include "lds_fft.h"

#include <limits.h>

namespace dsa {
namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_RED = 32;   // float64 words behind the arrays, for the reductions' exchange: DSA_PITCH_SPEC_LDS_BYTES counts them
static_assert(DSA_PITCH_SPEC_LDS_BYTES(0) == 8 * (3 + PS_RED), "2 L + 3 (L / 2 + 1) + PS_RED float64 words");

__device__ __forceinline__ int ps_int(double v, int lo, int hi)   // trunc, pinned to [lo, hi]; a NaN is lo: the indices stay inside
{
    if (!(v == v)) return lo;
    return v < (double)lo ? lo : v > (double)hi ? hi : (int)v;
}

// an inclusive running sum of a[0 .. n) in place, strictly in ascending order, by one thread: what the smoothing reads is the difference of
// two such sums a few bins apart, below a total that the harmonics' peaks dominate, so its last bits are the sum's rounding sequence.  A
// blocked scan has a different sequence and landed 20 times further from the reference's float64 result than this one does;
// the loads do not depend on the sum, so the chain is one float64 add per element
__device__ __forceinline__ void ps_scan(double* a, int n)
{
    if (threadIdx.x == 0) {
        double run = 0;
#pragma unroll 8
        for (int i = 0; i < n; ++i) {
            run += a[i];
            a[i] = run;
        }
    }
    __syncthreads();
}

template <typename T, bool VJP>
__global__ __launch_bounds__(PS_THREADS) void ps_frames_kernel(const T* __restrict__ x, const T* __restrict__ f0, const T* __restrict__ noise1,
                                                               const T* __restrict__ noise2, const double* __restrict__ tw, long N, long Tlen, int P,
                                                               int sr, int L, int lg, double default_f0, double q1, double eps, double floor_ratio,
                                                               int fmt, T* __restrict__ y, const T* __restrict__ gy, double* __restrict__ gframes)
{
    extern __shared__ double lds[];
    const int K = L / 2 + 1, half = L / 2, tid = threadIdx.x;
    double* re = lds;
    double* im = lds + L;
    double* XR = lds + 2 * L;
    double* XI = XR + K;
    double* SN = XI + K;
    double* red = SN + K;
    const long fr = blockIdx.x, b = fr / N, n = fr - b * N;
    const T* row = x + b * Tlen;

    // ---- what depends on f alone
    const double rate = (double)sr / (double)L, f_min = 3.0 * (double)sr / (double)(L - 3);
    double f = (double)f0[fr];
    if (f <= f_min) f = default_f0;
    const int h = ps_int(rint(1.5 * (double)sr / f), 0, half - 1);
    const double z0 = f / rate;
    const int Bd = ps_int(z0, 0, K - 1);
    const double fd = z0 - (double)Bd;
    const double width = f * (2.0 / 3.0);
    const int bnd = ps_int(width / rate, 0, K - 2) + 1;
    const double cl = (double)bnd - 0.5 - width / (2.0 * rate), ch = (double)bnd - 0.5 + width / (2.0 * rate);
    const int Bl = ps_int(cl, 0, 2 * bnd - 1), Bh = ps_int(ch, 0, 2 * bnd - 1);
    const double fl = cl - (double)Bl, fh = ch - (double)Bh;
    const double tiny = 2.220446049250313e-16;   // finfo(float64).eps for both dtypes: the floor noise of the arithmetic that runs
    auto win = [&](int i) {
        const int j = i - half;
        return (j < -h || j > h) ? 0.0 : 0.5 + 0.5 * cos(kPi * ((double)j / (1.5 * (double)sr)) * f);
    };
    auto lifter = [&](int q) {
        const double z = f * ((double)q / (double)sr);
        const double sinc = q == 0 ? 1.0 : sin(kPi * z) / (kPi * z);
        return sinc * ((1.0 - 2.0 * q1) + 2.0 * q1 * cos(kTau * z));
    };

    // ---- 1, 2: the window and the frame
    double s2 = 0, s1 = 0;
    for (int i = tid; i < L; i += PS_THREADS) {
        const double w = win(i);
        im[i] = w;
        s2 += w * w;
        s1 += w;
    }
    const double inv_norm = 1.0 / sqrt(block_sum(s2, red));
    const double W = block_sum(s1, red) * inv_norm;
    const long base = n * (long)P - half;
    double su = 0;
    for (int i = tid; i < L; i += PS_THREADS) {
        const double wn = im[i] * inv_norm;
        const int j = i - half;
        double u = 0;
        if (j >= -h && j <= h) {
            const long at = base + i;
            u = (double)row[at < 0 ? 0 : at > Tlen - 1 ? Tlen - 1 : at] * wn;
            if (noise1) u += 1e-12 * (double)noise1[fr * L + i];
        }
        re[i] = u;
        su += u;
    }
    const double mean = block_sum(su, red) / W;
    for (int i = tid; i < L; i += PS_THREADS) {
        re[i] -= im[i] * inv_norm * mean;
        im[i] = 0;
    }
    __syncthreads();

    // ---- 3: the power spectrum and its floor
    lds_fft_pow2(re, im, L, lg, tw);
    double amax = 0;
    for (int k = tid; k < K; k += PS_THREADS) {
        const int at = fft_brev(k, lg);
        const double xr = re[at], xi = im[at];
        XR[k] = xr;
        XI[k] = xi;
        const double a = xr * xr + xi * xi + eps;
        amax = a > amax ? a : amax;
    }
    const double M = block_max(amax, red);
    const double level = M * floor_ratio;
    for (int k = tid; k < K; k += PS_THREADS) {
        const double a = XR[k] * XR[k] + XI[k] * XI[k] + eps;
        SN[k] = floor_ratio > 0 && a < level ? level : a;
    }
    __syncthreads();

    // ---- 4, 5: the DC correction into the middle of the mirrored spectrum, the mirror, the running sum, the two reads
    for (int k = tid; k < K; k += PS_THREADS) {
        double d = SN[k];
        if ((double)k * rate < f) {
            const int i0 = Bd - k < 0 ? 0 : Bd - k, i1 = i0 + 1 > K - 1 ? K - 1 : i0 + 1;
            d += SN[i0] + (SN[i1] - SN[i0]) * fd;
        }
        lds[bnd + k] = d * rate;
    }
    __syncthreads();
    for (int t = tid; t < bnd; t += PS_THREADS) {
        lds[t] = lds[2 * bnd - t];
        lds[bnd + K + t] = lds[bnd + K - 2 - t];
    }
    __syncthreads();
    ps_scan(lds, K + 2 * bnd);
    for (int k = tid; k < K; k += PS_THREADS) {
        const double l0 = lds[k + Bl], h0 = lds[k + Bh];
        const double lo = l0 + (lds[k + Bl + 1] - l0) * fl, hi = h0 + (lds[k + Bh + 1] - h0) * fh;
        SN[k] = (hi - lo) / width + (noise2 ? fabs((double)noise2[fr * K + k]) * tiny : 0.0);
    }
    __syncthreads();

    // ---- 6, 7: the logarithm, the cepstrum, the lifters, back
    for (int i = tid; i < L; i += PS_THREADS) {
        re[i] = log(SN[i < K ? i : L - i]);
        im[i] = 0;
    }
    __syncthreads();
    lds_fft_pow2(re, im, L, lg, tw);
    for (int q = tid; q < K; q += PS_THREADS) {   // (the transform's imaginary output is rounding noise: its array takes the next input)
        const double v = re[fft_brev(q, lg)] / (double)L * lifter(q);
        im[q] = v;
        if (q > 0 && q < K - 1) im[L - q] = v;
    }
    __syncthreads();
    for (int i = tid; i < L; i += PS_THREADS) re[i] = 0;
    __syncthreads();
    lds_fft_pow2(im, re, L, lg, tw);

    // ---- 8: the output format
    const double db = 4.342944819032518;   // 10 / ln 10
    if (!VJP) {
        T* out = y + fr * K;
        for (int k = tid; k < K; k += PS_THREADS) {
            const double v = im[fft_brev(k, lg)];
            out[k] = (T)(fmt == 0 ? v * db : fmt == 1 ? 0.5 * v : fmt == 2 ? exp(0.5 * v) : exp(v));
        }
        return;
    }

    // ---- the adjoint.  The format, then hfft's transpose: a_q sum_k g[k] cos(2 pi k q / L)
    const T* gout = gy + fr * K;
    for (int i = tid; i < L; i += PS_THREADS) {
        double g = 0;
        if (i < K) {
            const double v = im[fft_brev(i, lg)];
            g = (double)gout[i] * (fmt == 0 ? db : fmt == 1 ? 0.5 : fmt == 2 ? 0.5 * exp(0.5 * v) : exp(v));
        }
        re[i] = g;
    }
    __syncthreads();
    for (int i = tid; i < L; i += PS_THREADS) im[i] = 0;
    __syncthreads();
    lds_fft_pow2(re, im, L, lg, tw);
    for (int i = tid; i < L; i += PS_THREADS)   // the lifters, then irfft's transpose: a_k / L sum_q g[q] cos(2 pi k q / L)
        im[i] = i < K ? ((i == 0 || i == K - 1) ? 1.0 : 2.0) * re[fft_brev(i, lg)] * lifter(i) : 0.0;
    __syncthreads();
    for (int i = tid; i < L; i += PS_THREADS) re[i] = 0;
    __syncthreads();
    lds_fft_pow2(im, re, L, lg, tw);
    for (int k = tid; k < K; k += PS_THREADS) {   // the logarithm; the cotangent of the smoothed spectrum, and (below) its prefix sums
        const double g = ((k == 0 || k == K - 1) ? 1.0 : 2.0) / (double)L * im[fft_brev(k, lg)] / SN[k];
        SN[k] = g;
        re[k] = g;
    }
    __syncthreads();
    ps_scan(re, K);
    // position u of the mirrored spectrum is inside every running sum read at or behind it: differences of the prefix sums G = re
    auto upto = [&](int i) { return i < 0 ? 0.0 : re[i > K - 1 ? K - 1 : i]; };
    auto gmirror = [&](int u) {
        return (-(1.0 - fh) * upto(u - Bh - 1) - fh * upto(u - Bh - 2) + (1.0 - fl) * upto(u - Bl - 1) + fl * upto(u - Bl - 2)) / width;
    };
    for (int i = tid; i < K; i += PS_THREADS) {   // the mirror folded back: the bin itself, its image below 0, its image above K - 1
        double g = gmirror(bnd + i);
        if (i >= 1 && i <= bnd) g += gmirror(bnd - i);
        const int r = K - 1 - i;
        if (r >= 1 && r <= bnd) g += gmirror(bnd + K - 1 + r);
        im[i] = g * rate;
    }
    __syncthreads();
    for (int i = tid; i < K; i += PS_THREADS) {   // the DC correction: bin i is read by the corrected bins Bd - i and Bd - i + 1
        double g = im[i];
        const int ka = Bd - i, kb = Bd - i + 1;
        if (ka >= 0 && ka < K && (double)ka * rate < f) g += (1.0 - fd) * im[ka];
        if (kb >= 0 && kb < K && (double)kb * rate < f && i <= K - 1) g += fd * im[kb];
        SN[i] = g;
    }
    __syncthreads();
    // the floor: a floored bin is M floor_ratio, so its cotangent goes to the first bin that holds the maximum
    double spill = 0, first = -1e300;
    for (int k = tid; k < K; k += PS_THREADS) {
        const double a = XR[k] * XR[k] + XI[k] * XI[k] + eps;
        if (floor_ratio > 0 && a < level) spill += SN[k];
        if (a == M) first = first > -(double)k ? first : -(double)k;
    }
    spill = floor_ratio > 0 ? block_sum(spill, red) * floor_ratio : 0.0;
    const int kmax = floor_ratio > 0 ? ps_int(-block_max(first, red), 0, K - 1) : 0;
    for (int i = tid; i < L; i += PS_THREADS) {   // |X|^2: the real part of sum_k 2 g[k] X[k] e^{+i theta} = Re FFT(conj(2 g X))
        double zr = 0, zi = 0;
        if (i < K) {
            const double a = XR[i] * XR[i] + XI[i] * XI[i] + eps;
            double g = floor_ratio > 0 && a < level ? 0.0 : SN[i];
            if (floor_ratio > 0 && i == kmax) g += spill;
            zr = 2.0 * g * XR[i];
            zi = -2.0 * g * XI[i];
        }
        re[i] = zr;
        im[i] = zi;
    }
    __syncthreads();
    lds_fft_pow2(re, im, L, lg, tw);
    double dot = 0;
    for (int i = tid; i < L; i += PS_THREADS) dot += re[fft_brev(i, lg)] * (win(i) * inv_norm);
    dot = block_sum(dot, red) / W;
    double* out = gframes + fr * L;
    for (int i = tid; i < L; i += PS_THREADS) {
        const int j = i - half;
        out[i] = (j < -h || j > h) ? 0.0 : (re[fft_brev(i, lg)] - dot) * (win(i) * inv_norm);
    }
}

// grid (blocks + 2, B): the last two workgroups take samples 0 and T - 1, which also collect what the replicate padding sent to them
template <typename T>
__global__ __launch_bounds__(PS_THREADS) void ps_gather_kernel(const double* __restrict__ gframes, long N, long Tlen, int P, int L, unsigned blocks,
                                                               T* __restrict__ gx)
{
    __shared__ double red[PS_THREADS / 64];
    const long b = blockIdx.y, half = L / 2;
    const double* g = gframes + b * N * L;
    T* out = gx + b * Tlen;
    if (blockIdx.x < blocks) {
        const long t = (long)blockIdx.x * PS_THREADS + threadIdx.x;
        if (t <= 0 || t >= Tlen - 1) return;
        // frame n holds sample t at column t - n P + L / 2, inside [0, L)
        long n0 = t - half + 1 <= 0 ? 0 : (t - half + P) / P, n1 = (t + half) / P;
        n1 = n1 > N - 1 ? N - 1 : n1;
        double acc = 0;
        for (long n = n0; n <= n1; ++n) acc += g[n * L + (t - n * P + half)];
        out[t] = (T)acc;
        return;
    }
    const bool head = blockIdx.x == blocks;
    const bool one = Tlen == 1;   // one sample: the padding clamps every column to it, on both sides, and the head's workgroup takes them all
    if (!head && one) return;
    long n0 = 0, n1 = half / P;
    if (!head) {
        n0 = Tlen - half <= 0 ? 0 : (Tlen - half + P - 1) / P;
        n1 = N - 1;
    }
    n1 = n1 > N - 1 ? N - 1 : n1;
    const long items = n1 >= n0 ? (n1 - n0 + 1) * L : 0;
    double acc = 0;
    for (long i = threadIdx.x; i < items; i += PS_THREADS) {
        const long n = n0 + i / L, c = i % L, at = n * P + c - half;
        if (head ? at <= 0 || one : at >= Tlen - 1) acc += g[n * L + c];
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[head ? 0 : Tlen - 1] = (T)acc;
}

// ---------------------------------------------------------------------------------------------------------------- host
int ps_check(int64_t B, int64_t N, int64_t T, int32_t P, int32_t L, int32_t dtype, int& lg)
{
    if (!(B >= 0 && N >= 0 && T >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: unknown dtype");
    if (!(L >= 16 && (L & (L - 1)) == 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: fft_length must be a power of two, at least 16");
    if (DSA_PITCH_SPEC_LDS_BYTES((int64_t)L) > DSA_PITCH_SPEC_MAX_LDS_BYTES)
        return fail(DSA_ERR_INVALID_ARGUMENT,
                    "pitch_spec: DSA_PITCH_SPEC_LDS_BYTES(fft_length) = 28 fft_length + 280 bytes exceed DSA_PITCH_SPEC_MAX_LDS_BYTES (163840 bytes per "
                    "workgroup)");
    if (!(P >= 1)) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: invalid options");
    if (N != (T > 0 ? (T - 1) / P + 1 : 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: f0 must have (T - 1) / frame_period + 1 frames");
    if (B > 65535 || T > INT64_MAX / 16 / (B > 0 ? B : 1) || (N > 0 && B > (int64_t)INT32_MAX / N))
        return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: invalid sizes (B N frames must fit one grid dimension)");
    lg = 0;
    while ((1 << lg) < L) ++lg;
    return DSA_OK;
}

// the unit's one launcher: the kernel, its geometry and the route's name
template <auto Kernel, typename... Args>
int ps_launch(const char* route, dim3 grid, size_t lds_bytes, hipStream_t st, Args... args)
{
    const int rc = launch_lds<Kernel>(lds_bytes ? DSA_PITCH_SPEC_MAX_LDS_BYTES : 0, "pitch_spec: cannot raise the dynamic LDS limit%s", grid,
                                      dim3(PS_THREADS), lds_bytes, st, args...);
    return rc ? rc : check_launch(route);
}

template <bool VJP>
int ps_frames(const char* what, const char* route, const void* x, const void* f0, const void* noise1, const void* noise2, const void* twiddle, int64_t B,
              int64_t N, int64_t T, int32_t P, int32_t sr, int32_t L, double default_f0, double q1, double eps, double floor_ratio, int32_t fmt,
              int32_t dtype, void* y, const void* gy, void* gframes, void* stream)
{
    int lg = 0;
    if (int rc = ps_check(B, N, T, P, L, dtype, lg)) return rc;
    if (!(sr >= 1 && fmt >= 0 && fmt <= 3 && eps >= 0 && floor_ratio >= 0 && floor_ratio < 1 && default_f0 > 0 && q1 == q1))
        return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: invalid options");
    if (B == 0 || N == 0) return DSA_OK;
    if (!(x && f0 && twiddle && (VJP ? gy && gframes : y != nullptr))) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * N));
    const size_t lds = (size_t)DSA_PITCH_SPEC_LDS_BYTES((int64_t)L);
    return with_dtype(dtype, what, [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        return ps_launch<ps_frames_kernel<V, VJP>>(route, grid, lds, st, (const V*)x, (const V*)f0, (const V*)noise1, (const V*)noise2,
                                                   (const double*)twiddle, (long)N, (long)T, (int)P, (int)sr, (int)L, lg, default_f0, q1, eps, floor_ratio,
                                                   (int)fmt, (V*)y, (const V*)gy, (double*)gframes);
    });
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_pitch_spec(const void* x, const void* f0, const void* noise1, const void* noise2, const void* twiddle, int64_t B, int64_t N, int64_t T,
                              int32_t P, int32_t sample_rate, int32_t L, double default_f0, double q1, double eps, double floor_ratio, int32_t out_format,
                              int32_t dtype, void* y, void* stream)
{
    const char* what = "pitch_spec";
    const char* route = dtype == DSA_F64 ? "pitch_spec_f64" : "pitch_spec_f32";
    return ps_frames<false>(what, route, x, f0, noise1, noise2, twiddle, B, N, T, P, sample_rate, L, default_f0, q1, eps, floor_ratio, out_format, dtype, y,
                            nullptr, nullptr, stream);
}

DSA_EXPORT int dsa_pitch_spec_vjp_frames(const void* gy, const void* x, const void* f0, const void* noise1, const void* noise2, const void* twiddle,
                                         int64_t B, int64_t N, int64_t T, int32_t P, int32_t sample_rate, int32_t L, double default_f0, double q1,
                                         double eps, double floor_ratio, int32_t out_format, int32_t dtype, void* gframes, void* stream)
{
    const char* what = "pitch_spec";
    const char* route = dtype == DSA_F64 ? "pitch_spec_vjp_frames_f64" : "pitch_spec_vjp_frames_f32";
    return ps_frames<true>(what, route, x, f0, noise1, noise2, twiddle, B, N, T, P, sample_rate, L, default_f0, q1, eps, floor_ratio, out_format, dtype,
                           nullptr, gy, gframes, stream);
}

DSA_EXPORT int dsa_pitch_spec_vjp_gather(const void* gframes, int64_t B, int64_t N, int64_t T, int32_t P, int32_t L, int32_t dtype, void* gx, void* stream)
{
    const char* what = "pitch_spec";
    const char* route = dtype == DSA_F64 ? "pitch_spec_vjp_gather_f64" : "pitch_spec_vjp_gather_f32";
    int lg = 0;
    if (int rc = ps_check(B, N, T, P, L, dtype, lg)) return rc;
    if (B == 0 || T == 0) return DSA_OK;
    if (T > (int64_t)(INT32_MAX - 2) * PS_THREADS) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: invalid sizes (a thread per sample must fit one grid dimension)");
    if (!(gframes && gx)) return fail(DSA_ERR_INVALID_ARGUMENT, "pitch_spec: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((T + PS_THREADS - 1) / PS_THREADS);
    const dim3 grid(blocks + 2, (unsigned)B);
    return with_dtype(dtype, what, [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        return ps_launch<ps_gather_kernel<V>>(route, grid, (size_t)0, st, (const double*)gframes, (long)N, (long)T, (int)P, (int)L, blocks, (V*)gx);
    });
}
