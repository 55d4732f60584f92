// Element-wise kernels of the inverse path and of Griffin-Lim: the irfft scaling in front of the adjoint transform (ifftr.py),
// Unframe's division by the overlap-added squared window (unframe.py), one Griffin-Lim phase update (griffin.py).
#include "common.h"

namespace dsa {

// ---- inverse path helpers ----
// irfft(Y)[n] = sum_k c_k / N Re(Y_k e^{+2 pi i k n / N}), c = 1 at DC / Nyquist, 2 in between (ifftr.py:138):
// that is the ADJOINT of rfft (the backward kernels of stft.hip and spec.hip) applied to G_k = c_k / N Y_k.
template <typename T>
__global__ void irfft_scale_kernel(const T* __restrict__ y, long total, int K, int nfft, T* __restrict__ out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // complex element index
    if (i >= total) return;
    const int k = (int)(i % K);
    const T c = ((k == 0 || k == nfft / 2) ? T(1) : T(2)) / T(nfft);
    out[2 * i] = y[2 * i] * c;
    out[2 * i + 1] = y[2 * i + 1] * c;
}
// Unframe._forward unframe.py:203-205: x / (sum of squared windows + 1e-16), the divisor shared by all rows
template <typename T>
__global__ void div_rows_kernel(const T* __restrict__ x, long B, long Tlen, const T* __restrict__ d, T eps,
                                T* __restrict__ out)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Tlen) return;
    const T r = T(1) / (d[t] + eps);
    for (long b = blockIdx.y; b < B; b += gridDim.y) out[b * Tlen + t] = x[b * Tlen + t] * r;
}

// One Griffin-Lim phase update (griffin.py:263-282), element-wise over (B, N, K) complex bins:
//   t' = t (first) or (1 - gamma) d_prev + gamma t;   diff = t' - t_prev;   c = t' + alpha diff;   d = t' + beta diff;
//   z = sqrt(y + 1e-16) * c / (|c| + eps);   t_prev <- t',  d_prev <- d.
// t:(B, Nt, K) is the STFT of the previous estimate (Nt >= N frames; the extra ones are dropped, griffin.py:270);
// t == nullptr initialises: z = sqrt(y + 1e-16) * exp(i phase) (phase == nullptr: zeros).
template <typename T>
__global__ void griffin_update_kernel(const T* __restrict__ t, long B, long Nt, long N, int K, const T* __restrict__ y,
                                      const T* __restrict__ phase, T* __restrict__ t_prev, T* __restrict__ d_prev, int first,
                                      T alpha, T beta, T gamma, T eps, T* __restrict__ z)
{
    const long NK = N * K, total = B * NK;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const T s = dsa_sqrt(y[i] + T(1e-16));   // griffin.py:263-264
        T cr, ci;
        if (!t) {
            const T ph = phase ? phase[i] : T(0);
            z[2 * i] = s * dsa_cos(ph);
            z[2 * i + 1] = s * dsa_sin(ph);
            continue;
        }
        const long b = i / NK;
        const long it = b * Nt * K + (i - b * NK);
        T tr = t[2 * it], ti = t[2 * it + 1], dr, di;
        if (first) {
            cr = dr = tr;
            ci = di = ti;
        } else {
            tr = (T(1) - gamma) * d_prev[2 * i] + gamma * tr;
            ti = (T(1) - gamma) * d_prev[2 * i + 1] + gamma * ti;
            const T fr = tr - t_prev[2 * i], fi = ti - t_prev[2 * i + 1];
            cr = tr + alpha * fr;
            ci = ti + alpha * fi;
            dr = tr + beta * fr;
            di = ti + beta * fi;
        }
        t_prev[2 * i] = tr;
        t_prev[2 * i + 1] = ti;
        d_prev[2 * i] = dr;
        d_prev[2 * i + 1] = di;
        const T r = s / (dsa_sqrt(cr * cr + ci * ci) + eps);   // griffin.py:281
        z[2 * i] = cr * r;
        z[2 * i + 1] = ci * r;
    }
}

}  // namespace dsa

using namespace dsa;

// --------------------------------------------------------------------------- inverse path (8(f) row 2)
DSA_EXPORT int dsa_irfft_scale(const void* y, int64_t F, int32_t nfft, int32_t dtype, void* out, void* stream)
{
    DSA_REQUIRE(nfft > 1 && nfft % 2 == 0, "irfft_scale: fft_length must be positive even");
    const int K = nfft / 2 + 1;
    const long total = (long)F * K;
    if (total == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    return with_dtype(dtype, "irfft_scale", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((irfft_scale_kernel<T>), dim3(blocks), dim3(256), 0, st, (const T*)y, total, K, nfft, (T*)out);
        return check_launch("irfft_scale");
    });
}

DSA_EXPORT int dsa_div_rows(const void* x, int64_t B, int64_t T, const void* d, double eps, int32_t dtype, void* out,
                            void* stream)
{
    DSA_REQUIRE(B >= 0 && T >= 0, "div_rows: sizes must be non-negative");
    if (B * T == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((T + 255) / 256), (unsigned)(B < 1024 ? B : 1024));
    return with_dtype(dtype, "div_rows", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's row length)
        hipLaunchKernelGGL((div_rows_kernel<V>), grid, dim3(256), 0, st, (const V*)x, (long)B, (long)T, (const V*)d, (V)eps, (V*)out);
        return check_launch("div_rows");
    });
}

DSA_EXPORT int dsa_griffin_update(const void* t, int64_t B, int64_t Nt, int64_t N, int32_t K, const void* y, const void* phase,
                                  void* t_prev, void* d_prev, int32_t first, double alpha, double beta, double gamma,
                                  double eps, int32_t dtype, void* z, void* stream)
{
    DSA_REQUIRE(B >= 0 && N >= 0 && K > 0 && Nt >= N, "griffin_update: the transform must cover the spectrogram's frames");
    DSA_REQUIRE(!t || (t_prev && d_prev), "griffin_update: the momentum buffers are required after the initial step");
    const long total = (long)B * N * K;
    if (total == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    return with_dtype(dtype, "griffin_update", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((griffin_update_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)t, (long)B, (long)Nt, (long)N, K,
                           (const T*)y, (const T*)phase, (T*)t_prev, (T*)d_prev, first, (T)alpha, (T)beta, (T)gamma, (T)eps, (T*)z);
        return check_launch("griffin_update");
    });
}
