// The generic family for gfx950: Frame (a1), Window (a2), fftr (a3), Spectrum (a4), and the generic route of the STFT (a5).
//
// Any frame length / period / even fft length, float32 and float64, every option of the reference.  One workgroup per
// frame, direct DFT against a host-built twiddle table (power-of-two lengths: the radix-2 transform of lds_fft.h).
// Correctness path for odd configurations and for float64 (gradcheck); never the fast path -- that is stft.hip, which
// falls back to this unit through stft_generic_fwd / stft_generic_bwd (common.h).
//
// Reference semantics: diffsptk/modules/{frame,window,fftr,spec,stft}.py (cited per kernel).
#include "common.h"
#include "lds_fft.h"

namespace dsa {

// =========================================================================== generic kernels

// Frame._forward frame.py:120-141.  grid = F frames, any block size.
template <typename T>
__global__ void frame_fwd_kernel(const T* __restrict__ x, long Tlen, long N, int L, int P, int left,
                                 int zmean, int mode, T* __restrict__ y)
{
    __shared__ T scratch[16];
    long f = blockIdx.x;
    long b = f / N, n = f - b * N;
    const T* xb = x + b * Tlen;
    T* row = y + f * L;
    T acc = 0;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        T v = load_padded(xb, n * P + l - left, Tlen, mode);
        row[l] = v;
        acc += v;
    }
    if (zmean) {  // frame.py:139-140
        T mean = block_sum(acc, scratch) / T(L);
        for (int l = threadIdx.x; l < L; l += blockDim.x) row[l] -= mean;
    }
}

// Frame without zmean, float32, L % 4 == 0: four samples per thread and a 16-byte store (the rows of y are 16-byte
// aligned then); the four samples come as one 16-byte load when the source run is inside the waveform and aligned
// (P, left multiples of 4), else one by one through the padding rule.  Persistent grid: the one-workgroup-per-frame
// kernel above launches B * N tiny workgroups (0.17 ms per 204 800 frames against 0.07 ms here).
__global__ __launch_bounds__(256) void frame_fwd_vec4_kernel(const float* __restrict__ x, long Tlen, long N, long F, int L, int P,
                                                             int left, int mode, int src_aligned, float* __restrict__ y)
{
    const int L4 = L >> 2;
    const long total = F * L4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long f = q / L4;
        const int l = (int)(q - f * L4) << 2;
        const long b = f / N, n = f - b * N;
        const float* xb = x + b * Tlen;
        const long s0 = n * P + l - left;
        float4 v;
        if (src_aligned && s0 >= 0 && s0 + 4 <= Tlen) {
            v = *reinterpret_cast<const float4*>(xb + s0);
        } else {
            v.x = load_padded(xb, s0, Tlen, mode);
            v.y = load_padded(xb, s0 + 1, Tlen, mode);
            v.z = load_padded(xb, s0 + 2, Tlen, mode);
            v.w = load_padded(xb, s0 + 3, Tlen, mode);
        }
        *reinterpret_cast<float4*>(y + f * (long)L + l) = v;
    }
}

// adjoint of Frame: gx[b,t] = sum over (n,l) whose source index is t of g'[b,n,l], where
// g' = gy - mean_l(gy) if zmean.  Gather formulation (deterministic, no atomics) for constant
// padding; the non-constant modes fold several padded positions onto one sample and use a
// per-utterance serial-over-frames scatter within one block (deterministic as well).
template <typename T>
__global__ void frame_bwd_const_kernel(const T* __restrict__ gy, const T* __restrict__ gmean,
                                       long Tlen, long N, int L, int P, int left,
                                       T* __restrict__ gx)
{
    const long tb = (Tlen + blockDim.x - 1) / blockDim.x;   // blocks per utterance: (utterance, block) folded into grid.x
    const long b = blockIdx.x / tb;
    long t = ((long)blockIdx.x - b * tb) * blockDim.x + threadIdx.x;
    if (t >= Tlen) return;
    // frames n with 0 <= t + left - n*P < L
    long p = t + left;
    long n_hi = p / P;
    if (n_hi > N - 1) n_hi = N - 1;
    long n_lo = p - L + 1 <= 0 ? 0 : (p - L + P) / P;  // ceil((p-L+1)/P)
    T acc = 0;
    for (long n = n_lo; n <= n_hi; ++n) {
        long l = p - n * P;
        T g = gy[(b * N + n) * L + l];
        if (gmean) g -= gmean[b * N + n];
        acc += g;
    }
    gx[b * Tlen + t] = acc;
}

template <typename T>
__global__ void row_mean_kernel(const T* __restrict__ g, int L, T* __restrict__ m)
{
    __shared__ T scratch[16];
    long f = blockIdx.x;
    T acc = 0;
    for (int l = threadIdx.x; l < L; l += blockDim.x) acc += g[f * L + l];
    T s = block_sum(acc, scratch);
    if (threadIdx.x == 0) m[f] = s / T(L);
}

// general-mode adjoint: one block per utterance, frames visited in order, each frame's L
// contributions added by distinct threads (a frame never maps two l onto the same t unless
// the padding folds, in which case the fold is resolved by a second serial pass) -- simple and
// deterministic; only used for reflect/replicate/circular padding.
template <typename T>
__global__ void frame_bwd_general_kernel(const T* __restrict__ gy, const T* __restrict__ gmean,
                                         long Tlen, long N, int L, int P, int left, int mode,
                                         T* __restrict__ gx)
{
    long b = blockIdx.x;
    T* gxb = gx + b * Tlen;
    for (long t = threadIdx.x; t < Tlen; t += blockDim.x) gxb[t] = 0;
    __syncthreads();
    // interior (un-folded) part: gather
    for (long t = threadIdx.x; t < Tlen; t += blockDim.x) {
        long p = t + left;
        long n_hi = p / P;
        if (n_hi > N - 1) n_hi = N - 1;
        long n_lo = p - L + 1 <= 0 ? 0 : (p - L + P) / P;
        T acc = 0;
        for (long n = n_lo; n <= n_hi; ++n) {
            T g = gy[(b * N + n) * L + (p - n * P)];
            if (gmean) g -= gmean[b * N + n];
            acc += g;
        }
        gxb[t] = acc;
    }
    __syncthreads();
    // folded part: padded positions i < 0 or i >= T, visited serially by thread 0
    if (threadIdx.x == 0) {
        for (long n = 0; n < N; ++n)
            for (int l = 0; l < L; ++l) {
                long i = n * P + l - left;
                if (i >= 0 && i < Tlen) continue;
                long j = pad_src_index(i, Tlen, mode);
                if (j < 0) continue;
                T g = gy[(b * N + n) * L + l];
                if (gmean) g -= gmean[b * N + n];
                gxb[j] += g;
            }
    }
}

// Window._forward window.py:185-193
template <typename T>
__global__ void window_fwd_kernel(const T* __restrict__ x, long F, int L, const T* __restrict__ w,
                                  int L2, T* __restrict__ y)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = F * L2;
    for (; i < total; i += (long)gridDim.x * blockDim.x) {
        long f = i / L2;
        int l = (int)(i - f * L2);
        y[i] = l < L ? x[f * L + l] * w[l] : T(0);
    }
}

// y = x * w row-wise for float32 rows whose length is a multiple of 4 and needs no padding / cropping (the forward and
// the backward of Window are the same product then): 16-byte accesses and a 32-bit remainder per float4 instead of
// a 64-bit division per element (0.16 -> 0.11 ms per 204 800 frames of 400 samples).
__global__ __launch_bounds__(256) void window_vec4_kernel(const float4* __restrict__ x, unsigned n4, unsigned L4,
                                                          const float4* __restrict__ w, float4* __restrict__ y)
{
    for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += gridDim.x * blockDim.x) {
        const float4 a = x[q], b = w[q % L4];
        y[q] = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
    }
}

static bool window_vec4_ok(const void* a, const void* b, const void* w, int64_t F, int L, int L2)
{
    return L == L2 && (L & 3) == 0 && F * (int64_t)L >= 4096 && F * (int64_t)(L >> 2) < (1LL << 31) &&
           ((((size_t)a) | ((size_t)b) | ((size_t)w)) & 15) == 0;
}

template <typename T>
__global__ void window_bwd_kernel(const T* __restrict__ gy, long F, int L, const T* __restrict__ w,
                                  int L2, T* __restrict__ gx)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = F * L;
    for (; i < total; i += (long)gridDim.x * blockDim.x) {
        long f = i / L;
        int l = (int)(i - f * L);
        gx[i] = l < L2 ? gy[f * L2 + l] * w[l] : T(0);
    }
}

// gw[l] = sum_f gy[f,l] * x[f,l]; one block per l, fixed summation order (deterministic)
template <typename T>
__global__ void window_gw_kernel(const T* __restrict__ gy, const T* __restrict__ x, long F, int L,
                                 int L2, T* __restrict__ gw)
{
    __shared__ T scratch[16];
    int l = blockIdx.x;
    T acc = 0;
    if (l < L2)
        for (long f = threadIdx.x; f < F; f += blockDim.x) acc += gy[f * L2 + l] * x[f * L + l];
    T s = block_sum(acc, scratch);
    if (threadIdx.x == 0) gw[l] = s;
}

// Generic fused row transform: (optional framing) -> (optional zmean) -> (optional window) ->
// direct DFT of length nfft -> formatter.  Covers fftr (fftr.py:136-151), the b-only branch of
// Spectrum (spec.py:165-178) and STFT (stft.py:237-241) for any configuration.
//   out_kind 0: fftr formats (DSA_FFTR_*), 1: spectrum formats (DSA_SPEC_*).
// twiddle: (nfft, 2) = (cos, -sin)(2 pi m / nfft).
// dynamic LDS: Lrow elements of T.
// dynamic LDS: L elements of T (FFT: + 2 nfft).
template <typename T, bool FFT = false>
__global__ void row_dft_kernel(const T* __restrict__ x, long Tlen, long N, int L, int P, int left,
                               int mode, int zmean, const T* __restrict__ w, int nfft,
                               const T* __restrict__ twiddle, int out_kind, int fmt, T eps,
                               int use_floor, T floor_lin, T* __restrict__ y)
{
    extern __shared__ unsigned char smem_raw[];
    T* xs = reinterpret_cast<T*>(smem_raw);
    T* fre = xs + L;        // FFT only
    T* fim = fre + nfft;
    __shared__ T scratch[16];
    long f = blockIdx.x;
    long b = f / N, n = f - b * N;
    const T* xb = x + b * Tlen;
    T acc = 0;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        T v = load_padded(xb, n * P + l - left, Tlen, mode);
        xs[l] = v;
        acc += v;
    }
    T mean = 0;
    if (zmean) mean = block_sum(acc, scratch) / T(L);
    __syncthreads();
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        T v = xs[l] - mean;
        xs[l] = w ? v * w[l] : v;
    }
    __syncthreads();
    const int K = nfft / 2 + 1;
    const int Lc = L < nfft ? L : nfft;  // rfft(x, n) crops when the row is longer than n
    const bool inverse_adj = out_kind == 1 && fmt == DSA_SPEC_COMPLEX_INV;   // complex output times c_k / nfft
    const bool complex_out = (out_kind == 0 && fmt == DSA_FFTR_COMPLEX) ||
                             (out_kind == 1 && fmt == DSA_SPEC_COMPLEX) || inverse_adj;
    const int lg = 31 - __clz(nfft);
    if (FFT) {
        for (int l = threadIdx.x; l < nfft; l += blockDim.x) {
            fre[l] = l < Lc ? xs[l] : T(0);
            fim[l] = T(0);
        }
        __syncthreads();
        lds_fft_pow2(fre, fim, nfft, lg, twiddle);
    }
    T smax = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        T re = 0, im = 0;
        if (FFT) {
            const int q = fft_brev(k, lg);
            re = fre[q], im = fim[q];
        } else {
            int idx = 0;
            for (int l = 0; l < Lc; ++l) {
                T c = twiddle[2 * idx], s = twiddle[2 * idx + 1];
                re += xs[l] * c;
                im += xs[l] * s;
                idx += k;
                if (idx >= nfft) idx -= nfft;
            }
        }
        if (complex_out) {
            const T sc = inverse_adj ? ((k == 0 || k == K - 1) ? T(1) : T(2)) / T(nfft) : T(1);
            y[(f * K + k) * 2] = re * sc;
            y[(f * K + k) * 2 + 1] = im * sc;
        } else if (out_kind == 0) {
            T v;
            switch (fmt) {
            case DSA_FFTR_REAL: v = re; break;
            case DSA_FFTR_IMAG: v = im; break;
            case DSA_FFTR_AMPLITUDE: v = dsa_sqrt(re * re + im * im); break;
            default: {
                T a = dsa_sqrt(re * re + im * im);  // abs() then square(), fftr.py:119
                v = a * a;
            }
            }
            y[f * K + k] = v;
        } else {
            T a = dsa_sqrt(re * re + im * im);  // fftr amplitude (spec.py:139), then spec.py:173
            T s = a * a + eps;
            if (use_floor) {
                y[f * K + k] = s;  // formatted after the row maximum is known
                smax = s > smax ? s : smax;
            } else {
                y[f * K + k] = spec_format(s, fmt);
            }
        }
    }
    if (out_kind == 1 && use_floor && !complex_out) {  // spec.py:174-176
        T m = block_max(smax, scratch);
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            T s = y[f * K + k];
            T fl = m * floor_lin;
            y[f * K + k] = spec_format(s > fl ? s : fl, fmt);
        }
    }
}

// Backward of row_dft_kernel.  Recomputes X (nothing but x is saved by the forward), forms the
// complex cotangent C[k] = dL/dRe X + i dL/dIm X for the requested format, applies the adjoint
// of the half-spectrum DFT  gxw[l] = sum_k Re(C[k] exp(+i theta k l)), then the adjoints of the
// window multiply and of zmean.  Output: gframe (F, L) = cotangent of the framed samples (the
// overlap-add into the waveform is done by frame_bwd); gwpart (F, L) = per-frame contribution
// to the window gradient (NULL unless the window is learnable).
// dynamic LDS: (L + 3K) elements of T (FFT: + 2 nfft).
template <typename T, bool FFT = false>
__global__ void row_dft_bwd_kernel(const T* __restrict__ x, long Tlen, long N, int L, int P, int left,
                                   int mode, int zmean, const T* __restrict__ w, int nfft,
                                   const T* __restrict__ twiddle, int out_kind, int fmt, T eps,
                                   int use_floor, T floor_lin, const T* __restrict__ gy,
                                   T* __restrict__ gframe, T* __restrict__ gwpart)
{
    extern __shared__ unsigned char smem_raw[];
    T* xc = reinterpret_cast<T*>(smem_raw);
    __shared__ T scratch[16];
    const int K = nfft / 2 + 1;
    const int Lc = L < nfft ? L : nfft;
    T* Cre = xc + L;
    T* Cim = Cre + K;
    T* fre = Cim + 2 * K;   // FFT only (behind the gs array)
    T* fim = fre + nfft;
    const int lg = 31 - __clz(nfft);
    long f = blockIdx.x;
    long b = f / N, n = f - b * N;
    const T* xb = x + b * Tlen;
    T acc = 0;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        T v = load_padded(xb, n * P + l - left, Tlen, mode);
        xc[l] = v;
        acc += v;
    }
    T mean = 0;
    if (zmean) mean = block_sum(acc, scratch) / T(L);
    __syncthreads();
    for (int l = threadIdx.x; l < L; l += blockDim.x) xc[l] -= mean;
    __syncthreads();
    const bool inverse_cot = out_kind == 1 && fmt == DSA_SPEC_COMPLEX_INV;
    const bool complex_out = (out_kind == 0 && fmt == DSA_FFTR_COMPLEX) ||
                             (out_kind == 1 && fmt == DSA_SPEC_COMPLEX) || inverse_cot;
    // a complex cotangent (format "complex", the inverse transforms) does not depend on the spectrum: no forward transform
    if (FFT && !complex_out) {
        for (int l = threadIdx.x; l < nfft; l += blockDim.x) {
            fre[l] = l < Lc ? (w ? xc[l] * w[l] : xc[l]) : T(0);
            fim[l] = T(0);
        }
        __syncthreads();
        lds_fft_pow2(fre, fim, nfft, lg, twiddle);
    }
    T smax = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        T re = 0, im = 0;
        if (complex_out) {
        } else if (FFT) {
            const int q = fft_brev(k, lg);
            re = fre[q], im = fim[q];
        } else {
            int idx = 0;
            for (int l = 0; l < Lc; ++l) {
                T xv = w ? xc[l] * w[l] : xc[l];
                re += xv * twiddle[2 * idx];
                im += xv * twiddle[2 * idx + 1];
                idx += k;
                if (idx >= nfft) idx -= nfft;
            }
        }
        T cr, ci;
        if (complex_out) {
            cr = gy[(f * K + k) * 2];
            ci = gy[(f * K + k) * 2 + 1];
            if (inverse_cot) {   // irfft weights c_k / nfft
                const T ck = ((k == 0 || k == K - 1) ? T(1) : T(2)) / T(nfft);
                cr *= ck;
                ci *= ck;
            }
        } else if (out_kind == 0) {
            T g = gy[f * K + k];
            switch (fmt) {
            case DSA_FFTR_REAL: cr = g; ci = 0; break;
            case DSA_FFTR_IMAG: cr = 0; ci = g; break;
            case DSA_FFTR_AMPLITUDE: {
                T a = dsa_sqrt(re * re + im * im);
                T sc = a > T(0) ? g / a : T(0);
                cr = sc * re; ci = sc * im;
                break;
            }
            default: cr = T(2) * g * re; ci = T(2) * g * im;
            }
        } else {
            // keep (re, im) for now; the cotangent of s needs the row maximum when floored
            cr = re; ci = im;
            T sv = re * re + im * im + eps;
            smax = sv > smax ? sv : smax;
        }
        Cre[k] = cr;
        Cim[k] = ci;
    }
    if (out_kind == 1 && !complex_out) {
        // cotangent of s = |X|^2 + eps through the formatter and the relative floor
        // s' = max(s, m * floor), m = amax(s) (spec.py:173-177): floored bins pass their
        // cotangent (times floor) to the arg-max bin.
        T* gsarr = Cim + K;
        T m = use_floor ? block_max(smax, scratch) : T(0);
        T fl = m * floor_lin;
        __syncthreads();
        T lost = 0;
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            T re = Cre[k], im = Cim[k];
            T sv = re * re + im * im + eps;
            bool floored = use_floor && sv < fl;
            T se = floored ? fl : sv;
            T g = gy[f * K + k];
            T gs;
            switch (fmt) {
            case DSA_SPEC_DB: gs = g * T(4.342944819032518) / se; break;  // 10 / ln 10
            case DSA_SPEC_LOGMAG: gs = g * T(0.5) / se; break;
            case DSA_SPEC_MAG: gs = g * T(0.5) / dsa_sqrt(se); break;
            default: gs = g;
            }
            if (floored) {
                lost += gs;
                gs = 0;
            }
            gsarr[k] = gs;
        }
        T tot = use_floor ? block_sum(lost, scratch) * floor_lin : T(0);
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            T re = Cre[k], im = Cim[k];
            T gs = gsarr[k];
            if (use_floor && (re * re + im * im + eps) == m) gs += tot;
            Cre[k] = T(2) * gs * re;
            Cim[k] = T(2) * gs * im;
        }
    }
    __syncthreads();
    if (FFT) {
        // sum_k Re(C[k] e^{+i theta k l}) = Re FFT(conj(C), zero-extended to nfft points)[l]
        for (int k = threadIdx.x; k < nfft; k += blockDim.x) {
            fre[k] = k < K ? Cre[k] : T(0);
            fim[k] = k < K ? -Cim[k] : T(0);
        }
        __syncthreads();
        lds_fft_pow2(fre, fim, nfft, lg, twiddle);
    }
    T gsum = 0;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        T g = 0;
        if (FFT) {
            if (l < Lc) g = fre[fft_brev(l, lg)];
        } else if (l < Lc) {
            int idx = 0;
            for (int k = 0; k < K; ++k) {
                g += Cre[k] * twiddle[2 * idx] + Cim[k] * twiddle[2 * idx + 1];
                idx += l;
                if (idx >= nfft) idx -= nfft;
            }
        }
        if (gwpart) gwpart[f * L + l] = g * xc[l];
        T gf = w ? g * w[l] : g;
        gsum += gf;
        gframe[f * L + l] = gf;
    }
    if (zmean) {
        T gm = block_sum(gsum, scratch) / T(L);
        for (int l = threadIdx.x; l < L; l += blockDim.x) gframe[f * L + l] -= gm;
    }
}

// out[l] = sum_f part[f, l] in a fixed order (deterministic window gradient)
template <typename T>
__global__ void colsum_kernel(const T* __restrict__ part, long F, int L, T* __restrict__ out)
{
    __shared__ T scratch[16];
    int l = blockIdx.x;
    T acc = 0;
    for (long f = threadIdx.x; f < F; f += blockDim.x) acc += part[f * L + l];
    T s = block_sum(acc, scratch);
    if (threadIdx.x == 0) out[l] = s;
}

// Spectrum with a denominator (spec.py:160-171): combines |B| and |A| amplitude rows.
// ab:(F,K) or NULL, aa:(F,K) or NULL (at least aa here), gain:(F) = a[:,0].
template <typename T>
__global__ void spec_ratio_kernel(const T* __restrict__ ab, const T* __restrict__ aa,
                                  const T* __restrict__ a, int la, int K, T eps, int use_floor,
                                  T floor_lin, int fmt, T* __restrict__ y)
{
    __shared__ T scratch[16];
    long f = blockIdx.x;
    T gain = a[f * la];
    T smax = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        T X = ab ? gain * (ab[f * K + k] / aa[f * K + k]) : gain / aa[f * K + k];
        T s = X * X + eps;
        smax = s > smax ? s : smax;
        y[f * K + k] = use_floor ? s : spec_format(s, fmt);
    }
    if (use_floor) {
        T m = block_max(smax, scratch);
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            T s = y[f * K + k];
            T fl = m * floor_lin;
            y[f * K + k] = spec_format(s > fl ? s : fl, fmt);
        }
    }
}

// Backward of Spectrum with a denominator (spec.py:160-177): X = K |B| / |A| (or K / |A| when b is
// absent), s = X^2 + eps -> floor -> format.  One block per row; B(w), A(w) recomputed by direct DFT.
//   Xbar = 2 X sbar;  |B|bar = Xbar K / |A|;  |A|bar = -Xbar X / |A|;  Kbar = sum_k Xbar X / K
//   bbar[l] = Re sum_k (|B|bar B/|B|) e^{+i theta k l}   (same for a[1:], a[0] = K gets Kbar)
// dynamic LDS: (lb + la + 5K) elements of T.
template <typename T>
__global__ void spec_ratio_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ b, int lb,
                                      const T* __restrict__ a, int la, int nfft, const T* __restrict__ twiddle,
                                      T eps, int use_floor, T floor_lin, int fmt, T* __restrict__ gb,
                                      T* __restrict__ ga)
{
    extern __shared__ unsigned char smem_raw[];
    __shared__ T scratch[16];
    const int K = nfft / 2 + 1;
    T* bs = reinterpret_cast<T*>(smem_raw);
    T* as = bs + lb;            // a1 = [1, a[1:]]
    T* Bre = as + la;
    T* Bim = Bre + K;
    T* Are = Bim + K;
    T* Aim = Are + K;
    T* gsv = Aim + K;           // cotangent of s per bin, later Xbar
    const long f = blockIdx.x;
    const int Lb = lb < nfft ? lb : nfft, La = la < nfft ? la : nfft;
    for (int l = threadIdx.x; l < lb; l += blockDim.x) bs[l] = b ? b[f * lb + l] : T(0);
    for (int l = threadIdx.x; l < la; l += blockDim.x) as[l] = l == 0 ? T(1) : a[f * la + l];
    __syncthreads();
    const T gain = a[f * la];
    T smax = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        T br = 0, bi = 0, ar = 0, ai = 0;
        int idx = 0;
        for (int l = 0; l < (Lb > La ? Lb : La); ++l) {
            const T c = twiddle[2 * idx], sn = twiddle[2 * idx + 1];
            if (b && l < Lb) { br += bs[l] * c; bi += bs[l] * sn; }
            if (l < La) { ar += as[l] * c; ai += as[l] * sn; }
            idx += k;
            if (idx >= nfft) idx -= nfft;
        }
        Bre[k] = br; Bim[k] = bi; Are[k] = ar; Aim[k] = ai;
        const T ab = b ? dsa_sqrt(br * br + bi * bi) : T(1), aa = dsa_sqrt(ar * ar + ai * ai);
        const T X = gain * ab / aa;
        const T sv = X * X + eps;
        smax = sv > smax ? sv : smax;
    }
    const T m = use_floor ? block_max(smax, scratch) : T(0);
    const T fl = m * floor_lin;
    __syncthreads();
    T lost = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const T ab = b ? dsa_sqrt(Bre[k] * Bre[k] + Bim[k] * Bim[k]) : T(1);
        const T aa = dsa_sqrt(Are[k] * Are[k] + Aim[k] * Aim[k]);
        const T X = gain * ab / aa;
        const T sv = X * X + eps;
        const bool floored = use_floor && sv < fl;
        const T se = floored ? fl : sv;
        T g = gy[f * K + k];
        switch (fmt) {
        case DSA_SPEC_DB: g *= T(4.342944819032518) / se; break;
        case DSA_SPEC_LOGMAG: g *= T(0.5) / se; break;
        case DSA_SPEC_MAG: g *= T(0.5) / dsa_sqrt(se); break;
        default: break;
        }
        if (floored) { lost += g; g = 0; }
        gsv[k] = g;
    }
    const T tot = use_floor ? block_sum(lost, scratch) * floor_lin : T(0);
    __syncthreads();
    T kacc = 0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const T ab = b ? dsa_sqrt(Bre[k] * Bre[k] + Bim[k] * Bim[k]) : T(1);
        const T aa = dsa_sqrt(Are[k] * Are[k] + Aim[k] * Aim[k]);
        const T X = gain * ab / aa;
        T gs = gsv[k];
        if (use_floor && (X * X + eps) == m) gs += tot;
        const T Xbar = T(2) * X * gs;
        kacc += Xbar * ab / aa;                       // dX/dK = |B|/|A|
        const T abar_b = Xbar * gain / aa;            // d/d|B|
        const T abar_a = -Xbar * X / aa;              // d/d|A|
        // complex cotangents of B and A through the amplitude (0 at an exact zero, like torch.abs)
        const T sb = (b && ab > T(0)) ? abar_b / ab : T(0), sa = aa > T(0) ? abar_a / aa : T(0);
        Bre[k] *= sb; Bim[k] *= sb; Are[k] *= sa; Aim[k] *= sa;
    }
    const T kbar = block_sum(kacc, scratch);
    __syncthreads();
    for (int l = threadIdx.x; l < (lb > la ? lb : la); l += blockDim.x) {
        T accb = 0, acca = 0;
        if (l < nfft) {
            int idx = 0;
            for (int k = 0; k < K; ++k) {
                const T c = twiddle[2 * idx], sn = twiddle[2 * idx + 1];
                accb += Bre[k] * c + Bim[k] * sn;
                acca += Are[k] * c + Aim[k] * sn;
                idx += l;
                if (idx >= nfft) idx -= nfft;
            }
        }
        if (gb && l < lb) gb[f * lb + l] = accb;
        if (l < la) ga[f * la + l] = l == 0 ? kbar : acca;
    }
}

// remove_gain (utils/private.py:200-209): a1 = [1, a[1:]]
template <typename T>
__global__ void remove_gain_kernel(const T* __restrict__ a, long F, int la, T* __restrict__ a1)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F * la) return;
    a1[i] = (i % la == 0) ? T(1) : a[i];
}

// ------------------------------------------------------------------ host-side dispatch helpers
template <typename T>
static int launch_row_dft(const void* x, int64_t B, int64_t Tlen, int64_t N, int L, int P, int left,
                          int mode, int zmean, const void* w, int nfft, const void* twiddle,
                          int out_kind, int fmt, double eps, int use_floor, double floor_db,
                          void* y, hipStream_t st)
{
    int64_t F = B * N;
    if (F == 0) return DSA_OK;
    T floor_lin = use_floor ? (T)pow(10.0, floor_db / 10.0) : T(0);
    size_t lds = sizeof(T) * (size_t)L;
    int threads = nfft / 2 + 1 >= 192 ? 256 : (nfft / 2 + 1 >= 96 ? 128 : 64);
    // power-of-two lengths: radix-2 FFT in LDS (DSA_ROWDFT_DIRECT=1 keeps the direct sum, for A/B runs and tests)
    const bool direct_only = env_int("DSA_ROWDFT_DIRECT", 0) != 0;
    const size_t lds_fft = lds + sizeof(T) * 2 * (size_t)nfft;
    if (!direct_only && nfft >= 32 && (nfft & (nfft - 1)) == 0 && lds_fft <= 150 * 1024) {
        if (int rc = launch_lds<row_dft_kernel<T, true>>(lds_fft > 48 * 1024 ? 150 * 1024 : 0, "row_fft: cannot raise the dynamic LDS limit%s",
                                                         dim3((unsigned)F), dim3(nfft >= 512 ? 256 : threads), lds_fft, st, (const T*)x, (long)Tlen,
                                                         (long)N, L, P, left, mode, zmean, (const T*)w, nfft, (const T*)twiddle, out_kind, fmt, (T)eps,
                                                         use_floor, floor_lin, (T*)y))
            return rc;
        return check_launch("row_fft_generic");
    }
    if (lds > 60 * 1024) return fail(DSA_ERR_UNSUPPORTED, "row_dft: frame too long for LDS%s");
    hipLaunchKernelGGL((row_dft_kernel<T>), dim3((unsigned)F), dim3(threads), lds, st, (const T*)x,
                       (long)Tlen, (long)N, L, P, left, mode, zmean, (const T*)w, nfft,
                       (const T*)twiddle, out_kind, fmt, (T)eps, use_floor, floor_lin, (T*)y);
    return check_launch("row_dft_generic");
}

}  // namespace dsa

using namespace dsa;

// =========================================================================== C-ABI

DSA_EXPORT int dsa_frame_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t center,
                             int32_t zmean, int32_t pad_mode, int32_t dtype, void* y, void* stream)
{
    DSA_REQUIRE(L > 0 && P > 0 && T > 0 && B >= 0, "frame: sizes must be positive");
    DSA_REQUIRE(pad_mode >= 0 && pad_mode <= 3, "frame: unknown pad mode");
    // F.pad(mode="reflect") needs every pad amount -- (L//2, (L-1)//2) centred, (0, L-1) otherwise, frame.py:130-137 --
    // below the signal length
    DSA_REQUIRE(pad_mode != DSA_PAD_REFLECT || (center ? L / 2 : L - 1) < T || L == 1,
                "frame: reflect padding needs pad < input length");
    int64_t N = dsa_num_frames(T, P), F = B * N;
    if (F == 0) return DSA_OK;
    int left = center ? L / 2 : 0;
    int threads = L >= 192 ? 256 : (L >= 96 ? 128 : 64);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DSA_F32 && !zmean && (L & 3) == 0 && (((size_t)y) & 15) == 0 && F * (int64_t)L >= 4096) {
        const int src_aligned = (P & 3) == 0 && (left & 3) == 0 && (T & 3) == 0 && (((size_t)x) & 15) == 0;
        long blocks = (long)((F * (int64_t)(L >> 2) + 255) / 256);
        if (blocks > 256 * 16) blocks = 256 * 16;
        hipLaunchKernelGGL(frame_fwd_vec4_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x, (long)T, (long)N,
                           (long)F, L, P, left, pad_mode, src_aligned, (float*)y);
        return check_launch("frame_fwd_vec4");
    }
    return with_dtype(dtype, "frame", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's signal length)
        hipLaunchKernelGGL((frame_fwd_kernel<V>), dim3((unsigned)F), dim3(threads), 0, st, (const V*)x, (long)T, (long)N, L, P, left, zmean, pad_mode,
                           (V*)y);
        return check_launch("frame_fwd");
    });
}

template <typename T>
static int frame_bwd_impl(const void* gy, int64_t B, int64_t Tlen, int L, int P, int center,
                          int zmean, int pad_mode, void* gx, hipStream_t st)
{
    int64_t N = dsa_num_frames(Tlen, P), F = B * N;
    int left = center ? L / 2 : 0;
    T* gmean = nullptr;
    if (zmean) {
        // d/dx of (y - mean(y)) = g - mean(g): per-frame mean of the cotangent
        if (hipMallocAsync((void**)&gmean, sizeof(T) * (size_t)F, st) != hipSuccess)
            return fail(DSA_ERR_LAUNCH, "frame_bwd: workspace allocation failed%s");
        hipLaunchKernelGGL((row_mean_kernel<T>), dim3((unsigned)F), dim3(64), 0, st, (const T*)gy, L, gmean);
    }
    if (pad_mode == DSA_PAD_CONSTANT) {
        const int64_t nblk = ((Tlen + 255) / 256) * B;
        if (nblk > 0x7fffffffLL) return fail(DSA_ERR_UNSUPPORTED, "frame_bwd: batch too large for one launch%s");
        dim3 grid((unsigned)nblk);
        hipLaunchKernelGGL((frame_bwd_const_kernel<T>), grid, dim3(256), 0, st, (const T*)gy, gmean,
                           (long)Tlen, (long)N, L, P, left, (T*)gx);
    } else {
        hipLaunchKernelGGL((frame_bwd_general_kernel<T>), dim3((unsigned)B), dim3(256), 0, st,
                           (const T*)gy, gmean, (long)Tlen, (long)N, L, P, left, pad_mode, (T*)gx);
    }
    int rc = check_launch("frame_bwd");
    if (gmean) hipFreeAsync(gmean, st);
    return rc;
}

DSA_EXPORT int dsa_frame_bwd(const void* gy, int64_t B, int64_t T, int32_t L, int32_t P, int32_t center,
                             int32_t zmean, int32_t pad_mode, int32_t dtype, void* gx, void* stream)
{
    DSA_REQUIRE(L > 0 && P > 0 && T > 0 && B >= 0, "frame_bwd: sizes must be positive");
    if (B == 0) return DSA_OK;
    return with_dtype(dtype, "frame_bwd", [&](auto tag) {
        return frame_bwd_impl<decltype(tag)>(gy, B, T, L, P, center, zmean, pad_mode, gx, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_window_fwd(const void* x, int64_t F, int32_t L, const void* w, int32_t L2, int32_t dtype,
                              void* y, void* stream)
{
    DSA_REQUIRE(L > 0 && L2 > 0 && F >= 0, "window: sizes must be positive");
    if (F == 0) return DSA_OK;
    int64_t total = F * L2;
    unsigned grid = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == DSA_F32 && window_vec4_ok(x, y, w, F, L, L2)) {
        const unsigned n4 = (unsigned)(F * (int64_t)(L >> 2));
        hipLaunchKernelGGL(window_vec4_kernel, dim3((n4 + 255) / 256 > 16384 ? 16384 : (n4 + 255) / 256), dim3(256), 0, st,
                           (const float4*)x, n4, (unsigned)(L >> 2), (const float4*)w, (float4*)y);
        return check_launch("window_vec4");
    }
    return with_dtype(dtype, "window", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((window_fwd_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)x, (long)F, L, (const T*)w, L2, (T*)y);
        return check_launch("window_fwd");
    });
}

DSA_EXPORT int dsa_window_bwd(const void* gy, const void* x, int64_t F, int32_t L, const void* w, int32_t L2,
                              int32_t dtype, void* gx, void* gw, void* stream)
{
    DSA_REQUIRE(L > 0 && L2 > 0 && F >= 0, "window_bwd: sizes must be positive");
    if (F == 0) return DSA_OK;
    int64_t total = F * L;
    unsigned grid = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "window_bwd", [&](auto tag) {
        using T = decltype(tag);
        if (dtype == DSA_F32 && window_vec4_ok(gy, gx, w, F, L, L2)) {   // the float32-only vector route of the forward
            const unsigned n4 = (unsigned)(F * (int64_t)(L >> 2));
            hipLaunchKernelGGL(window_vec4_kernel, dim3((n4 + 255) / 256 > 16384 ? 16384 : (n4 + 255) / 256), dim3(256), 0, st,
                               (const float4*)gy, n4, (unsigned)(L >> 2), (const float4*)w, (float4*)gx);
        } else
            hipLaunchKernelGGL((window_bwd_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)gy, (long)F, L, (const T*)w, L2, (T*)gx);
        if (gw) hipLaunchKernelGGL((window_gw_kernel<T>), dim3(L), dim3(256), 0, st, (const T*)gy, (const T*)x, (long)F, L, L2, (T*)gw);
        return check_launch("window_bwd");
    });
}

DSA_EXPORT int dsa_fftr_fwd(const void* x, int64_t F, int32_t len_in, int32_t nfft, int32_t out_format,
                            const void* twiddle, int32_t dtype, void* y, void* stream)
{
    DSA_REQUIRE(len_in > 0 && nfft > 0 && nfft % 2 == 0, "fftr: fft_length must be positive even");
    DSA_REQUIRE(out_format >= 0 && out_format <= 4, "fftr: unknown out_format");
    hipStream_t st = (hipStream_t)stream;
    // rows are "utterances" of len_in samples holding exactly one frame each
    return with_dtype(dtype, "fftr", [&](auto tag) {
        return launch_row_dft<decltype(tag)>(x, F, len_in, 1, len_in, len_in, 0, 0, 0, nullptr, nfft, twiddle, 0, out_format, 0.0, 0, 0.0, y, st);
    });
}

template <typename T>
static int spec_fwd_impl(const void* b, int lb, const void* a, int la, int64_t F, int nfft, double eps,
                         int use_floor, double floor_db, int fmt, const void* twiddle, void* y,
                         hipStream_t st)
{
    if (!a)
        return launch_row_dft<T>(b, F, lb, 1, lb, lb, 0, 0, 0, nullptr, nfft, twiddle, 1, fmt, eps,
                                 use_floor, floor_db, y, st);
    // denominator present: amplitude rows of b and of remove_gain(a), then the ratio kernel
    const int K = nfft / 2 + 1;
    T *amp_b = nullptr, *amp_a = nullptr, *a1 = nullptr;
    size_t rows = sizeof(T) * (size_t)F * K;
    if (hipMallocAsync((void**)&amp_a, rows, st) != hipSuccess ||
        hipMallocAsync((void**)&a1, sizeof(T) * (size_t)F * la, st) != hipSuccess ||
        (b && hipMallocAsync((void**)&amp_b, rows, st) != hipSuccess))
        return fail(DSA_ERR_LAUNCH, "spec: workspace allocation failed%s");
    int64_t tot = F * la;
    hipLaunchKernelGGL((remove_gain_kernel<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st,
                       (const T*)a, (long)F, la, a1);
    int rc = launch_row_dft<T>(a1, F, la, 1, la, la, 0, 0, 0, nullptr, nfft, twiddle, 0, DSA_FFTR_AMPLITUDE,
                               0.0, 0, 0.0, amp_a, st);
    if (rc == DSA_OK && b)
        rc = launch_row_dft<T>(b, F, lb, 1, lb, lb, 0, 0, 0, nullptr, nfft, twiddle, 0, DSA_FFTR_AMPLITUDE,
                               0.0, 0, 0.0, amp_b, st);
    if (rc == DSA_OK) {
        T floor_lin = use_floor ? (T)pow(10.0, floor_db / 10.0) : T(0);
        hipLaunchKernelGGL((spec_ratio_kernel<T>), dim3((unsigned)F), dim3(64), 0, st, (const T*)amp_b,
                           (const T*)amp_a, (const T*)a, la, K, (T)eps, use_floor, floor_lin, fmt, (T*)y);
        rc = check_launch("spec_ratio");
    }
    hipFreeAsync(amp_a, st);
    hipFreeAsync(a1, st);
    if (amp_b) hipFreeAsync(amp_b, st);
    return rc;
}

DSA_EXPORT int dsa_spec_fwd(const void* b, int32_t lb, const void* a, int32_t la, int64_t F, int32_t nfft,
                            double eps, int32_t use_floor, double relative_floor_db, int32_t out_format,
                            const void* twiddle, int32_t dtype, void* y, void* stream)
{
    DSA_REQUIRE(F == 0 || b || a, "spec: either b or a must be specified");
    DSA_REQUIRE(nfft > 1 && nfft % 2 == 0, "spec: fft_length must be positive even");
    DSA_REQUIRE(out_format >= 0 && out_format <= 3, "spec: unknown out_format");
    if (F == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "spec", [&](auto tag) {
        return spec_fwd_impl<decltype(tag)>(b, lb, a, la, F, nfft, eps, use_floor, relative_floor_db, out_format, twiddle, y, st);
    });
}

// --------------------------------------------------------------------------- backward entries
namespace dsa {

template <typename T>
static int launch_row_dft_bwd(const void* x, int64_t B, int64_t Tlen, int64_t N, int L, int P, int left,
                              int mode, int zmean, const void* w, int nfft, const void* twiddle,
                              int out_kind, int fmt, double eps, int use_floor, double floor_db,
                              const void* gy, void* gframe, void* gwpart, hipStream_t st)
{
    int64_t F = B * N;
    if (F == 0) return DSA_OK;
    T floor_lin = use_floor ? (T)pow(10.0, floor_db / 10.0) : T(0);
    const int K = nfft / 2 + 1;
    size_t lds = sizeof(T) * ((size_t)L + 3 * (size_t)K);
    const bool direct_only = env_int("DSA_ROWDFT_DIRECT", 0) != 0;
    const size_t lds_fft = lds + sizeof(T) * 2 * (size_t)nfft;
    if (!direct_only && nfft >= 32 && (nfft & (nfft - 1)) == 0 && lds_fft <= 150 * 1024) {
        if (int rc = launch_lds<row_dft_bwd_kernel<T, true>>(lds_fft > 48 * 1024 ? 150 * 1024 : 0, "row_fft_bwd: cannot raise the dynamic LDS limit%s",
                                                             dim3((unsigned)F), dim3(256), lds_fft, st, (const T*)x, (long)Tlen, (long)N, L, P, left,
                                                             mode, zmean, (const T*)w, nfft, (const T*)twiddle, out_kind, fmt, (T)eps, use_floor,
                                                             floor_lin, (const T*)gy, (T*)gframe, (T*)gwpart))
            return rc;
        return check_launch("row_fft_bwd_generic");
    }
    if (lds > 60 * 1024) return fail(DSA_ERR_UNSUPPORTED, "row_dft_bwd: frame too long for LDS%s");
    hipLaunchKernelGGL((row_dft_bwd_kernel<T>), dim3((unsigned)F), dim3(256), lds, st, (const T*)x, (long)Tlen,
                       (long)N, L, P, left, mode, zmean, (const T*)w, nfft, (const T*)twiddle, out_kind, fmt,
                       (T)eps, use_floor, floor_lin, (const T*)gy, (T*)gframe, (T*)gwpart);
    return check_launch("row_dft_bwd_generic");
}

template <typename T>
static int stft_bwd_generic(const void* gy, const void* x, int64_t B, int64_t Tlen, int L, int P, int nfft,
                            const void* w, const void* twiddle, int center, int zmean, int pad_mode,
                            double eps, int use_floor, double floor_db, int fmt, void* gx, void* gw,
                            hipStream_t st)
{
    int64_t N = dsa_num_frames(Tlen, P), F = B * N;
    int left = center ? L / 2 : 0;
    T *gframe = nullptr, *gwpart = nullptr;
    size_t bytes = sizeof(T) * (size_t)F * L;
    if (hipMallocAsync((void**)&gframe, bytes, st) != hipSuccess ||
        (gw && hipMallocAsync((void**)&gwpart, bytes, st) != hipSuccess))
        return fail(DSA_ERR_LAUNCH, "stft_bwd: workspace allocation failed%s");
    int rc = launch_row_dft_bwd<T>(x, B, Tlen, N, L, P, left, pad_mode, zmean, w, nfft, twiddle, 1, fmt, eps,
                                   use_floor, floor_db, gy, gframe, gwpart, st);
    // overlap-add (zmean already folded into gframe)
    if (rc == DSA_OK) rc = frame_bwd_impl<T>(gframe, B, Tlen, L, P, center, 0, pad_mode, gx, st);
    if (rc == DSA_OK && gw) {
        hipLaunchKernelGGL((colsum_kernel<T>), dim3(L), dim3(256), 0, st, (const T*)gwpart, (long)F, L, (T*)gw);
        rc = check_launch("window_grad_colsum");
    }
    (void)hipFreeAsync(gframe, st);
    if (gwpart) (void)hipFreeAsync(gwpart, st);
    return rc;
}

// The generic fallback of dsa_stft_fwd / dsa_stft_bwd (stft.hip), by dtype: any configuration, never the fast path.
int stft_generic_fwd(int dtype, const void* x, int64_t B, int64_t Tlen, int64_t N, int L, int P, int left, int mode, int zmean,
                     const void* w, int nfft, const void* twiddle, int fmt, double eps, int use_floor, double floor_db, void* y,
                     hipStream_t st)
{
    return with_dtype(dtype, "stft", [&](auto tag) {
        return launch_row_dft<decltype(tag)>(x, B, Tlen, N, L, P, left, mode, zmean, w, nfft, twiddle, 1, fmt, eps, use_floor, floor_db, y, st);
    });
}

int stft_generic_bwd(int dtype, const void* gy, const void* x, int64_t B, int64_t Tlen, int L, int P, int nfft, const void* w,
                     const void* twiddle, int center, int zmean, int pad_mode, double eps, int use_floor, double floor_db, int fmt,
                     void* gx, void* gw, hipStream_t st)
{
    return with_dtype(dtype, "stft_bwd", [&](auto tag) {
        return stft_bwd_generic<decltype(tag)>(gy, x, B, Tlen, L, P, nfft, w, twiddle, center, zmean, pad_mode, eps, use_floor, floor_db, fmt, gx, gw,
                                               st);
    });
}

}  // namespace dsa

DSA_EXPORT int dsa_fftr_bwd(const void* gy, const void* x, int64_t F, int32_t len_in, int32_t nfft,
                            int32_t out_format, const void* twiddle, int32_t dtype, void* gx, void* stream)
{
    DSA_REQUIRE(len_in > 0 && nfft > 0 && nfft % 2 == 0, "fftr_bwd: fft_length must be positive even");
    DSA_REQUIRE(out_format >= 0 && out_format <= 4, "fftr_bwd: unknown out_format");
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "fftr_bwd", [&](auto tag) {
        return launch_row_dft_bwd<decltype(tag)>(x, F, len_in, 1, len_in, len_in, 0, 0, 0, nullptr, nfft, twiddle, 0, out_format, 0.0, 0, 0.0, gy, gx,
                                                 nullptr, st);
    });
}

DSA_EXPORT int dsa_spec_bwd(const void* gy, const void* b, int32_t lb, const void* a, int32_t la, int64_t F,
                            int32_t nfft, double eps, int32_t use_floor, double relative_floor_db,
                            int32_t out_format, const void* twiddle, int32_t dtype, void* gb, void* ga,
                            void* stream)
{
    DSA_REQUIRE(F == 0 || b || a, "spec_bwd: either b or a must be specified");
    DSA_REQUIRE(nfft > 1 && nfft % 2 == 0, "spec_bwd: fft_length must be positive even");
    hipStream_t st = (hipStream_t)stream;
    if (a) {
        DSA_REQUIRE(F == 0 || ga != nullptr, "spec_bwd: ga is required when a is given");
        if (F == 0) return DSA_OK;
        const int K = nfft / 2 + 1;
        const size_t esz = dtype == DSA_F32 ? 4 : 8;
        const size_t lds = esz * ((size_t)lb + la + 5 * (size_t)K);
        if (lds > 60 * 1024) return fail(DSA_ERR_UNSUPPORTED, "spec_bwd: rows too long for LDS%s");
        const double fl = use_floor ? pow(10.0, relative_floor_db / 10.0) : 0.0;
        return with_dtype(dtype, "spec_bwd", [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL((spec_ratio_bwd_kernel<T>), dim3((unsigned)F), dim3(128), lds, st, (const T*)gy, (const T*)b, b ? lb : 0, (const T*)a, la,
                               nfft, (const T*)twiddle, (T)eps, use_floor, (T)fl, out_format, (T*)gb, (T*)ga);
            return check_launch("spec_ratio_bwd");
        });
    }
    return with_dtype(dtype, "spec_bwd", [&](auto tag) {
        return launch_row_dft_bwd<decltype(tag)>(b, F, lb, 1, lb, lb, 0, 0, 0, nullptr, nfft, twiddle, 1, out_format, eps, use_floor,
                                                 relative_floor_db, gy, gb, nullptr, st);
    });
}
