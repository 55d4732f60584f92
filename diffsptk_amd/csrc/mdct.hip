// Lapped transforms (include/diffsptk_amd.h, section a18):
//   mdct / mdst    ModifiedDiscreteCosineTransform._forward, mdct.py:166-176 with the basis of mdct.py:253-285
//   imdct / imdst  InverseModifiedDiscreteCosineTransform._forward, imdct.py:169-181
// (there: pad -> unfold -> mul -> matmul with a dense (L, L/2) basis, and back matmul -> mul -> fold -> divide: the framed (F, L)
// tensor in memory twice and L^2 / 2 multiply-adds per frame).  Here one launch each way, and two kernel families:
//
// FAST (float32, L a power of two in DSA_MDCT_FAST_MIN_LENGTH .. DSA_MDCT_FAST_MAX_LENGTH).  P = L/2, M = P/2.
//   analysis   a workgroup takes F consecutive frames of one utterance (F P about MD_TILE samples), stages their common span of
//              (F + 1) P samples in LDS -- every sample leaves memory once despite the 50 % overlap --, windows and folds each
//              frame L -> P (time-domain aliasing; v below), forms the DCT-IV of v through an M-point complex FFT
//                  t_n = (v_2n + i v_{P-1-2n}) e_n,  U = FFT_M(t),  c_k = U_k e_k,  X_2k = Re c_k,  X_{P-1-2k} = -Im c_k,
//                  e_n = exp(-i pi (8n + 1) / (8P)),
//              and writes the rows through LDS, coalesced.
//   synthesis  the mirror image: a workgroup owns F P consecutive output samples, which the F + 1 frames n0 .. n0 + F reach;
//              coefficients -> the same DCT-IV (it is its own transpose) -> q in LDS; then one thread per output sample unfolds
//              and windows the two frames that cover it and adds them -- older frame first --, scales and stores: no atomics, no
//              second pass, every sample written once.  (The frame n0 is transformed by this tile and by the one before it: F + 1
//              transforms for F frames of output.)
//   The sine transforms run the same path: sin(a(n+1/2)(k+1/2)) = (-1)^n cos(a(n+1/2)(P-1-k+1/2)), so the DST-IV is the DCT-IV of the
//   sign-alternated input read backwards, and only the signs of the fold change.
//   The M-point transforms of a tile run TOGETHER, radix 2^2 in place over [frame][M] arrays in LDS (one barrier per two stages
//   whatever F is; lds_fft_pow2 of lds_fft.h gives the whole workgroup to ONE transform, which leaves three waves of four idle at
//   M <= 256, and squares a twiddle where this one reads the table).  Output bit-reversed, undone by the index of the post-twiddle.
//   Samples outside [0, T) and frames outside [0, N) enter as zeros through the same arithmetic: a frame's bits depend on its own 2P
//   samples (or P coefficients), not on its place in a tile, an utterance or a batch.
//
// GENERIC (float64, and every other even L): the plain sums against the basis table the host layer builds in float64,
//   analysis   16 frames per workgroup; the windowed samples pass through LDS 64 at a time as [term][frame], thread = coefficient k, the basis read
//              coalesced along k; partial sums of 64 terms are added to the total (shorter error growth than one long chain);
//   synthesis  256 output samples per workgroup, thread = sample, the coefficient rows of the frames that reach them pass through LDS
//              64 at a time, the TRANSPOSED basis (P, L) read coalesced along the sample.
// Neither materialises the framed tensor.
#include "common.h"

namespace dsa {
namespace {

constexpr int MD_THREADS = 256;
constexpr int MD_TILE = 4096;   // samples of output (synthesis) or of hop (analysis) per fast tile
constexpr int MD_FG = 16;       // frames per generic analysis tile
constexpr int MD_JC = 64;       // terms per chunk of the generic sums
constexpr int MD_YS = 512;      // LDS elements of the generic synthesis: at most 255 / P + 3 frames of min(P, 64) coefficients, which is
                                // 255 + 3 P <= 444 for P < 64 and 6 * 64 = 384 from there on
static_assert(MD_THREADS - 1 + 3 * (MD_JC - 1) <= MD_YS && (MD_THREADS / MD_JC + 2) * MD_JC <= MD_YS, "the generic synthesis' LDS rows");

// ---- the M-point transforms of `nf` frames at once: radix 2^2 decimation in frequency, in place, bit-reversed output.
// ft: (cos, -sin)(2 pi m / M), m < M / 2.
__device__ __forceinline__ void md_fft_batch(float* re, float* im, int nf, int lgM, const float* __restrict__ ft)
{
    const int M = 1 << lgM;
    int s = lgM - 1;
    for (; s >= 1; s -= 2) {
        const int h = 1 << s, h2 = h >> 1;
        const int tstep = M >> (s + 1);
        const int groups = nf << (lgM - 2);
        for (int g = threadIdx.x; g < groups; g += MD_THREADS) {
            const int f = g >> (lgM - 2), t = g & ((M >> 2) - 1);
            const int j = t & (h2 - 1);
            const int i0 = (f << lgM) + (((t >> (s - 1)) << (s + 1)) | j);
            const float a0r = re[i0], a0i = im[i0], a1r = re[i0 + h2], a1i = im[i0 + h2];
            const float a2r = re[i0 + h], a2i = im[i0 + h], a3r = re[i0 + h + h2], a3i = im[i0 + h + h2];
            const float c1 = ft[2 * (j * tstep)], s1 = ft[2 * (j * tstep) + 1];
            const float c2 = s1, s2 = -c1;   // a quarter turn further
            const float c3 = ft[4 * (j * tstep)], s3 = ft[4 * (j * tstep) + 1];   // the twiddle of stage s - 1
            const float u0r = a0r + a2r, u0i = a0i + a2i, d0r = a0r - a2r, d0i = a0i - a2i;
            const float u1r = a1r + a3r, u1i = a1i + a3i, d1r = a1r - a3r, d1i = a1i - a3i;
            const float v0r = d0r * c1 - d0i * s1, v0i = d0r * s1 + d0i * c1;
            const float v1r = d1r * c2 - d1i * s2, v1i = d1r * s2 + d1i * c2;
            re[i0] = u0r + u1r;
            im[i0] = u0i + u1i;
            const float e0r = u0r - u1r, e0i = u0i - u1i;
            re[i0 + h2] = e0r * c3 - e0i * s3;
            im[i0 + h2] = e0r * s3 + e0i * c3;
            re[i0 + h] = v0r + v1r;
            im[i0 + h] = v0i + v1i;
            const float e1r = v0r - v1r, e1i = v0i - v1i;
            re[i0 + h + h2] = e1r * c3 - e1i * s3;
            im[i0 + h + h2] = e1r * s3 + e1i * c3;
        }
        __syncthreads();
    }
    if (s == 0) {   // an odd number of stages: the last one alone (twiddle 1)
        const int pairs = nf << (lgM - 1);
        for (int g = threadIdx.x; g < pairs; g += MD_THREADS) {
            const int i = g << 1;
            const float ar = re[i], ai = im[i], br = re[i + 1], bi = im[i + 1];
            re[i] = ar + br;
            im[i] = ai + bi;
            re[i + 1] = ar - br;
            im[i + 1] = ai - bi;
        }
        __syncthreads();
    }
}

// the folded frame: v_m of the windowed 2P samples u (cosine: (-c_r - d, a - b_r) of the quarters a b c d; sine: (c_r - d, a + b_r)
// with alternating sign)
__device__ __forceinline__ float md_fold(const float* u, const float* __restrict__ w, int m, int h, int sine)
{
    float r;
    if (m < h) {
        const float a = w[3 * h - 1 - m] * u[3 * h - 1 - m], b = w[3 * h + m] * u[3 * h + m];
        r = sine ? a - b : -a - b;
    } else {
        const float a = w[m - h] * u[m - h], b = w[3 * h - 1 - m] * u[3 * h - 1 - m];
        r = sine ? a + b : a - b;
    }
    return (sine && (m & 1)) ? -r : r;
}
// its transpose: sample j < 2P of the frame whose transform is q
__device__ __forceinline__ float md_unfold(const float* q, int j, int h, int sine)
{
    if (j < h) return q[j + h];
    if (j < 3 * h) return sine ? q[3 * h - 1 - j] : -q[3 * h - 1 - j];
    return -q[j - 3 * h];
}

// post-twiddle of the nf transforms in re / im into out[frame][P] (natural order; sine: read backwards), times z
__device__ __forceinline__ void md_post(const float* re, const float* im, int nf, int P, int lgM, const float* __restrict__ tw, float z, int sine,
                                        float* out)
{
    const int M = 1 << lgM;
    for (int g = threadIdx.x; g < (nf << lgM); g += MD_THREADS) {
        const int f = g >> lgM, k = g & (M - 1);
        const int pos = (f << lgM) + fft_brev(k, lgM);
        const float tr = re[pos], ti = im[pos], pr = tw[2 * k], pi = tw[2 * k + 1];
        const float cr = tr * pr - ti * pi, ci = tr * pi + ti * pr;
        const int i0 = 2 * k, i1 = P - 1 - 2 * k;
        out[f * P + (sine ? i1 : i0)] = z * cr;
        out[f * P + (sine ? i0 : i1)] = -(z * ci);
    }
}

__global__ __launch_bounds__(MD_THREADS) void mdct_analysis_fast(const float* __restrict__ x, long T, long N, int P, int lgM, int F, long tiles,
                                                                 const float* __restrict__ w, const float* __restrict__ tw, float z, int sine,
                                                                 int overlap, float* __restrict__ y)
{
    extern __shared__ float md_lds[];
    const int M = 1 << lgM, tid = threadIdx.x;
    float* xs = md_lds;              // (F + 1) P: the span, later the F rows of output
    float* re = xs + (F + 1) * P;    // F M
    float* im = re + F * M;          // F M
    const long b = blockIdx.x / tiles, n0 = (blockIdx.x % tiles) * F;
    const float* xb = x + b * T;
    const long s0 = (n0 - 1) * P, halved = (N - 1) * P;
    for (int i = tid; i < (F + 1) * P; i += MD_THREADS) {
        const long s = s0 + i;
        float v = 0.f;
        if (s >= 0 && s < T) {
            v = xb[s];
            if (overlap && s < halved) v *= 0.5f;
        }
        xs[i] = v;
    }
    __syncthreads();
    for (int g = tid; g < (F << lgM); g += MD_THREADS) {
        const int f = g >> lgM, n = g & (M - 1);
        const float* u = xs + f * P;
        const float ve = md_fold(u, w, 2 * n, M, sine), vo = md_fold(u, w, P - 1 - 2 * n, M, sine);
        const float pr = tw[2 * n], pi = tw[2 * n + 1];
        re[g] = ve * pr - vo * pi;
        im[g] = ve * pi + vo * pr;
    }
    __syncthreads();
    md_fft_batch(re, im, F, lgM, tw + 2 * M);
    md_post(re, im, F, P, lgM, tw, z, sine, xs);
    __syncthreads();
    const long rows = N - n0 < F ? N - n0 : F;
    float* yb = y + (b * N + n0) * P;
    for (long i = tid; i < rows * P; i += MD_THREADS) yb[i] = xs[i];
}

__global__ __launch_bounds__(MD_THREADS) void mdct_synthesis_fast(const float* __restrict__ y, long N, int P, int lgM, int F, long tiles,
                                                                  const float* __restrict__ w, const float* __restrict__ tw, float z, int sine,
                                                                  int overlap, long T, float* __restrict__ x)
{
    extern __shared__ float md_lds[];
    const int M = 1 << lgM, tid = threadIdx.x, G = F + 1, lgP = lgM + 1;
    float* re = md_lds;          // G M
    float* im = re + G * M;      // G M
    float* q = im + G * M;       // G P
    const long b = blockIdx.x / tiles, n0 = (blockIdx.x % tiles) * F;
    const float* yb = y + b * N * P;
    for (int g = tid; g < (G << lgM); g += MD_THREADS) {
        const int f = g >> lgM, n = g & (M - 1);
        float ve = 0.f, vo = 0.f;
        if (n0 + f < N) {
            const float* yr = yb + (n0 + f) * P;
            ve = yr[2 * n];
            vo = yr[P - 1 - 2 * n];
            if (sine) vo = -vo;
        }
        const float pr = tw[2 * n], pi = tw[2 * n + 1];
        re[g] = ve * pr - vo * pi;
        im[g] = ve * pi + vo * pr;
    }
    __syncthreads();
    md_fft_batch(re, im, G, lgM, tw + 2 * M);
    md_post(re, im, G, P, lgM, tw, z, sine, q);
    __syncthreads();
    const long t0 = n0 * P, halved = (N - 1) * P;
    float* xb = x + b * T;
    for (int i = tid; i < (F << lgP); i += MD_THREADS) {
        const long t = t0 + i;
        if (t >= T) break;
        const int fa = i >> lgP, jb = i & (P - 1), ja = jb + P;   // the older frame t / P reaches t + P with its second half
        const float o = w[ja] * md_unfold(q + fa * P, ja, M, sine) + w[jb] * md_unfold(q + (fa + 1) * P, jb, M, sine);
        xb[t] = overlap && t < halved ? 0.5f * o : o;
    }
}

template <typename T>
__global__ __launch_bounds__(MD_THREADS) void mdct_analysis_generic(const T* __restrict__ x, long Tlen, long N, int P, long tiles,
                                                                    const T* __restrict__ w, const T* __restrict__ C, int overlap,
                                                                    T* __restrict__ y)
{
    __shared__ __attribute__((aligned(16))) T wx[MD_JC][MD_FG];   // [term][frame]: a thread reads its 16 frames of one term as wide LDS reads
    const int tid = threadIdx.x, L = 2 * P;
    const long b = blockIdx.x / tiles, n0 = (blockIdx.x % tiles) * MD_FG;
    const T* xb = x + b * Tlen;
    const long halved = (N - 1) * P;
    for (int k0 = 0; k0 < P; k0 += MD_THREADS) {
        const int k = k0 + tid;
        T acc[MD_FG];
#pragma unroll
        for (int f = 0; f < MD_FG; ++f) acc[f] = T(0);
        for (int j0 = 0; j0 < L; j0 += MD_JC) {
            __syncthreads();
            for (int i = tid; i < MD_FG * MD_JC; i += MD_THREADS) {
                const int f = i / MD_JC, jj = i % MD_JC, j = j0 + jj;
                const long s = (n0 + f - 1) * P + j;
                T v = T(0);
                if (j < L && n0 + f < N && s >= 0 && s < Tlen) {
                    v = xb[s];
                    if (overlap && s < halved) v *= T(0.5);
                    v *= w[j];
                }
                wx[jj][f] = v;
            }
            __syncthreads();
            if (k < P) {
                T part[MD_FG];
#pragma unroll
                for (int f = 0; f < MD_FG; ++f) part[f] = T(0);
                const int jn = L - j0 < MD_JC ? L - j0 : MD_JC;
                for (int jj = 0; jj < jn; ++jj) {
                    const T c = C[(long)(j0 + jj) * P + k];
#pragma unroll
                    for (int f = 0; f < MD_FG; ++f) part[f] += wx[jj][f] * c;
                }
#pragma unroll
                for (int f = 0; f < MD_FG; ++f) acc[f] += part[f];
            }
        }
        if (k < P) {
#pragma unroll
            for (int f = 0; f < MD_FG; ++f)
                if (n0 + f < N) y[(b * N + n0 + f) * P + k] = acc[f];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(MD_THREADS) void mdct_synthesis_generic(const T* __restrict__ y, long N, int P, long tiles, const T* __restrict__ w,
                                                                     const T* __restrict__ Ct, int overlap, long Tlen, T* __restrict__ x)
{
    __shared__ T ys[MD_YS];
    const int tid = threadIdx.x, L = 2 * P;
    const long b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * MD_THREADS, t = t0 + tid;
    const long nlo = t0 / P;                                   // the older frame of the tile's first sample
    const int nf = (int)((t0 + MD_THREADS - 1) / P + 2 - nlo);   // frames nlo .. nlo + nf - 1 reach the tile
    const long na = t / P;
    const int fa = (int)(na - nlo), jb = (int)(t - na * P), ja = jb + P;
    const T* yb = y + b * N * P;
    T acc_a = T(0), acc_b = T(0);
    for (int k0 = 0; k0 < P; k0 += MD_JC) {
        const int kc = P - k0 < MD_JC ? P - k0 : MD_JC;
        __syncthreads();
        for (int i = tid; i < nf * kc; i += MD_THREADS) {
            const int f = i / kc, kk = i % kc;
            ys[i] = nlo + f < N ? yb[(nlo + f) * P + k0 + kk] : T(0);
        }
        __syncthreads();
        if (t < Tlen) {
            T pa = T(0), pb = T(0);
            for (int kk = 0; kk < kc; ++kk) {
                const T* row = Ct + (long)(k0 + kk) * L;
                pa += ys[fa * kc + kk] * row[ja];
                pb += ys[(fa + 1) * kc + kk] * row[jb];
            }
            acc_a += pa;
            acc_b += pb;
        }
    }
    if (t < Tlen) {
        const T o = w[ja] * acc_a + w[jb] * acc_b;
        x[b * Tlen + t] = overlap && t < (N - 1) * P ? T(0.5) * o : o;
    }
}

// sizes and options both entries share; 0: run, 1: nothing to do
int md_check(const char* what, int64_t B, int64_t T, int64_t N, int32_t L, int32_t transform, int32_t scale, int32_t dtype, int32_t algo,
             bool* fast, const void* twiddle, const void* basis)
{
    if (!(L >= 2 && L % 2 == 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: the frame length must be at least 2 and even", what);
    if (!(B >= 0 && N >= 0 && T >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: invalid sizes", what);
    const int64_t P = L / 2;
    if (N > INT64_MAX / P || T > N * P) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: T exceeds N * L / 2", what);
    if (N > 0 && B > INT64_MAX / (N * P) / 2) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: invalid sizes", what);   // B N P is an int64 offset
    if (transform != DSA_MDCT_COSINE && transform != DSA_MDCT_SINE) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: unknown transform", what);
    if (scale != DSA_MDCT_SCALE_NONE && scale != DSA_MDCT_SCALE_OVERLAP) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: unknown scale", what);
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: unknown dtype", what);
    if (algo != DSA_ALGO_AUTO && algo != DSA_ALGO_GENERIC && algo != DSA_ALGO_TUNED) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: unknown algo", what);
    const bool can = dtype == DSA_F32 && (L & (L - 1)) == 0 && L >= DSA_MDCT_FAST_MIN_LENGTH && L <= DSA_MDCT_FAST_MAX_LENGTH;
    if (algo == DSA_ALGO_TUNED && !can)
        return fail(DSA_ERR_UNSUPPORTED, "%s: the fast kernels take float32 and a power-of-two frame length in their range", what);
    *fast = can && algo != DSA_ALGO_GENERIC && (twiddle || algo == DSA_ALGO_TUNED || !basis);
    return DSA_OK;
}

int md_lg(int v)
{
    int lg = 0;
    while ((1 << lg) < v) ++lg;
    return lg;
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_mdct_analysis(const void* x, int64_t B, int64_t T, int64_t N, int32_t L, const void* w, const void* basis, const void* twiddle,
                                 double z, int32_t transform, int32_t scale, int32_t dtype, int32_t algo, void* y, void* stream)
{
    bool fast = false;
    if (int rc = md_check("mdct analysis", B, T, N, L, transform, scale, dtype, algo, &fast, twiddle, basis)) return rc;
    if (B == 0 || N == 0) return DSA_OK;
    if (T < 1) return fail(DSA_ERR_INVALID_ARGUMENT, "mdct analysis: an empty waveform");
    if (!(x && w && y && (fast ? twiddle : basis))) return fail(DSA_ERR_INVALID_ARGUMENT, "mdct analysis: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int P = L / 2, sine = transform == DSA_MDCT_SINE, overlap = scale == DSA_MDCT_SCALE_OVERLAP;
    if (fast) {
        int64_t F = MD_TILE / P < 1 ? 1 : MD_TILE / P;
        if (F > N) F = N;
        const int64_t tiles = (N + F - 1) / F;
        if (tiles > INT32_MAX / B) return fail(DSA_ERR_INVALID_ARGUMENT, "mdct analysis: too many tiles for one launch");
        const size_t lds = (size_t)((F + 1) * P + F * P) * sizeof(float);
        hipLaunchKernelGGL(mdct_analysis_fast, dim3((unsigned)(B * tiles)), dim3(MD_THREADS), lds, st, (const float*)x, (long)T, (long)N, P,
                           md_lg(P / 2), (int)F, (long)tiles, (const float*)w, (const float*)twiddle, (float)z, sine, overlap, (float*)y);
        return check_launch("mdct_analysis_fast");
    }
    const int64_t tiles = (N + MD_FG - 1) / MD_FG;
    if (tiles > INT32_MAX / B) return fail(DSA_ERR_INVALID_ARGUMENT, "mdct analysis: too many tiles for one launch");
    const dim3 grid((unsigned)(B * tiles));
    return with_dtype(dtype, "mdct analysis", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's waveform length)
        hipLaunchKernelGGL((mdct_analysis_generic<V>), grid, dim3(MD_THREADS), 0, st, (const V*)x, (long)T, (long)N, P, (long)tiles, (const V*)w,
                           (const V*)basis, overlap, (V*)y);
        return check_launch("mdct_analysis_generic");
    });
}

DSA_EXPORT int dsa_mdct_synthesis(const void* y, int64_t B, int64_t N, int32_t L, const void* w, const void* basis_t, const void* twiddle, double z,
                                  int32_t transform, int32_t scale, int64_t T, int32_t dtype, int32_t algo, void* x, void* stream)
{
    bool fast = false;
    if (int rc = md_check("mdct synthesis", B, T, N, L, transform, scale, dtype, algo, &fast, twiddle, basis_t)) return rc;
    if (B == 0 || N == 0 || T == 0) return DSA_OK;
    if (!(y && w && x && (fast ? twiddle : basis_t))) return fail(DSA_ERR_INVALID_ARGUMENT, "mdct synthesis: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int P = L / 2, sine = transform == DSA_MDCT_SINE, overlap = scale == DSA_MDCT_SCALE_OVERLAP;
    if (fast) {
        int64_t F = MD_TILE / P < 1 ? 1 : MD_TILE / P;
        const int64_t hops = (T + P - 1) / P;
        if (F > hops) F = hops;
        const int64_t tiles = (hops + F - 1) / F;
        if (tiles > INT32_MAX / B) return fail(DSA_ERR_INVALID_ARGUMENT, "mdct synthesis: too many tiles for one launch");
        const size_t lds = (size_t)(2 * (F + 1) * P) * sizeof(float);
        hipLaunchKernelGGL(mdct_synthesis_fast, dim3((unsigned)(B * tiles)), dim3(MD_THREADS), lds, st, (const float*)y, (long)N, P, md_lg(P / 2),
                           (int)F, (long)tiles, (const float*)w, (const float*)twiddle, (float)z, sine, overlap, (long)T, (float*)x);
        return check_launch("mdct_synthesis_fast");
    }
    const int64_t tiles = (T + MD_THREADS - 1) / MD_THREADS;
    if (tiles > INT32_MAX / B) return fail(DSA_ERR_INVALID_ARGUMENT, "mdct synthesis: too many tiles for one launch");
    const dim3 grid((unsigned)(B * tiles));
    return with_dtype(dtype, "mdct synthesis", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's waveform length)
        hipLaunchKernelGGL((mdct_synthesis_generic<V>), grid, dim3(MD_THREADS), 0, st, (const V*)y, (long)N, P, (long)tiles, (const V*)w,
                           (const V*)basis_t, overlap, (long)T, (V*)x);
        return check_launch("mdct_synthesis_generic");
    });
}
