// Pseudo-QMF bank: PseudoQuadratureMirrorFilterBankAnalysis / Synthesis (pqmf.py:226-258, ipqmf.py:105-141 of the reference), with
// the Decimation after the analysis and the Interpolation before the synthesis folded in (decimate.py:88-93, interpolate.py:85-96),
// and Interpolation on its own.  f:(K, M+1) are the filters in the reference's stored, time-flipped layout, so each product is the
// correlation F.conv1d computes:
//   analysis   y[b,k,m] = sum_i f[k,i] xp[b, s + m P + i]          xp = dl zeros | x | dr copies of x[T-1]
//   synthesis  x[b,t]   = sum_k sum_i f[k,i] yp[b,k,t + i]         yp = dl zeros | yu | dr copies of yu[Tu-1]
//              yu[b,k,n] = y[b,k,(n - s) / U] on the grid n = s + m U, 0 elsewhere;  Tu = T U + s
// (P, s) = (1, 0) is the plain analysis and (U, s) = (1, 0) the plain synthesis.  The decimated analysis computes only the kept
// outputs; the up-sampled synthesis evaluates only the taps that land on the grid (about (M+1)/U per band) and never writes yu.
// Every output is ONE fma chain in a fixed order -- taps ascending (analysis), bands then taps (synthesis), padded positions then
// bands then taps (the adjoints) -- whatever the tiling or the batch.  A skipped tap is an exact zero product, so the folded routes
// give the bits of the module chain for finite data, and a row's bits do not depend on the batch.
// The filter gradients are per-utterance partials (each a sum over time in ascending order) in a caller-owned workspace, then a
// second pass sums them in a fixed order: no atomics, the same bits run to run.
#include "common.h"

#include <climits>

namespace dsa {
namespace {

constexpr int kPqTile = 256;    // outputs per workgroup of the tuned forward kernels
constexpr int kPqChunk = 256;   // time samples per LDS chunk of the filter-gradient partials

__device__ __forceinline__ long pq_mod(long a, long b)
{
    const long r = a % b;
    return r < 0 ? r + b : r;
}
__device__ __forceinline__ long pq_floordiv(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__device__ __forceinline__ long pq_ceildiv(long a, long b) { return -pq_floordiv(-a, b); }

// the analysis' padded signal: dl zeros, x, x[T-1] repeated (T >= 1)
template <typename T>
__device__ __forceinline__ T pq_xp(const T* __restrict__ xb, long q, long Tlen, int dl)
{
    if (q < dl) return T(0);
    const long i = q - dl;
    return xb[i < Tlen ? i : Tlen - 1];
}

inline unsigned pq_blocks(long n) { return (unsigned)((n + 255) / 256 < (1L << 20) ? (n + 255) / 256 : (1L << 20)); }

// ---------------------------------------------------------------------------------------------------------------- analysis
// tuned: one workgroup = 256 consecutive kept outputs of one utterance, all K bands.  The padded signal the tile reads is staged
// in LDS split by phase modulo P (xs[r][u] = xp[q0 + u P + r]) so that the lanes of one tap read consecutive words whatever the
// period; the filter taps are wave-uniform loads.
template <typename T, int K>
__global__ __launch_bounds__(256) void pqmf_fwd_tuned_kernel(const T* __restrict__ x, const T* __restrict__ f, long Tlen, long Tout,
                                                             long ntile, int M, int P, int s, int dl, T* __restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* fs = reinterpret_cast<T*>(smem_raw);   // [M+1][K]
    const int tid = threadIdx.x, M1 = M + 1, Wp = kPqTile + M / P;
    T* xs = fs + ((M1 * K + 3) & ~3);         // [P][Wp]
    const long b = blockIdx.x / ntile, m0 = (blockIdx.x - b * ntile) * (long)kPqTile;
    const T* xb = x + b * Tlen;
    const long q0 = s + m0 * P;
    for (int e = tid; e < M1 * K; e += 256) fs[e] = f[(e % K) * M1 + e / K];
    for (int e = tid; e < P * Wp; e += 256) {
        const int r = e / Wp, u = e - r * Wp;
        xs[e] = pq_xp(xb, q0 + (long)u * P + r, Tlen, dl);
    }
    __syncthreads();
    const long m = m0 + tid;
    if (m >= Tout) return;
    T acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = T(0);
    int r = 0, u = tid;
#pragma unroll 4
    for (int i = 0; i < M1; ++i) {
        const T v = xs[r * Wp + u];
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = fma(fs[i * K + k], v, acc[k]);
        if (++r == P) {
            r = 0;
            ++u;
        }
    }
    T* yb = y + b * K * Tout + m;
#pragma unroll
    for (int k = 0; k < K; ++k) yb[k * Tout] = acc[k];
}

// generic: one thread per output element
template <typename T>
__global__ __launch_bounds__(256) void pqmf_fwd_generic_kernel(const T* __restrict__ x, const T* __restrict__ f, long B, long Tlen, long Tout,
                                                               int K, int M, int P, int s, int dl, T* __restrict__ y)
{
    const long n = B * K * Tout;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long m = e % Tout, bk = e / Tout, k = bk % K, b = bk / K;
        const T* xb = x + b * Tlen;
        const T* fk = f + k * (M + 1);
        const long q0 = s + m * P;
        T acc = T(0);
        for (int i = 0; i <= M; ++i) acc = fma(fk[i], pq_xp(xb, q0 + i, Tlen, dl), acc);
        y[e] = acc;
    }
}

// gx[b,j]: over the padded positions q that read x[j] (q = dl + j, and the dr replicate positions for j = T-1), ascending, the sum
// over bands and taps of f[k,i] gy[b,k,m] with s + m P = q - i -- only the taps on the grid are visited
template <typename T, bool PLAIN>
__global__ __launch_bounds__(256) void pqmf_bwd_x_kernel(const T* __restrict__ gy, const T* __restrict__ f, long B, long Tlen, long Tout,
                                                         int K, int M, int P, int s, int dl, int dr, T* __restrict__ gx)
{
    const long n = B * Tlen;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long j = e % Tlen, b = e / Tlen;
        const T* gb = gy + b * K * Tout;
        const long q1 = dl + j, q2 = j == Tlen - 1 ? q1 + dr : q1;
        T acc = T(0);
        for (long q = q1; q <= q2; ++q) {
            const int i0 = PLAIN ? 0 : (int)pq_mod(q - s, P);
            for (int k = 0; k < K; ++k) {
                const T* fk = f + k * (M + 1);
                const T* gk = gb + k * Tout;
                for (int i = i0; i <= M; i += (PLAIN ? 1 : P)) {
                    const long t = q - i;   // an output time of the undecimated analysis
                    if (t < s) break;
                    const long m = (t - s) / P;
                    if (m < Tout) acc = fma(fk[i], gk[m], acc);
                }
            }
        }
        gx[e] = acc;
    }
}

// tuned gx of the plain analysis (P = 1, s = 0): one workgroup = 256 consecutive samples of one utterance, with the gy values of all K
// bands the tile reads and the filters in LDS; the terms and their order are pqmf_bwd_x_kernel's
template <typename T, int K>
__global__ __launch_bounds__(256) void pqmf_bwd_x_tuned_kernel(const T* __restrict__ gy, const T* __restrict__ f, long Tlen, long ntile, int M,
                                                               int dl, int dr, T* __restrict__ gx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* fs = reinterpret_cast<T*>(smem_raw);   // [K][M+1]
    const int tid = threadIdx.x, M1 = M + 1, W = kPqTile + M + dr;
    T* gs = fs + ((M1 * K + 3) & ~3);         // [K][W]: gy[t], t = tlo + u
    const long b = blockIdx.x / ntile, j0 = (blockIdx.x - b * ntile) * (long)kPqTile;
    const long tlo = j0 + dl - M;             // the lowest t the tile reads
    for (int e = tid; e < M1 * K; e += 256) fs[e] = f[e];
    for (int e = tid; e < K * W; e += 256) {
        const int k = e / W, u = e - k * W;
        const long t = tlo + u;
        gs[e] = (t >= 0 && t < Tlen) ? gy[(b * K + k) * Tlen + t] : T(0);
    }
    __syncthreads();
    const long j = j0 + tid;
    if (j >= Tlen) return;
    const long q1 = dl + j, q2 = j == Tlen - 1 ? q1 + dr : q1;
    T acc = T(0);
    for (long q = q1; q <= q2; ++q) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T* fk = fs + k * M1;
            const T* gk = gs + k * W - tlo;
#pragma unroll 4
            for (int i = 0; i <= M; ++i) {
                const long t = q - i;
                if (t >= Tlen) continue;
                if (t < 0) break;
                acc = fma(fk[i], gk[t], acc);
            }
        }
    }
    gx[b * Tlen + j] = acc;
}

// per-utterance partials of gf[k,i] = sum_m gy[b,k,m] xp[b, s + m P + i], over time in ascending order (LDS chunks of xp)
template <typename T>
__global__ __launch_bounds__(256) void pqmf_bwd_f_kernel(const T* __restrict__ gy, const T* __restrict__ x, long Tlen, long Tout, int K,
                                                         int M, int P, int s, int dl, T* __restrict__ work)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* xs = reinterpret_cast<T*>(smem_raw);   // [kPqChunk + M]: xp from c0
    const int tid = threadIdx.x, M1 = M + 1, KM1 = K * M1;
    const long b = blockIdx.x;
    const T* xb = x + b * Tlen;
    for (int g0 = 0; g0 < KM1; g0 += 256) {
        const int kj = g0 + tid, k = kj / M1, i = kj - k * M1;
        const T* gk = gy + (b * K + (kj < KM1 ? k : 0)) * Tout;
        T acc = T(0);
        for (long c0 = 0; c0 < Tlen; c0 += kPqChunk) {
            __syncthreads();
            for (int e = tid; e < kPqChunk + M; e += 256) xs[e] = pq_xp(xb, c0 + e, Tlen, dl);
            __syncthreads();
            if (kj < KM1) {
                long mlo = pq_ceildiv(c0 - s, P), mhi = pq_floordiv(c0 + kPqChunk - 1 - s, P);
                if (mlo < 0) mlo = 0;
                if (mhi > Tout - 1) mhi = Tout - 1;
                for (long m = mlo; m <= mhi; ++m) acc = fma(gk[m], xs[s + m * P - c0 + i], acc);
            }
        }
        if (kj < KM1) work[b * KM1 + kj] = acc;
    }
}

// --------------------------------------------------------------------------------------------------------------- synthesis
// tuned: one workgroup = 256 consecutive outputs of one utterance; the grid samples of all K bands the tile reads in LDS.
// (T >= 1: the entry writes the zeros of an empty input itself)
template <typename T, int K, bool PLAIN>
__global__ __launch_bounds__(256) void ipqmf_fwd_tuned_kernel(const T* __restrict__ y, const T* __restrict__ f, long Tin, long Tu, long ntile,
                                                              int M, int U, int s, int dl, T* __restrict__ x)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* fs = reinterpret_cast<T*>(smem_raw);   // [K][M+1]
    const int tid = threadIdx.x, M1 = M + 1, Wm = (kPqTile - 1 + M) / U + 2;
    T* ys = fs + ((M1 * K + 3) & ~3);         // [K][Wm]
    for (int e = tid; e < M1 * K; e += 256) fs[e] = f[e];
    const long b = blockIdx.x / ntile, t0 = (blockIdx.x - b * ntile) * (long)kPqTile;
    long nhi = t0 + kPqTile - 1 + M - dl;
    if (nhi > Tu - 1) nhi = Tu - 1;
    long mlo = pq_ceildiv(t0 - dl - s, U), mhi = pq_floordiv(nhi - s, U);
    if (mlo < 0) mlo = 0;
    if (mhi > Tin - 1) mhi = Tin - 1;
    const int cnt = mhi >= mlo ? (int)(mhi - mlo + 1) : 0;   // <= Wm
    for (int e = tid; e < K * cnt; e += 256) {
        const int k = e / cnt, u = e - k * cnt;
        ys[k * Wm + u] = y[(b * K + k) * Tin + mlo + u];
    }
    __syncthreads();
    const long t = t0 + tid;
    if (t >= Tu) return;
    T acc = T(0);
    if (PLAIN) {   // U = 1: every tap, the same tap in every lane
        const long n0 = t - dl - s;   // index into y of tap 0 (clamped to [0, T-1] where the pads are read)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T* fk = fs + k * M1;
            const T* yk = ys + k * Wm - mlo;
#pragma unroll 4
            for (int i = 0; i <= M; ++i) {
                long n = n0 + i;
                if (n < 0) continue;
                if (n > Tin - 1) n = Tin - 1;
                acc = fma(fk[i], yk[n], acc);
            }
        }
    } else {
        const int i0 = (int)pq_mod(s + dl - t, U);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T* fk = fs + k * M1;
            const T* yk = ys + k * Wm - mlo;
            for (int i = i0; i <= M; i += U) {
                long n = t + i - dl;
                if (n < s) continue;
                if (n > Tu - 1) {
                    if (U > 1) break;   // the replicated last sample is off the grid: zero
                    n = Tu - 1;
                }
                acc = fma(fk[i], yk[(n - s) / U], acc);
            }
        }
    }
    x[b * Tu + t] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void ipqmf_fwd_generic_kernel(const T* __restrict__ y, const T* __restrict__ f, long B, long Tin, long Tu,
                                                                int K, int M, int U, int s, int dl, T* __restrict__ x)
{
    const long n = B * Tu;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long t = e % Tu, b = e / Tu;
        const int i0 = (int)pq_mod(s + dl - t, U);
        T acc = T(0);
        for (int k = 0; k < K; ++k) {
            const T* fk = f + k * (M + 1);
            const T* yk = y + (b * K + k) * Tin;
            for (int i = i0; i <= M; i += U) {
                long nn = t + i - dl;
                if (nn < s) continue;
                if (nn > Tu - 1) {
                    if (U > 1) break;
                    nn = Tu - 1;
                }
                acc = fma(fk[i], yk[(nn - s) / U], acc);
            }
        }
        x[e] = acc;
    }
}

// gy[b,k,m] at the grid position n = s + m U: over the padded positions q that read yu[n] (q = dl + n, and the dr replicate
// positions for n = Tu - 1), ascending, the sum over taps of f[k,i] gx[b, q - i]
template <typename T>
__global__ __launch_bounds__(256) void ipqmf_bwd_y_kernel(const T* __restrict__ gx, const T* __restrict__ f, long B, long Tin, long Tu, int K,
                                                          int M, int U, int s, int dl, int dr, T* __restrict__ gy)
{
    const long n = B * K * Tin;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long m = e % Tin, bk = e / Tin, k = bk % K, b = bk / K;
        const T* fk = f + k * (M + 1);
        const T* gb = gx + b * Tu;
        const long nn = s + m * U, q1 = dl + nn, q2 = nn == Tu - 1 ? q1 + dr : q1;
        T acc = T(0);
        for (long q = q1; q <= q2; ++q)
            for (int i = 0; i <= M; ++i) {
                const long t = q - i;
                if (t >= Tu) continue;
                if (t < 0) break;
                acc = fma(fk[i], gb[t], acc);
            }
        gy[e] = acc;
    }
}

// tuned gy of the plain synthesis (U = 1, s = 0): one workgroup = 256 consecutive samples of one utterance, all K bands, with the gx
// values the tile reads and the filters ([i][K]: one wide broadcast read per tap) in LDS; per band the terms and their order are
// ipqmf_bwd_y_kernel's
template <typename T, int K>
__global__ __launch_bounds__(256) void ipqmf_bwd_y_tuned_kernel(const T* __restrict__ gx, const T* __restrict__ f, long Tu, long ntile, int M,
                                                                int dl, int dr, T* __restrict__ gy)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* fs = reinterpret_cast<T*>(smem_raw);   // [M+1][K]
    const int tid = threadIdx.x, M1 = M + 1, W = kPqTile + M + dr;
    T* gs = fs + ((M1 * K + 3) & ~3);         // [W]: gx[t], t = tlo + u
    const long b = blockIdx.x / ntile, n0 = (blockIdx.x - b * ntile) * (long)kPqTile;
    const long tlo = n0 + dl - M;
    for (int e = tid; e < M1 * K; e += 256) fs[e] = f[(e % K) * M1 + e / K];
    for (int e = tid; e < W; e += 256) {
        const long t = tlo + e;
        gs[e] = (t >= 0 && t < Tu) ? gx[b * Tu + t] : T(0);
    }
    __syncthreads();
    const long n = n0 + tid;
    if (n >= Tu) return;
    const long q1 = dl + n, q2 = n == Tu - 1 ? q1 + dr : q1;
    T acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = T(0);
    for (long q = q1; q <= q2; ++q) {
#pragma unroll 4
        for (int i = 0; i <= M; ++i) {
            const long t = q - i;
            if (t >= Tu) continue;
            if (t < 0) break;
            const T v = gs[t - tlo];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = fma(fs[i * K + k], v, acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) gy[(b * K + k) * Tu + n] = acc[k];
}

// per-utterance partials of gf[k,i] = sum_t gx[b,t] yp[b,k,t + i], over time in ascending order (LDS chunks of gx); T >= 1
template <typename T>
__global__ __launch_bounds__(256) void ipqmf_bwd_f_kernel(const T* __restrict__ gx, const T* __restrict__ y, long Tin, long Tu, int K, int M,
                                                          int U, int s, int dl, T* __restrict__ work)
{
    __shared__ T gs[kPqChunk];
    const int tid = threadIdx.x, M1 = M + 1, KM1 = K * M1;
    const long b = blockIdx.x;
    const T* gb = gx + b * Tu;
    for (int g0 = 0; g0 < KM1; g0 += 256) {
        const int kj = g0 + tid, k = kj / M1, i = kj - k * M1;
        const T* yk = y + (b * K + (kj < KM1 ? k : 0)) * Tin;
        T acc = T(0);
        for (long c0 = 0; c0 < Tu; c0 += kPqChunk) {
            const int cl = (int)(Tu - c0 < kPqChunk ? Tu - c0 : kPqChunk);
            __syncthreads();
            for (int e = tid; e < cl; e += 256) gs[e] = gb[c0 + e];
            __syncthreads();
            if (kj < KM1) {
                long e = s + dl - i - c0;   // the first t of the chunk with n = t + i - dl >= s ...
                if (e < 0) e = 0;
                e += pq_mod(s + dl - i - c0 - e, U);   // ... on the grid
                for (; e < cl; e += U) {
                    long nn = c0 + e + i - dl;
                    if (nn > Tu - 1) {
                        if (U > 1) break;
                        nn = Tu - 1;
                    }
                    acc = fma(gs[e], yk[(nn - s) / U], acc);
                }
            }
        }
        if (kj < KM1) work[b * KM1 + kj] = acc;
    }
}

// gf[kj] = the B partials summed: four waves over the rows (row r to wave r % 4), then the four in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void pqmf_f_sum_kernel(const T* __restrict__ work, long B, int KM1, T* __restrict__ gf)
{
    __shared__ T red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int kj = blockIdx.x * 64 + lane;
    T acc = T(0);
    if (kj < KM1)
        for (long r = w; r < B; r += 4) acc += work[r * KM1 + kj];
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && kj < KM1) gf[kj] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// ------------------------------------------------------------------------------------------------------------ interpolation
// over the (outer, T, inner) view: y[o, n, i] = x[o, (n - s) / P, i] on the grid n = s + m P, 0 elsewhere (every element written)
template <typename T>
__global__ __launch_bounds__(256) void interp_fwd_kernel(const T* __restrict__ x, long outer, long Tin, long inner, int P, int s,
                                                         T* __restrict__ y)
{
    const long Tu = Tin * P + s, n = outer * Tu * inner;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long i = e % inner, r = e / inner, nn = r % Tu, o = r / Tu, d = nn - s;
        y[e] = (d >= 0 && d % P == 0) ? x[(o * Tin + d / P) * inner + i] : T(0);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void interp_bwd_kernel(const T* __restrict__ gy, long outer, long Tin, long inner, int P, int s,
                                                         T* __restrict__ gx)
{
    const long Tu = Tin * P + s, n = outer * Tin * inner;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        const long i = e % inner, r = e / inner, m = r % Tin, o = r / Tin;
        gx[e] = gy[(o * Tu + s + m * P) * inner + i];
    }
}

// ------------------------------------------------------------------------------------------------------------------ launches
bool pq_tuned(int K, int M, int P) { return K <= 8 && M <= 127 && P <= 16; }

void pq_pads(int M, bool analysis, int& dl, int& dr)
{
    if (M % 2 == 0) {
        dl = dr = M / 2;
    } else if (analysis) {
        dl = (M + 1) / 2;
        dr = (M - 1) / 2;
    } else {
        dl = (M - 1) / 2;
        dr = (M + 1) / 2;
    }
}

template <typename T>
int pqmf_launch_fwd(const void* x, const void* f, long B, long Tlen, long Tout, int K, int M, int P, int s, void* y, hipStream_t st)
{
    int dl, dr;
    pq_pads(M, true, dl, dr);
    const long ntile = (Tout + kPqTile - 1) / kPqTile;
    if (pq_tuned(K, M, P) && B * ntile <= (long)UINT_MAX) {
        const size_t lds = ((size_t)(((M + 1) * K + 3) & ~3) + (size_t)P * (kPqTile + M / P)) * sizeof(T);
#define DSA_PQ_FWD(KK)                                                                                                             \
    case KK:                                                                                                                       \
        hipLaunchKernelGGL((pqmf_fwd_tuned_kernel<T, KK>), dim3((unsigned)(B * ntile)), dim3(256), lds, st, (const T*)x, (const T*)f, \
                           Tlen, Tout, ntile, M, P, s, dl, (T*)y);                                                                 \
        break
        switch (K) {
            DSA_PQ_FWD(1);
            DSA_PQ_FWD(2);
            DSA_PQ_FWD(3);
            DSA_PQ_FWD(4);
            DSA_PQ_FWD(5);
            DSA_PQ_FWD(6);
            DSA_PQ_FWD(7);
            DSA_PQ_FWD(8);
        }
#undef DSA_PQ_FWD
        return check_launch("pqmf_fwd_tuned");
    }
    hipLaunchKernelGGL((pqmf_fwd_generic_kernel<T>), dim3(pq_blocks(B * K * Tout)), dim3(256), 0, st, (const T*)x, (const T*)f, B, Tlen, Tout,
                       K, M, P, s, dl, (T*)y);
    return check_launch("pqmf_fwd_generic");
}

template <typename T>
int pqmf_launch_bwd(const void* gy, const void* x, const void* f, long B, long Tlen, long Tout, int K, int M, int P, int s, void* gx, void* gf,
                    void* work, hipStream_t st)
{
    int dl, dr;
    pq_pads(M, true, dl, dr);
    const long ntile = (Tlen + kPqTile - 1) / kPqTile;
    if (gx && P == 1 && s == 0 && pq_tuned(K, M, 1) && B * ntile <= (long)UINT_MAX) {
        const size_t lds = ((size_t)(((M + 1) * K + 3) & ~3) + (size_t)K * (kPqTile + M + dr)) * sizeof(T);
#define DSA_PQ_BWD(KK)                                                                                                              \
    case KK:                                                                                                                        \
        hipLaunchKernelGGL((pqmf_bwd_x_tuned_kernel<T, KK>), dim3((unsigned)(B * ntile)), dim3(256), lds, st, (const T*)gy, (const T*)f, \
                           Tlen, ntile, M, dl, dr, (T*)gx);                                                                         \
        break
        switch (K) {
            DSA_PQ_BWD(1);
            DSA_PQ_BWD(2);
            DSA_PQ_BWD(3);
            DSA_PQ_BWD(4);
            DSA_PQ_BWD(5);
            DSA_PQ_BWD(6);
            DSA_PQ_BWD(7);
            DSA_PQ_BWD(8);
        }
#undef DSA_PQ_BWD
        const int rc = check_launch("pqmf_bwd_x_tuned");
        if (rc != DSA_OK) return rc;
    } else if (gx) {
        if (P == 1 && s == 0)
            hipLaunchKernelGGL((pqmf_bwd_x_kernel<T, true>), dim3(pq_blocks(B * Tlen)), dim3(256), 0, st, (const T*)gy, (const T*)f, B, Tlen, Tout,
                               K, M, P, s, dl, dr, (T*)gx);
        else
            hipLaunchKernelGGL((pqmf_bwd_x_kernel<T, false>), dim3(pq_blocks(B * Tlen)), dim3(256), 0, st, (const T*)gy, (const T*)f, B, Tlen,
                               Tout, K, M, P, s, dl, dr, (T*)gx);
        const int rc = check_launch("pqmf_bwd_x");
        if (rc != DSA_OK) return rc;
    }
    if (!gf) return DSA_OK;
    const int KM1 = K * (M + 1);
    hipLaunchKernelGGL((pqmf_bwd_f_kernel<T>), dim3((unsigned)B), dim3(256), (kPqChunk + M) * sizeof(T), st, (const T*)gy, (const T*)x, Tlen,
                       Tout, K, M, P, s, dl, (T*)work);
    const int rc = check_launch("pqmf_bwd_f");
    if (rc != DSA_OK) return rc;
    hipLaunchKernelGGL((pqmf_f_sum_kernel<T>), dim3((unsigned)((KM1 + 63) / 64)), dim3(256), 0, st, (const T*)work, B, KM1, (T*)gf);
    return check_launch("pqmf_f_sum");
}

template <typename T>
int ipqmf_launch_fwd(const void* y, const void* f, long B, long Tin, long Tu, int K, int M, int U, int s, void* x, hipStream_t st)
{
    int dl, dr;
    pq_pads(M, false, dl, dr);
    const long ntile = (Tu + kPqTile - 1) / kPqTile;
    if (pq_tuned(K, M, U) && B * ntile <= (long)UINT_MAX) {
        const size_t lds = ((size_t)(((M + 1) * K + 3) & ~3) + (size_t)K * ((kPqTile - 1 + M) / U + 2)) * sizeof(T);
#define DSA_IPQ_FWD(KK)                                                                                                             \
    case KK:                                                                                                                        \
        if (U == 1)                                                                                                                 \
            hipLaunchKernelGGL((ipqmf_fwd_tuned_kernel<T, KK, true>), dim3((unsigned)(B * ntile)), dim3(256), lds, st, (const T*)y,   \
                               (const T*)f, Tin, Tu, ntile, M, U, s, dl, (T*)x);                                                    \
        else                                                                                                                        \
            hipLaunchKernelGGL((ipqmf_fwd_tuned_kernel<T, KK, false>), dim3((unsigned)(B * ntile)), dim3(256), lds, st, (const T*)y,  \
                               (const T*)f, Tin, Tu, ntile, M, U, s, dl, (T*)x);                                                    \
        break
        switch (K) {
            DSA_IPQ_FWD(1);
            DSA_IPQ_FWD(2);
            DSA_IPQ_FWD(3);
            DSA_IPQ_FWD(4);
            DSA_IPQ_FWD(5);
            DSA_IPQ_FWD(6);
            DSA_IPQ_FWD(7);
            DSA_IPQ_FWD(8);
        }
#undef DSA_IPQ_FWD
        return check_launch("ipqmf_fwd_tuned");
    }
    hipLaunchKernelGGL((ipqmf_fwd_generic_kernel<T>), dim3(pq_blocks(B * Tu)), dim3(256), 0, st, (const T*)y, (const T*)f, B, Tin, Tu, K, M, U,
                       s, dl, (T*)x);
    return check_launch("ipqmf_fwd_generic");
}

template <typename T>
int ipqmf_launch_bwd(const void* gx, const void* y, const void* f, long B, long Tin, long Tu, int K, int M, int U, int s, void* gy, void* gf,
                     void* work, hipStream_t st)
{
    int dl, dr;
    pq_pads(M, false, dl, dr);
    const long ntile = (Tu + kPqTile - 1) / kPqTile;
    if (gy && U == 1 && s == 0 && pq_tuned(K, M, 1) && B * ntile <= (long)UINT_MAX) {
        const size_t lds = ((size_t)(((M + 1) * K + 3) & ~3) + (size_t)(kPqTile + M + dr)) * sizeof(T);
#define DSA_IPQ_BWD(KK)                                                                                                             \
    case KK:                                                                                                                        \
        hipLaunchKernelGGL((ipqmf_bwd_y_tuned_kernel<T, KK>), dim3((unsigned)(B * ntile)), dim3(256), lds, st, (const T*)gx,          \
                           (const T*)f, Tu, ntile, M, dl, dr, (T*)gy);                                                              \
        break
        switch (K) {
            DSA_IPQ_BWD(1);
            DSA_IPQ_BWD(2);
            DSA_IPQ_BWD(3);
            DSA_IPQ_BWD(4);
            DSA_IPQ_BWD(5);
            DSA_IPQ_BWD(6);
            DSA_IPQ_BWD(7);
            DSA_IPQ_BWD(8);
        }
#undef DSA_IPQ_BWD
        const int rc = check_launch("ipqmf_bwd_y_tuned");
        if (rc != DSA_OK) return rc;
    } else if (gy) {
        hipLaunchKernelGGL((ipqmf_bwd_y_kernel<T>), dim3(pq_blocks(B * K * Tin)), dim3(256), 0, st, (const T*)gx, (const T*)f, B, Tin, Tu, K, M,
                           U, s, dl, dr, (T*)gy);
        const int rc = check_launch("ipqmf_bwd_y");
        if (rc != DSA_OK) return rc;
    }
    if (!gf) return DSA_OK;
    const int KM1 = K * (M + 1);
    hipLaunchKernelGGL((ipqmf_bwd_f_kernel<T>), dim3((unsigned)B), dim3(256), 0, st, (const T*)gx, (const T*)y, Tin, Tu, K, M, U, s, dl,
                       (T*)work);
    const int rc = check_launch("ipqmf_bwd_f");
    if (rc != DSA_OK) return rc;
    hipLaunchKernelGGL((pqmf_f_sum_kernel<T>), dim3((unsigned)((KM1 + 63) / 64)), dim3(256), 0, st, (const T*)work, B, KM1, (T*)gf);
    return check_launch("pqmf_f_sum");
}

bool pq_sizes_ok(int64_t B, int64_t T, int32_t K, int32_t M, int32_t P, int32_t s)
{
    const int64_t lim = (int64_t)1 << 40;
    return B >= 0 && T >= 0 && K >= 1 && K <= DSA_PQMF_MAX_BANDS && M >= 2 && M <= DSA_PQMF_MAX_ORDER && P >= 1 && s >= 0 &&
           B <= (int64_t)UINT_MAX && T <= lim && (int64_t)P * T + s <= lim && B * K <= lim && B * K * ((int64_t)P * T + s + M) <= lim * 1024;
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_pqmf_fwd(const void* x, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t period, int32_t start,
                            int32_t dtype, void* y, void* stream)
{
    DSA_REQUIRE(pq_sizes_ok(B, T, K, M, period, start), "pqmf: invalid sizes");
    const int64_t Tout = T > start ? (T - start + period - 1) / period : 0;
    if (B * Tout == 0) return DSA_OK;
    DSA_REQUIRE(x && f && y, "pqmf: null pointer");
    return with_dtype(dtype, "pqmf", [&](auto tag) {
        return pqmf_launch_fwd<decltype(tag)>(x, f, B, T, Tout, K, M, period, start, y, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_pqmf_bwd(const void* gy, const void* x, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t period,
                            int32_t start, int32_t dtype, void* gx, void* gf, void* work, void* stream)
{
    DSA_REQUIRE(pq_sizes_ok(B, T, K, M, period, start), "pqmf_bwd: invalid sizes");
    if (B * T == 0) return DSA_OK;
    const int64_t Tout = T > start ? (T - start + period - 1) / period : 0;
    DSA_REQUIRE(f && (gy || Tout == 0), "pqmf_bwd: f and gy are required");
    DSA_REQUIRE(!gf || (x && work), "pqmf_bwd: gf needs the forward's x and the workspace");
    return with_dtype(dtype, "pqmf_bwd", [&](auto tag) {
        return pqmf_launch_bwd<decltype(tag)>(gy, x, f, B, T, Tout, K, M, period, start, gx, gf, work, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_ipqmf_fwd(const void* y, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t up, int32_t start,
                             int32_t dtype, void* x, void* stream)
{
    DSA_REQUIRE(pq_sizes_ok(B, T, K, M, up, start), "ipqmf: invalid sizes");
    const int64_t Tu = T * up + start;
    if (B * Tu == 0) return DSA_OK;
    return with_dtype(dtype, "ipqmf", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        DSA_REQUIRE(f && x && (y || T == 0), "ipqmf: null pointer");
        if (T == 0) {   // all of yu is padding: zero
            if (hipMemsetAsync(x, 0, (size_t)(B * Tu) * sizeof(V), (hipStream_t)stream) != hipSuccess)
                return fail(DSA_ERR_LAUNCH, "ipqmf: memset failed%s");
            return (int)DSA_OK;
        }
        return ipqmf_launch_fwd<V>(y, f, B, T, Tu, K, M, up, start, x, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_ipqmf_bwd(const void* gx, const void* y, const void* f, int64_t B, int64_t T, int32_t K, int32_t M, int32_t up,
                             int32_t start, int32_t dtype, void* gy, void* gf, void* work, void* stream)
{
    DSA_REQUIRE(pq_sizes_ok(B, T, K, M, up, start), "ipqmf_bwd: invalid sizes");
    const int64_t Tu = T * up + start;
    if (B * Tu == 0) return DSA_OK;
    return with_dtype(dtype, "ipqmf_bwd", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        DSA_REQUIRE(f && gx, "ipqmf_bwd: f and gx are required");
        DSA_REQUIRE(!gf || ((y || T == 0) && work), "ipqmf_bwd: gf needs the forward's y and the workspace");
        if (T == 0) {   // no input samples: gy is empty and the filter gradient zero
            if (gf && hipMemsetAsync(gf, 0, (size_t)K * (M + 1) * sizeof(V), (hipStream_t)stream) != hipSuccess)
                return fail(DSA_ERR_LAUNCH, "ipqmf_bwd: memset failed%s");
            return (int)DSA_OK;
        }
        return ipqmf_launch_bwd<V>(gx, y, f, B, T, Tu, K, M, up, start, gy, gf, work, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_interpolate_fwd(const void* x, int64_t outer, int64_t T, int64_t inner, int32_t period, int32_t start, int32_t dtype,
                                   void* y, void* stream)
{
    const int64_t lim = (int64_t)1 << 40;
    DSA_REQUIRE(outer >= 0 && T >= 0 && inner >= 0 && period >= 1 && start >= 0 && T <= lim && outer <= lim && inner <= lim,
                "interpolate: invalid sizes");
    const int64_t Tu = T * period + start;
    if (outer * Tu * inner == 0) return DSA_OK;
    DSA_REQUIRE(y && (x || T == 0), "interpolate: null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nb = pq_blocks(outer * Tu * inner);
    return with_dtype(dtype, "interpolate", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        hipLaunchKernelGGL((interp_fwd_kernel<V>), dim3(nb), dim3(256), 0, st, (const V*)x, outer, T, inner, period, start, (V*)y);
        return check_launch("interpolate_fwd");
    });
}

DSA_EXPORT int dsa_interpolate_bwd(const void* gy, int64_t outer, int64_t T, int64_t inner, int32_t period, int32_t start, int32_t dtype,
                                   void* gx, void* stream)
{
    const int64_t lim = (int64_t)1 << 40;
    DSA_REQUIRE(outer >= 0 && T >= 0 && inner >= 0 && period >= 1 && start >= 0 && T <= lim && outer <= lim && inner <= lim,
                "interpolate_bwd: invalid sizes");
    if (outer * T * inner == 0) return DSA_OK;
    DSA_REQUIRE(gy && gx, "interpolate_bwd: null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nb = pq_blocks(outer * T * inner);
    return with_dtype(dtype, "interpolate_bwd", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        hipLaunchKernelGGL((interp_bwd_kernel<V>), dim3(nb), dim3(256), 0, st, (const V*)gy, outer, T, inner, period, start, (V*)gx);
        return check_launch("interpolate_bwd");
    });
}
