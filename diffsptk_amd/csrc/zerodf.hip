// Time-variant all-zero filter (AllZeroDigitalFilter, zerodf.py) and its Taylor-stage form for the MLSA filter: the sibling of
// poledf.hip.
#include "common.h"

namespace dsa {

// ------------------------------------------------------------------------------------------------------------------
// Time-variant all-zero filter: AllZeroDigitalFilter._forward_efficient, zerodf.py:207-243 -- the
// FIR core of the multi-stage / single-stage MLSA filter (mglsadf.py:254-527).
//   y[t] = sum_{k=0}^{M} h_t[k] x[t - k + z0],   h_t = (1 - w) b[n] + w b[min(n + 1, N - 1)],  n = t / P, w = (t % P) / P
// (x is zero outside [0, T); z0 = zeroth_index: taps k < z0 look ahead).  ignore_gain divides by the interpolated b[.][0]
// (z0 < M) or b[.][M] (z0 = M).  One workgroup per frame: both coefficient rows and the frame's stretch of x in LDS.
template <typename T>
__global__ __launch_bounds__(256) void zerodf_fwd_kernel(const T* __restrict__ x, const T* __restrict__ b, long Tlen, long N,
                                                         int M, int P, int z0, int ignore_gain, T* __restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* b0 = reinterpret_cast<T*>(smem_raw);   // [M + 1]
    T* b1 = b0 + (M + 1);                     // [M + 1]
    T* xs = b1 + (M + 1);                     // [P + M]: x[t0 - M + z0 .. t0 + P - 1 + z0]
    const long f = blockIdx.x;                // flattened (utterance, frame)
    const long u = f / N, n = f - u * N;
    const long n1 = n + 1 < N ? n + 1 : N - 1;
    const T* br0 = b + (u * N + n) * (M + 1);
    const T* br1 = b + (u * N + n1) * (M + 1);
    for (int k = threadIdx.x; k <= M; k += blockDim.x) {
        b0[k] = br0[k];
        b1[k] = br1[k];
    }
    const long t0 = n * P;
    const T* xu = x + u * Tlen;
    for (int i = threadIdx.x; i < P + M; i += blockDim.x) {
        const long s = t0 - M + z0 + i;
        xs[i] = (s >= 0 && s < Tlen) ? xu[s] : T(0);
    }
    __syncthreads();
    const int gk = z0 == M ? M : 0;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const T w = (T)i / (T)P;
        T a0 = 0, a1 = 0;
        // x[t - k + z0] = xs[i + M - k]
        for (int k = 0; k <= M; ++k) {
            const T xv = xs[i + M - k];
            a0 += b0[k] * xv;
            a1 += b1[k] * xv;
        }
        T v = a0 + w * (a1 - a0);             // torch.lerp(y1, y2, ramp)
        if (ignore_gain) v /= b0[gk] + w * (b1[gk] - b0[gk]);
        y[u * Tlen + t0 + i] = v;
    }
}

// gx[s] = sum_k gyn[t] h_t[k], t = s - z0 + k (gather: deterministic); gyn = gy / gain when ignore_gain
template <typename T>
__global__ __launch_bounds__(256) void zerodf_bwd_x_kernel(const T* __restrict__ gy, const T* __restrict__ b, long B, long Tlen,
                                                           long N, int M, int P, int z0, int ignore_gain, T* __restrict__ gx)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long u = idx / Tlen, s = idx - u * Tlen;
    if (u >= B) return;
    const int gk = z0 == M ? M : 0;
    T acc = 0;
    for (int k = 0; k <= M; ++k) {
        const long t = s - z0 + k;
        if (t < 0 || t >= Tlen) continue;
        const long n = t / P;
        const long n1 = n + 1 < N ? n + 1 : N - 1;
        const T w = (T)(t - n * P) / (T)P;
        const T* r0 = b + (u * N + n) * (M + 1);
        const T* r1 = b + (u * N + n1) * (M + 1);
        T g = gy[u * Tlen + t];
        if (ignore_gain) g /= r0[gk] + w * (r1[gk] - r0[gk]);
        acc += g * (r0[k] + w * (r1[k] - r0[k]));
    }
    gx[idx] = acc;
}

// gb[n][k] = sum over the samples of frame n (weight 1 - w) and of frame n - 1 (weight w; the last frame also takes its
// own w part) of gyn[t] x[t - k + z0]; with ignore_gain the gain tap additionally receives -gy y / gain.
template <typename T>
__global__ __launch_bounds__(256) void zerodf_bwd_b_kernel(const T* __restrict__ gy, const T* __restrict__ x, const T* __restrict__ b,
                                                           const T* __restrict__ y, long Tlen, long N, int M, int P, int z0,
                                                           int ignore_gain, T* __restrict__ gb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* gs = reinterpret_cast<T*>(smem_raw);   // [2P]: normalised cotangent times the frame weight, frames n - 1 and n
    T* xs = gs + 2 * P;                       // [2P + M]
    T* red = xs + 2 * P + M;                  // [blockDim.x] reduction scratch for the gain tap
    const long f = blockIdx.x;
    const long u = f / N, n = f - u * N;
    const int gk = z0 == M ? M : 0;
    const long tbase = (n - 1) * P;           // first sample of frame n - 1
    T gain_part = 0;
    for (int i = threadIdx.x; i < 2 * P; i += blockDim.x) {
        const long t = tbase + i;
        T v = 0;
        if (t >= 0 && t < Tlen) {
            const long nt = t / P;            // n - 1 or n
            const long nt1 = nt + 1 < N ? nt + 1 : N - 1;
            const T w = (T)(t - nt * P) / (T)P;
            T wt = 0;                         // weight with which b[n] enters h_t
            if (nt == n) wt += T(1) - w;
            if (nt1 == n) wt += w;
            T g = gy[u * Tlen + t];
            if (ignore_gain) {
                const T* r0 = b + (u * N + nt) * (M + 1);
                const T* r1 = b + (u * N + nt1) * (M + 1);
                const T gain = r0[gk] + w * (r1[gk] - r0[gk]);
                g /= gain;
                gain_part -= wt * g * y[u * Tlen + t];   // d/d gain of (u / gain) = -y / gain, gain = sum wt b[.][gk]
            }
            v = wt * g;
        }
        gs[i] = v;
    }
    const T* xu = x + u * Tlen;
    for (int i = threadIdx.x; i < 2 * P + M; i += blockDim.x) {
        const long s = tbase - M + z0 + i;
        xs[i] = (s >= 0 && s < Tlen) ? xu[s] : T(0);
    }
    red[threadIdx.x] = gain_part;
    __syncthreads();
    for (int k = threadIdx.x; k <= M; k += blockDim.x) {
        T acc = 0;
        for (int i = 0; i < 2 * P; ++i) acc += gs[i] * xs[i + M - k];
        if (ignore_gain && k == gk)
            for (int q = 0; q < (int)blockDim.x; ++q) acc += red[q];
        gb[(u * N + n) * (M + 1) + k] = acc;
    }
}

// Long filters (M >= 64: the 200-tap cepstra of the multi-stage MLSA filter, the 2000-tap impulse responses of the
// single-stage one) with P <= 128: the taps are dealt to 8 slices of 32 threads, a thread keeps up to four output samples
// (i = l, l + 32, ..) in registers -- two coefficient reads feed eight multiply-adds instead of two, and all 256 threads work
// where the kernel above keeps P of them busy -- and the slices' partial sums meet in LDS (fixed order: deterministic).
template <typename T>
__global__ __launch_bounds__(256) void zerodf_fwd_sliced_kernel(const T* __restrict__ x, const T* __restrict__ b, long Tlen, long N,
                                                                int M, int P, int z0, int ignore_gain, T* __restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* b0 = reinterpret_cast<T*>(smem_raw);   // [M + 1]
    T* b1 = b0 + (M + 1);                     // [M + 1]
    T* xs = b1 + (M + 1);                     // [128 + M]: x[t0 - M + z0 ..], zero beyond the frame's stretch
    T* part = xs + (128 + M);                 // [8][2][128]
    const long f = blockIdx.x;
    const long u = f / N, n = f - u * N;
    const long n1 = n + 1 < N ? n + 1 : N - 1;
    const T* br0 = b + (u * N + n) * (M + 1);
    const T* br1 = b + (u * N + n1) * (M + 1);
    for (int k = threadIdx.x; k <= M; k += blockDim.x) {
        b0[k] = br0[k];
        b1[k] = br1[k];
    }
    const long t0 = n * P;
    const T* xu = x + u * Tlen;
    for (int i = threadIdx.x; i < 128 + M; i += blockDim.x) {
        const long s = t0 - M + z0 + i;
        xs[i] = (i < P + M && s >= 0 && s < Tlen) ? xu[s] : T(0);
    }
    __syncthreads();
    const int g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int per = (M + 8) / 8;              // ceil((M + 1) / 8)
    const int k0 = g * per, k1 = (k0 + per < M + 1) ? k0 + per : M + 1;
    T a0[4] = {T(0), T(0), T(0), T(0)}, a1[4] = {T(0), T(0), T(0), T(0)};
    for (int k = k0; k < k1; ++k) {
        const T c0 = b0[k], c1 = b1[k];
        const T* xp = xs + (M - k) + l;       // x[t - k + z0] = xs[i + M - k]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const T xv = xp[32 * j];
            a0[j] += c0 * xv;
            a1[j] += c1 * xv;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        part[(g * 2 + 0) * 128 + l + 32 * j] = a0[j];
        part[(g * 2 + 1) * 128 + l + 32 * j] = a1[j];
    }
    __syncthreads();
    const int gk = z0 == M ? M : 0;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        T s0 = 0, s1 = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            s0 += part[(q * 2 + 0) * 128 + i];
            s1 += part[(q * 2 + 1) * 128 + i];
        }
        const T w = (T)i / (T)P;
        T v = s0 + w * (s1 - s0);             // torch.lerp(y1, y2, ramp)
        if (ignore_gain) v /= b0[gk] + w * (b1[gk] - b0[gk]);
        y[u * Tlen + t0 + i] = v;
    }
}

// The same filters with the taps AND the samples blocked by four: a thread owns four consecutive output samples and a
// contiguous range of 4-tap blocks; with the taps stored reversed (br[kk] = b[M - kk]) a block needs the eight samples
// xs[4 (l + m) .. + 7] -- two aligned 16-byte reads, one of them carried over from the previous block -- and two
// 16-byte coefficient reads (broadcasts): 3 LDS reads per 32 multiply-adds (the kernel above: 6 per 8, which bound it).
// The tap ranges of the 256 / ceil(P / 4) thread groups meet in LDS in a fixed order (deterministic).
template <typename T>
__global__ __launch_bounds__(256) void zerodf_fwd_blocked_kernel(const T* __restrict__ x, const T* __restrict__ b, long Tlen, long N,
                                                                 int M, int P, int z0, int ignore_gain, T* __restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int NB = (M + 4) / 4;               // 4-tap blocks: ceil((M + 1) / 4)
    const int nt = (P + 3) / 4;               // threads per group (four samples each)
    const int G = 256 / nt;                   // tap-range groups
    const int PP = nt * 4;
    T* br0 = reinterpret_cast<T*>(smem_raw);  // [4 NB] reversed taps of frame n, zero-padded
    T* br1 = br0 + 4 * NB;                    // [4 NB] ... of frame n + 1
    T* xs = br1 + 4 * NB;                     // [PP + 4 NB + 4]: x[t0 - M + z0 ..], zero beyond the frame's stretch
    T* part = xs + (PP + 4 * NB + 4);         // [G][2][PP]
    const long f = blockIdx.x;
    const long u = f / N, n = f - u * N;
    const long n1 = n + 1 < N ? n + 1 : N - 1;
    const T* r0 = b + (u * N + n) * (M + 1);
    const T* r1 = b + (u * N + n1) * (M + 1);
    // (four independent loads per round: a load -> store loop waits out one round trip to memory per element)
    const long t0 = n * P;
    const T* xu = x + u * Tlen;
    for (int kb = threadIdx.x; kb < 4 * NB; kb += 4 * blockDim.x) {
        T v0[4], v1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kk = kb + q * blockDim.x;
            const bool ok = kk <= M;
            v0[q] = ok ? r0[M - (ok ? kk : M)] : T(0);
            v1[q] = ok ? r1[M - (ok ? kk : M)] : T(0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kk = kb + q * blockDim.x;
            if (kk < 4 * NB) {
                br0[kk] = v0[q];
                br1[kk] = v1[q];
            }
        }
    }
    for (int ib = threadIdx.x; ib < PP + 4 * NB + 4; ib += 4 * blockDim.x) {
        T v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = ib + q * blockDim.x;
            const long sidx = t0 - M + z0 + i;
            const bool ok = i < P + M && sidx >= 0 && sidx < Tlen;
            v[q] = ok ? xu[ok ? sidx : 0] : T(0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = ib + q * blockDim.x;
            if (i < PP + 4 * NB + 4) xs[i] = v[q];
        }
    }
    __syncthreads();
    const int g = threadIdx.x / nt, l = threadIdx.x - g * nt;
    if (g < G) {
        const int per = (NB + G - 1) / G;
        const int m0 = g * per, m1 = (m0 + per < NB) ? m0 + per : NB;
        T a0[4] = {T(0), T(0), T(0), T(0)}, a1[4] = {T(0), T(0), T(0), T(0)};
        T wv[8];
        if (m0 < m1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) wv[q] = xs[4 * (l + m0) + q];
        }
        for (int m = m0; m < m1; ++m) {
            T c0[4], c1[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                wv[4 + q] = xs[4 * (l + m + 1) + q];
                c0[q] = br0[4 * m + q];
                c1[q] = br1[4 * m + q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    a0[q] += c0[r] * wv[q + r];
                    a1[q] += c1[r] * wv[q + r];
                }
#pragma unroll
            for (int q = 0; q < 4; ++q) wv[q] = wv[4 + q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            part[(g * 2 + 0) * PP + 4 * l + q] = a0[q];
            part[(g * 2 + 1) * PP + 4 * l + q] = a1[q];
        }
    }
    __syncthreads();
    const int gk = z0 == M ? M : 0;
    const T g0 = r0[gk], g1 = r1[gk];
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        T s0 = 0, s1 = 0;
        for (int q = 0; q < G; ++q) {
            s0 += part[(q * 2 + 0) * PP + i];
            s1 += part[(q * 2 + 1) * PP + i];
        }
        const T w = (T)i / (T)P;
        T v = s0 + w * (s1 - s0);             // torch.lerp(y1, y2, ramp)
        if (ignore_gain) v /= g0 + w * (g1 - g0);
        y[u * Tlen + t0 + i] = v;
    }
}

// Round 3: several frames per workgroup, every tap of a sample block in ONE thread, float32 on packed multiply-adds.
// The blocked kernel above spends most of a launch around its inner loop (one frame per workgroup: two barriers, the
// partial sums of twelve tap ranges through LDS, ~5 blocks of taps per thread).  Here a workgroup takes `nf` consecutive
// frames of one utterance: a thread owns four consecutive output samples of one frame and (G = 1) all of its taps, so the
// sums stay in registers; the rows of frame n and n + 1 are stored INTERLEAVED in LDS -- (b_n[k], b_n+1[k]) as one 8-byte
// pair -- so that the two filters of the interpolation are the two halves of one v_pk_fma_f32 whose other factor is the
// sample, broadcast by op_sel: 16 packed instructions per 4 taps x 4 samples x 2 rows instead of 32 v_fma_f32 (the packed
// form is the only one that issues two float32 multiply-adds per lane in 4 cycles: DESIGN 3.2).  Long filters (the
// 2000-tap impulse responses of the single-stage form) split the taps over G groups of threads that meet in LDS in a fixed
// order.  Optional epilogue for the Taylor stages of the multi-stage form: y = scale * filter(x), ysum = acc + y.
// NaN containment: taps beyond M (padding of the last block of four) are skipped, not multiplied by zero.
typedef float zd_v2f __attribute__((ext_vector_type(2)));
typedef float zd_v4f __attribute__((ext_vector_type(4)));
typedef float zd_v4f_u __attribute__((ext_vector_type(4), aligned(4)));
typedef double zd_v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void zd_fma_lo(zd_v2f& acc, zd_v2f c, zd_v2f w)   // acc += c * w.x (both halves)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(c), "v"(w));
}
__device__ __forceinline__ void zd_fma_hi(zd_v2f& acc, zd_v2f c, zd_v2f w)   // acc += c * w.y (both halves)
{
    // the odd sample as the LOW half of its own pair (a move the compiler shares between the uses of a ring slot), then the
    // low-half broadcast of zd_fma_lo: the one-instruction form "op_sel:[0,1,0] op_sel_hi:[1,1,1]" has a set op_sel bit -- its
    // low result reads a high source half -- and no shipped kernel executes that class (pk_math.h, DSA_PK_CROSSED)
    const zd_v2f wh = __builtin_shufflevector(w, w, 1, 1);
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(c), "v"(wh));
}
// two adjacent pairs from a 16-byte aligned LDS address (float: one ds_read_b128); `both` false: only the first is wanted
__device__ __forceinline__ void zd_load2(const zd_v2f* p, zd_v2f& a, zd_v2f& b, bool both)
{
    if (both) {
        const zd_v4f v = *reinterpret_cast<const zd_v4f*>(p);
        a = zd_v2f{v.x, v.y};
        b = zd_v2f{v.z, v.w};
    } else {
        a = p[0];
    }
}
__device__ __forceinline__ void zd_load2(const zd_v2d* p, zd_v2d& a, zd_v2d& b, bool both)
{
    a = p[0];
    if (both) b = p[1];
}
__device__ __forceinline__ void zd_fma2(zd_v2f& acc, zd_v2f c, zd_v2f w)     // acc += c * w, half by half
{
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(c), "v"(w));
}
__device__ __forceinline__ void zd_fma2(zd_v2d& acc, zd_v2d c, zd_v2d w) { acc += c * w; }
__device__ __forceinline__ void zd_fma_lo(zd_v2d& acc, zd_v2d c, zd_v2d w) { acc += c * w.x; }
__device__ __forceinline__ void zd_fma_hi(zd_v2d& acc, zd_v2d c, zd_v2d w) { acc += c * w.y; }

template <typename T, int S>
__global__ __launch_bounds__(256) DSA_PK_TARGET void zerodf_fwd_rows_kernel(const T* __restrict__ x, const T* __restrict__ b, long Tlen, long N,
                                                              int M, int P, int z0, int ignore_gain, int nf, int G, int ldb, T scale,
                                                              const T* acc, T* __restrict__ y, T* ysum)
{
    // (`b` may point at a run of M + 1 taps inside rows of ldb coefficients, with a zeroth index outside [0, M]: a filter too long
    // for LDS is the sum of its tap pieces, zerodf_launch_fwd)
    using V2 = T __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int NB = (M + 4) / 4;                 // 4-tap blocks
    const int nt = P / S;                       // threads per (frame, tap group): S consecutive samples each
    V2* brp = reinterpret_cast<V2*>(smem_raw);  // [nf][4 NB]: (b[n][M - kk], b[n + 1][M - kk]), zero beyond kk = M
    T* xs = reinterpret_cast<T*>(brp + (size_t)nf * 4 * NB);   // [nf P + 4 NB + 8]: x[t0 - M + z0 ..]
    V2* part = reinterpret_cast<V2*>(xs + ((size_t)nf * P + 4 * NB + 8));   // [nf][G][P] when G > 1
    const long chunks = (N + nf - 1) / nf;
    const long u = blockIdx.x / chunks, n0 = (blockIdx.x - u * chunks) * nf;
    const int frames = (int)((N - n0 < nf) ? N - n0 : nf);
    const T* bu = b + u * N * ldb;
    // (all loads of a batch first, then the stores: a load -> store loop waits out one trip to memory per element)
    for (int kk = threadIdx.x; kk < 4 * NB; kk += blockDim.x) {   // a thread walks down one tap: every row is read once
        const bool tap = kk <= M;
        const T* col = bu + (M - (tap ? kk : M));
        T cv[17];
#pragma unroll
        for (int p = 0; p <= 16; ++p) {
            const long row = n0 + p < N ? n0 + p : N - 1;
            cv[p] = (tap && p <= frames) ? col[row * ldb] : T(0);
        }
#pragma unroll
        for (int p = 0; p < 16; ++p)
            if (p < frames) brp[(size_t)p * 4 * NB + kk] = V2{cv[p], cv[p + 1]};
    }
    const long t0 = n0 * P;
    const T* xu = x + u * Tlen;
    const int xlen = frames * P + 4 * NB + 8;
    for (int i0 = threadIdx.x; i0 < xlen; i0 += 8 * blockDim.x) {
        T xv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const long sidx = t0 - M + z0 + i0 + q * (int)blockDim.x;
            xv[q] = (i0 + q * (int)blockDim.x < xlen && sidx >= 0 && sidx < Tlen) ? xu[sidx] : T(0);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (i0 + q * (int)blockDim.x < xlen) xs[i0 + q * (int)blockDim.x] = xv[q];
    }
    __syncthreads();
    const int grp = threadIdx.x / nt, l = threadIdx.x - grp * nt;   // grp = fr * G + g
    const int fr = grp / G, g = grp - fr * G;
    const bool active = fr < frames;
    V2 a[S];
#pragma unroll
    for (int q = 0; q < S; ++q) a[q] = V2{0, 0};
    if (active) {
        // (host: G divides the number of full blocks, so the loop count is the same for every thread of the launch)
        const int rem = (M + 1) & 3;                       // taps in the last block when it is a partial one
        const int per = (rem ? NB - 1 : NB) / G;
        const int m0 = g * per, m_full = m0 + per;
        const int m1 = (rem != 0 && g == G - 1) ? m_full + 1 : m_full;
        const V2* cp = brp + (size_t)fr * 4 * NB;
        const T* xf = xs + fr * P + S * l;
        // A block of four taps on S samples reads the S + 4 samples xf[4 m .. 4 m + S + 3]: NP = (S + 4) / 2 pairs kept in a
        // ring of NP registers pairs that advances by two pairs per block -- after NP / 2 blocks (a trip, unrolled) every pair
        // is back in its slot, so nothing is copied; per block two 16-byte tap reads (broadcasts) and one 16-byte sample read
        // feed 4 S packed multiply-adds (S = 8: the LDS pipe, which the S = 4 form loads as much as the vector unit, idles).
        constexpr int NP = (S + 4) / 2, TRIP = NP / 2;
        V2 R[NP];
#pragma unroll
        for (int i = 0; i < NP - 2; ++i) R[i] = *reinterpret_cast<const V2*>(xf + 4 * m0 + 2 * i);
        auto block = [&](int m, int b) __attribute__((always_inline)) {   // b = (m - m0) % TRIP: the ring's phase
            V2 c[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = cp[4 * m + r];
            zd_load2(reinterpret_cast<const V2*>(xf + 4 * m + 2 * (NP - 2)), R[(2 * b + NP - 2) % NP], R[(2 * b + NP - 1) % NP], true);
#pragma unroll
            for (int q = 0; q < S; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if ((q + r) & 1) zd_fma_hi(a[q], c[r], R[(2 * b + ((q + r) >> 1)) % NP]);
                    else zd_fma_lo(a[q], c[r], R[(2 * b + ((q + r) >> 1)) % NP]);
                }
        };
        int j = 0;
        for (; j + TRIP <= per; j += TRIP) {   // (uniform trip count: a scalar loop)
#pragma unroll
            for (int b = 0; b < TRIP; ++b) block(m0 + j + b, b);
        }
        int tail_b = 0;   // blocks left after the last whole trip (the ring's phase restarts at 0 there)
#pragma unroll
        for (int b = 0; b < TRIP - 1; ++b)
            if (j + b < per) {
                block(m0 + j + b, b);
                tail_b = b + 1;
            }
        if (m_full < m1) {   // the partial last block: only its real taps
            const int m = m_full;
            // bring the ring back to phase 0 (at most once per thread)
            V2 Wn[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) Wn[i] = tail_b == 0 ? R[i] : (tail_b == 1 ? R[(i + 2) % NP] : R[(i + 4) % NP]);
            Wn[NP - 2] = *reinterpret_cast<const V2*>(xf + 4 * m + 2 * (NP - 2));
#pragma unroll
            for (int r = 0; r < 3; ++r)
                if (r < rem) {
                    const V2 cr = cp[4 * m + r];
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        if ((q + r) & 1) zd_fma_hi(a[q], cr, Wn[(q + r) >> 1]);
                        else zd_fma_lo(a[q], cr, Wn[(q + r) >> 1]);
                    }
                }
        }
    }
    if (G > 1) {
        if (active) {
#pragma unroll
            for (int q = 0; q < S; ++q) part[((size_t)fr * G + g) * P + S * l + q] = a[q];
        }
        __syncthreads();
        if (active && g == 0) {
#pragma unroll
            for (int q = 0; q < S; ++q) {
                V2 sacc = part[((size_t)fr * G) * P + S * l + q];
                for (int gg = 1; gg < G; ++gg) sacc += part[((size_t)fr * G + gg) * P + S * l + q];
                a[q] = sacc;
            }
        }
    }
    if (active && g == 0) {
        const int gk = z0 == M ? M : 0;
        const V2 gain = brp[(size_t)fr * 4 * NB + (M - gk)];
        const long o = u * Tlen + t0 + (long)fr * P + S * l;
        T v[S];
#pragma unroll
        for (int q = 0; q < S; ++q) {
            const T wt = (T)(S * l + q) / (T)P;
            T r = a[q].x + wt * (a[q].y - a[q].x);          // torch.lerp(y1, y2, ramp)
            if (ignore_gain) r /= gain.x + wt * (gain.y - gain.x);
            v[q] = r * scale;
        }
        if (y) {
#pragma unroll
            for (int q = 0; q < S; ++q) y[o + q] = v[q];
        }
        if (ysum) {
#pragma unroll
            for (int q = 0; q < S; ++q) ysum[o + q] = acc[o + q] + v[q];
        }
    }
}

// nf frames x G tap groups of P / S threads per 256-thread workgroup within 64 KB of LDS; false: shape not covered
static bool zerodf_rows_plan(int M, int P, size_t elt, int& S, int& nf, int& G, size_t& lds)
{
    if (P % 4 != 0 || P / 4 > 256 || M < 16) return false;
    S = 4;   // (S = 8 -- half the LDS reads per multiply-add, 160 of 256 threads busy at P = 80 -- measured the same: 1.50 vs 1.46 ms)
    const int NB = (M + 4) / 4, nt = P / S, groups = 256 / nt;
    const int nb_full = ((M + 1) & 3) ? NB - 1 : NB;
    for (nf = groups < 16 ? groups : 16; nf >= 1; --nf) {
        G = groups / nf;
        while (G > 1 && nb_full % G != 0) --G;   // equal tap ranges: one loop count for the whole launch
        lds = (size_t)nf * 4 * NB * 2 * elt + ((size_t)nf * P + 4 * NB + 8) * elt + (G > 1 ? (size_t)nf * G * P * 2 * elt : 0);
        lds = (lds + 15) & ~(size_t)15;
        if (lds <= 64 * 1024) return true;
    }
    return false;
}

template <typename T>
static int zerodf_launch_fwd(const void* x, const void* b, int64_t B, int64_t Tlen, int64_t N, int M, int P, int z0, int ig,
                             void* y, hipStream_t st, double scale = 1.0, const void* acc = nullptr, void* ysum = nullptr)
{
    {
        int S, nf, G;
        size_t lds_r;
        if (zerodf_rows_plan(M, P, sizeof(T), S, nf, G, lds_r)) {
            const long chunks = (N + nf - 1) / nf;
            // (the kernel is written for S = 4 or 8 samples per thread; 8 measured the same at P = 80 and is not instantiated)
            hipLaunchKernelGGL((zerodf_fwd_rows_kernel<T, 4>), dim3((unsigned)(B * chunks)), dim3(256), lds_r, st, (const T*)x,
                               (const T*)b, (long)Tlen, (long)N, M, P, z0, ig, nf, G, M + 1, (T)scale, (const T*)acc, (T*)y, (T*)ysum);
            return check_launch("zerodf_rows_fwd");
        }
        if (ysum || scale != 1.0) return fail(DSA_ERR_UNSUPPORTED, "zerodf: the scaled / accumulating form needs P % 4 == 0 and M >= 16%s");
    }
    {   // long filters: taps and samples blocked by four (the sliced kernel below takes what does not fit)
        const int NB = (M + 4) / 4, nt = (P + 3) / 4;
        const size_t lds_b = sizeof(T) * ((size_t)8 * NB + (size_t)(4 * nt + 4 * NB + 4) + (size_t)(256 / (nt > 0 ? nt : 1)) * 2 * 4 * nt);
        if (M >= 64 && P >= 4 && P <= 128 && lds_b <= 64 * 1024) {
            hipLaunchKernelGGL((zerodf_fwd_blocked_kernel<T>), dim3((unsigned)(B * N)), dim3(256), lds_b, st, (const T*)x, (const T*)b,
                               (long)Tlen, (long)N, M, P, z0, ig, (T*)y);
            return check_launch("zerodf_blocked_fwd");
        }
    }
    const size_t lds_s = sizeof(T) * (2 * (size_t)(M + 1) + 128 + M + 8 * 2 * 128);
    if (M >= 64 && P <= 128 && lds_s <= 64 * 1024) {
        hipLaunchKernelGGL((zerodf_fwd_sliced_kernel<T>), dim3((unsigned)(B * N)), dim3(256), lds_s, st, (const T*)x, (const T*)b,
                           (long)Tlen, (long)N, M, P, z0, ig, (T*)y);
        return check_launch("zerodf_sliced_fwd");
    }
    const size_t lds = sizeof(T) * (2 * (size_t)(M + 1) + P + M);
    if (lds > 64 * 1024) {
        // A filter whose rows fit none of the kernels above (float64 from about 2700 taps at P = 80: the 3999 taps of the zero- and
        // mixed-phase single-stage MLSA filter at its defaults) as a sum of tap pieces, as the backward does: piece c = taps
        // [c KC, c KC + Mc] with z0 - c KC as its (possibly negative) zeroth index, each on the rows kernel; the first piece writes
        // y, the others add theirs to it (acc = ysum = y), in stream order.  The fewest pieces that all fit; everything is decided
        // before anything is launched.  ignore_gain divides by a tap of the whole filter: not by pieces.
        for (int np = 2; np <= 64 && !ig; ++np) {
            const int KC = (((M + 1 + np - 1) / np) + 3) & ~3;
            const int Ml = M - (np - 1) * KC;                  // order of the last piece
            int S, nf[2], G[2];
            size_t lds_p[2];
            if (Ml < 16 || !zerodf_rows_plan(KC - 1, P, sizeof(T), S, nf[0], G[0], lds_p[0]) ||
                !zerodf_rows_plan(Ml, P, sizeof(T), S, nf[1], G[1], lds_p[1]))
                continue;
            for (int c = 0; c < np; ++c) {
                const int w = c == np - 1;
                const long chunks = (N + nf[w] - 1) / nf[w];
                hipLaunchKernelGGL((zerodf_fwd_rows_kernel<T, 4>), dim3((unsigned)(B * chunks)), dim3(256), lds_p[w], st, (const T*)x,
                                   (const T*)b + c * KC, (long)Tlen, (long)N, w ? Ml : KC - 1, P, z0 - c * KC, 0, nf[w], G[w], M + 1, T(1),
                                   (const T*)(c ? y : nullptr), (T*)(c ? nullptr : y), (T*)(c ? y : nullptr));
            }
            return check_launch("zerodf_rows_fwd");
        }
        return fail(DSA_ERR_UNSUPPORTED, "zerodf: filter too long for LDS%s");
    }
    hipLaunchKernelGGL((zerodf_fwd_kernel<T>), dim3((unsigned)(B * N)), dim3(P >= 192 ? 256 : (P >= 96 ? 128 : 64)), lds, st,
                       (const T*)x, (const T*)b, (long)Tlen, (long)N, M, P, z0, ig, (T*)y);
    return check_launch("zerodf_fwd");
}

// Round 3: the backward of the time-variant FIR on the forward's pattern (rows of frames n and n + 1 interleaved as pairs,
// several frames per workgroup, four consecutive samples / taps per thread).  Without ignore_gain:
//   gx[s] = sum_k gy[t] h_t[k],  t = s - z0 + k  =  sum_t (b[n(t)][k], b[n(t) + 1][k]) . ((1 - w_t) gy[t], w_t gy[t])
// -- the dot product of two pairs, i.e. ONE packed multiply-add into a pair accumulator whose halves are added at the end.
// A thread owns four consecutive s and walks t in blocks of four that never straddle a frame (P % 4 == 0; z0 is rounded up
// to a multiple of 4 by shifting the taps): block m needs the tap pairs 4 m - 3 .. 4 m + 3 of ITS frame's row (stored from
// position 3, so the window starts 16-byte aligned) and the four weighted cotangent pairs.  Lanes cross frame boundaries at
// different m, so the window is re-read every block (the kernel is bound by LDS reads, ~1.4 x the multiply-adds).
// The old kernel: a thread per sample over all taps with two row reads from memory per tap.
template <typename T, int S>
__global__ __launch_bounds__(256) DSA_PK_TARGET void zerodf_bwd_x_rows_kernel(const T* __restrict__ gy, const T* __restrict__ b, long Tlen, long N,
                                                                int M, int P, int z0, int nf, int nrows, int ldb, int accumulate,
                                                                T scale, const T* add, T* gx)
{
    // gx = (accumulate ? gx : (add ? add : 0)) + scale * (the sum): `add` / `scale` serve the Taylor stages of the multi-stage
    // MLSA filter's backward (G_{i-1} = gy + F^T G_i / i)
    // (`b` may point at a run of M + 1 taps inside rows of ldb coefficients -- long filters are handled as a sum of
    // 200-tap pieces: piece c has z0 - c KC as its (possibly negative) zeroth index and accumulates into gx)
    using V2 = T __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int dz = (4 - (((z0 % 4) + 4) & 3)) & 3, Mp = M + dz, z0p = z0 + dz;
    const int NBt = (Mp + S - 1) / 4 + 1;              // blocks of four t per block of S output samples
    const int RW = (Mp + S + 6 + 3) & ~3;              // pairs per row: tap k' at position k' + S - 1, zeros around
    const int nt = P / S;
    V2* rows = reinterpret_cast<V2*>(smem_raw);        // [nrows][RW]
    V2* up = rows + (size_t)nrows * RW;                // [nf P + 4 NBt]: ((1 - w) gy, w gy) of t = Tstart + j
    const long chunks = (N + nf - 1) / nf;
    const long u = blockIdx.x / chunks, n0 = (blockIdx.x - u * chunks) * nf;
    const int frames = (int)((N - n0 < nf) ? N - n0 : nf);
    const long Tstart = n0 * P - z0p;                  // t of up[0]
    // floor division by P for a possibly negative Tstart
    const long nlo = Tstart >= 0 ? Tstart / P : -((-Tstart + P - 1) / P);
    const int r0 = (int)(Tstart - nlo * P);            // in [0, P)
    const T* bu = b + u * N * ldb;
    for (int pos = threadIdx.x; pos < RW; pos += blockDim.x) {
        const int k = pos - (S - 1) - dz;
        const bool tap = k >= 0 && k <= M;
        T cv[25];
#pragma unroll
        for (int i = 0; i <= 24; ++i) {
            const long nn = nlo + i;
            const long row = nn < 0 ? 0 : (nn < N ? nn : N - 1);
            cv[i] = (tap && i <= nrows) ? bu[row * ldb + (tap ? k : 0)] : T(0);
        }
#pragma unroll
        for (int i = 0; i < 24; ++i)
            if (i < nrows) rows[(size_t)i * RW + pos] = V2{cv[i], cv[i + 1]};
    }
    const int ulen = frames * P + 4 * NBt;
    const T* gyu = gy + u * Tlen;
    for (int j0 = threadIdx.x; j0 < ulen; j0 += 8 * blockDim.x) {
        T gv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = j0 + q * (int)blockDim.x;
            const long t = Tstart + j;
            gv[q] = (j < ulen && t >= 0 && t < Tlen) ? gyu[t] : T(0);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = j0 + q * (int)blockDim.x;
            if (j < ulen) {
                const int ph = (r0 + j) % P;
                const T w = (T)ph / (T)P;
                up[j] = V2{gv[q] - w * gv[q], w * gv[q]};
            }
        }
    }
    __syncthreads();
    const int fr = threadIdx.x / nt, l = threadIdx.x - fr * nt;
    if (fr >= frames) return;
    const int jb0 = fr * P + S * l;                    // this thread's samples are s = n0 P + jb0 + q; block m reads up[jb0 + 4 m ..]
    int ph = (r0 + jb0) % P;
    const V2* rp = rows + (size_t)((r0 + jb0) / P) * RW;
    const V2* upp = up + jb0;
    V2 a[S];
#pragma unroll
    for (int q = 0; q < S; ++q) a[q] = V2{0, 0};
    for (int m = 0; m < NBt; ++m) {                    // (uniform trip count: a scalar loop)
        // (two pairs per 16-byte aligned read: the rows and `up` start 32-byte aligned and advance by four pairs a block;
        // left as pair reads the compiler emits ds_read2_b64, which moves half as many bytes per LDS cycle as ds_read_b128)
        V2 w[S + 4], uu[4];
#pragma unroll
        for (int i = 0; i < S + 3; i += 2) zd_load2(rp + 4 * m + i, w[i], w[i + 1], i + 1 < S + 3);
#pragma unroll
        for (int i = 0; i < 4; i += 2) zd_load2(upp + 4 * m + i, uu[i], uu[i + 1], true);
#pragma unroll
        for (int q = 0; q < S; ++q)
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) zd_fma2(a[q], w[jt - q + S - 1], uu[jt]);
        ph += 4;
        if (ph >= P) {
            ph -= P;
            rp += RW;
        }
    }
    T* dst = gx + u * Tlen + n0 * P + jb0;
#pragma unroll
    for (int q = 0; q < S; ++q) {
        const T base = accumulate ? dst[q] : (add ? add[u * Tlen + n0 * P + jb0 + q] : T(0));
        dst[q] = base + scale * (a[q].x + a[q].y);
    }
}

// gb[n][k] = sum over the samples i of frames n - 1 and n of gs[i] x[t - k + z0], gs = the frame weight of b[n] in h_t times gy
// (frame n: 1 - w, frame n - 1: w; the last frame also takes its own w part).  A thread owns four consecutive taps and walks
// the 2 P samples in blocks of four on a sliding window of seven x values (one aligned 16-byte read of x and one of gs per 16
// multiply-adds); 256 / ceil((M + 1) / 4) frames per workgroup.  The old kernel: a thread per tap, two LDS reads per
// multiply-add, one frame per workgroup.
template <typename T>
__global__ __launch_bounds__(256) void zerodf_bwd_b_rows_kernel(const T* __restrict__ gy, const T* __restrict__ x, long Tlen, long N,
                                                                long BN, int M, int P, int z0, int nfw, int ldb, T scale, int accumulate,
                                                                T* __restrict__ gb)
{
    using V4 = T __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int NBk = (M + 4) / 4;                       // 4-tap blocks
    const int o = (3 - M) & 3;                         // shift that aligns the x window: (M - k0 - 3 + o) % 4 == 0
    const int XL = (2 * P + M + 8 + 3) & ~3;           // floats of x per frame
    T* gs = reinterpret_cast<T*>(smem_raw);            // [nfw][2 P]
    T* xs = gs + (size_t)nfw * 2 * P;                  // [nfw][XL]: xs[j + o] = x[(n - 1) P - M + z0 + j]
    const long f0 = (long)blockIdx.x * nfw;
    for (int fw = 0; fw < nfw; ++fw) {                 // (frame indices per frame, not per element: 64-bit divisions)
        const long f = f0 + fw;
        const bool fok = f < BN;
        const long u = fok ? f / N : 0, n = fok ? f - u * N : 0;
        const T* gyu = gy + u * Tlen;
        const T* xu = x + u * Tlen;
        for (int i = threadIdx.x; i < 2 * P; i += blockDim.x) {
            const long t = (n - 1) * P + i;
            T v = 0;
            if (fok && t >= 0) {
                // frame of t: n - 1 for i < P, n otherwise; the row b[n] enters h_t with 1 - w in its own frame, with w in the
                // frame before, and the clamped last frame takes both
                const int ph = i < P ? i : i - P;
                const T w = (T)ph / (T)P;
                const T wt = i < P ? w : ((n == N - 1) ? T(1) : T(1) - w);
                v = wt * gyu[t];
            }
            gs[(size_t)fw * 2 * P + i] = v;
        }
        for (int jj = threadIdx.x; jj < XL; jj += blockDim.x) {
            const int j = jj - o;
            const long sidx = (n - 1) * P - M + z0 + j;
            xs[(size_t)fw * XL + jj] = (fok && j >= 0 && sidx >= 0 && sidx < Tlen) ? xu[sidx] : T(0);
        }
    }
    __syncthreads();
    const int fw = threadIdx.x / NBk, kb = threadIdx.x - fw * NBk;
    const long f = f0 + fw;
    if (fw >= nfw || f >= BN) return;
    const int k0 = 4 * kb;
    // acc[q] (tap k0 + q) += gs[i + j] xs[i + j + M - k0 - q]: window xw[c] = xs[i + e + c], e = M - k0 - 3, c = j - q + 3
    const T* gp = gs + (size_t)fw * 2 * P;
    const T* xp = xs + (size_t)fw * XL + (M - k0 - 3 + o);   // 16-byte aligned
    T acc[4] = {T(0), T(0), T(0), T(0)};
    V4 lo = *reinterpret_cast<const V4*>(xp);
    for (int i = 0; i < 2 * P; i += 4) {
        const V4 hi = *reinterpret_cast<const V4*>(xp + i + 4);
        const V4 gv = *reinterpret_cast<const V4*>(gp + i);
        const T xw[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[q] += gv[j] * xw[j - q + 3];
        lo = hi;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (k0 + q <= M) gb[f * ldb + k0 + q] = (accumulate ? gb[f * ldb + k0 + q] : T(0)) + scale * acc[q];
}

template <typename T>
static int zerodf_launch_bwd(const void* gy, const void* x, const void* b, const void* y, int64_t B, int64_t Tlen, int64_t N, int M,
                             int P, int z0, int ig, void* gx, void* gb, hipStream_t st, double scale = 1.0, const void* gx_add = nullptr,
                             bool gb_accumulate = false)
{
    const bool plain = scale == 1.0 && gx_add == nullptr && !gb_accumulate;
    const bool rows_ok = !ig && P % 4 == 0 && P / 4 <= 64 && M >= 16;
    if (rows_ok) {
        // filters of more than ~200 taps as a sum of pieces (the kernels keep one piece's rows of a few frames in LDS): piece c
        // = taps [c KC, c KC + Mc], zeroth index z0 - c KC; gx accumulates over the pieces, gb's columns are disjoint
        const int npieces = (M + 1 + 199) / 200;
        const int KC = (((M + 1 + npieces - 1) / npieces) + 3) & ~3;
        // feasibility of BOTH kernels for EVERY piece is decided before anything is launched (round 3 launched gx first and could
        // then find that gb's rows did not fit LDS: P = 252 / 256 in float32, P >= 124 in float64 -- a half-written backward)
        struct PiecePlan { int Mc, z0c, nf, nrows, nfw; size_t lds_x, lds_b; };
        PiecePlan plan[64];
        bool ok = npieces <= 64;
        int np_used = 0;
        constexpr int S = 4;   // (eight samples per thread -- 2/3 of the LDS reads per multiply-add, 160 of 256 threads at P = 80 -- measured slower)
        for (int c = 0; c < npieces && ok; ++c) {
            PiecePlan& pl = plan[c];
            pl.Mc = ((M + 1 - c * KC) < KC ? (M + 1 - c * KC) : KC) - 1;
            pl.z0c = z0 - c * KC;
            if (pl.Mc < 0) break;
            np_used = c + 1;
            pl.nf = pl.nrows = pl.nfw = 0;
            pl.lds_x = pl.lds_b = 0;
            if (gx) {
                const int dz = (4 - (((pl.z0c % 4) + 4) & 3)) & 3, Mp = pl.Mc + dz, NBt = (Mp + S - 1) / 4 + 1, RW = (Mp + S + 6 + 3) & ~3, nt = P / S;
                int nf = 256 / nt;
                if (nf > 16) nf = 16;
                for (; nf >= 1; --nf) {
                    pl.nrows = nf + (Mp + P - 1) / P + 2;      // frames the t range of nf output frames can touch
                    pl.lds_x = sizeof(T) * 2 * ((size_t)pl.nrows * RW + (size_t)nf * P + 4 * NBt);
                    if (pl.nrows <= 24 && pl.lds_x <= 64 * 1024) break;
                }
                if (nf < 1) { ok = false; break; }
                pl.nf = nf;
            }
            if (gb) {
                const int NBk = (pl.Mc + 4) / 4;
                const int XL = (2 * P + pl.Mc + 8 + 3) & ~3;
                int nfw = 256 / NBk;
                if (nfw > 16) nfw = 16;
                for (; nfw >= 1; --nfw) {                      // fewer frames per workgroup until their rows fit LDS
                    pl.lds_b = sizeof(T) * (size_t)nfw * (2 * P + XL);
                    if (pl.lds_b <= 64 * 1024) break;
                }
                if (nfw < 1) { ok = false; break; }
                pl.nfw = nfw;
            }
        }
        for (int c = 0; c < np_used && ok; ++c) {
            const PiecePlan& pl = plan[c];
            if (gx) {
                const long chunks = (N + pl.nf - 1) / pl.nf;
                hipLaunchKernelGGL((zerodf_bwd_x_rows_kernel<T, S>), dim3((unsigned)(B * chunks)), dim3(256), pl.lds_x, st, (const T*)gy,
                                   (const T*)b + c * KC, (long)Tlen, (long)N, pl.Mc, P, pl.z0c, pl.nf, pl.nrows, M + 1, c > 0 ? 1 : 0, (T)scale,
                                   (const T*)gx_add, (T*)gx);
            }
            if (gb) {
                hipLaunchKernelGGL((zerodf_bwd_b_rows_kernel<T>), dim3((unsigned)((B * N + pl.nfw - 1) / pl.nfw)), dim3(256), pl.lds_b, st,
                                   (const T*)gy, (const T*)x, (long)Tlen, (long)N, (long)(B * N), pl.Mc, P, pl.z0c, pl.nfw, M + 1, (T)scale,
                                   gb_accumulate ? 1 : 0, (T*)gb + c * KC);
            }
        }
        // (nothing was launched unless every piece of both kernels fits)
        if (ok) return check_launch("zerodf_rows_bwd");
    }
    if (!plain) return fail(DSA_ERR_UNSUPPORTED, "zerodf_bwd: the scaled / accumulating form needs P % 4 == 0 and M >= 16%s");
    if (gx) {
        hipLaunchKernelGGL((zerodf_bwd_x_kernel<T>), dim3((unsigned)((B * Tlen + 255) / 256)), dim3(256), 0, st, (const T*)gy,
                           (const T*)b, (long)B, (long)Tlen, (long)N, M, P, z0, ig, (T*)gx);
    }
    if (gb) {
        const size_t lds = sizeof(T) * ((size_t)2 * P + 2 * P + M + 256);
        if (lds > 64 * 1024) return fail(DSA_ERR_UNSUPPORTED, "zerodf_bwd: filter too long for LDS%s");
        hipLaunchKernelGGL((zerodf_bwd_b_kernel<T>), dim3((unsigned)(B * N)), dim3(256), lds, st, (const T*)gy, (const T*)x,
                           (const T*)b, (const T*)y, (long)Tlen, (long)N, M, P, z0, ig, (T*)gb);
    }
    return check_launch("zerodf_bwd");
}

}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_zerodf_fwd(const void* x, const void* b, int64_t B, int64_t T, int32_t M, int32_t P, int32_t zeroth_index,
                              int32_t ignore_gain, int32_t dtype, void* y, void* stream)
{
    DSA_REQUIRE(M >= 0 && P > 0 && B >= 0 && T >= 0 && zeroth_index >= 0 && zeroth_index <= M, "zerodf: invalid sizes");
    DSA_REQUIRE(T % P == 0, "zerodf: the sequence length must be frames x frame_period");
    if (B * T == 0) return DSA_OK;
    const int64_t N = T / P;
    return with_dtype(dtype, "zerodf", [&](auto tag) {
        return zerodf_launch_fwd<decltype(tag)>(x, b, B, T, N, M, P, zeroth_index, ignore_gain, y, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_zerodf_taylor_fwd(const void* x, const void* b, int64_t B, int64_t T, int32_t M, int32_t P, int32_t zeroth_index,
                                     double scale, const void* acc, int32_t dtype, void* y, void* ysum, void* stream)
{
    DSA_REQUIRE(M >= 0 && P > 0 && B >= 0 && T >= 0 && zeroth_index >= 0 && zeroth_index <= M, "zerodf_taylor: invalid sizes");
    DSA_REQUIRE(T % P == 0, "zerodf_taylor: the sequence length must be frames x frame_period");
    if (B * T == 0) return DSA_OK;   // (an empty batch: its tensors have no storage)
    DSA_REQUIRE((acc != nullptr) == (ysum != nullptr), "zerodf_taylor: acc and ysum come together");
    DSA_REQUIRE(y != nullptr || ysum != nullptr, "zerodf_taylor: no output");
    const int64_t N = T / P;
    return with_dtype(dtype, "zerodf_taylor", [&](auto tag) {
        return zerodf_launch_fwd<decltype(tag)>(x, b, B, T, N, M, P, zeroth_index, 0, y, (hipStream_t)stream, scale, acc, ysum);
    });
}

DSA_EXPORT int dsa_zerodf_bwd(const void* gy, const void* x, const void* b, const void* y, int64_t B, int64_t T, int32_t M, int32_t P,
                              int32_t zeroth_index, int32_t ignore_gain, int32_t dtype, void* gx, void* gb, void* stream)
{
    DSA_REQUIRE(M >= 0 && P > 0 && B >= 0 && T >= 0 && zeroth_index >= 0 && zeroth_index <= M && T % P == 0, "zerodf_bwd: invalid sizes");
    if (B * T == 0) return DSA_OK;
    const int64_t N = T / P;
    return with_dtype(dtype, "zerodf_bwd", [&](auto tag) {
        return zerodf_launch_bwd<decltype(tag)>(gy, x, b, y, B, T, N, M, P, zeroth_index, ignore_gain, gx, gb, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_zerodf_taylor_bwd(const void* G, const void* x, const void* b, int64_t B, int64_t T, int32_t M, int32_t P,
                                     int32_t zeroth_index, double scale, const void* gy, int32_t dtype, void* G_out, void* gb,
                                     void* stream)
{
    DSA_REQUIRE(M >= 0 && P > 0 && B >= 0 && T >= 0 && zeroth_index >= 0 && zeroth_index <= M && T % P == 0, "zerodf_taylor_bwd: invalid sizes");
    if (B * T == 0) return DSA_OK;
    DSA_REQUIRE(G_out != nullptr && G_out != G, "zerodf_taylor_bwd: G_out must be a buffer of its own");
    const int64_t N = T / P;
    return with_dtype(dtype, "zerodf_taylor_bwd", [&](auto tag) {
        return zerodf_launch_bwd<decltype(tag)>(G, x, b, nullptr, B, T, N, M, P, zeroth_index, 0, G_out, gb, (hipStream_t)stream, scale, gy, true);
    });
}
