// Parameter generation (include/diffsptk_amd.h, section a19): the stage between an acoustic model's output and the synthesis chain.
//   delta  Delta._forward, delta.py:181-201                       (there: a replicate pad, conv2d over a permuted copy, a permute back)
//   mlpg   MaximumLikelihoodParameterGeneration, mlpg.py:118-171  (there: a dense (T, T H) matrix from a loop over T and the inverse of a
//          (T, T) matrix at construction, a dense product per call)
//   mcpf   MelCepstrumPostfiltering._forward, mcpf.py:191-209     (there: freqt -> rfft -> exp -> hfft twice, then mc2b and b2mc)
//
// delta: one thread per (b, t, d), d fastest; the H rows of the window are uniform across the lanes.  The adjoint GATHERS: the
// replicate padding folds the taps that fall before row 0 or behind row T - 1 onto those two rows, so row 0 and row T - 1 sum up to
// N + 1 cotangent rows per tap and every other row exactly one.
//
// mlpg: W^T W c = W^T u with W the (T H, T) window matrix of mlpg.py:146-156.  W^T W is symmetric positive definite and banded with
// half-bandwidth K = 2N; the host passes its banded Cholesky factor (T, K + 1), row s = G[s, s-K .. s-1] and 1 / G[s, s].  Two
// launches.  The right-hand side r = W^T u is a gather with one thread per (b, s, d), written into the output.  The sweep has one
// LANE per column (b, d), d fastest: forward substitution runs s upwards and back substitution downwards, in place, with the last K
// values of the recurrence in registers (K = 0, 2, .. 8; any other K reads them back from the column: the same lane wrote them) and
// the next chunk of right-hand sides and factor rows in flight while a chunk is computed (a first version formed r inside the
// sweep and waited for memory at every step: 1.7 ms for one utterance of 1000 frames).  The factor's rows are uniform across
// lanes.  The adjoint runs the same sweeps on the cotangent into a (B, T, D) workspace and applies W to it in a second launch.  All
// sums are float64 for either dtype.  The sweep is a dependent chain of length T with B D lanes of parallelism: a single utterance
// is bound by latency, not by anything a wider launch could buy.
//
// mcpf: b2mc(mc2b(.)) is the identity and b[0] enters only mc[0], so the operator is out = w * mc, out[0] += log(e1 / e2) / 2 with
// e = sum_k u_k exp(2 s_k) over the bins k <= ir_length / 2 of the ir_length-point spectrum of the de-warped cepstrum (u = 1 at both
// ends, 2 between: the reference's hfft), s = R mc, R = cos times the -alpha freqt matrix, (bins, M + 1), from the host.  One wave
// per frame, the bins over the lanes; s of the weighted cepstrum comes from the same table product, split at the onset.  The
// backward keeps u_k exp(2 s_k) of both energies in LDS and takes one pass with the coefficients over the lanes.  float64 arithmetic.
#include "common.h"

namespace dsa {
namespace {

constexpr int PG_THREADS = 256;
constexpr int PG_MAX_TAPS = 1 << 10;   // H and L: far beyond any window, keeps every index product in 32 bits

// ------------------------------------------------------------------------------------------------ delta
template <typename T>
__global__ __launch_bounds__(PG_THREADS) void delta_fwd_kernel(const T* __restrict__ x, long n, long Tn, long D, const T* __restrict__ window,
                                                               int H, int L, T* __restrict__ y)
{
    const long idx = (long)blockIdx.x * PG_THREADS + threadIdx.x;
    if (idx >= n) return;
    const long d = idx % D, bt = idx / D, t = bt % Tn, b = bt / Tn;
    const int N = (L - 1) / 2;
    const T* xc = x + b * Tn * D + d;
    T* yc = y + bt * H * D + d;
    for (int h = 0; h < H; ++h) {
        double acc = 0.0;
        for (int j = 0; j < L; ++j) {
            const T w = window[h * L + j];
            if (w == (T)0) continue;   // (uniform across the lanes)
            long s = t + j - N;
            s = s < 0 ? 0 : (s > Tn - 1 ? Tn - 1 : s);
            acc += (double)w * (double)xc[s * D];
        }
        yc[(long)h * D] = (T)acc;
    }
}

template <typename T>
__global__ __launch_bounds__(PG_THREADS) void delta_bwd_kernel(const T* __restrict__ g, long n, long Tn, long D, const T* __restrict__ window,
                                                               int H, int L, T* __restrict__ gx)
{
    const long idx = (long)blockIdx.x * PG_THREADS + threadIdx.x;
    if (idx >= n) return;
    const long d = idx % D, bt = idx / D, s = bt % Tn, b = bt / Tn;
    const int N = (L - 1) / 2;
    const T* gc = g + b * Tn * H * D + d;
    double acc = 0.0;
    for (int h = 0; h < H; ++h)
        for (int j = 0; j < L; ++j) {
            const T w = window[h * L + j];
            if (w == (T)0) continue;
            // the rows t whose tap j reads row s: clamp(t + j - N) = s
            long lo = s == 0 ? 0 : s - j + N, hi = s == Tn - 1 ? Tn - 1 : s - j + N;
            lo = lo < 0 ? 0 : lo;
            hi = hi > Tn - 1 ? Tn - 1 : hi;
            double sum = 0.0;
            for (long t = lo; t <= hi; ++t) sum += (double)gc[(t * H + h) * D];
            acc += (double)w * sum;
        }
    gx[idx] = (T)acc;
}

// ------------------------------------------------------------------------------------------------ mlpg
// whether row (t, h) of W keeps its window (mlpg.py:151-154): within N rows of either end only where the half-width fits
__device__ __forceinline__ bool mlpg_keep(long t, int thh, long Tn, int N) { return t < N ? thh <= t : (t > Tn - N - 1 ? thh < Tn - t : true); }

// r = W^T u: one thread per (b, s, d).  u:(B,T,H,D) -> r:(B,T,D)
template <typename T>
__global__ __launch_bounds__(PG_THREADS) void mlpg_rhs_kernel(const T* __restrict__ u, long n, long Tn, long D, const T* __restrict__ window,
                                                              const int* __restrict__ th, int H, int L, T* __restrict__ r)
{
    const long idx = (long)blockIdx.x * PG_THREADS + threadIdx.x;
    if (idx >= n) return;
    const long d = idx % D, bt = idx / D, s = bt % Tn, b = bt / Tn;
    const int N = (L - 1) / 2;
    const T* uc = u + b * Tn * H * D + d;
    double acc = 0.0;
    for (int j = 0; j < L; ++j) {
        const long t = s + N - j;
        if (t < 0 || t >= Tn) continue;
        for (int h = 0; h < H; ++h) {
            const T w = window[h * L + j];
            if (w == (T)0 || !mlpg_keep(t, th[h], Tn, N)) continue;   // (uniform across the lanes but for t at the ends)
            acc += (double)w * (double)uc[(t * H + h) * D];
        }
    }
    r[idx] = (T)acc;
}

// out = W v: one thread per (b, t, d), all H rows.  v:(B,T,D) -> out:(B,T,H,D)
template <typename T>
__global__ __launch_bounds__(PG_THREADS) void mlpg_apply_kernel(const T* __restrict__ v, long n, long Tn, long D, const T* __restrict__ window,
                                                                const int* __restrict__ th, int H, int L, T* __restrict__ out)
{
    const long idx = (long)blockIdx.x * PG_THREADS + threadIdx.x;
    if (idx >= n) return;
    const long d = idx % D, bt = idx / D, t = bt % Tn, b = bt / Tn;
    const int N = (L - 1) / 2;
    const T* vc = v + b * Tn * D + d;
    T* oc = out + bt * H * D + d;
    for (int h = 0; h < H; ++h) {
        double acc = 0.0;
        if (mlpg_keep(t, th[h], Tn, N))
            for (int j = 0; j < L; ++j) {
                const T w = window[h * L + j];
                const long s = t + j - N;
                if (w == (T)0 || s < 0 || s >= Tn) continue;
                acc += (double)w * (double)vc[s * D];
            }
        oc[(long)h * D] = (T)acc;
    }
}

template <int K> struct MlpgRing {
    double v[K > 0 ? K : 1];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < K; ++i) v[i] = 0.0;
    }
    __device__ __forceinline__ void push(double z)
    {
#pragma unroll
        for (int i = K - 1; i > 0; --i) v[i] = v[i - 1];
        if (K > 0) v[0] = z;
    }
};

// one value of a wave-wide register, from the lane `l` (a compile-time constant once the loops are unrolled), as a scalar.  The
// double keeps this spelling of its own: with wave_readlane's the compiler schedules mlpg_sweep_kernel<double, 0> differently.
__device__ __forceinline__ float pg_lane(float v, int l) { return wave_readlane(v, l); }
__device__ __forceinline__ double pg_lane(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// The two substitution sweeps on one column per lane, half-bandwidth K in registers.  rhs may be z itself (the forward direction
// sweeps in place).  Steps go in chunks of CH.  A chunk's right-hand sides are CH loads per lane; the factor values it needs are one
// contiguous run of the table, loaded ONCE per wave -- value e by lane e % 64 of register e / 64 -- and read out lane by lane as
// scalars.  Both are requested while the chunk before is computed, so that the dependent chain waits for arithmetic and not for
// memory.  Every lane stays alive for those loads: a lane beyond the last column works on a copy of it and stores nothing.
template <typename T, int K>
__global__ __launch_bounds__(64) void mlpg_sweep_kernel(const T* rhs, long cols, long Tn, long D, const T* __restrict__ factor, T* z)
{
    constexpr int CH = K <= 2 ? 32 : 16, F = K + 1;
    constexpr int NQ = ((CH + K) * F + 63) / 64;   // registers for the (CH + K) rows the back sweep reads; the forward sweep reads CH
    const int lane = threadIdx.x;
    long col = (long)blockIdx.x * 64 + lane;
    const bool live = col < cols;
    col = live ? col : cols - 1;
    const long b = col / D, d = col % D;
    const T* rc = rhs + b * Tn * D + d;
    T* zc = z + b * Tn * D + d;
    const long nfull = Tn / CH, last = Tn - 1, fend = Tn * F - 1;
    MlpgRing<K> ring;
    T rv[CH], nr[CH], fq[NQ], nq[NQ];
    // ---- forward substitution, s upwards: chunk c is rows c CH .. c CH + CH - 1, factor values from (c CH) F on
    ring.clear();
    if (nfull > 0) {
#pragma unroll
        for (int i = 0; i < CH; ++i) rv[i] = rc[(long)i * D];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const long e = (long)q * 64 + lane;
            fq[q] = factor[e > fend ? fend : e];
        }
    }
    for (long c = 0; c < nfull; ++c) {
        const long s0 = c * CH;
        const bool more = c + 1 < nfull;
        if (more) {
#pragma unroll
            for (int i = 0; i < CH; ++i) nr[i] = rc[(s0 + CH + i) * D];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const long e = (s0 + CH) * F + (long)q * 64 + lane;
                nq[q] = factor[e > fend ? fend : e];
            }
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            double acc = (double)rv[i];
#pragma unroll
            for (int k = K; k >= 1; --k) acc -= (double)pg_lane(fq[(i * F + K - k) / 64], (i * F + K - k) % 64) * ring.v[k - 1];   // (zero left of column 0)
            const double zz = acc * (double)pg_lane(fq[(i * F + K) / 64], (i * F + K) % 64);
            ring.push(zz);
            if (live) zc[(s0 + i) * D] = (T)zz;
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < CH; ++i) rv[i] = nr[i];
#pragma unroll
            for (int q = 0; q < NQ; ++q) fq[q] = nq[q];
        }
    }
    for (long s = nfull * CH; s < Tn; ++s) {
        double acc = (double)rc[s * D];
#pragma unroll
        for (int k = K; k >= 1; --k) acc -= (double)factor[s * F + K - k] * ring.v[k - 1];
        const double zz = acc * (double)factor[s * F + K];
        ring.push(zz);
        if (live) zc[s * D] = (T)zz;
    }
    // ---- back substitution, s downwards: step s reads 1 / G[s, s] and G[s + k, s] = factor[s + k, K - k], zero times whatever
    // lies past the last row.  Chunk c is rows s0 = last - c CH down to lo = s0 - CH + 1; its values start at row lo.
    ring.clear();
    if (nfull > 0) {
        const long lo = last - CH + 1;
#pragma unroll
        for (int i = 0; i < CH; ++i) rv[i] = zc[(last - i) * D];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const long e = lo * F + (long)q * 64 + lane;
            fq[q] = factor[e > fend ? fend : e];
        }
    }
    for (long c = 0; c < nfull; ++c) {
        const long s0 = last - c * CH;
        const bool more = c + 1 < nfull;
        if (more) {
            const long lo = s0 - 2 * CH + 1;
#pragma unroll
            for (int i = 0; i < CH; ++i) nr[i] = zc[(s0 - CH - i) * D];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const long e = lo * F + (long)q * 64 + lane;
                nq[q] = factor[e > fend ? fend : e];
            }
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {   // row s = s0 - i is row CH - 1 - i of the chunk's values
            double acc = (double)rv[i];
#pragma unroll
            for (int k = K; k >= 1; --k) {
                const int e = (CH - 1 - i + k) * F + K - k;
                acc -= (double)pg_lane(fq[e / 64], e % 64) * ring.v[k - 1];
            }
            const int e = (CH - 1 - i) * F + K;
            const double cc = acc * (double)pg_lane(fq[e / 64], e % 64);
            ring.push(cc);
            if (live) zc[(s0 - i) * D] = (T)cc;
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < CH; ++i) rv[i] = nr[i];
#pragma unroll
            for (int q = 0; q < NQ; ++q) fq[q] = nq[q];
        }
    }
    for (long s = last - nfull * CH; s >= 0; --s) {
        double acc = (double)zc[s * D];
#pragma unroll
        for (int k = K; k >= 1; --k) acc -= (double)factor[(s + k > last ? last : s + k) * F + K - k] * ring.v[k - 1];
        const double cc = acc * (double)factor[s * F + K];
        ring.push(cc);
        if (live) zc[s * D] = (T)cc;
    }
}

// the same for any half-bandwidth: the last K values are read back from the column (this lane wrote them)
template <typename T>
__global__ __launch_bounds__(64) void mlpg_sweep_any_kernel(const T* rhs, long cols, long Tn, long D, const T* __restrict__ factor, int K, T* z)
{
    const long col = (long)blockIdx.x * 64 + threadIdx.x;
    if (col >= cols) return;
    const long b = col / D, d = col % D;
    const int F = K + 1;
    const T* rc = rhs + b * Tn * D + d;
    T* zc = z + b * Tn * D + d;
    for (long s = 0; s < Tn; ++s) {
        double acc = (double)rc[s * D];
        for (int k = K; k >= 1; --k)
            if (s - k >= 0) acc -= (double)factor[s * F + K - k] * (double)zc[(s - k) * D];
        zc[s * D] = (T)(acc * (double)factor[s * F + K]);
    }
    for (long s = Tn - 1; s >= 0; --s) {
        double acc = (double)zc[s * D];
        for (int k = K; k >= 1; --k)
            if (s + k < Tn) acc -= (double)factor[(s + k) * F + K - k] * (double)zc[(s + k) * D];
        zc[s * D] = (T)(acc * (double)factor[s * F + K]);
    }
}

// ------------------------------------------------------------------------------------------------ mcpf
// this lane's share of e1 = sum_k u_k exp(2 s1_k) and e2 (the weighted cepstrum); q, when given, keeps the terms: q[k], q[bins + k]
template <typename T>
__device__ __forceinline__ void mcpf_energies(const T* __restrict__ c, int M1, const double* __restrict__ table_t, int bins, double scale,
                                              int onset, int lane, double* q, double& e1, double& e2)
{
    e1 = 0.0;
    e2 = 0.0;
    const int split = onset < M1 ? onset : M1;
    for (int k = lane; k < bins; k += 64) {
        double lo = 0.0, hi = 0.0;
        for (int j = 0; j < split; ++j) lo += table_t[(long)j * bins + k] * (double)c[j];
        for (int j = split; j < M1; ++j) hi += table_t[(long)j * bins + k] * (double)c[j];
        const double uk = k == 0 || k == bins - 1 ? 1.0 : 2.0;
        const double q1 = uk * exp(2.0 * (lo + hi)), q2 = uk * exp(2.0 * (lo + scale * hi));
        if (q) {
            q[k] = q1;
            q[bins + k] = q2;
        }
        e1 += q1;
        e2 += q2;
    }
    e1 = wave_sum(e1);
    e2 = wave_sum(e2);
}

template <typename T>
__global__ __launch_bounds__(64) void mcpf_fwd_kernel(const T* __restrict__ mc, long frames, int M1, const double* __restrict__ table_t, int bins,
                                                      double scale, int onset, T* __restrict__ out)
{
    const int lane = threadIdx.x;
    for (long f = blockIdx.x; f < frames; f += gridDim.x) {
        const T* c = mc + f * M1;
        double e1, e2;
        mcpf_energies<T>(c, M1, table_t, bins, scale, onset, lane, nullptr, e1, e2);
        const double shift = 0.5 * log(e1 / e2);
        for (int j = lane; j < M1; j += 64) {
            double v = (j < onset ? 1.0 : scale) * (double)c[j];
            if (j == 0) v += shift;
            out[f * M1 + j] = (T)v;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64) void mcpf_bwd_kernel(const T* __restrict__ mc, const T* __restrict__ g, long frames, int M1,
                                                      const double* __restrict__ table, const double* __restrict__ table_t, int bins, double scale,
                                                      int onset, T* __restrict__ gmc)
{
    extern __shared__ double pg_q[];   // 2 bins
    const int lane = threadIdx.x;
    for (long f = blockIdx.x; f < frames; f += gridDim.x) {
        const T* c = mc + f * M1;
        double e1, e2;
        __syncthreads();   // the frame before this one has been read out of pg_q
        mcpf_energies<T>(c, M1, table_t, bins, scale, onset, lane, pg_q, e1, e2);
        __syncthreads();
        const double g0 = (double)g[f * M1], r1 = 1.0 / e1, r2 = 1.0 / e2;
        // d out[0] / d mc[j] = w_j [j = 0] + sum_k (q1_k / e1 - w_j q2_k / e2) R[k, j]
        for (int j = lane; j < M1; j += 64) {
            double a1 = 0.0, a2 = 0.0;
            for (int k = 0; k < bins; ++k) {
                const double r = table[(long)k * M1 + j];
                a1 += pg_q[k] * r;
                a2 += pg_q[bins + k] * r;
            }
            const double w = j < onset ? 1.0 : scale;
            gmc[f * M1 + j] = (T)(w * (double)g[f * M1 + j] + g0 * (a1 * r1 - w * (a2 * r2)));
        }
    }
}

inline bool pg_grid(long n, int per, unsigned& grid)
{
    const long blocks = (n + per - 1) / per;
    if (blocks > 0x7fffffffL) return false;
    grid = (unsigned)blocks;
    return true;
}

template <typename T>
void mlpg_sweep_launch(int K, unsigned grid, hipStream_t st, const void* rhs, long cols, long Tn, long D, const void* factor, void* z)
{
#define DSA_MLPG_CASE(KK) \
    hipLaunchKernelGGL((mlpg_sweep_kernel<T, KK>), dim3(grid), dim3(64), 0, st, (const T*)rhs, cols, Tn, D, (const T*)factor, (T*)z)
    switch (K) {
    case 0: DSA_MLPG_CASE(0); break;
    case 2: DSA_MLPG_CASE(2); break;
    case 4: DSA_MLPG_CASE(4); break;
    case 6: DSA_MLPG_CASE(6); break;
    case 8: DSA_MLPG_CASE(8); break;
    default:
        hipLaunchKernelGGL((mlpg_sweep_any_kernel<T>), dim3(grid), dim3(64), 0, st, (const T*)rhs, cols, Tn, D, (const T*)factor, K, (T*)z);
        break;
    }
#undef DSA_MLPG_CASE
}

// forward: rhs into out, the sweeps in place.  adjoint: the sweeps on the cotangent into work, W applied to it.
template <typename T>
void mlpg_launch(hipStream_t st, unsigned grid_n, unsigned grid_c, const void* u, long n, long cols, long Tn, long D, const void* window,
                 const void* th, int H, int L, const void* factor, bool adjoint, void* work, void* out)
{
    if (!adjoint) {
        hipLaunchKernelGGL((mlpg_rhs_kernel<T>), dim3(grid_n), dim3(PG_THREADS), 0, st, (const T*)u, n, Tn, D, (const T*)window, (const int*)th, H, L,
                           (T*)out);
        mlpg_sweep_launch<T>(L - 1, grid_c, st, out, cols, Tn, D, factor, out);
    } else {
        mlpg_sweep_launch<T>(L - 1, grid_c, st, u, cols, Tn, D, factor, work);
        hipLaunchKernelGGL((mlpg_apply_kernel<T>), dim3(grid_n), dim3(PG_THREADS), 0, st, (const T*)work, n, Tn, D, (const T*)window,
                           (const int*)th, H, L, (T*)out);
    }
}

// the sizes every entry of the family shares; n = B T D is an int64 count and so is n H
inline bool pg_sizes(int64_t B, int64_t T, int64_t D, int32_t H, int32_t L)
{
    if (!(B >= 0 && T >= 0 && D >= 0 && H >= 1 && H <= PG_MAX_TAPS && L >= 1 && L <= PG_MAX_TAPS && L % 2 == 1)) return false;
    if (T > 0 && D > 0 && B > INT64_MAX / T / D / H) return false;
    return true;
}

}  // namespace
}  // namespace dsa

using namespace dsa;

static int delta_entry(bool bwd, const void* in, int64_t B, int64_t T, int64_t D, const void* window, int32_t H, int32_t L, int32_t dtype, void* out,
                       void* stream)
{
    if (!pg_sizes(B, T, D, H, L)) return fail(DSA_ERR_INVALID_ARGUMENT, "delta: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "delta: unknown dtype");
    if (B == 0 || T == 0 || D == 0) return DSA_OK;
    if (!(in && window && out)) return fail(DSA_ERR_INVALID_ARGUMENT, "delta: null pointer");
    const long n = (long)(B * T * D);
    unsigned grid;
    if (!pg_grid(n, PG_THREADS, grid)) return fail(DSA_ERR_INVALID_ARGUMENT, "delta: too many elements for one launch");
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "delta", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's sequence length)
        if (bwd)
            hipLaunchKernelGGL((delta_bwd_kernel<V>), dim3(grid), dim3(PG_THREADS), 0, st, (const V*)in, n, (long)T, (long)D, (const V*)window, H, L,
                               (V*)out);
        else
            hipLaunchKernelGGL((delta_fwd_kernel<V>), dim3(grid), dim3(PG_THREADS), 0, st, (const V*)in, n, (long)T, (long)D, (const V*)window, H, L,
                               (V*)out);
        return check_launch(bwd ? "delta_bwd" : "delta_fwd");
    });
}

DSA_EXPORT int dsa_delta(const void* x, int64_t B, int64_t T, int64_t D, const void* window, int32_t H, int32_t L, int32_t dtype, void* y,
                             void* stream)
{
    return delta_entry(false, x, B, T, D, window, H, L, dtype, y, stream);
}

DSA_EXPORT int dsa_delta_vjp(const void* gy, int64_t B, int64_t T, int64_t D, const void* window, int32_t H, int32_t L, int32_t dtype, void* gx,
                             void* stream)
{
    return delta_entry(true, gy, B, T, D, window, H, L, dtype, gx, stream);
}

DSA_EXPORT int dsa_mlpg(const void* u, int64_t B, int64_t T, int64_t D, const void* window, const void* th, int32_t H, int32_t L, const void* factor,
                        int32_t direction, int32_t dtype, void* work, void* out, void* stream)
{
    if (!pg_sizes(B, T, D, H, L)) return fail(DSA_ERR_INVALID_ARGUMENT, "mlpg: invalid sizes");
    if (direction != DSA_MLPG_FORWARD && direction != DSA_MLPG_ADJOINT) return fail(DSA_ERR_INVALID_ARGUMENT, "mlpg: unknown direction");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "mlpg: unknown dtype");
    if (B == 0 || T == 0 || D == 0) return DSA_OK;
    if (T < L - 1) return fail(DSA_ERR_INVALID_ARGUMENT, "mlpg: the sequence is shorter than 2N = L - 1 frames");
    const bool adjoint = direction == DSA_MLPG_ADJOINT;
    if (!(u && window && th && factor && out && (work || !adjoint))) return fail(DSA_ERR_INVALID_ARGUMENT, "mlpg: null pointer");
    const long cols = (long)(B * D), n = (long)(B * T * D);
    unsigned grid_c, grid_n;
    if (!pg_grid(cols, 64, grid_c) || !pg_grid(n, PG_THREADS, grid_n)) return fail(DSA_ERR_INVALID_ARGUMENT, "mlpg: too many elements for one launch");
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "mlpg", [&](auto tag) {
        mlpg_launch<decltype(tag)>(st, grid_n, grid_c, u, n, cols, (long)T, (long)D, window, th, H, L, factor, adjoint, work, out);
        return check_launch(L - 1 <= DSA_MLPG_MAX_REGISTER_BAND ? (adjoint ? "mlpg_adjoint_reg" : "mlpg_forward_reg")
                                                                : (adjoint ? "mlpg_adjoint_any" : "mlpg_forward_any"));
    });
}

static int mcpf_check(int64_t F, int32_t M1, int32_t bins, double scale, int32_t onset, int32_t dtype)
{
    if (!(F >= 0 && M1 >= 0 && bins >= 2 && bins <= DSA_MCPF_MAX_BINS && onset >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "mcpf: invalid sizes");
    if (M1 > 0 && F > INT64_MAX / M1) return fail(DSA_ERR_INVALID_ARGUMENT, "mcpf: invalid sizes");
    if (!(scale == scale) || scale - scale != 0.0) return fail(DSA_ERR_INVALID_ARGUMENT, "mcpf: 1 + beta is not finite");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "mcpf: unknown dtype");
    return DSA_OK;
}

DSA_EXPORT int dsa_mcpf(const void* mc, int64_t F, int32_t M1, const void* table_t, int32_t bins, double scale, int32_t onset, int32_t dtype,
                            void* out, void* stream)
{
    if (int rc = mcpf_check(F, M1, bins, scale, onset, dtype)) return rc;
    if (F == 0 || M1 == 0) return DSA_OK;
    if (!(mc && table_t && out)) return fail(DSA_ERR_INVALID_ARGUMENT, "mcpf: null pointer");
    const unsigned grid = (unsigned)(F < (1 << 20) ? F : (1 << 20));
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "mcpf", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((mcpf_fwd_kernel<T>), dim3(grid), dim3(64), 0, st, (const T*)mc, (long)F, M1, (const double*)table_t, bins, scale, onset,
                           (T*)out);
        return check_launch("mcpf_fwd");
    });
}

DSA_EXPORT int dsa_mcpf_vjp(const void* mc, const void* g, int64_t F, int32_t M1, const void* table, const void* table_t, int32_t bins, double scale,
                            int32_t onset, int32_t dtype, void* gmc, void* stream)
{
    if (int rc = mcpf_check(F, M1, bins, scale, onset, dtype)) return rc;
    if (F == 0 || M1 == 0) return DSA_OK;
    if (!(mc && g && table && table_t && gmc)) return fail(DSA_ERR_INVALID_ARGUMENT, "mcpf: null pointer");
    const unsigned grid = (unsigned)(F < (1 << 20) ? F : (1 << 20));
    const size_t lds = (size_t)2 * bins * sizeof(double);   // at most 2 * DSA_MCPF_MAX_BINS * 8 = 32 784 bytes
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "mcpf", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((mcpf_bwd_kernel<T>), dim3(grid), dim3(64), lds, st, (const T*)mc, (const T*)g, (long)F, M1, (const double*)table,
                           (const double*)table_t, bins, scale, onset, (T*)gmc);
        return check_launch("mcpf_bwd");
    });
}
