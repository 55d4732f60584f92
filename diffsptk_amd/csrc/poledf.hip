// Time-variant all-pole (LPC synthesis) filter: AllPoleDigitalFilter, poledf.py:117-140 (the reference hands the recursion to
// torchlpc.sample_wise_lpc).  x:(B,T), a:(B,N,M+1) with T = N P;  a row is [K, a_1 .. a_M]:
//   c_t = lerp(a[t / P], a[min(t / P + 1, N - 1)], (t % P) / P)     (linear_intpl.py:85-117)
//   g_t = c_t[0]  (1 with ignore_gain)
//   y[t] = g_t x[t] - sum_{k=1..M} c_t[k] y[t - k]                  (zero initial state)
// Adjoint (u = A^{-T} gy, run backward in time):
//   u[t] = gy[t] - sum_{k=1..M} c_{t+k}[k] u[t + k],   gx[t] = g_t u[t],
//   dc_t[k] = -u[t] y[t - k] (k >= 1),   dc_t[0] = u[t] x[t] (0 with ignore_gain),
// and the per-sample coefficient gradients go back through the interpolation to ga:(B,N,M+1).
//
// The recursion is sequential in time, so the ring kernels put ONE wave on an utterance and make each sample cost two dependent
// instructions.  The 64 lanes hold a ring over OUTPUT times: in block b (times 64 b .. 64 b + 63) lane s accumulates time
// tau = 64 b + s.  At step j the finished value of lane j is read with a wave-uniform v_readlane, and every lane takes one
// multiply-add with it:  acc -= E[j][s] y_j,  E[j][s] = c_tau[tau - t_j] (zero outside 1 .. M).  A lane that has been read is
// re-seeded with the excitation of tau + 64 -- in groups of Q lanes every Q steps (Q = 32 for M <= 32), which is exact as long
// as M <= 64 - Q: a re-seeded lane receives its first term at step 64 + s - M, after its group's re-seed.  E for a block lives
// in LDS as [j][s], so step j reads it at an immediate offset; it is built ahead of the chain from the frames' coefficient rows,
// which are prefetched one block ahead through registers into an LDS row window.  The backward runs the same ring on reversed
// time: there every lane at step j uses the coefficients of the SAME time t_j, c_{t_j}[k].
// Each utterance is one wave whatever the batch: results are independent of B, bit for bit.
// Anything the ring does not cover (M = 0, M > 63, a row window beyond kPdR registers a lane) takes the generic kernels: one
// thread per utterance, plain loops -- correct, not fast.
#include "common.h"

#include <atomic>
#include <climits>

namespace dsa {
namespace {

constexpr int kPdR = 8;         // registers per lane of the row-window prefetch: 512 coefficient values a block
constexpr int kPdE = 64 * 64;   // one E table
constexpr int kPdCh = 256;      // samples per LDS chunk of the ga kernel

__device__ __forceinline__ long pd_clamp(long t, long Tlen) { return t < 0 ? 0 : (t >= Tlen ? Tlen - 1 : t); }

__device__ __forceinline__ long pd_div(long t, int P, bool small) { return small ? (long)((unsigned)t / (unsigned)P) : t / P; }

// frames [nlo, nhi] that the times tlo .. tlo + 63 (clamped into [0, T)) interpolate between: at most 63 / P + 3 rows
__device__ __forceinline__ void pd_window(long tlo, long Tlen, long N, int P, bool small, long& nlo, long& nhi)
{
    nlo = pd_div(pd_clamp(tlo, Tlen), P, small);
    nhi = pd_div(pd_clamp(tlo + 63, Tlen), P, small) + 1;
    if (nhi > N - 1) nhi = N - 1;
}

template <typename T>
__device__ __forceinline__ void pd_load_rows(const T* __restrict__ au, long tlo, long Tlen, long N, int P, int M1, bool small, int lane,
                                             T (&r)[kPdR])
{
    long nlo, nhi;
    pd_window(tlo, Tlen, N, P, small, nlo, nhi);
    const long base = nlo * M1, cnt = (nhi - nlo + 1) * M1;
#pragma unroll
    for (int i = 0; i < kPdR; ++i) {
        const long e = lane + 64 * i;
        r[i] = e < cnt ? au[base + e] : T(0);
    }
}

template <typename T>
__device__ __forceinline__ void pd_store_rows(T* Wb, const T (&r)[kPdR], int lane)
{
#pragma unroll
    for (int i = 0; i < kPdR; ++i) Wb[lane + 64 * i] = r[i];
}

// the interpolation of time t (clamped) from the row window of the block starting at tlo: row pointers and weight
template <typename T>
__device__ __forceinline__ void pd_rows(const T* Wb, long t, long tlo, long Tlen, long N, int P, int M1, bool small, const T*& r0,
                                        const T*& r1, T& w)
{
    long nlo, nhi;
    pd_window(tlo, Tlen, N, P, small, nlo, nhi);
    const long tc = pd_clamp(t, Tlen);
    const long n = pd_div(tc, P, small);
    const long n1 = n + 1 < N ? n + 1 : N - 1;
    w = (T)(tc - n * P) / (T)P;
    r0 = Wb + (n - nlo) * M1;
    r1 = Wb + (n1 - nlo) * M1;
}

// c[q] = c_t[k0 + q] for k0 + q <= M: all reads of the row window before any write to E (the same LDS array to the compiler:
// a term at a time, each one waits out an LDS round trip -- measured 3/4 of a block's time at M = 24)
template <typename T>
__device__ __forceinline__ void pd_lerp8(const T* r0, const T* r1, T w, int k0, int M, T (&c)[8])
{
    T v0[8], v1[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = k0 + q <= M ? k0 + q : M;
        v0[q] = r0[k];
        v1[q] = r1[k];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) c[q] = v0[q] + w * (v1[q] - v0[q]);
}

// 64 steps of the ring on table Eb; yv receives the block's finished values, acc leaves holding the next block's seeds
template <typename T, int Q>
__device__ __forceinline__ void pd_ring(T& acc, T& yv, T seed, const T* Eb, int lane)
{
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        if (j > 0 && j % Q == 0) {   // lanes j - Q .. j - 1 have been read: keep their values, start their next times
            const bool m = (unsigned)(lane - (j - Q)) < (unsigned)Q;
            yv = m ? acc : yv;
            acc = m ? seed : acc;
        }
        const T yj = wave_readlane(acc, j);
        acc = fma(-Eb[j * 64 + lane], yj, acc);
    }
    const bool m = lane >= 64 - Q;
    yv = m ? acc : yv;
    acc = m ? seed : acc;
}

template <typename T, int Q>
__global__ __launch_bounds__(64) void poledf_ring_fwd_kernel(const T* __restrict__ x, const T* __restrict__ a, long Tlen, long N, int M,
                                                             int P, int ignore_gain, T* __restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* E = reinterpret_cast<T*>(smem_raw);   // [2][64][64]: E[buf][j][s], the coefficient lane s applies at step j
    T* W = E + 2 * kPdE;                     // [2][64 kPdR]: coefficient rows of a block's frames
    const int lane = threadIdx.x, M1 = M + 1;
    const long u = blockIdx.x;
    const bool small = Tlen < INT_MAX;
    const T* xu = x + u * Tlen;
    const T* au = a + u * N * M1;
    T* yu = y + u * Tlen;
    for (int i = lane; i < 2 * kPdE; i += 64) E[i] = T(0);
    T rr[kPdR];
    pd_load_rows(au, 0, Tlen, N, P, M1, small, lane, rr);
    pd_store_rows(W, rr, lane);
    pd_load_rows(au, 64, Tlen, N, P, M1, small, lane, rr);
    pd_store_rows(W + 64 * kPdR, rr, lane);
    __syncthreads();
    // the coefficients of block X's times: lane s, tau = 64 X + s, term k goes to step s - k of block X (k <= s) or to step
    // 64 + s - k of block X - 1 (k > s: tau is then the re-seeded time of lane s).  Column s is written and read by lane s only.
    auto prepare = [&](long X) -> T {
        const T *r0, *r1;
        T w;
        pd_rows(W + (X & 1) * 64 * kPdR, 64 * X + lane, 64 * X, Tlen, N, P, M1, small, r0, r1, w);
        T* Ec = E + (X & 1) * kPdE;
        T* Ep = E + ((X + 1) & 1) * kPdE;
        for (int k0 = 1; k0 <= M; k0 += 8) {
            T c[8];
            pd_lerp8(r0, r1, w, k0, M, c);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k = k0 + q;
                if (k <= M) (k <= lane ? Ec : Ep)[((lane - k) & 63) * 64 + lane] = c[q];
            }
        }
        return ignore_gain ? T(1) : r0[0] + w * (r1[0] - r0[0]);
    };
    const long nb = (Tlen + 63) / 64;
    const T g0 = prepare(0);
    T acc = g0 * (lane < Tlen ? xu[lane] : T(0));
    T xn = 64 + lane < Tlen ? xu[64 + lane] : T(0);   // excitation of block b + 1
    T yv = T(0);
    for (long b = 0; b < nb; ++b) {
        pd_load_rows(au, 64 * (b + 2), Tlen, N, P, M1, small, lane, rr);   // lands while the chain runs
        const long t2 = 64 * (b + 2) + lane;
        const T xnn = t2 < Tlen ? xu[t2] : T(0);
        const T seed = prepare(b + 1) * xn;
        __syncthreads();
        pd_ring<T, Q>(acc, yv, seed, E + (b & 1) * kPdE, lane);
        const long t = 64 * b + lane;
        if (t < Tlen) yu[t] = yv;
        pd_store_rows(W + (b & 1) * 64 * kPdR, rr, lane);   // rows of block b + 2 replace those of block b
        __syncthreads();
        xn = xnn;
    }
}

// reversed time: block b holds t = T - 1 - 64 b - s at step s
template <typename T, int Q>
__global__ __launch_bounds__(64) void poledf_ring_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ a, long Tlen, long N, int M,
                                                             int P, int ignore_gain, T* __restrict__ uo, T* __restrict__ gx)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* E = reinterpret_cast<T*>(smem_raw);
    T* W = E + 2 * kPdE;
    const int lane = threadIdx.x, M1 = M + 1;
    const long u = blockIdx.x;
    const bool small = Tlen < INT_MAX;
    const T* gu = gy + u * Tlen;
    const T* au = a + u * N * M1;
    for (int i = lane; i < 2 * kPdE; i += 64) E[i] = T(0);
    T rr[kPdR];
    pd_load_rows(au, Tlen - 64, Tlen, N, P, M1, small, lane, rr);
    pd_store_rows(W, rr, lane);
    __syncthreads();
    // step j of block X reads u at t_j; lane j writes c_{t_j}[k] to the lane that holds t_j - k: lane j + k, or lane j + k - 64
    // after its re-seed -- all of block X's table.
    auto prepare = [&](long X) -> T {
        const T *r0, *r1;
        T w;
        const long tlo = Tlen - 64 - 64 * X;
        pd_rows(W + (X & 1) * 64 * kPdR, tlo + 63 - lane, tlo, Tlen, N, P, M1, small, r0, r1, w);
        T* Eb = E + (X & 1) * kPdE + lane * 64;
        for (int k0 = 1; k0 <= M; k0 += 8) {
            T c[8];
            pd_lerp8(r0, r1, w, k0, M, c);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (k0 + q <= M) Eb[(lane + k0 + q) & 63] = c[q];
        }
        return ignore_gain ? T(1) : r0[0] + w * (r1[0] - r0[0]);
    };
    const long nb = (Tlen + 63) / 64;
    T acc = Tlen - 1 - lane >= 0 ? gu[Tlen - 1 - lane] : T(0);
    T gn = Tlen - 65 - lane >= 0 ? gu[Tlen - 65 - lane] : T(0);
    T yv = T(0);
    for (long b = 0; b < nb; ++b) {
        pd_load_rows(au, Tlen - 128 - 64 * b, Tlen, N, P, M1, small, lane, rr);   // rows of block b + 1
        const long t2 = Tlen - 1 - 64 * (b + 2) - lane;
        const T gnn = t2 >= 0 ? gu[t2] : T(0);
        const T g = prepare(b);
        __syncthreads();
        pd_ring<T, Q>(acc, yv, gn, E + (b & 1) * kPdE, lane);
        const long t = Tlen - 1 - 64 * b - lane;
        if (t >= 0) {
            uo[u * Tlen + t] = yv;
            if (gx) gx[u * Tlen + t] = g * yv;
        }
        pd_store_rows(W + ((b + 1) & 1) * 64 * kPdR, rr, lane);
        __syncthreads();
        gn = gnn;
    }
}

// generic: one thread per utterance
template <typename T>
__global__ __launch_bounds__(64) void poledf_generic_fwd_kernel(const T* __restrict__ x, const T* __restrict__ a, long B, long Tlen, long N,
                                                                int M, int P, int ignore_gain, T* __restrict__ y)
{
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= B) return;
    const int M1 = M + 1;
    const T* xu = x + u * Tlen;
    const T* au = a + u * N * M1;
    T* yu = y + u * Tlen;
    for (long t = 0; t < Tlen; ++t) {
        const long n = t / P, n1 = n + 1 < N ? n + 1 : N - 1;
        const T w = (T)(t - n * P) / (T)P;
        const T* r0 = au + n * M1;
        const T* r1 = au + n1 * M1;
        T acc = (ignore_gain ? T(1) : r0[0] + w * (r1[0] - r0[0])) * xu[t];
        for (int k = (long)M < t ? M : (int)t; k >= 1; --k) acc = fma(-(r0[k] + w * (r1[k] - r0[k])), yu[t - k], acc);
        yu[t] = acc;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void poledf_generic_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ a, long B, long Tlen, long N,
                                                                int M, int P, int ignore_gain, T* __restrict__ uo, T* __restrict__ gx)
{
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= B) return;
    const int M1 = M + 1;
    const T* gu = gy + u * Tlen;
    const T* au = a + u * N * M1;
    T* uu = uo + u * Tlen;
    for (long t = Tlen - 1; t >= 0; --t) {
        T acc = gu[t];
        const long kmax = (long)M < Tlen - 1 - t ? M : Tlen - 1 - t;
        for (long k = kmax; k >= 1; --k) {
            const long tk = t + k, n = tk / P, n1 = n + 1 < N ? n + 1 : N - 1;
            const T w = (T)(tk - n * P) / (T)P;
            const T c = au[n * M1 + k] + w * (au[n1 * M1 + k] - au[n * M1 + k]);
            acc = fma(-c, uu[tk], acc);
        }
        uu[t] = acc;
        if (gx) {
            const long n = t / P, n1 = n + 1 < N ? n + 1 : N - 1;
            const T w = (T)(t - n * P) / (T)P;
            gx[u * Tlen + t] = ignore_gain ? acc : (au[n * M1] + w * (au[n1 * M1] - au[n * M1])) * acc;
        }
    }
}

// ga[n][k] = sum over the samples of frames n - 1 and n of wt(t) dc_t[k], wt the weight with which a[n] enters c_t (1 - w in
// frame n, w in frame n - 1, both in the last frame) -- the pattern of zerodf_bwd_b_kernel (csrc/zerodf.hip).  One wave per
// (utterance, frame), lane k per coefficient, the samples staged in LDS chunks; fixed summation order (deterministic).
template <typename T>
__global__ __launch_bounds__(64) void poledf_bwd_a_kernel(const T* __restrict__ uo, const T* __restrict__ x, const T* __restrict__ y,
                                                          long Tlen, long N, int M, int P, int ignore_gain, T* __restrict__ ga)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* gs = reinterpret_cast<T*>(smem_raw);   // [kPdCh]: wt u
    T* xs = gs + kPdCh;                       // [kPdCh]
    T* ys = xs + kPdCh;                       // [kPdCh + M]: y from t - M
    const int lane = threadIdx.x, M1 = M + 1;
    const long f = blockIdx.x;
    const long u = f / N, n = f - u * N;
    const long tbase = (n - 1) * P, len = 2 * (long)P;
    const T* uu = uo + u * Tlen;
    const T* xu = x + u * Tlen;
    const T* yu = y + u * Tlen;
    for (int k0 = 0; k0 <= M; k0 += 64) {
        const int k = k0 + lane;
        T acc = T(0);
        for (long c0 = 0; c0 < len; c0 += kPdCh) {
            const int cl = (int)(len - c0 < kPdCh ? len - c0 : kPdCh);
            __syncthreads();
            for (int i = lane; i < cl; i += 64) {
                const long t = tbase + c0 + i;
                T v = T(0), xv = T(0);
                if (t >= 0 && t < Tlen) {
                    const long nt = t < n * P ? n - 1 : n;
                    const long nt1 = nt + 1 < N ? nt + 1 : N - 1;
                    const T w = (T)(t - nt * P) / (T)P;
                    T wt = T(0);
                    if (nt == n) wt += T(1) - w;
                    if (nt1 == n) wt += w;
                    v = wt * uu[t];
                    xv = xu[t];
                }
                gs[i] = v;
                xs[i] = xv;
            }
            for (int i = lane; i < cl + M; i += 64) {
                const long t = tbase + c0 + i - M;
                ys[i] = (t >= 0 && t < Tlen) ? yu[t] : T(0);
            }
            __syncthreads();
            if (k == 0) {
                if (!ignore_gain)
#pragma unroll 8
                    for (int i = 0; i < cl; ++i) acc = fma(gs[i], xs[i], acc);
            } else if (k <= M) {
#pragma unroll 8
                for (int i = 0; i < cl; ++i) acc = fma(-gs[i], ys[i + M - k], acc);
            }
        }
        if (k <= M) ga[f * M1 + k] = acc;
    }
}

bool poledf_ring_ok(int M, int P) { return M >= 1 && M <= 63 && (long)(63 / P + 3) * (M + 1) <= 64 * kPdR; }

template <typename T>
int poledf_launch_fwd(const void* x, const void* a, int64_t B, int64_t Tlen, int64_t N, int M, int P, int ig, void* y, hipStream_t st)
{
    if (poledf_ring_ok(M, P)) {
        const int lds = (int)((2 * kPdE + 2 * 64 * kPdR) * sizeof(T));
        auto ring = [&](auto q) {   // q: the kernel's second parameter, by order bucket
            return launch_lds<poledf_ring_fwd_kernel<T, decltype(q)::value>>(lds > 48 * 1024 ? lds : 0, "poledf: cannot reserve LDS%s", dim3((unsigned)B),
                                                                             dim3(64), lds, st, (const T*)x, (const T*)a, (long)Tlen, (long)N, M, P, ig,
                                                                             (T*)y);
        };
        if (int rc = M <= 32 ? ring(int_c<32>{}) : M <= 48 ? ring(int_c<16>{}) : ring(int_c<1>{})) return rc;
        return check_launch("poledf_ring_fwd");
    }
    hipLaunchKernelGGL((poledf_generic_fwd_kernel<T>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (const T*)x, (const T*)a, (long)B,
                       (long)Tlen, (long)N, M, P, ig, (T*)y);
    return check_launch("poledf_generic_fwd");
}

template <typename T>
int poledf_launch_bwd(const void* gy, const void* x, const void* a, const void* y, int64_t B, int64_t Tlen, int64_t N, int M, int P, int ig,
                      void* uo, void* gx, void* ga, hipStream_t st)
{
    int rc;
    if (poledf_ring_ok(M, P)) {
        const int lds = (int)((2 * kPdE + 2 * 64 * kPdR) * sizeof(T));
        auto ring = [&](auto q) {
            return launch_lds<poledf_ring_bwd_kernel<T, decltype(q)::value>>(lds > 48 * 1024 ? lds : 0, "poledf_bwd: cannot reserve LDS%s",
                                                                             dim3((unsigned)B), dim3(64), lds, st, (const T*)gy, (const T*)a, (long)Tlen,
                                                                             (long)N, M, P, ig, (T*)uo, (T*)gx);
        };
        if (int rc2 = M <= 32 ? ring(int_c<32>{}) : M <= 48 ? ring(int_c<16>{}) : ring(int_c<1>{})) return rc2;
        rc = check_launch("poledf_ring_bwd");
    } else {
        hipLaunchKernelGGL((poledf_generic_bwd_kernel<T>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (const T*)gy, (const T*)a,
                           (long)B, (long)Tlen, (long)N, M, P, ig, (T*)uo, (T*)gx);
        rc = check_launch("poledf_generic_bwd");
    }
    if (rc != DSA_OK || !ga) return rc;
    const size_t lds = (3 * (size_t)kPdCh + M) * sizeof(T);
    hipLaunchKernelGGL((poledf_bwd_a_kernel<T>), dim3((unsigned)(B * N)), dim3(64), lds, st, (const T*)uo, (const T*)x, (const T*)y,
                       (long)Tlen, (long)N, M, P, ig, (T*)ga);
    return check_launch("poledf_bwd_a");
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_poledf_fwd(const void* x, const void* a, int64_t B, int64_t T, int32_t M, int32_t P, int32_t ignore_gain,
                              int32_t dtype, void* y, void* stream)
{
    DSA_REQUIRE(M >= 0 && M <= DSA_POLEDF_MAX_ORDER && P > 0 && B >= 0 && T >= 0, "poledf: invalid sizes");
    DSA_REQUIRE(T % P == 0, "poledf: the sequence length must be frames x frame_period");
    if (B * T == 0) return DSA_OK;
    DSA_REQUIRE(x && a && y, "poledf: null pointer");
    const int64_t N = T / P;
    return with_dtype(dtype, "poledf", [&](auto tag) {
        return poledf_launch_fwd<decltype(tag)>(x, a, B, T, N, M, P, ignore_gain, y, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_poledf_bwd(const void* gy, const void* x, const void* a, const void* y, int64_t B, int64_t T, int32_t M, int32_t P,
                              int32_t ignore_gain, int32_t dtype, void* u, void* gx, void* ga, void* stream)
{
    DSA_REQUIRE(M >= 0 && M <= DSA_POLEDF_MAX_ORDER && P > 0 && B >= 0 && T >= 0 && T % P == 0, "poledf_bwd: invalid sizes");
    if (B * T == 0) return DSA_OK;
    DSA_REQUIRE(gy && a && u, "poledf_bwd: gy, a and the u buffer are required");
    DSA_REQUIRE(!ga || (x && y), "poledf_bwd: ga needs the forward's x and y");
    const int64_t N = T / P;
    return with_dtype(dtype, "poledf_bwd", [&](auto tag) {
        return poledf_launch_bwd<decltype(tag)>(gy, x, a, y, B, T, N, M, P, ignore_gain, u, gx, ga, (hipStream_t)stream);
    });
}
