// Toeplitz-plus-Hankel solve of the mel-generalized cepstral analysis:
//   MelGeneralizedCepstralAnalysis.forward, mgcep.py:226-229:  R = symmetric_toeplitz(pt), Q = hankel(qt),
//   gradient = torch.linalg.solve(R + Q, rt)     (utils/private.py:291-302 for the two builders).
// One wave per frame: the M x (M + 1) augmented system lives in LDS, lane i owns row i; Gauss-Jordan elimination
// with row pivoting by magnitude (the reference's LAPACK call pivots too; the system is not guaranteed positive
// definite for gamma != 0).  Backward: with A = T(p) + H(q) symmetric, u = A^{-1} gbar, rbar = u, Abar = -u g^T,
// pbar[k] = sum over |i - j| = k of Abar[i][j], qbar[k] = sum over i + j = k.  float32 and float64; M <= 64.
// The rest of the analysis (warping / FFT stages composed into row products, pointwise spectrum arithmetic) is
// assembled by the host layer from the library's row-product kernel (modules/mgcep.py).
#include "common.h"
#include "th_solve_reg.h"

#include <cstdlib>

namespace dsa {

constexpr int kThMax = 64;

// Solves the n x n system in LDS (row stride W >= n + nrhs) for nrhs right-hand sides; on return column n + c of row
// piv_row[k] divided by its pivot is x_c[k].  One wave, lane i owns row i (n <= 64).
template <typename T>
__device__ void th_gauss_jordan(T* Aug, int n, int W, int nrhs, int* rowof, int lane)
{
    unsigned long long used = 0ull;   // rows already chosen as pivots (uniform)
    for (int k = 0; k < n; ++k) {
        // pivot: the unused row with the largest |Aug[i][k]|
        T mag = (lane < n && !((used >> lane) & 1ull)) ? (Aug[lane * W + k] < T(0) ? -Aug[lane * W + k] : Aug[lane * W + k]) : T(-1);
        int arg = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const T m2 = __shfl_xor(mag, o, 64);
            const int a2 = __shfl_xor(arg, o, 64);
            if (m2 > mag || (m2 == mag && a2 < arg)) {
                mag = m2;
                arg = a2;
            }
        }
        const int p = arg;   // uniform
        used |= 1ull << p;
        if (lane == 0) rowof[k] = p;
        const T inv = T(1) / Aug[p * W + k];
        const T fac = (lane < n && lane != p) ? Aug[lane * W + k] * inv : T(0);
        __builtin_amdgcn_wave_barrier();
        if (lane < n && lane != p)
            for (int j = k + 1; j < n + nrhs; ++j) Aug[lane * W + j] -= fac * Aug[p * W + j];
        __builtin_amdgcn_wave_barrier();
    }
}

template <typename T>
__device__ void th_build(T* Aug, const T* p, const T* q, int n, int W, int lane)
{
    if (lane < n)
        for (int j = 0; j < n; ++j) {
            const int d = lane > j ? lane - j : j - lane;
            Aug[lane * W + j] = p[d] + q[lane + j];
        }
}

template <typename T, int NMAX = 0>   // NMAX > 0: register version (n <= NMAX)
__global__ __launch_bounds__(64) void th_solve_fwd_kernel(const T* __restrict__ p, const T* __restrict__ q,
                                                          const T* __restrict__ r, long F, int n, T* __restrict__ g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* Aug = reinterpret_cast<T*>(smem_raw);
    const int W = n + 1;
    int* rowof = reinterpret_cast<int*>(Aug + (size_t)n * W);
    const int lane = threadIdx.x;
    for (long f = blockIdx.x; f < F; f += gridDim.x) {
        __builtin_amdgcn_wave_barrier();
        if (NMAX > 0) {
            T* ps = Aug;          // [n]
            T* qs = Aug + n;      // [2n - 1]
            if (lane < n) ps[lane] = p[f * n + lane];
            for (int i = lane; i < 2 * n - 1; i += 64) qs[i] = q[f * (2 * n - 1) + i];
            const T rhs = lane < n ? r[f * n + lane] : T(0);
            __builtin_amdgcn_wave_barrier();
            int col;
            T sol;
            th_solve_reg<T, (NMAX > 0 ? NMAX : 1)>(ps, qs, rhs, n, lane, col, sol);
            if (lane < n) g[f * n + col] = sol;
            continue;
        }
        th_build(Aug, p + f * n, q + f * (2 * n - 1), n, W, lane);
        if (lane < n) Aug[lane * W + n] = r[f * n + lane];
        __builtin_amdgcn_wave_barrier();
        th_gauss_jordan(Aug, n, W, 1, rowof, lane);
        if (lane < n) {
            const int row = rowof[lane];
            g[f * n + lane] = Aug[row * W + n] / Aug[row * W + lane];
        }
    }
}

template <typename T, int NMAX = 0>
__global__ __launch_bounds__(64) void th_solve_bwd_kernel(const T* __restrict__ gg, const T* __restrict__ p,
                                                          const T* __restrict__ q, const T* __restrict__ g, long F, int n,
                                                          T* __restrict__ gp, T* __restrict__ gq, T* __restrict__ gr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* Aug = reinterpret_cast<T*>(smem_raw);
    const int W = n + 1;
    int* rowof = reinterpret_cast<int*>(Aug + (size_t)n * W);
    T* u = reinterpret_cast<T*>(rowof + kThMax);
    T* gs = u + kThMax;
    const int lane = threadIdx.x;
    for (long f = blockIdx.x; f < F; f += gridDim.x) {
        __builtin_amdgcn_wave_barrier();
        if (NMAX > 0) {
            T* ps = Aug;
            T* qs = Aug + n;
            if (lane < n) {
                ps[lane] = p[f * n + lane];
                gs[lane] = g[f * n + lane];
            }
            for (int i = lane; i < 2 * n - 1; i += 64) qs[i] = q[f * (2 * n - 1) + i];
            const T rhs = lane < n ? gg[f * n + lane] : T(0);   // A is symmetric: u = A^{-T} gbar = A^{-1} gbar
            __builtin_amdgcn_wave_barrier();
            int col;
            T sol;
            th_solve_reg<T, (NMAX > 0 ? NMAX : 1)>(ps, qs, rhs, n, lane, col, sol);
            if (lane < n) {
                u[col] = sol;
                gr[f * n + col] = sol;
            }
        } else {
            th_build(Aug, p + f * n, q + f * (2 * n - 1), n, W, lane);
            if (lane < n) {
                Aug[lane * W + n] = gg[f * n + lane];   // A is symmetric: u = A^{-T} gbar = A^{-1} gbar
                gs[lane] = g[f * n + lane];
            }
            __builtin_amdgcn_wave_barrier();
            th_gauss_jordan(Aug, n, W, 1, rowof, lane);
            if (lane < n) {
                const int row = rowof[lane];
                const T ul = Aug[row * W + n] / Aug[row * W + lane];
                u[lane] = ul;
                gr[f * n + lane] = ul;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // Abar = -u g^T on the Toeplitz diagonals |i - j| = k (k < n) and the Hankel anti-diagonals i + j = k (k < 2n-1)
        for (int k = lane; k < 2 * n - 1; k += 64) {
            T sq = 0;
            const int lo = k - (n - 1) > 0 ? k - (n - 1) : 0, hi = k < n - 1 ? k : n - 1;
            for (int i = lo; i <= hi; ++i) sq -= u[i] * gs[k - i];
            gq[f * (2 * n - 1) + k] = sq;
            if (k < n) {
                T sp = 0;
                for (int i = 0; i + k < n; ++i) sp -= u[i] * gs[i + k] + (k > 0 ? u[i + k] * gs[i] : T(0));
                gp[f * n + k] = sp;
            }
        }
    }
}

// Cotangents of the Toeplitz column p and the Hankel sequence q from u = A^{-1} gbar and the forward's solution g:
// Abar = -u g^T summed along the diagonals |i - j| = k and the anti-diagonals i + j = k.  64 threads per system.
__global__ __launch_bounds__(256) void th_bwd_sums_kernel(const float* __restrict__ u, const float* __restrict__ g, long F, int n,
                                                         float* __restrict__ gp, float* __restrict__ gq)
{
    __shared__ float us[4][64], gs[4][64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long f = (long)blockIdx.x * 4 + w;
    const bool ok = f < F;
    us[w][lane] = ok && lane < n ? u[f * n + lane] : 0.f;
    gs[w][lane] = ok && lane < n ? g[f * n + lane] : 0.f;
    __syncthreads();
    if (!ok) return;
    for (int k = lane; k < 2 * n - 1; k += 64) {
        float sq = 0.f;
        const int lo = k - (n - 1) > 0 ? k - (n - 1) : 0, hi = k < n - 1 ? k : n - 1;
        for (int i = lo; i <= hi; ++i) sq -= us[w][i] * gs[w][k - i];
        gq[f * (2 * n - 1) + k] = sq;
        if (k < n) {
            float sp = 0.f;
            for (int i = 0; i + k < n; ++i) sp -= us[w][i] * gs[w][i + k] + (k > 0 ? us[w][i + k] * gs[w][i] : 0.f);
            gp[f * n + k] = sp;
        }
    }
}

template <typename T>
static int th_launch(bool bwd, const void* gg, const void* p, const void* q, const void* r_or_g, int64_t F, int n, void* o1,
                     void* o2, void* o3, hipStream_t st)
{
    const size_t lds = sizeof(T) * ((size_t)n * (n + 1) + 2 * kThMax) + sizeof(int) * kThMax;
    long grid = F < 256L * 16 ? (long)F : 256L * 16;
#define DSA_TH_LAUNCH(NM)                                                                                                  \
    do {                                                                                                                   \
        if (!bwd)                                                                                                          \
            hipLaunchKernelGGL((th_solve_fwd_kernel<T, NM>), dim3((unsigned)grid), dim3(64), lds, st, (const T*)p, (const T*)q, \
                               (const T*)r_or_g, (long)F, n, (T*)o1);                                                      \
        else                                                                                                               \
            hipLaunchKernelGGL((th_solve_bwd_kernel<T, NM>), dim3((unsigned)grid), dim3(64), lds, st, (const T*)gg, (const T*)p, \
                               (const T*)q, (const T*)r_or_g, (long)F, n, (T*)o1, (T*)o2, (T*)o3);                         \
    } while (0)
    if (n <= 24) DSA_TH_LAUNCH(24);
    else if (n <= 32) DSA_TH_LAUNCH(32);
    else if (n <= 48) DSA_TH_LAUNCH(48);   // the orders of the 48 kHz set-ups (34 .. 60): rows in registers too
    else if (n <= 64) DSA_TH_LAUNCH(64);
    else DSA_TH_LAUNCH(0);
#undef DSA_TH_LAUNCH
    return check_launch(bwd ? "th_solve_bwd" : "th_solve_fwd");
}

}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_thsolve_fwd(const void* p, const void* q, const void* r, int64_t F, int32_t n, int32_t dtype, void* g,
                               void* stream)
{
    DSA_REQUIRE(n >= 1 && n <= kThMax && F >= 0, "thsolve: order must be in [1, 64]");
    if (F == 0) return DSA_OK;
    // cepstral order 24, float32: the unpivoted quad-layout solve of the mel-cepstral kernels (DSA_THSOLVE_QUAD=0: A/B)
    const bool quad = env_int("DSA_THSOLVE_QUAD", 1) != 0;
    if (dtype == DSA_F32 && n == 24 && quad && F > 0) return thsolve_quad24_fwd(p, q, r, F, g, (hipStream_t)stream);
    // other orders up to 55, float32: the same scheme as a template over the size -- chosen from (n, dtype) ALONE, like
    // dsa_mcep_newton_update: a frame's rounding must not depend on how many frames travel with it (round 6: the F >= 64 test is gone)
    if (dtype == DSA_F32 && n >= 2 && n <= 55 && quad && F > 0)
        return thsolve_quadn_fwd(p, n, q, 2 * n - 1, r, n, nullptr, nullptr, F, n, g, (hipStream_t)stream);
    return with_dtype(dtype, "thsolve", [&](auto tag) {
        return th_launch<decltype(tag)>(false, nullptr, p, q, r, F, n, g, nullptr, nullptr, (hipStream_t)stream);
    });
}

// mcep.py:216-222 for the geometries without a tuned kernel: mc_out = mc_in + solve(T(rt[:n]) + H(rt), rt[:n] - alpha_vec), rt:(F, 2n-1)
DSA_EXPORT int dsa_mcep_newton_update(const void* rt, int64_t F, int32_t n, const void* alpha_vec, int32_t dtype, const void* mc_in,
                                      void* mc_out, void* stream)
{
    DSA_REQUIRE(n >= 2 && n <= 55 && F >= 0, "mcep_newton_update: order must be in [2, 55]");
    DSA_REQUIRE(F == 0 || (rt && alpha_vec && mc_out), "mcep_newton_update: null pointer");   // mc_in = NULL: the solution alone
    if (dtype != DSA_F32) return fail(DSA_ERR_UNSUPPORTED, "mcep_newton_update: float32 only%s");
    if (F == 0) return DSA_OK;
    return thsolve_quadn_fwd(rt, 2 * n - 1, rt, 2 * n - 1, rt, 2 * n - 1, alpha_vec, mc_in, F, n, mc_out, (hipStream_t)stream);
}

// Cotangent of rt from the cotangent of the solution s = solve(T(rt[:n]) + H(rt), rt[:n] - alpha_vec):
//   u = A^-1 gs (A is symmetric: the same batched solve), then per system
//   grt[k] = -sum_{i + j = k} u_i s_j  -  [k < n] sum_{|i - j| = k} u_i s_j  +  [k < n] u_k      (Hankel, Toeplitz, right-hand side)
namespace dsa {
// Round 6: the sums with ONE FRAME PER LANE, everything in registers.  The round-5 kernel gave a wave to a frame and a lane one or two
// of its 2 n - 1 sums, every multiply-add behind two LDS reads (143 us per 102 400 frames of order 49: a tenth of the 48 kHz analysis'
// forward + backward).  Here a lane loads its frame's u and s rows (zero-padded to NMAX), runs the three sums fully unrolled at compile
// time -- 2 NMAX^2 + NMAX multiply-adds, no memory access, no cross-lane operation -- and stores four results at a time.  The rows of a
// wave's 64 consecutive frames are one contiguous block, so the per-lane 16-byte accesses use every byte of the lines they touch.
// sums k = K4 .. K4 + 3 of a lane's frame, then the next group: a compile-time recursion (as a loop of 28 x 450 instructions the unroller
// gives up and the arrays live in private memory)
template <int NMAX, int K4>
__device__ __forceinline__ void sums_lane_groups(const float (&uu)[NMAX], const float (&sv)[NMAX], float* orow, int nout)
{
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    if constexpr (K4 < 2 * NMAX - 1) {
        if (K4 < nout) {   // (uniform)
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = K4 + e;
                float acc = 0.f;
                if (k < 2 * NMAX - 1) {
                    // Hankel: sum_{i + j = k} u_i s_j (zero padding makes the sum over the padded range the sum over the order's)
#pragma unroll
                    for (int i = (k - (NMAX - 1) > 0 ? k - (NMAX - 1) : 0); i <= (k < NMAX - 1 ? k : NMAX - 1); ++i) acc = __builtin_fmaf(-uu[i], sv[k - i], acc);
                    if (k < NMAX) {
                        // Toeplitz: sum_{|i - j| = k} u_i s_j, and the right-hand side's u_k (u_k = 0 from the order on)
#pragma unroll
                        for (int i = 0; i + k < NMAX; ++i) {
                            acc = __builtin_fmaf(-uu[i], sv[i + k], acc);
                            if (k > 0) acc = __builtin_fmaf(-uu[i + k], sv[i], acc);
                        }
                        acc += uu[k];
                    }
                }
                o[e] = acc;
            }
            if (K4 + 3 < nout) {
                *reinterpret_cast<f4u*>(orow + K4) = f4u{o[0], o[1], o[2], o[3]};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (K4 + e < nout) orow[K4 + e] = o[e];
            }
            sums_lane_groups<NMAX, K4 + 4>(uu, sv, orow, nout);
        }
    }
}

template <int NMAX>
__global__ __launch_bounds__(256) void newton_update_bwd_sums_lane_kernel(const float* __restrict__ u, const float* __restrict__ s, long F, int n,
                                                                         float* __restrict__ grt)
{
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float* ur = u + f * n;
    const float* sr = s + f * n;
    float uu[NMAX], sv[NMAX];
#pragma unroll
    for (int i4 = 0; i4 < NMAX; i4 += 4) {
        // (the group's values first, the array elements assigned unconditionally afterwards: element assignments on conditional paths keep
        //  the arrays in private memory)
        f4u a, b;
        if (i4 + 3 < n) {   // (uniform)
            a = *reinterpret_cast<const f4u*>(ur + i4);
            b = *reinterpret_cast<const f4u*>(sr + i4);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = i4 + e < n ? ur[i4 + e] : 0.f;
                b[e] = i4 + e < n ? sr[i4 + e] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { uu[i4 + e] = a[e]; sv[i4 + e] = b[e]; }
    }
    float* orow = grt + f * (2 * n - 1);
    sums_lane_groups<NMAX, 0>(uu, sv, orow, 2 * n - 1);
}
}  // namespace dsa

DSA_EXPORT int dsa_mcep_newton_update_bwd(const void* gs, const void* rt, const void* sol, int64_t F, int32_t n, int32_t dtype, void* u,
                                          void* grt, void* stream)
{
    DSA_REQUIRE(n >= 2 && n <= 55 && F >= 0, "mcep_newton_update_bwd: order must be in [2, 55]");
    DSA_REQUIRE(F == 0 || (gs && rt && sol && u && grt), "mcep_newton_update_bwd: null pointer");
    if (dtype != DSA_F32) return fail(DSA_ERR_UNSUPPORTED, "mcep_newton_update_bwd: float32 only%s");
    if (F == 0) return DSA_OK;
    if (int rc = thsolve_quadn_fwd(rt, 2 * n - 1, rt, 2 * n - 1, gs, n, nullptr, nullptr, F, n, u, (hipStream_t)stream)) return rc;
    // one frame per lane (round 6), whatever the batch: the two kernels sum in different orders, and a frame's bits must not depend on
    // how many frames travel with it
    const dim3 g((unsigned)((F + 255) / 256));
    if (n <= 36)
        hipLaunchKernelGGL((dsa::newton_update_bwd_sums_lane_kernel<36>), g, dim3(256), 0, (hipStream_t)stream, (const float*)u, (const float*)sol,
                           (long)F, (int)n, (float*)grt);
    else
        hipLaunchKernelGGL((dsa::newton_update_bwd_sums_lane_kernel<56>), g, dim3(256), 0, (hipStream_t)stream, (const float*)u, (const float*)sol,
                           (long)F, (int)n, (float*)grt);
    return dsa::check_launch("mcep_newton_update_bwd");
}

DSA_EXPORT int dsa_thsolve_update_fwd(const void* p, const void* q, const void* r, int64_t r_stride, int64_t r_offset, int64_t F,
                                      int32_t n, int32_t dtype, const void* b_in, void* b_out, void* stream)
{
    DSA_REQUIRE(n >= 1 && n <= kThMax && F >= 0, "thsolve_update: order must be in [1, 64]");
    DSA_REQUIRE(r_offset >= 0 && r_stride >= r_offset + n, "thsolve_update: the right-hand side does not fit its row stride");
    DSA_REQUIRE(F == 0 || (b_in != nullptr && b_out != nullptr && b_in != b_out), "thsolve_update: b_in and b_out must be distinct buffers");
    if (F == 0) return DSA_OK;
    if (dtype == DSA_F32 && n == 24)
        return thsolve_quad24_fwd(p, q, r, F, b_out, (hipStream_t)stream, (int)r_stride, (int)r_offset, b_in);
    return fail(DSA_ERR_UNSUPPORTED, "thsolve_update: order 24 in float32 only (dsa_thsolve_fwd + an addition otherwise)%s");
}

DSA_EXPORT int dsa_thsolve_bwd(const void* gg, const void* p, const void* q, const void* g, int64_t F, int32_t n,
                               int32_t dtype, void* gp, void* gq, void* gr, void* stream)
{
    DSA_REQUIRE(n >= 1 && n <= kThMax && F >= 0, "thsolve_bwd: order must be in [1, 64]");
    if (F == 0) return DSA_OK;
    // order 24, float32: u = A^{-1} gbar on the quad-layout solve (A is symmetric; marked systems re-solved with pivoting as in
    // the forward), then the diagonal sums (DSA_THSOLVE_QUAD=0: the one-wave-per-system kernel, A/B)
    const bool quad = env_int("DSA_THSOLVE_QUAD", 1) != 0;
    if (dtype == DSA_F32 && n == 24 && quad && gp && gq && gr) {
        if (int rc = thsolve_quad24_fwd(p, q, gg, F, gr, (hipStream_t)stream)) return rc;
        hipLaunchKernelGGL(th_bwd_sums_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float*)gr,
                           (const float*)g, (long)F, (int)n, (float*)gp, (float*)gq);
        return check_launch("th_solve_quad_bwd");
    }
    // the other orders the batched forward covers (csrc/thsolve_quad.hip: 2 .. 55, batches from 64 systems): the same two launches.
    // (The one-wave-per-system backward -- a second pivoted elimination per system -- took 220 us per 12 800 systems of order 50,
    // 37 % of a forward + backward of the 48 kHz analysis; this takes 39 + 7.)
    if (dtype == DSA_F32 && n >= 2 && n <= 55 && n != 24 && F > 0 && quad && gp && gq && gr) {
        if (int rc = thsolve_quadn_fwd(p, n, q, 2 * n - 1, gg, n, nullptr, nullptr, F, n, gr, (hipStream_t)stream)) return rc;
        hipLaunchKernelGGL(th_bwd_sums_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float*)gr,
                           (const float*)g, (long)F, (int)n, (float*)gp, (float*)gq);
        return check_launch("th_solve_quadn_bwd");
    }
    return with_dtype(dtype, "thsolve_bwd", [&](auto tag) {
        return th_launch<decltype(tag)>(true, gg, p, q, g, F, n, gp, gq, gr, (hipStream_t)stream);
    });
}
