// LPC <-> PARCOR conversions and the LPC stability check (include/diffsptk_amd.h, section a14):
//   lpc2par   LinearPredictiveCoefficientsToParcorCoefficients._forward, lpc2par.py:103-120  (the step-down recursion)
//   par2lpc   ParcorCoefficientsToLinearPredictiveCoefficients._forward, par2lpc.py:101-107  (the step-up recursion)
//   lpccheck  LinearPredictiveCoefficientsStabilityCheck._forward, lpccheck.py:104-121       (step-down, clip, step-up)
// each forward and adjoint in one launch.
//
// Rows are [K, c_1 .. c_M].  With a^(m) the order-m predictor and k_m = a^(m)_m:
//   step-up    a^(m)_j   = a^(m-1)_j + k_m a^(m-1)_{m-j}                 j = 1 .. m-1
//   step-down  a^(m-1)_j = (a^(m)_j - k_m a^(m)_{m-j}) / (1 - k_m^2)
// Both run in place on one array: level m touches entries 1 .. m-1 only, entry m is k_m before and after.
//
// Layout: one frame per lane, the recursion in float64 registers whatever the data's dtype, as the Levinson stage of
// frame_window_lpc24_kernel (lpc24.hip): no cross-lane traffic.  A workgroup is one wave = 64 frames; their rows are one contiguous
// stretch of memory that is copied to LDS (odd row stride) with coalesced loads, and each lane then reads its own row.  The loops
// are unrolled to the order bucket NM (8, 16, 24, 32) and guarded by wave-uniform tests against M, so that every array index is a
// constant and the arrays stay in registers.  Orders above DSA_PARCOR_MAX_ORDER take one wave per frame with the row in LDS.
//
// The adjoints take the PARCOR row and nothing else from the forward:
//   lpc2par  needs a^(m-1) in ASCENDING m -- the order in which stepping up from k yields them;
//   par2lpc  needs a^(m-1) in DESCENDING m -- each one is recomputed by stepping up from k (O(M^3) multiply-adds per frame).
//            Stepping DOWN from the output instead would divide by 1 - k_m^2, which is zero exactly where lpccheck puts a
//            clipped coefficient (its default bound 1 - 1e-16 is 1 in float32).
#include "common.h"

namespace dsa {
namespace {

enum { PC_LPC2PAR_FWD = 0, PC_LPC2PAR_BWD, PC_PAR2LPC_FWD, PC_PAR2LPC_BWD, PC_CHECK_FWD, PC_CHECK_BWD };
const char* const kPcLaneNames[] = {"parcor_lane_lpc2par_fwd", "parcor_lane_lpc2par_bwd", "parcor_lane_par2lpc_fwd",
                                    "parcor_lane_par2lpc_bwd", "parcor_lane_lpccheck_fwd", "parcor_lane_lpccheck_bwd"};
const char* const kPcRowNames[] = {"parcor_row_lpc2par_fwd", "parcor_row_lpc2par_bwd", "parcor_row_par2lpc_fwd",
                                   "parcor_row_par2lpc_bwd", "parcor_row_lpccheck_fwd", "parcor_row_lpccheck_bwd"};

__device__ __forceinline__ double pc_clip(double v, double b) { return v < -b ? -b : (v > b ? b : v); }   // NaN passes, as torch.clip
__device__ __forceinline__ bool pc_inside(double v, double b) { return v >= -b && v <= b; }              // torch.clip's gradient mask

// ---------------------------------------------------------------------------------------------- one frame per lane
// (tiles of rows travel between global memory and LDS rows of stride S by wave_tile_in / wave_tile_out, common.h)
template <typename T, int NM>
__device__ __forceinline__ void pc_row_get(double (&v)[NM + 1], const T* lds, int S, int M, bool live)
{
#pragma unroll
    for (int j = 0; j <= NM; ++j) {
        v[j] = 0.0;
        if (j <= M) v[j] = live ? (double)lds[threadIdx.x * S + j] : 0.0;
    }
}
template <typename T, int NM>
__device__ __forceinline__ void pc_row_put(const double (&v)[NM + 1], T* lds, int S, int M)
{
#pragma unroll
    for (int j = 0; j <= NM; ++j)
        if (j <= M) lds[threadIdx.x * S + j] = (T)v[j];
}

// level m of the step-up recursion, in place on entries 1 .. m-1:  b <- b + km flip(b)
template <int NM>
__device__ __forceinline__ void pc_up_level(double (&b)[NM + 1], const int m, const double km)
{
#pragma unroll
    for (int j = 1; j <= NM / 2; ++j) {
        if (2 * j < m) {
            const double x = b[j], y = b[m - j];
            b[j] = fma(km, y, x);
            b[m - j] = fma(km, x, y);
        } else if (2 * j == m) {
            b[j] = fma(km, b[j], b[j]);
        }
    }
}
// level m of the step-down recursion, in place:  a <- (a - km flip(a)) rz,  rz = 1 / (1 - km^2)
template <int NM>
__device__ __forceinline__ void pc_down_level(double (&a)[NM + 1], const int m, const double km, const double rz)
{
#pragma unroll
    for (int j = 1; j <= NM / 2; ++j) {
        if (2 * j < m) {
            const double x = a[j], y = a[m - j];
            a[j] = fma(-km, y, x) * rz;
            a[m - j] = fma(-km, x, y) * rz;
        } else if (2 * j == m) {
            a[j] = fma(-km, a[j], a[j]) * rz;
        }
    }
}
template <int NM>
__device__ __forceinline__ void pc_step_up(double (&b)[NM + 1], int M)
{
#pragma unroll
    for (int m = 2; m <= NM; ++m)
        if (m <= M) pc_up_level<NM>(b, m, b[m]);
}
template <int NM>
__device__ __forceinline__ void pc_step_down(double (&a)[NM + 1], int M)
{
#pragma unroll
    for (int m = NM; m >= 2; --m)
        if (m <= M) {
            const double km = a[m];
            pc_down_level<NM>(a, m, km, 1.0 / fma(-km, km, 1.0));
        }
}
// the adjoint of the step-down recursion: g holds the cotangent of k = [., k_1 .. k_M] on entry and that of a^(M) on return
template <int NM>
__device__ __forceinline__ void pc_step_down_adj(const double (&k)[NM + 1], double (&g)[NM + 1], int M)
{
    double b[NM + 1];   // a^(m-1), stepped up beside the adjoint
#pragma unroll
    for (int j = 0; j <= NM; ++j) b[j] = k[j];
#pragma unroll
    for (int m = 2; m <= NM; ++m)
        if (m <= M) {
            const double km = k[m], rz = 1.0 / fma(-km, km, 1.0);
            double s = 0.0;   // d a^(m-1)_j / d k_m = (k_m a^(m-1)_j - a^(m-1)_{m-j}) rz
#pragma unroll
            for (int j = 1; j < NM; ++j)
                if (j < m) s = fma(g[j], fma(km, b[j], -b[m - j]), s);
            pc_down_level<NM>(g, m, km, rz);   // the recursion's matrix is symmetric: the same map on the cotangent
            g[m] = fma(s, rz, g[m]);
            pc_up_level<NM>(b, m, km);
        }
}
// the adjoint of the step-up recursion: g holds the cotangent of a^(M) on entry and that of k on return
template <int NM>
__device__ __forceinline__ void pc_step_up_adj(const double (&k)[NM + 1], double (&g)[NM + 1], int M)
{
#pragma unroll
    for (int m = NM; m >= 2; --m)
        if (m <= M) {
            double b[NM + 1];   // a^(m-1), stepped up from k
#pragma unroll
            for (int j = 0; j <= NM; ++j) b[j] = k[j];
#pragma unroll
            for (int l = 2; l < NM; ++l)
                if (l < m) pc_up_level<NM>(b, l, k[l]);
            double s = 0.0;
#pragma unroll
            for (int j = 1; j < NM; ++j)
                if (j < m) s = fma(g[j], b[m - j], s);
            pc_up_level<NM>(g, m, k[m]);
            g[m] += s;
        }
}

// in0 / in1 / out0 / out1 / p per OP:
//   LPC2PAR_FWD a  -  k   -  gamma        LPC2PAR_BWD gk   k  ga  -  gamma
//   PAR2LPC_FWD k  -  a   -  gamma        PAR2LPC_BWD ga   k  gk  -  gamma
//   CHECK_FWD   a  -  out k? bound        CHECK_BWD   gout k  ga  -  bound      (bound already rounded to T)
template <typename T, int NM, int OP>
__global__ __launch_bounds__(64) void parcor_lane_kernel(const T* __restrict__ in0, const T* __restrict__ in1, long F, int M, double p,
                                                         T* __restrict__ out0, T* __restrict__ out1, int* __restrict__ unstable)
{
    __shared__ T lds[64 * (NM + 2)];
    const int M1 = M + 1, S = M1 | 1;
    const long f0 = (long)blockIdx.x * 64;
    const int n = (int)(F - f0 < 64 ? F - f0 : 64);
    const int cnt = n * M1;
    const long base = f0 * M1;
    const bool live = (int)threadIdx.x < n;
    double v[NM + 1], k[NM + 1];

    wave_tile_in(lds, in0, base, cnt, M1, S);
    __syncthreads();
    pc_row_get<T, NM>(v, lds, S, M, live);
    if (OP == PC_LPC2PAR_BWD || OP == PC_PAR2LPC_BWD || OP == PC_CHECK_BWD) {
        __syncthreads();
        wave_tile_in(lds, in1, base, cnt, M1, S);
        __syncthreads();
        pc_row_get<T, NM>(k, lds, S, M, live);
    }

    if (OP == PC_LPC2PAR_FWD) {
#pragma unroll
        for (int j = 1; j <= NM; ++j) v[j] *= p;
        pc_step_down<NM>(v, M);
    } else if (OP == PC_LPC2PAR_BWD) {
        pc_step_down_adj<NM>(k, v, M);
#pragma unroll
        for (int j = 1; j <= NM; ++j) v[j] *= p;
    } else if (OP == PC_PAR2LPC_FWD) {
        pc_step_up<NM>(v, M);
        if (p != 1.0) {
#pragma unroll
            for (int j = 0; j <= NM; ++j) v[j] /= p;   // the whole row, K included (par2lpc.py:102)
        }
    } else if (OP == PC_PAR2LPC_BWD) {
        if (p != 1.0) {
#pragma unroll
            for (int j = 0; j <= NM; ++j) v[j] /= p;
        }
        pc_step_up_adj<NM>(k, v, M);
    } else if (OP == PC_CHECK_FWD) {
        pc_step_down<NM>(v, M);
        bool bad = false;
#pragma unroll
        for (int j = 1; j <= NM; ++j) {
            v[j] = (double)(T)v[j];   // the PARCOR in the data's dtype: what the reference clips and what the backward reads
            bad = bad || fabs(v[j]) >= 1.0;
        }
        if (unstable && live && bad) *unstable = 1;
        if (out1) {
            __syncthreads();
            pc_row_put<T, NM>(v, lds, S, M);
            __syncthreads();
            wave_tile_out(lds, out1, base, cnt, M1, S);
        }
#pragma unroll
        for (int j = 1; j <= NM; ++j) v[j] = pc_clip(v[j], p);
        pc_step_up<NM>(v, M);
    } else {
        double kc[NM + 1];
#pragma unroll
        for (int j = 0; j <= NM; ++j) kc[j] = pc_clip(k[j], p);
        pc_step_up_adj<NM>(kc, v, M);
#pragma unroll
        for (int j = 1; j <= NM; ++j) v[j] = pc_inside(k[j], p) ? v[j] : 0.0;
        pc_step_down_adj<NM>(k, v, M);
    }

    __syncthreads();
    pc_row_put<T, NM>(v, lds, S, M);
    __syncthreads();
    wave_tile_out(lds, out0, base, cnt, M1, S);
}

// ---------------------------------------------------------------------------------------------- one frame per wave, the row in LDS
// Every helper is called by the whole (one-wave) workgroup; j is spread over the lanes.  t is a row of temporary space.
__device__ __forceinline__ void pr_up_level(double* b, double* t, int m, double km)
{
    for (int j = 1 + threadIdx.x; j < m; j += 64) t[j] = fma(km, b[m - j], b[j]);
    __syncthreads();
    for (int j = 1 + threadIdx.x; j < m; j += 64) b[j] = t[j];
    __syncthreads();
}
__device__ __forceinline__ void pr_down_level(double* a, double* t, int m, double km, double rz)
{
    for (int j = 1 + threadIdx.x; j < m; j += 64) t[j] = fma(-km, a[m - j], a[j]) * rz;
    __syncthreads();
    for (int j = 1 + threadIdx.x; j < m; j += 64) a[j] = t[j];
    __syncthreads();
}
__device__ __forceinline__ void pr_step_up(double* b, double* t, int M)
{
    for (int m = 2; m <= M; ++m) pr_up_level(b, t, m, b[m]);
}
__device__ __forceinline__ void pr_step_down(double* a, double* t, int M)
{
    for (int m = M; m >= 2; --m) {
        const double km = a[m];
        pr_down_level(a, t, m, km, 1.0 / fma(-km, km, 1.0));
    }
}
__device__ __forceinline__ void pr_step_down_adj(const double* k, double* g, double* b, double* t, int M)
{
    for (int j = threadIdx.x; j <= M; j += 64) b[j] = k[j];
    __syncthreads();
    for (int m = 2; m <= M; ++m) {
        const double km = k[m], rz = 1.0 / fma(-km, km, 1.0);
        double s = 0.0;
        for (int j = 1 + threadIdx.x; j < m; j += 64) s = fma(g[j], fma(km, b[j], -b[m - j]), s);
        s = wave_sum(s);
        pr_down_level(g, t, m, km, rz);
        if (threadIdx.x == 0) g[m] = fma(s, rz, g[m]);
        pr_up_level(b, t, m, km);
    }
}
__device__ __forceinline__ void pr_step_up_adj(const double* k, double* g, double* b, double* t, int M)
{
    for (int m = M; m >= 2; --m) {
        for (int j = threadIdx.x; j < m; j += 64) b[j] = k[j];
        __syncthreads();
        for (int l = 2; l < m; ++l) pr_up_level(b, t, l, k[l]);
        double s = 0.0;
        for (int j = 1 + threadIdx.x; j < m; j += 64) s = fma(g[j], b[m - j], s);
        s = wave_sum(s);
        pr_up_level(g, t, m, k[m]);
        if (threadIdx.x == 0) g[m] += s;
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(64) void parcor_row_kernel(int op, const T* __restrict__ in0, const T* __restrict__ in1, long F, int M,
                                                        double p, T* __restrict__ out0, T* __restrict__ out1,
                                                        int* __restrict__ unstable)
{
    extern __shared__ double pc_rows[];
    const int M1 = M + 1;
    double *v = pc_rows, *k = v + M1, *b = k + M1, *t = b + M1;
    const bool two = op == PC_LPC2PAR_BWD || op == PC_PAR2LPC_BWD || op == PC_CHECK_BWD;
    for (long f = blockIdx.x; f < F; f += gridDim.x) {
        const long base = f * M1;
        __syncthreads();
        for (int j = threadIdx.x; j <= M; j += 64) {
            v[j] = (double)in0[base + j];
            if (two) k[j] = (double)in1[base + j];
        }
        __syncthreads();
        if (op == PC_LPC2PAR_FWD) {
            for (int j = 1 + threadIdx.x; j <= M; j += 64) v[j] *= p;
            __syncthreads();
            pr_step_down(v, t, M);
        } else if (op == PC_LPC2PAR_BWD) {
            pr_step_down_adj(k, v, b, t, M);
            for (int j = 1 + threadIdx.x; j <= M; j += 64) v[j] *= p;
        } else if (op == PC_PAR2LPC_FWD) {
            pr_step_up(v, t, M);
            if (p != 1.0)
                for (int j = threadIdx.x; j <= M; j += 64) v[j] /= p;
        } else if (op == PC_PAR2LPC_BWD) {
            if (p != 1.0)
                for (int j = threadIdx.x; j <= M; j += 64) v[j] /= p;
            __syncthreads();
            pr_step_up_adj(k, v, b, t, M);
        } else if (op == PC_CHECK_FWD) {
            pr_step_down(v, t, M);
            bool bad = false;
            for (int j = 1 + threadIdx.x; j <= M; j += 64) {
                v[j] = (double)(T)v[j];
                bad = bad || fabs(v[j]) >= 1.0;
                if (out1) out1[base + j] = (T)v[j];
                v[j] = pc_clip(v[j], p);
            }
            if (out1 && threadIdx.x == 0) out1[base] = (T)v[0];
            if (unstable && bad) *unstable = 1;
            __syncthreads();
            pr_step_up(v, t, M);
        } else {
            double* kc = b;   // the clipped row; pr_step_up_adj's own a^(m-1) then goes to a fifth row
            double* b2 = t + M1;
            for (int j = threadIdx.x; j <= M; j += 64) kc[j] = j ? pc_clip(k[j], p) : k[j];
            __syncthreads();
            pr_step_up_adj(kc, v, b2, t, M);
            for (int j = 1 + threadIdx.x; j <= M; j += 64) v[j] = pc_inside(k[j], p) ? v[j] : 0.0;
            __syncthreads();
            pr_step_down_adj(k, v, b2, t, M);
        }
        __syncthreads();
        for (int j = threadIdx.x; j <= M; j += 64) out0[base + j] = (T)v[j];
    }
}

template <typename T, int OP>
int parcor_launch_t(const void* in0, const void* in1, int64_t F, int M, double p, void* out0, void* out1, void* unstable, hipStream_t st)
{
    if (OP == PC_CHECK_FWD || OP == PC_CHECK_BWD) p = (double)(T)p;   // torch.clip with a Python scalar: the bound in the data's dtype
    if (M <= DSA_PARCOR_MAX_ORDER) {
        const dim3 grid((unsigned)((F + 63) / 64));
#define DSA_PC_LANE(NM)                                                                                                               \
    hipLaunchKernelGGL((parcor_lane_kernel<T, NM, OP>), grid, dim3(64), 0, st, (const T*)in0, (const T*)in1, (long)F, M, p, (T*)out0, \
                       (T*)out1, (int*)unstable)
        if (M <= 8) DSA_PC_LANE(8);
        else if (M <= 16) DSA_PC_LANE(16);
        else if (M <= 24) DSA_PC_LANE(24);
        else DSA_PC_LANE(32);
#undef DSA_PC_LANE
        return check_launch(kPcLaneNames[OP]);
    }
    const size_t lds = 5 * (size_t)(M + 1) * sizeof(double);
    const int64_t blocks = F < (1 << 20) ? F : (1 << 20);
    hipLaunchKernelGGL((parcor_row_kernel<T>), dim3((unsigned)blocks), dim3(64), lds, st, OP, (const T*)in0, (const T*)in1, (long)F, M, p,
                       (T*)out0, (T*)out1, (int*)unstable);
    return check_launch(kPcRowNames[OP]);
}

template <int OP>
int parcor_launch(const char* what, const void* in0, const void* in1, bool two, int64_t F, int32_t M, double p, int32_t dtype, void* out0,
                  void* out1, void* unstable, void* stream)
{
    if (!(F >= 0 && M >= 0 && M <= DSA_PARCOR_ROW_MAX_ORDER)) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: invalid sizes", what);
    if (F == 0) return DSA_OK;
    if (!(in0 && out0 && (!two || in1))) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    return with_dtype(dtype, what, [&](auto tag) {
        return parcor_launch_t<decltype(tag), OP>(in0, in1, F, M, p, out0, out1, unstable, (hipStream_t)stream);
    });
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_lpc2par_fwd(const void* a, int64_t F, int32_t M, double gamma, int32_t dtype, void* k, void* stream)
{
    return parcor_launch<PC_LPC2PAR_FWD>("lpc2par_fwd", a, nullptr, false, F, M, gamma, dtype, k, nullptr, nullptr, stream);
}

DSA_EXPORT int dsa_lpc2par_bwd(const void* gk, const void* k, int64_t F, int32_t M, double gamma, int32_t dtype, void* ga, void* stream)
{
    return parcor_launch<PC_LPC2PAR_BWD>("lpc2par_bwd", gk, k, true, F, M, gamma, dtype, ga, nullptr, nullptr, stream);
}

DSA_EXPORT int dsa_par2lpc_fwd(const void* k, int64_t F, int32_t M, double gamma, int32_t dtype, void* a, void* stream)
{
    return parcor_launch<PC_PAR2LPC_FWD>("par2lpc_fwd", k, nullptr, false, F, M, gamma, dtype, a, nullptr, nullptr, stream);
}

DSA_EXPORT int dsa_par2lpc_bwd(const void* ga, const void* k, int64_t F, int32_t M, double gamma, int32_t dtype, void* gk, void* stream)
{
    return parcor_launch<PC_PAR2LPC_BWD>("par2lpc_bwd", ga, k, true, F, M, gamma, dtype, gk, nullptr, nullptr, stream);
}

DSA_EXPORT int dsa_lpccheck_fwd(const void* a, int64_t F, int32_t M, double bound, int32_t dtype, void* out, void* k, int32_t* unstable,
                                void* stream)
{
    return parcor_launch<PC_CHECK_FWD>("lpccheck_fwd", a, nullptr, false, F, M, bound, dtype, out, k, unstable, stream);
}

DSA_EXPORT int dsa_lpccheck_bwd(const void* gout, const void* k, int64_t F, int32_t M, double bound, int32_t dtype, void* ga, void* stream)
{
    return parcor_launch<PC_CHECK_BWD>("lpccheck_bwd", gout, k, true, F, M, bound, dtype, ga, nullptr, nullptr, stream);
}
