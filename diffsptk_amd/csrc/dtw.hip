// Dynamic time warping with a soft minimum (include/diffsptk_amd.h, section a20):
//   dtw       DynamicTimeWarping._forward, dtw.py:301-338, and the forward loop of its core, dtw.py:44-104   (there: T1 T2 Python
//             iterations of a handful of one-element tensor operations each, on a (B, T1, T2) distance matrix from cdist; B = 1 only)
//   dtw_vjp   the autograd-derived backward of the same, in closed form as a reverse sweep
//   dtw_path  the backtracking of dtw.py:106-123, on back-pointers recomputed from the saved tables
//
// One workgroup per pair (x_b:(T1, D), y_b:(T2, D)); x_b is staged in LDS once.  The cells of an anti-diagonal s = i + j do not depend
// on each other: they are computed together, the diagonals one after another.  A step (a, b) of the seven step sets reads row i - a of
// diagonal s - a - b, with a <= 2 and a + b <= 3, so the last three diagonals are all the recursion needs:
//   wave route   T1 <= 64: lane = row.  Each lane keeps its own last three values in registers and takes rows i - 1, i - 2 from the lanes
//                below by __shfl_up; no LDS traffic, no barrier between diagonals.
//   block route  rows strided over up to 1024 threads, a ring of four diagonals of R and R_ in LDS, one __syncthreads() per diagonal (the
//                slot written on diagonal s was last read on diagonal s - 1, before that barrier).
// d(i, j) is formed in the kernel from x_i (LDS) and y_j (global memory, L1-resident: a diagonal reads consecutive rows of y); the
// distance matrix never exists.  R (and R_ for the two-step sets) reach memory only when the caller passes the tables, packed BY DIAGONAL
// (dtw_cell below) so that a diagonal's stores and the backward's loads are consecutive addresses.
//
// The backward walks the diagonals downwards.  A cell whose adjoints G, G_ are complete (every successor lies on a later diagonal)
// recomputes its candidates from the saved tables and the soft-min weights from the candidates, leaves ONE message per step -- G pi_k (+ G_ pi'_k) -- where its
// predecessors will gather it (registers and __shfl_down / the LDS ring), and adds gD dd/dx_i to gx[i] and gD dd/dy_j to gy[j].  Row i
// belongs to one thread for the whole sweep; on one diagonal every j occurs once, and diagonals are separated by the barrier (block) or a
// workgroup fence (wave): every sum has one fixed order, there are no atomics, and gD is never stored.
#include "common.h"

#include <limits>

namespace dsa {
namespace {

// dsa_last_kernel() of the three entries: [entry][route][dtype]  (tests/kernel_routes.py reads the table: PINNED_ELSEWHERE has every name)
enum { DTW_FORWARD = 0, DTW_VJP = 1, DTW_PATH = 2 };
enum { DTW_WAVE = 0, DTW_BLOCK = 1 };
const char* const kDtwRoutes[3][2][2] = {
    {{"dtw_wave_f32", "dtw_wave_f64"}, {"dtw_block_f32", "dtw_block_f64"}},
    {{"dtw_vjp_wave_f32", "dtw_vjp_wave_f64"}, {"dtw_vjp_block_f32", "dtw_vjp_block_f64"}},
    {{"dtw_path_f32", "dtw_path_f64"}, {"dtw_path_f32", "dtw_path_f64"}},
};

constexpr int DTW_WAVE_ROWS = 64;        // the wave route's largest T1
constexpr int DTW_BLOCK_THREADS = 1024;  // the block route's workgroup
constexpr int DTW_RING = 4;              // diagonals s, s-1, s-2, s-3
constexpr int DTW_LDS_PER_ROW = 12;      // elements of LDS per row besides x_i: the backward's ring of 3 messages (the forward's R, R_ ring: 8)
constexpr int DTW_MAX_GRID = 1 << 16;

// the local path constraints (dtw.py:255-284): steps in the reference's order, and whether axis steps read the second table
struct DtwSteps {
    int n, two;
    int a[3], b[3];
};
inline DtwSteps dtw_steps(int p)
{
    switch (p) {
    case 0: return {2, 0, {1, 0, 0}, {0, 1, 0}};
    case 1: return {3, 0, {1, 0, 1}, {0, 1, 1}};
    case 2: return {2, 0, {1, 1, 0}, {0, 1, 0}};
    case 3: return {3, 0, {1, 1, 1}, {0, 1, 2}};
    case 4: return {3, 1, {1, 0, 1}, {0, 1, 1}};
    case 5: return {3, 0, {1, 1, 2}, {1, 2, 1}};
    default: return {3, 1, {1, 1, 1}, {0, 1, 2}};
    }
}

// the tables' layout: cell (i, j) of a T1 x T2 grid, diagonals s = i + j one after another, a diagonal's cells by ascending row
__device__ __forceinline__ long dtw_cell(long i, long j, long T1, long T2)
{
    const long s = i + j, m = T1 < T2 ? T1 : T2, M = T1 < T2 ? T2 : T1, L = T1 + T2 - 1;
    long off;
    if (s <= m)
        off = s * (s + 1) / 2;
    else if (s <= M)
        off = m * (m + 1) / 2 + (s - m) * m;
    else
        off = T1 * T2 - (L - s) * (L - s + 1) / 2;
    const long i0 = s - T2 + 1 > 0 ? s - T2 + 1 : 0;
    return off + (i - i0);
}

// the local distance, from differences
template <typename T>
__device__ __forceinline__ T dtw_dist(const T* xi, const T* __restrict__ yj, int D, int metric)
{
    T s = (T)0;
    switch (metric) {
    case DSA_DTW_MANHATTAN:
        for (int k = 0; k < D; ++k) s += dsa_abs(xi[k] - yj[k]);
        return s;
    case DSA_DTW_EUCLIDEAN:
    case DSA_DTW_SQUARED_EUCLIDEAN: {
        for (int k = 0; k < D; ++k) {
            const T e = xi[k] - yj[k];
            s += e * e;
        }
        const T r = dsa_sqrt(s);
        return metric == DSA_DTW_EUCLIDEAN ? r : r * r;   // (the reference squares cdist's root)
    }
    default: {   // DSA_DTW_SYMMETRIC_KL
        const T c = (T)1e-10;
        T s2 = (T)0;
        for (int k = 0; k < D; ++k) {
            const T a = xi[k], b = yj[k], q1 = a / b, q2 = b / a;
            s += a * dsa_log(q1 < c ? c : q1);
            s2 += b * dsa_log(q2 < c ? c : q2);
        }
        return s + s2;
    }
    }
}

// gxi += g dd/dx_i, gyj += g dd/dy_j at a cell of local distance d
template <typename T>
__device__ __forceinline__ void dtw_dist_vjp(const T* xi, const T* __restrict__ yj, int D, int metric, T d, T g, T* __restrict__ gxi,
                                             T* __restrict__ gyj)
{
    for (int k = 0; k < D; ++k) {
        const T a = xi[k], b = yj[k], e = a - b;
        T dx, dy;
        switch (metric) {
        case DSA_DTW_MANHATTAN:
            dx = (T)((e > (T)0) - (e < (T)0));
            dy = -dx;
            break;
        case DSA_DTW_EUCLIDEAN:
            dx = d == (T)0 ? (T)0 : e / d;
            dy = -dx;
            break;
        case DSA_DTW_SQUARED_EUCLIDEAN:
            dx = (T)2 * e;
            dy = -dx;
            break;
        default: {
            const T c = (T)1e-10, q1 = a / b, q2 = b / a;
            const bool in1 = q1 >= c, in2 = q2 >= c;   // a clipped quotient passes no derivative
            dx = dsa_log(in1 ? q1 : c) + (in1 ? (T)1 : (T)0) - (in2 ? q2 : (T)0);
            dy = dsa_log(in2 ? q2 : c) + (in2 ? (T)1 : (T)0) - (in1 ? q1 : (T)0);
        }
        }
        gxi[k] += g * dx;
        gyj[k] += g * dy;
    }
}

// -gamma logsumexp(-c / gamma) over the candidates that are not +inf; +inf when there is none
template <typename T>
__device__ __forceinline__ T dtw_softmin(const T* c, const bool* use, int n, T gamma)
{
    T m = dsa_inf<T>();
    for (int k = 0; k < 3; ++k)
        if (k < n && use[k] && c[k] < m) m = c[k];
    if (m == dsa_inf<T>()) return m;
    T sum = (T)0;
    for (int k = 0; k < 3; ++k)
        if (k < n && use[k] && c[k] != dsa_inf<T>()) sum += dsa_exp(-(c[k] - m) / gamma);
    return m - gamma * dsa_log(sum);
}

// one pair's lengths: false when they do not fit the tensors (the pair's distance is then NaN and its gradients zero)
__device__ __forceinline__ bool dtw_lengths(const int64_t* __restrict__ lengths, long u, long T1, long T2, long& len1, long& len2)
{
    len1 = lengths ? (long)lengths[2 * u] : T1;
    len2 = lengths ? (long)lengths[2 * u + 1] : T2;
    return len1 >= 1 && len1 <= T1 && len2 >= 1 && len2 <= T2;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <typename T, bool WAVE>
__global__ __launch_bounds__(WAVE ? DTW_WAVE_ROWS : DTW_BLOCK_THREADS) void dtw_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const int64_t* __restrict__ lengths, long B, int T1, long T2, int D, int metric,
    DtwSteps st, T gamma, T* __restrict__ R, T* __restrict__ Q, T* __restrict__ dist)
{
    extern __shared__ __align__(16) unsigned char dtw_lds[];
    T* xs = reinterpret_cast<T*>(dtw_lds);                        // (T1, D)
    T* ring_r = xs + (size_t)T1 * D;                              // block route: (DTW_RING, T1) of R
    T* ring_q = ring_r + (size_t)DTW_RING * T1;                   //              (DTW_RING, T1) of R_
    const int t = threadIdx.x, NT = blockDim.x;
    const T inf = dsa_inf<T>();

    for (long u = blockIdx.x; u < B; u += gridDim.x) {
        long len1, len2;
        const bool fits = dtw_lengths(lengths, u, T1, T2, len1, len2);
        if (!fits) {
            if (t == 0) dist[u] = std::numeric_limits<T>::quiet_NaN();
            continue;
        }
        __syncthreads();   // the pair before this one has been read out of LDS
        const T* xu = x + u * (long)T1 * D;
        const T* yu = y + u * T2 * D;
        for (long e = t; e < len1 * D; e += NT) xs[e] = xu[e];
        __syncthreads();
        T* Ru = R ? R + u * (long)T1 * T2 : nullptr;
        T* Qu = Q ? Q + u * (long)T1 * T2 : nullptr;

        T r1 = inf, r2 = inf, r3 = inf, q1 = inf;   // wave route: this lane's row on diagonals s-1, s-2, s-3
        const long last = len1 + len2 - 2;
        for (long s = 0; s <= last; ++s) {
            T src[3] = {inf, inf, inf};
            if (WAVE) {   // every lane takes part in the exchange
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (k >= st.n) continue;
                    const int a = st.a[k], ab = a + st.b[k];
                    const bool axis = st.two && (a == 0 || st.b[k] == 0);
                    T v = axis ? q1 : (ab == 1 ? r1 : (ab == 2 ? r2 : r3));
                    src[k] = a ? __shfl_up(v, (unsigned)a, 64) : v;
                }
            }
            T rn = inf, qn = inf;
            for (int i = t; i < len1; i += NT) {
                const long j = s - i;
                if (j < 0 || j >= len2) continue;
                const T d = dtw_dist<T>(xs + (size_t)i * D, yu + j * D, D, metric);
                rn = qn = inf;
                if (s == 0) {
                    rn = d;   // R[0,0] = d(0,0); R_[0,0] stays +inf
                } else {
                    T c[3];
                    bool all[3], diag[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        c[k] = inf;
                        all[k] = diag[k] = false;
                        if (k >= st.n) continue;
                        const int a = st.a[k], b = st.b[k];
                        if (i - a < 0 || j - b < 0) continue;
                        const bool axis = st.two && (a == 0 || b == 0);
                        T v;
                        if (WAVE)
                            v = src[k];
                        else
                            v = (axis ? ring_q : ring_r)[(size_t)((s - a - b) & (DTW_RING - 1)) * T1 + (i - a)];
                        if (v == inf) continue;
                        c[k] = (T)(a + b) * d + v;
                        all[k] = true;
                        diag[k] = st.two && !axis;
                    }
                    rn = dtw_softmin<T>(c, all, st.n, gamma);
                    if (st.two) qn = dtw_softmin<T>(c, diag, st.n, gamma);
                }
                if (!WAVE) {
                    ring_r[(size_t)(s & (DTW_RING - 1)) * T1 + i] = rn;
                    ring_q[(size_t)(s & (DTW_RING - 1)) * T1 + i] = qn;
                }
                if (Ru) {
                    const long at = dtw_cell(i, j, T1, T2);
                    Ru[at] = rn;
                    if (Qu) Qu[at] = qn;
                }
                if (s == last) dist[u] = rn / (T)(len1 + len2);   // i = len1 - 1, j = len2 - 1
            }
            if (WAVE) {
                r3 = r2;
                r2 = r1;
                r1 = rn;
                q1 = qn;
            } else {
                __syncthreads();
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
template <typename T, bool WAVE>
__global__ __launch_bounds__(WAVE ? DTW_WAVE_ROWS : DTW_BLOCK_THREADS) void dtw_vjp_kernel(
    const T* __restrict__ x, const T* __restrict__ y, const int64_t* __restrict__ lengths, const T* __restrict__ R, const T* __restrict__ Q,
    const T* __restrict__ gdist, long B, int T1, long T2, int D, int metric, DtwSteps st, T gamma, T* gx, T* gy)
{
    extern __shared__ __align__(16) unsigned char dtw_lds[];
    T* xs = reinterpret_cast<T*>(dtw_lds);      // (T1, D)
    T* ring = xs + (size_t)T1 * D;              // block route: (DTW_RING, 3, T1) messages
    const int t = threadIdx.x, NT = blockDim.x;
    const T inf = dsa_inf<T>();

    for (long u = blockIdx.x; u < B; u += gridDim.x) {
        long len1, len2;
        const bool fits = dtw_lengths(lengths, u, T1, T2, len1, len2);
        __syncthreads();   // the pair before this one has been read out of LDS
        const T* xu = x + u * (long)T1 * D;
        const T* yu = y + u * T2 * D;
        T* gxu = gx + u * (long)T1 * D;
        T* gyu = gy + u * T2 * D;
        for (long e = t; e < (long)T1 * D; e += NT) gxu[e] = (T)0;
        for (long e = t; e < T2 * D; e += NT) gyu[e] = (T)0;
        if (!fits) continue;
        for (long e = t; e < len1 * D; e += NT) xs[e] = xu[e];
        __syncthreads();   // (also orders the zeros above before the sums below)
        const T* Ru = R + u * (long)T1 * T2;
        const T* Qu = st.two ? Q + u * (long)T1 * T2 : nullptr;

        const long last = len1 + len2 - 2;
        const T rend = Ru[dtw_cell(len1 - 1, len2 - 1, T1, T2)];
        const T seed = rend == inf ? (T)0 : gdist[u] / (T)(len1 + len2);
        T m1[3] = {0, 0, 0}, m2[3] = {0, 0, 0}, m3[3] = {0, 0, 0};   // wave route: this lane's messages on diagonals s+1, s+2, s+3
        for (long s = last; s >= 0; --s) {
            T in[3] = {0, 0, 0};
            if (WAVE) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (k >= st.n) continue;
                    const int a = st.a[k], ab = a + st.b[k];
                    T v = ab == 1 ? m1[k] : (ab == 2 ? m2[k] : m3[k]);
                    in[k] = a ? __shfl_down(v, (unsigned)a, 64) : v;
                }
            }
            T out[3] = {0, 0, 0};
            for (int i = t; i < len1; i += NT) {
                const long j = s - i;
                if (j < 0 || j >= len2) continue;
                // the adjoints: what the successors left for this cell, in step order
                T G = s == last ? seed : (T)0, G2 = (T)0;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (k >= st.n) continue;
                    const int a = st.a[k], b = st.b[k];
                    if (i + a >= len1 || j + b >= len2) continue;
                    const T v = WAVE ? in[k] : ring[((size_t)((s + a + b) & (DTW_RING - 1)) * 3 + k) * T1 + (i + a)];
                    if (st.two && (a == 0 || b == 0))
                        G2 += v;
                    else
                        G += v;
                }
                out[0] = out[1] = out[2] = (T)0;
                if (G != (T)0 || G2 != (T)0) {
                    const T d = dtw_dist<T>(xs + (size_t)i * D, yu + j * D, D, metric);
                    T gd = (T)0;
                    if (s == 0) {
                        gd = G;   // R[0,0] = d(0,0)
                    } else {
                        // the candidates again, and the soft-min weights as a normalised softmax over them (pi_k = exp(-(c_k - R) / gamma)
                        // without the rounding of the stored R: at a small gamma that rounding is a relative error of ulp(R) / gamma)
                        T c[3], e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
                        bool all[3], diag[3];
                        T lo = inf, lo2 = inf;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            c[k] = inf;
                            all[k] = diag[k] = false;
                            if (k >= st.n) continue;
                            const int a = st.a[k], b = st.b[k];
                            if (i - a < 0 || j - b < 0) continue;
                            const bool axis = st.two && (a == 0 || b == 0);
                            const T v = (axis ? Qu : Ru)[dtw_cell(i - a, j - b, T1, T2)];
                            if (v == inf) continue;
                            c[k] = (T)(a + b) * d + v;
                            all[k] = true;
                            diag[k] = st.two && !axis;
                            lo = c[k] < lo ? c[k] : lo;
                            if (diag[k]) lo2 = c[k] < lo2 ? c[k] : lo2;
                        }
                        T sum = (T)0, sum2 = (T)0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            if (all[k] && G != (T)0) sum += e1[k] = dsa_exp(-(c[k] - lo) / gamma);
                            if (diag[k] && G2 != (T)0) sum2 += e2[k] = dsa_exp(-(c[k] - lo2) / gamma);
                        }
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            if (!all[k]) continue;
                            T msg = G != (T)0 ? G * (e1[k] / sum) : (T)0;
                            if (diag[k] && G2 != (T)0) msg += G2 * (e2[k] / sum2);
                            out[k] = msg;
                            gd += msg * (T)(st.a[k] + st.b[k]);
                        }
                    }
                    if (gd != (T)0) dtw_dist_vjp<T>(xs + (size_t)i * D, yu + j * D, D, metric, d, gd, gxu + (size_t)i * D, gyu + j * D);
                }
                if (!WAVE)
#pragma unroll
                    for (int k = 0; k < 3; ++k) ring[((size_t)(s & (DTW_RING - 1)) * 3 + k) * T1 + i] = out[k];
            }
            if (WAVE) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    m3[k] = m2[k];
                    m2[k] = m1[k];
                    m1[k] = out[k];
                }
                __threadfence_block();   // gy[j] of this diagonal is another lane's on the next
            } else {
                __syncthreads();
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- path
// one thread per pair: the hard argmin of each visited cell recomputed from the saved tables; the path is written from the END of the
// pair's (T1 + T2 - 1, 2) rows backwards, so that rows [T1 + T2 - 1 - count, T1 + T2 - 1) are the path in forward order
template <typename T>
__global__ __launch_bounds__(64) void dtw_path_kernel(const T* __restrict__ x, const T* __restrict__ y, const int64_t* __restrict__ lengths,
                                                      const T* __restrict__ R, const T* __restrict__ Q, long B, long T1, long T2, int D, int metric,
                                                      DtwSteps st, int64_t* __restrict__ idx, int32_t* __restrict__ count)
{
    const long u = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= B) return;
    const T inf = dsa_inf<T>();
    long len1, len2;
    if (!dtw_lengths(lengths, u, T1, T2, len1, len2)) {
        count[u] = 0;
        return;
    }
    const T* xu = x + u * T1 * D;
    const T* yu = y + u * T2 * D;
    const T* Ru = R + u * T1 * T2;
    const T* Qu = st.two ? Q + u * T1 * T2 : nullptr;
    const long L = T1 + T2 - 1;
    int64_t* out = idx + u * L * 2;
    long i = len1 - 1, j = len2 - 1, pos = L - 1;
    out[2 * pos] = i;
    out[2 * pos + 1] = j;
    bool second = false;   // the move just traced kept one coordinate: the next back-pointer is R_'s
    while (i > 0 || j > 0) {
        const T d = dtw_dist<T>(xu + i * D, yu + j * D, D, metric);
        int best = -1;
        T bestc = inf;
        for (int k = 0; k < st.n; ++k) {
            const int a = st.a[k], b = st.b[k];
            if (i - a < 0 || j - b < 0) continue;
            const bool axis = st.two && (a == 0 || b == 0);
            if (second && axis) continue;   // R_ is made of the other steps
            const T v = (axis ? Qu : Ru)[dtw_cell(i - a, j - b, T1, T2)];
            if (v == inf) continue;
            const T c = (T)(a + b) * d + v;
            if (best < 0 || c < bestc) {   // ties: the first in step order
                best = k;
                bestc = c;
            }
        }
        if (best < 0) break;   // no predecessor: the cell is unreachable
        i -= st.a[best];
        j -= st.b[best];
        second = st.two && (st.a[best] == 0 || st.b[best] == 0);
        --pos;
        out[2 * pos] = i;
        out[2 * pos + 1] = j;
    }
    count[u] = (int32_t)(L - pos);
}

int dtw_check(const char*& route, int entry, int64_t B, int64_t T1, int64_t T2, int64_t D, int32_t metric, int32_t p, int32_t dtype)
{
    if (!(B >= 0 && T1 >= 1 && T2 >= 1 && D >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: invalid sizes");
    if (metric < DSA_DTW_MANHATTAN || metric > DSA_DTW_SYMMETRIC_KL) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: unknown metric");
    if (p < 0 || p > 6) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: unknown local path constraint");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: unknown dtype");
    const int64_t size = dtype == DSA_F32 ? 4 : 8;
    if (D > DSA_DTW_MAX_LDS_BYTES || T1 > DSA_DTW_MAX_LDS_BYTES || T1 * (D + DTW_LDS_PER_ROW) * size > DSA_DTW_MAX_LDS_BYTES)
        return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: T1 (D + 12) elements exceed DSA_DTW_MAX_LDS_BYTES (163840 bytes per pair)");
    // every tensor's byte offset is an int64: B T1 T2, B T1 D and B T2 D
    const int64_t lim = INT64_MAX / 16, w = D > T1 ? D : T1;
    if (T2 > lim / w) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: invalid sizes");
    const int64_t t12 = T1 > T2 ? T1 : T2, per = T1 * T2 > t12 * D ? T1 * T2 : t12 * D;
    if (B > 0 && per > lim / B) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: invalid sizes");
    route = kDtwRoutes[entry][T1 <= DTW_WAVE_ROWS ? DTW_WAVE : DTW_BLOCK][dtype == DSA_F64];
    return DSA_OK;
}

constexpr const char* kDtwLdsError = "dtw: cannot raise the dynamic LDS limit";
inline int dtw_block_threads(int64_t T1) { return T1 >= DTW_BLOCK_THREADS ? DTW_BLOCK_THREADS : (int)((T1 + 63) / 64 * 64); }

template <typename T>
int dtw_forward(const void* x, const void* y, const void* lengths, int64_t B, int64_t T1, int64_t T2, int64_t D, int metric, const DtwSteps& st,
                double gamma, void* R, void* Q, void* dist, hipStream_t stream)
{
    const bool wave = T1 <= DTW_WAVE_ROWS;
    const size_t lds = (size_t)T1 * (D + (wave ? 0 : 2 * DTW_RING)) * sizeof(T);
    const dim3 grid((unsigned)(B < DTW_MAX_GRID ? B : DTW_MAX_GRID));
    auto launch = [&](auto wave_tag, int threads) {
        return launch_lds<dtw_kernel<T, decltype(wave_tag)::value>>(DSA_DTW_MAX_LDS_BYTES, kDtwLdsError, grid, dim3(threads), lds, stream, (const T*)x,
                                                                    (const T*)y, (const int64_t*)lengths, (long)B, (int)T1, (long)T2, (int)D, metric, st,
                                                                    (T)gamma, (T*)R, (T*)Q, (T*)dist);
    };
    return wave ? launch(std::true_type{}, DTW_WAVE_ROWS) : launch(std::false_type{}, dtw_block_threads(T1));
}

template <typename T>
int dtw_backward(const void* x, const void* y, const void* lengths, const void* R, const void* Q, const void* gdist, int64_t B, int64_t T1,
                 int64_t T2, int64_t D, int metric, const DtwSteps& st, double gamma, void* gx, void* gy, hipStream_t stream)
{
    const bool wave = T1 <= DTW_WAVE_ROWS;
    const size_t lds = (size_t)T1 * (D + (wave ? 0 : 3 * DTW_RING)) * sizeof(T);
    const dim3 grid((unsigned)(B < DTW_MAX_GRID ? B : DTW_MAX_GRID));
    auto launch = [&](auto wave_tag, int threads) {
        return launch_lds<dtw_vjp_kernel<T, decltype(wave_tag)::value>>(DSA_DTW_MAX_LDS_BYTES, kDtwLdsError, grid, dim3(threads), lds, stream,
                                                                        (const T*)x, (const T*)y, (const int64_t*)lengths, (const T*)R, (const T*)Q,
                                                                        (const T*)gdist, (long)B, (int)T1, (long)T2, (int)D, metric, st, (T)gamma,
                                                                        (T*)gx, (T*)gy);
    };
    return wave ? launch(std::true_type{}, DTW_WAVE_ROWS) : launch(std::false_type{}, dtw_block_threads(T1));
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_dtw(const void* x, const void* y, const void* lengths, int64_t B, int64_t T1, int64_t T2, int64_t D, int32_t metric, int32_t p,
                       double softness, int32_t dtype, void* R, void* R2, void* distance, void* stream)
{
    const char* route = "";
    if (int rc = dtw_check(route, DTW_FORWARD, B, T1, T2, D, metric, p, dtype)) return rc;
    if (!(softness > 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: softness must be positive");
    if (B == 0) return DSA_OK;
    const DtwSteps st = dtw_steps(p);
    if (!(x && y && distance) || (R && st.two && !R2)) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: null pointer");
    if (!st.two || !R) R2 = nullptr;
    const int rc = with_dtype(dtype, "dtw", [&](auto tag) {
        return dtw_forward<decltype(tag)>(x, y, lengths, B, T1, T2, D, metric, st, softness, R, R2, distance, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_dtw_vjp(const void* x, const void* y, const void* lengths, const void* R, const void* R2, const void* gdistance, int64_t B,
                           int64_t T1, int64_t T2, int64_t D, int32_t metric, int32_t p, double softness, int32_t dtype, void* gx, void* gy,
                           void* stream)
{
    const char* route = "";
    if (int rc = dtw_check(route, DTW_VJP, B, T1, T2, D, metric, p, dtype)) return rc;
    if (!(softness > 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: softness must be positive");
    if (B == 0) return DSA_OK;
    const DtwSteps st = dtw_steps(p);
    if (!(x && y && R && gdistance && gx && gy) || (st.two && !R2)) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: null pointer");
    const int rc = with_dtype(dtype, "dtw", [&](auto tag) {
        return dtw_backward<decltype(tag)>(x, y, lengths, R, R2, gdistance, B, T1, T2, D, metric, st, softness, gx, gy, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_dtw_path(const void* x, const void* y, const void* lengths, const void* R, const void* R2, int64_t B, int64_t T1, int64_t T2,
                            int64_t D, int32_t metric, int32_t p, int32_t dtype, void* indices, void* count, void* stream)
{
    const char* route = "";
    if (int rc = dtw_check(route, DTW_PATH, B, T1, T2, D, metric, p, dtype)) return rc;
    if (B == 0) return DSA_OK;
    const DtwSteps st = dtw_steps(p);
    if (!(x && y && R && indices && count) || (st.two && !R2)) return fail(DSA_ERR_INVALID_ARGUMENT, "dtw: null pointer");
    const dim3 grid((unsigned)((B + 63) / 64));
    return with_dtype(dtype, "dtw", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((dtw_path_kernel<T>), grid, dim3(64), 0, (hipStream_t)stream, (const T*)x, (const T*)y, (const int64_t*)lengths, (const T*)R,
                           (const T*)R2, (long)B, (long)T1, (long)T2, (int)D, metric, st, (int64_t*)indices, (int32_t*)count);
        return check_launch(route);
    });
}
