// Gaussian mixture models (include/diffsptk_amd.h, section a21): one EM iteration of GaussianMixtureModeling.forward, gmm.py:299-378, and
// the conversion of GaussianMixtureModeling.transform, gmm.py:394-432.  (There: three passes over the data per iteration, outer(x) of
// T L^2 values in memory, (B, K, L, 1) intermediates of broadcast matmuls and an einsum for the second moments.)
//   prepare    per component: the inverse W of the Cholesky factor of sigma's leading (L', L') block (sigma = C C^T, W = C^-1), or the
//              reciprocal variances on the diagonal route, and c_k = log w_k - (L' log 2 pi + log det sigma_k) / 2.  A pivot that is not
//              positive sets fail[k] and leaves W = 0, c_k = -inf: the launch finishes, the host raises after its one read.
//   estep      numer[t,k] = c_k - |W_k (x_t - mu_k)|^2 / 2, the log-sum-exp over k and the posterior.  One thread per vector; a tile of
//              vectors and of differences in LDS (row stride L' | 1: conflict-free), one component's W and mu staged in LDS at a time, so K
//              has no ceiling.  Four rows of W per pass over a difference: one LDS read of d per four products.  The per-vector
//              log-likelihoods are summed per workgroup (float64, fixed order), the partials by one workgroup of a second kernel, which also
//              writes the two-element read-back: the total and the first failed component + 1.
//   accum      the zeroth, first and second moments as ONE weighted SYRK of the augmented vector [x_t, 1]: (L + 1)^2 sums per component
//              whose last row is px and whose corner is z.  Grid (component x lower 32 x 32 tile, segment of T), one wave per workgroup, a 4 x 4
//              register block per lane, rows staged through LDS 32 at a time.  The diagonal route sums p x and p x^2 per column, four
//              components per workgroup.  Every output element's partial sum belongs to one thread: no atomics, the same bits every run.
//   update     the M-step from the segments' partials, summed in segment order: weights with floor and renormalisation, means,
//              covariances (MAP or not), mask and variance floor, in place.  One workgroup per component; skipped when the read-back says
//              that a factorisation failed, so that the parameters stay as they were.
//   regress    Myx_k = sigma_yx sigma_xx^-1 by Gauss-Jordan elimination with partial pivoting on sigma_xx as it is (no symmetry assumed).
//   transform  the first largest posterior per vector and y_t = mu_y[k] + Myx_k (x_t - mu_x[k]).
#include "common.h"

namespace dsa {
namespace {

// dsa_last_kernel() of the six entries: [entry][diagonal route][dtype]
enum { GMM_PREPARE = 0, GMM_ESTEP = 1, GMM_ACCUM = 2, GMM_UPDATE = 3, GMM_REGRESS = 4, GMM_TRANSFORM = 5 };
const char* const kGmmRoutes[6][2][2] = {
    {{"gmm_prepare_full_f32", "gmm_prepare_full_f64"}, {"gmm_prepare_diag_f32", "gmm_prepare_diag_f64"}},
    {{"gmm_estep_full_f32", "gmm_estep_full_f64"}, {"gmm_estep_diag_f32", "gmm_estep_diag_f64"}},
    {{"gmm_accum_full_f32", "gmm_accum_full_f64"}, {"gmm_accum_diag_f32", "gmm_accum_diag_f64"}},
    {{"gmm_update_full_f32", "gmm_update_full_f64"}, {"gmm_update_diag_f32", "gmm_update_diag_f64"}},
    {{"gmm_regress_f32", "gmm_regress_f64"}, {"gmm_regress_f32", "gmm_regress_f64"}},
    {{"gmm_transform_f32", "gmm_transform_f64"}, {"gmm_transform_f32", "gmm_transform_f64"}},
};

constexpr int GMM_SYRK_TILE = 32;      // the accumulation's output tile, one wave: 8 x 8 lanes of 4 x 4 sums
constexpr int GMM_SYRK_ROWS = 32;      // vectors staged per pass
constexpr int GMM_DIAG_COMPONENTS = 4; // components per workgroup of the diagonal accumulation
constexpr int GMM_MAX_SEGMENTS = 64;
constexpr int GMM_FILL_WAVES = 4096;   // waves below which T is split into segments: four per SIMD of 256 compute units
constexpr int GMM_SEGMENT_MIN = 256;   // vectors per segment at least
constexpr double GMM_LOG_2PI = 1.8378770664093453;

inline int64_t gmm_lds_bytes(int64_t L, int64_t size) { return 2 * DSA_GMM_TILE_BYTES * (L + 1) + L * (L + 1) * size + 64; }

inline int gmm_segments(int64_t T, int64_t waves)
{
    if (waves >= GMM_FILL_WAVES) return 1;
    int64_t s = (GMM_FILL_WAVES + waves - 1) / waves;
    const int64_t by_t = (T + GMM_SEGMENT_MIN - 1) / GMM_SEGMENT_MIN;
    s = s < by_t ? s : by_t;
    s = s < GMM_MAX_SEGMENTS ? s : GMM_MAX_SEGMENTS;
    return (int)(s < 1 ? 1 : s);
}
inline int64_t gmm_syrk_tiles(int64_t L)
{
    const int64_t nt = (L + 1 + GMM_SYRK_TILE - 1) / GMM_SYRK_TILE;
    return nt * (nt + 1) / 2;
}
inline int gmm_accum_segments(int64_t T, int64_t K, int64_t L, int diag)
{
    return gmm_segments(T, diag ? 4 * ((K + GMM_DIAG_COMPONENTS - 1) / GMM_DIAG_COMPONENTS) : K * gmm_syrk_tiles(L));   // the waves of one segment
}
inline int64_t gmm_row_elements(int64_t L, int diag) { return diag ? 2 * L + 1 : (L + 1) * (L + 1); }

// ---------------------------------------------------------------------------------------------------------------- prepare
template <typename T>
__global__ __launch_bounds__(64) void gmm_prepare_full_kernel(const T* __restrict__ w, const T* __restrict__ sigma, int L, int Lp,
                                                              T* __restrict__ prec, T* __restrict__ cst, int32_t* __restrict__ fail)
{
    extern __shared__ __align__(16) unsigned char gmm_lds[];
    T* A = reinterpret_cast<T*>(gmm_lds);   // (Lp, Lp): sigma's block, its lower triangle becomes the factor C
    T* W = A + Lp * Lp;                     // (Lp, Lp): C^-1, zero above the diagonal
    const int k = blockIdx.x, lane = threadIdx.x;
    const T* S = sigma + (long)k * L * L;
    T* P = prec + (long)k * Lp * Lp;
    for (int e = lane; e < Lp * Lp; e += 64) {
        A[e] = S[(e / Lp) * L + e % Lp];
        W[e] = (T)0;
    }
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < Lp; ++j) {
        const T d = A[j * Lp + j];   // the same value in every lane: the branch is uniform
        if (!(d > (T)0)) {
            bad = true;
            break;
        }
        const T l = dsa_sqrt(d);
        __syncthreads();
        for (int i = j + lane; i < Lp; i += 64) A[i * Lp + j] = i == j ? l : A[i * Lp + j] / l;
        __syncthreads();
        for (int i = j + 1 + lane; i < Lp; i += 64) {
            const T lij = A[i * Lp + j];
            for (int c = j + 1; c <= i; ++c) A[i * Lp + c] -= lij * A[c * Lp + j];
        }
        __syncthreads();
    }
    if (bad) {
        for (int e = lane; e < Lp * Lp; e += 64) P[e] = (T)0;
        if (lane == 0) {
            cst[k] = -dsa_inf<T>();
            fail[k] = 1;
        }
        return;
    }
    for (int c = lane; c < Lp; c += 64) {   // column c of C^-1 by forward substitution: a lane reads what it wrote itself
        W[c * Lp + c] = (T)1 / A[c * Lp + c];
        for (int i = c + 1; i < Lp; ++i) {
            T s = (T)0;
            for (int m = c; m < i; ++m) s += A[i * Lp + m] * W[m * Lp + c];
            W[i * Lp + c] = -s / A[i * Lp + i];
        }
    }
    __syncthreads();
    for (int e = lane; e < Lp * Lp; e += 64) P[e] = W[e];
    if (lane == 0) {
        T s = (T)0;
        for (int j = 0; j < Lp; ++j) s += dsa_log(A[j * Lp + j]);
        cst[k] = dsa_log(w[k]) - (T)0.5 * ((T)(Lp * GMM_LOG_2PI) + s * (T)2);
        fail[k] = 0;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void gmm_prepare_diag_kernel(const T* __restrict__ w, const T* __restrict__ sigma, int L, int Lp,
                                                              T* __restrict__ prec, T* __restrict__ cst, int32_t* __restrict__ fail)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    const T* S = sigma + (long)k * L * L;
    for (int j = lane; j < Lp; j += 64) prec[(long)k * Lp + j] = (T)1 / S[(long)j * L + j];
    if (lane == 0) {
        T s = (T)0;
        for (int j = 0; j < Lp; ++j) s += dsa_log(S[(long)j * L + j]);
        cst[k] = dsa_log(w[k]) - (T)0.5 * ((T)(Lp * GMM_LOG_2PI) + s);
        fail[k] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- E-step
template <typename T, bool DIAG>
__global__ __launch_bounds__(DSA_GMM_TILE_BYTES / sizeof(T)) void gmm_estep_kernel(const T* __restrict__ x, const T* __restrict__ mu,
                                                                                   const T* __restrict__ prec, const T* __restrict__ cst, long Tn,
                                                                                   int K, int L, int Lp, T* post, T* __restrict__ ll,
                                                                                   double* __restrict__ partial)
{
    constexpr int TILE = DSA_GMM_TILE_BYTES / sizeof(T);
    extern __shared__ __align__(16) unsigned char gmm_lds[];
    __shared__ double red[TILE / 64];
    const int S = Lp | 1;
    T* xs = reinterpret_cast<T*>(gmm_lds);   // (TILE, S) vectors
    T* ds = xs + TILE * S;                   // (TILE, S) differences from the component's mean
    T* Ws = ds + TILE * S;                   // (Lp, Lp), or (Lp) reciprocal variances
    T* ms = Ws + (DIAG ? Lp : Lp * Lp);      // (Lp)
    const int tid = threadIdx.x;
    const long t0 = (long)blockIdx.x * TILE, t = t0 + tid;
    const long rows = Tn - t0 < TILE ? Tn - t0 : TILE;
    for (long e = tid; e < rows * Lp; e += TILE) xs[(e / Lp) * S + e % Lp] = x[t0 * Lp + e];
    const bool live = t < Tn;
    const T* xt = xs + tid * S;
    T* dt = ds + tid * S;
    T* pt = post + t * K;
    T top = -dsa_inf<T>();
    for (int k = 0; k < K; ++k) {
        __syncthreads();   // the component before this one has been read out of LDS (and, at k = 0, the tile is in)
        const int nw = DIAG ? Lp : Lp * Lp;
        for (int e = tid; e < nw; e += TILE) Ws[e] = prec[(long)k * nw + e];
        for (int e = tid; e < Lp; e += TILE) ms[e] = mu[(long)k * L + e];
        __syncthreads();
        if (!live) continue;
        T m = (T)0;
        if (DIAG) {
            for (int j = 0; j < Lp; ++j) {
                const T e = xt[j] - ms[j];
                m += e * e * Ws[j];
            }
        } else {
            for (int j = 0; j < Lp; ++j) dt[j] = xt[j] - ms[j];
            for (int i0 = 0; i0 < Lp; i0 += 4) {   // four rows of W per pass; a row past the end repeats the last one and is not added
                const int last = Lp - 1;
                const T* w0 = Ws + i0 * Lp;
                const T* w1 = Ws + (i0 + 1 < last ? i0 + 1 : last) * Lp;
                const T* w2 = Ws + (i0 + 2 < last ? i0 + 2 : last) * Lp;
                const T* w3 = Ws + (i0 + 3 < last ? i0 + 3 : last) * Lp;
                const int jn = i0 + 4 < Lp ? i0 + 4 : Lp;   // W is zero above its diagonal
                T a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                for (int j = 0; j < jn; ++j) {
                    const T d = dt[j];
                    a0 += w0[j] * d;
                    a1 += w1[j] * d;
                    a2 += w2[j] * d;
                    a3 += w3[j] * d;
                }
                m += a0 * a0;
                if (i0 + 1 < Lp) m += a1 * a1;
                if (i0 + 2 < Lp) m += a2 * a2;
                if (i0 + 3 < Lp) m += a3 * a3;
            }
        }
        const T numer = cst[k] - (T)0.5 * m;
        pt[k] = numer;
        top = numer > top ? numer : top;
    }
    double mine = 0.0;
    if (live) {   // torch.logsumexp: the maximum first (0 in its place when it is not finite), then log sum exp(numer - maximum)
        const T ref = dsa_isfinite(top) ? top : (T)0;
        T sum = (T)0;
        for (int k = 0; k < K; ++k) sum += dsa_exp(pt[k] - ref);
        const T denom = dsa_log(sum) + ref;
        for (int k = 0; k < K; ++k) pt[k] = dsa_exp(pt[k] - denom);
        ll[t] = denom;
        mine = (double)denom;
    }
    const double all = block_sum<double>(mine, red);
    if (tid == 0) partial[blockIdx.x] = all;
}

template <typename T>
__global__ __launch_bounds__(256) void gmm_total_kernel(const double* __restrict__ partial, long n, const int32_t* __restrict__ fail, int K,
                                                        T* __restrict__ total, double* __restrict__ readback)
{
    __shared__ double red[4];
    __shared__ int first[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long i = tid; i < n; i += 256) s += partial[i];
    const double all = block_sum<double>(s, red);
    int f = 0x7fffffff;
    for (int k = tid; k < K; k += 256)
        if (fail[k] && k + 1 < f) f = k + 1;
    first[tid] = f;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 256; ++i) f = first[i] < f ? first[i] : f;
        if (total) total[0] = (T)all;
        if (readback) {
            readback[0] = all;
            readback[1] = f == 0x7fffffff ? 0.0 : (double)f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- moments
// ws[(s K + k) (L + 1)^2 + i (L + 1) + j] = sum over segment s of p[t,k] a_i a_j, a = [x_t, 1], for the 32 x 32 tiles on and below the
// diagonal (a diagonal tile is written whole)
template <typename T>
__global__ __launch_bounds__(64) void gmm_accum_full_kernel(const T* __restrict__ x, const T* __restrict__ post, long Tn, int K, int L,
                                                            long seglen, int ntiles, T* __restrict__ ws)
{
    __shared__ __align__(16) T as[GMM_SYRK_ROWS][GMM_SYRK_TILE];
    __shared__ __align__(16) T bs[GMM_SYRK_ROWS][GMM_SYRK_TILE];
    const int A = L + 1, lane = threadIdx.x, k = blockIdx.x / ntiles, seg = blockIdx.y;
    int R = 0, pair = blockIdx.x % ntiles;   // the pair-th tile of the lower triangle, by rows
    while (pair > R) pair -= ++R;
    const int C = pair;
    const long tbeg = seg * seglen, tend = tbeg + seglen < Tn ? tbeg + seglen : Tn;
    const int li = lane >> 3, lj = lane & 7;
    T acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (T)0;
    for (long tb = tbeg; tb < tend; tb += GMM_SYRK_ROWS) {
        __syncthreads();
        for (int e = lane; e < GMM_SYRK_ROWS * GMM_SYRK_TILE; e += 64) {
            const int tt = e / GMM_SYRK_TILE, c = e % GMM_SYRK_TILE;
            const long t = tb + tt;
            const int gi = R * GMM_SYRK_TILE + c, gj = C * GMM_SYRK_TILE + c;
            T va = (T)0, vb = (T)0;
            if (t < tend) {
                const T p = post[t * K + k];
                va = gi < L ? p * x[t * L + gi] : (gi == L ? p : (T)0);
                vb = gj < L ? x[t * L + gj] : (gj == L ? (T)1 : (T)0);
            }
            as[tt][c] = va;
            bs[tt][c] = vb;
        }
        __syncthreads();
#pragma unroll 4
        for (int tt = 0; tt < GMM_SYRK_ROWS; ++tt) {
            T a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = as[tt][4 * li + q];
                b[q] = bs[tt][4 * lj + q];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] += a[p] * b[q];
        }
    }
    T* out = ws + ((long)seg * K + k) * A * A;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gi = R * GMM_SYRK_TILE + 4 * li + p, gj = C * GMM_SYRK_TILE + 4 * lj + q;
            if (gi < A && gj < A) out[(long)gi * A + gj] = acc[p][q];
        }
}

// ws[(s K + k) (2 L + 1) + c]: c < L sum p x_c, c = L sum p, L < c sum p x_(c - L - 1)^2
template <typename T>
__global__ __launch_bounds__(256) void gmm_accum_diag_kernel(const T* __restrict__ x, const T* __restrict__ post, long Tn, int K, int L,
                                                             long seglen, T* __restrict__ ws)
{
    __shared__ T red[4][GMM_DIAG_COMPONENTS * 4][64];
    const int A = L + 1, tid = threadIdx.x, lane = tid & 63, g = tid >> 6, seg = blockIdx.y;
    const int k0 = blockIdx.x * GMM_DIAG_COMPONENTS;
    const long tbeg = seg * seglen, tend = tbeg + seglen < Tn ? tbeg + seglen : Tn;
    const int c0 = lane, c1 = lane + 64;   // L + 1 <= 128: the ceiling keeps L below 70
    T s1[GMM_DIAG_COMPONENTS][2], s2[GMM_DIAG_COMPONENTS][2];
#pragma unroll
    for (int q = 0; q < GMM_DIAG_COMPONENTS; ++q) s1[q][0] = s1[q][1] = s2[q][0] = s2[q][1] = (T)0;
    for (long t = tbeg + g; t < tend; t += 4) {
        const T v0 = c0 < L ? x[t * L + c0] : (c0 == L ? (T)1 : (T)0);
        const T v1 = c1 < L ? x[t * L + c1] : (c1 == L ? (T)1 : (T)0);
#pragma unroll
        for (int q = 0; q < GMM_DIAG_COMPONENTS; ++q) {
            const T p = k0 + q < K ? post[t * K + k0 + q] : (T)0;
            const T pv0 = p * v0, pv1 = p * v1;
            s1[q][0] += pv0;
            s1[q][1] += pv1;
            s2[q][0] += pv0 * v0;
            s2[q][1] += pv1 * v1;
        }
    }
#pragma unroll
    for (int q = 0; q < GMM_DIAG_COMPONENTS; ++q) {
        red[g][q * 4 + 0][lane] = s1[q][0];
        red[g][q * 4 + 1][lane] = s1[q][1];
        red[g][q * 4 + 2][lane] = s2[q][0];
        red[g][q * 4 + 3][lane] = s2[q][1];
    }
    __syncthreads();
    for (int e = tid; e < GMM_DIAG_COMPONENTS * 4 * 64; e += 256) {
        const int row = e >> 6, l = e & 63, q = row >> 2, second = (row >> 1) & 1, c = l + 64 * (row & 1);
        if (k0 + q >= K || c >= A || (second && c >= L)) continue;
        const T sum = ((red[0][row][l] + red[1][row][l]) + red[2][row][l]) + red[3][row][l];
        ws[((long)seg * K + k0 + q) * (2 * L + 1) + (second ? A + c : c)] = sum;
    }
}

// ---------------------------------------------------------------------------------------------------------------- M-step
template <typename T, bool DIAG>
__global__ __launch_bounds__(256) void gmm_update_kernel(const T* __restrict__ ws, int nseg, const double* __restrict__ readback,
                                                         const T* __restrict__ ubm_w, const T* __restrict__ ubm_mu, const T* __restrict__ ubm_sigma,
                                                         const T* __restrict__ mask, double Tn, int K, int L, double alpha, double weight_floor,
                                                         double var_floor, T* __restrict__ w, T* __restrict__ mu, T* __restrict__ sigma)
{
    extern __shared__ __align__(16) unsigned char gmm_lds[];
    __shared__ T red[4];
    T* mus = reinterpret_cast<T*>(gmm_lds);   // (L) the new mean
    T* nus = mus + L;                         // (L) px / y, for MAP
    if (readback && readback[1] != 0.0) return;   // a factorisation failed: the parameters stay (uniform over the grid)
    const int k = blockIdx.x, tid = threadIdx.x, A = L + 1;
    const long row = DIAG ? 2 * L + 1 : (long)A * A, zat = DIAG ? L : (long)L * A + L;
    const bool map = alpha != 0.0;
    const T wf = (T)weight_floor, count = (T)(Tn + alpha);
    // the sum of the floored weights: every workgroup forms it in the same order
    T part = (T)0;
    for (int kk = tid; kk < K; kk += 256) {
        T z = (T)0;
        for (int s = 0; s < nseg; ++s) z += ws[((long)s * K + kk) * row + zat];
        if (map) z += ubm_w[kk] * (T)alpha;
        T wk = z / count;
        wk = wk < wf ? wf : wk;
        part += wk;
    }
    const T sumw = block_sum<T>(part, red);
    T y = (T)0;
    for (int s = 0; s < nseg; ++s) y += ws[((long)s * K + k) * row + zat];
    const T xi = map ? ubm_w[k] * (T)alpha : (T)0;
    const T z = y + xi, zi = (T)1 / z;
    if (tid == 0) {
        T wk = z / count;
        wk = wk < wf ? wf : wk;
        const T sf = (T)(weight_floor * K);
        const T a = ((T)1 - sf) / (sumw - sf);
        const T b = wf * ((T)1 - a);
        w[k] = a * wk + b;
    }
    for (int j = tid; j < L; j += 256) {
        T px = (T)0;
        for (int s = 0; s < nseg; ++s) px += ws[((long)s * K + k) * row + (DIAG ? j : (long)L * A + j)];
        const T m = map ? (px + xi * ubm_mu[(long)k * L + j]) * zi : px * zi;
        mus[j] = m;
        nus[j] = px / y;
        mu[(long)k * L + j] = m;
    }
    __syncthreads();
    const T vf = (T)var_floor;
    T* Sk = sigma + (long)k * L * L;
    if (DIAG) {
        for (int j = tid; j < L; j += 256) {
            T pxx = (T)0;
            for (int s = 0; s < nseg; ++s) pxx += ws[((long)s * K + k) * row + A + j];
            const T mm = mus[j] * mus[j];
            T v;
            if (!map) {
                v = pxx * zi - mm;
            } else {
                T a = pxx - y * ((T)2 * (nus[j] * mus[j]) - mm);
                a = dsa_isfinite(a) ? a : (T)0;
                const T um = ubm_mu[(long)k * L + j] - mus[j];
                v = (a + xi * ubm_sigma[((long)k * L + j) * L + j] + xi * (um * um)) * zi;
            }
            Sk[(long)j * L + j] = v < vf ? vf : v;
        }
    } else {
        for (int e = tid; e < L * L; e += 256) {
            const int i = e / L, j = e % L, hi = i > j ? i : j, lo = i > j ? j : i;
            T pxx = (T)0;
            for (int s = 0; s < nseg; ++s) pxx += ws[((long)s * K + k) * row + (long)hi * A + lo];
            const T mm = mus[i] * mus[j];
            T v;
            if (!map) {
                v = pxx * zi - mm;
            } else {
                T a = pxx - y * ((nus[i] * mus[j] + nus[j] * mus[i]) - mm);
                a = dsa_isfinite(a) ? a : (T)0;
                const T ui = ubm_mu[(long)k * L + i] - mus[i], uj = ubm_mu[(long)k * L + j] - mus[j];
                v = (a + xi * ubm_sigma[(long)k * L * L + e] + xi * (ui * uj)) * zi;
            }
            v *= mask[e];
            if (i == j) v = v < vf ? vf : v;
            Sk[e] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- transform
template <typename T>
__global__ __launch_bounds__(256) void gmm_regress_kernel(const T* __restrict__ sigma, int L, int Lx, T* __restrict__ M)
{
    extern __shared__ __align__(16) unsigned char gmm_lds[];
    __shared__ int pivot;
    T* Am = reinterpret_cast<T*>(gmm_lds);   // (Lx, Lx) sigma_xx, reduced to the identity
    T* Bm = Am + Lx * Lx;                    // (Lx, Lx) the identity, becoming sigma_xx^-1
    T* col = Bm + Lx * Lx;                   // (Lx) the column being eliminated
    const int k = blockIdx.x, tid = threadIdx.x, Ly = L - Lx;
    const T* S = sigma + (long)k * L * L;
    for (int e = tid; e < Lx * Lx; e += 256) {
        Am[e] = S[(e / Lx) * L + e % Lx];
        Bm[e] = e / Lx == e % Lx ? (T)1 : (T)0;
    }
    __syncthreads();
    for (int c = 0; c < Lx; ++c) {
        if (tid == 0) {
            int p = c;
            T best = dsa_abs(Am[c * Lx + c]);
            for (int i = c + 1; i < Lx; ++i)
                if (dsa_abs(Am[i * Lx + c]) > best) {
                    best = dsa_abs(Am[i * Lx + c]);
                    p = i;
                }
            pivot = p;
        }
        __syncthreads();
        const int p = pivot;
        if (p != c)
            for (int j = tid; j < Lx; j += 256) {
                T v = Am[c * Lx + j];
                Am[c * Lx + j] = Am[p * Lx + j];
                Am[p * Lx + j] = v;
                v = Bm[c * Lx + j];
                Bm[c * Lx + j] = Bm[p * Lx + j];
                Bm[p * Lx + j] = v;
            }
        __syncthreads();
        const T d = Am[c * Lx + c];
        for (int i = tid; i < Lx; i += 256) col[i] = i == c ? (T)0 : Am[i * Lx + c];
        __syncthreads();
        for (int j = tid; j < Lx; j += 256) {
            Am[c * Lx + j] /= d;
            Bm[c * Lx + j] /= d;
        }
        __syncthreads();
        for (int e = tid; e < Lx * Lx; e += 256) {
            const int i = e / Lx, j = e % Lx;
            if (i == c) continue;
            Am[e] -= col[i] * Am[c * Lx + j];
            Bm[e] -= col[i] * Bm[c * Lx + j];
        }
        __syncthreads();
    }
    T* Mk = M + (long)k * Ly * Lx;
    for (int e = tid; e < Ly * Lx; e += 256) {
        const int r = e / Lx, j = e % Lx;
        T s = (T)0;
        for (int m = 0; m < Lx; ++m) s += S[(long)(Lx + r) * L + m] * Bm[m * Lx + j];
        Mk[e] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void gmm_transform_kernel(const T* __restrict__ x, const T* __restrict__ post, const T* __restrict__ mu,
                                                            const T* __restrict__ M, long Tn, int K, int L, int Lx, int64_t* __restrict__ idx,
                                                            T* __restrict__ y)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= Tn) return;
    const T* pt = post + t * K;
    int k = 0;
    T best = pt[0];
    for (int q = 1; q < K; ++q)
        if (pt[q] > best) {   // ties: the first
            best = pt[q];
            k = q;
        }
    idx[t] = k;
    if (!y) return;
    const int Ly = L - Lx;
    const T* xt = x + t * Lx;
    const T* mk = mu + (long)k * L;
    const T* Mk = M + (long)k * Ly * Lx;
    for (int r = 0; r < Ly; ++r) {
        T s = (T)0;
        for (int j = 0; j < Lx; ++j) s += Mk[r * Lx + j] * (xt[j] - mk[j]);
        y[t * Ly + r] = mk[Lx + r] + s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
int gmm_check(const char*& route, int entry, int64_t T, int64_t K, int64_t L, int64_t Lp, int32_t diag, int32_t dtype)
{
    if (!(T >= 1 && K >= 1 && L >= 1 && Lp >= 1 && Lp <= L)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: unknown dtype");
    const int64_t size = dtype == DSA_F32 ? 4 : 8;
    const int64_t bound = entry == GMM_ACCUM || entry == GMM_UPDATE ? L : Lp;   // the dimension the entry works on
    if (bound > DSA_GMM_MAX_LDS_BYTES || gmm_lds_bytes(bound, size) > DSA_GMM_MAX_LDS_BYTES)
        return fail(DSA_ERR_INVALID_ARGUMENT,
                    "gmm: 2048 (L + 1) + L (L + 1) sizeof(dtype) + 64 bytes exceed DSA_GMM_MAX_LDS_BYTES (163840 bytes per workgroup)");
    // every tensor's byte offset is an int64, every launch dimension an int32: T K, T L, 64 K (L + 1)^2
    if (K > (int64_t)1 << 24 || L > (int64_t)1 << 24) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: invalid sizes");
    const int64_t wide = K > L ? K : L;
    if (T > INT64_MAX / 16 / wide || T / (DSA_GMM_TILE_BYTES / 8) >= INT32_MAX || GMM_MAX_SEGMENTS * K * (L + 1) * (L + 1) > INT64_MAX / 16)
        return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: invalid sizes");
    route = kGmmRoutes[entry][diag ? 1 : 0][dtype == DSA_F64];
    return DSA_OK;
}

template <typename T>
int gmm_prepare(const void* w, const void* sigma, int64_t K, int64_t L, int64_t Lp, int diag, void* prec, void* cst, void* failed, hipStream_t st)
{
    if (diag) {
        hipLaunchKernelGGL((gmm_prepare_diag_kernel<T>), dim3((unsigned)K), dim3(64), 0, st, (const T*)w, (const T*)sigma, (int)L, (int)Lp, (T*)prec,
                           (T*)cst, (int32_t*)failed);
        return DSA_OK;
    }
    // 2 L'^2 elements: below the 64 KiB every kernel may ask for, at every L' inside the ceiling
    hipLaunchKernelGGL((gmm_prepare_full_kernel<T>), dim3((unsigned)K), dim3(64), (size_t)(2 * Lp * Lp) * sizeof(T), st, (const T*)w,
                       (const T*)sigma, (int)L, (int)Lp, (T*)prec, (T*)cst, (int32_t*)failed);
    return DSA_OK;
}

template <typename T, bool DIAG>
int gmm_estep(const void* x, const void* mu, const void* prec, const void* cst, const void* failed, int64_t Tn, int64_t K, int64_t L, int64_t Lp,
              void* post, void* ll, void* partial, void* total, void* readback, hipStream_t st)
{
    constexpr int TILE = DSA_GMM_TILE_BYTES / sizeof(T);
    const int64_t blocks = (Tn + TILE - 1) / TILE;
    const size_t lds = ((size_t)2 * TILE * (Lp | 1) + (DIAG ? Lp : Lp * Lp) + Lp) * sizeof(T);
    if (int rc = launch_lds<gmm_estep_kernel<T, DIAG>>(DSA_GMM_MAX_LDS_BYTES - 64, "gmm: cannot raise the dynamic LDS limit", dim3((unsigned)blocks),
                                                       dim3(TILE), lds, st, (const T*)x, (const T*)mu, (const T*)prec, (const T*)cst, (long)Tn, (int)K,
                                                       (int)L, (int)Lp, (T*)post, (T*)ll, (double*)partial))
        return rc;
    if (total || readback)
        hipLaunchKernelGGL((gmm_total_kernel<T>), dim3(1), dim3(256), 0, st, (const double*)partial, (long)blocks, (const int32_t*)failed, (int)K,
                           (T*)total, (double*)readback);
    return DSA_OK;
}

template <typename T>
int gmm_accum(const void* x, const void* post, int64_t Tn, int64_t K, int64_t L, int diag, void* ws, hipStream_t st)
{
    const int nseg = gmm_accum_segments(Tn, K, L, diag);
    const long seglen = (long)((Tn + nseg - 1) / nseg);
    if (diag)
        hipLaunchKernelGGL((gmm_accum_diag_kernel<T>), dim3((unsigned)((K + GMM_DIAG_COMPONENTS - 1) / GMM_DIAG_COMPONENTS), (unsigned)nseg), dim3(256),
                           0, st, (const T*)x, (const T*)post, (long)Tn, (int)K, (int)L, seglen, (T*)ws);
    else
        hipLaunchKernelGGL((gmm_accum_full_kernel<T>), dim3((unsigned)(gmm_syrk_tiles(L) * K), (unsigned)nseg), dim3(64), 0, st, (const T*)x,
                           (const T*)post, (long)Tn, (int)K, (int)L, seglen, (int)gmm_syrk_tiles(L), (T*)ws);
    return DSA_OK;
}

template <typename T>
int gmm_update(const void* ws, const void* readback, const void* ubm_w, const void* ubm_mu, const void* ubm_sigma, const void* mask, int64_t Tn,
               int64_t K, int64_t L, int diag, double alpha, double weight_floor, double var_floor, void* w, void* mu, void* sigma, hipStream_t st)
{
    const int nseg = gmm_accum_segments(Tn, K, L, diag);
    const size_t lds = (size_t)2 * L * sizeof(T);
    if (diag)
        hipLaunchKernelGGL((gmm_update_kernel<T, true>), dim3((unsigned)K), dim3(256), lds, st, (const T*)ws, nseg, (const double*)readback,
                           (const T*)ubm_w, (const T*)ubm_mu, (const T*)ubm_sigma, (const T*)mask, (double)Tn, (int)K, (int)L, alpha, weight_floor,
                           var_floor, (T*)w, (T*)mu, (T*)sigma);
    else
        hipLaunchKernelGGL((gmm_update_kernel<T, false>), dim3((unsigned)K), dim3(256), lds, st, (const T*)ws, nseg, (const double*)readback,
                           (const T*)ubm_w, (const T*)ubm_mu, (const T*)ubm_sigma, (const T*)mask, (double)Tn, (int)K, (int)L, alpha, weight_floor,
                           var_floor, (T*)w, (T*)mu, (T*)sigma);
    return DSA_OK;
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_gmm_prepare(const void* w, const void* sigma, int64_t K, int64_t L, int64_t Lp, int32_t diag, int32_t dtype, void* prec,
                               void* cst, void* failed, void* stream)
{
    const char* route = "";
    if (int rc = gmm_check(route, GMM_PREPARE, 1, K, L, Lp, diag, dtype)) return rc;
    if (!(w && sigma && prec && cst && failed)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: null pointer");
    const int rc = with_dtype(dtype, "gmm", [&](auto tag) {
        return gmm_prepare<decltype(tag)>(w, sigma, K, L, Lp, diag, prec, cst, failed, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_gmm_estep(const void* x, const void* mu, const void* prec, const void* cst, const void* failed, int64_t T, int64_t K,
                             int64_t L, int64_t Lp, int32_t diag, int32_t dtype, void* posterior, void* loglik, void* partial, void* total,
                             void* readback, void* stream)
{
    const char* route = "";
    if (int rc = gmm_check(route, GMM_ESTEP, T, K, L, Lp, diag, dtype)) return rc;
    if (!(x && mu && prec && cst && failed && posterior && loglik && partial)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = with_dtype(dtype, "gmm", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's row count)
        return diag ? gmm_estep<V, true>(x, mu, prec, cst, failed, T, K, L, Lp, posterior, loglik, partial, total, readback, st)
                    : gmm_estep<V, false>(x, mu, prec, cst, failed, T, K, L, Lp, posterior, loglik, partial, total, readback, st);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int64_t dsa_gmm_accum_workspace_bytes(int64_t T, int64_t K, int64_t L, int32_t diag, int32_t dtype)
{
    const char* route = "";
    if (gmm_check(route, GMM_ACCUM, T, K, L, L, diag, dtype)) return -1;
    return gmm_accum_segments(T, K, L, diag) * K * gmm_row_elements(L, diag) * (dtype == DSA_F32 ? 4 : 8);
}

DSA_EXPORT int dsa_gmm_accum(const void* x, const void* posterior, int64_t T, int64_t K, int64_t L, int32_t diag, int32_t dtype, void* workspace,
                             void* stream)
{
    const char* route = "";
    if (int rc = gmm_check(route, GMM_ACCUM, T, K, L, L, diag, dtype)) return rc;
    if (!(x && posterior && workspace)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: null pointer");
    const int rc = with_dtype(dtype, "gmm", [&](auto tag) {
        return gmm_accum<decltype(tag)>(x, posterior, T, K, L, diag, workspace, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_gmm_update(const void* workspace, const void* readback, const void* ubm_w, const void* ubm_mu, const void* ubm_sigma,
                              const void* mask, int64_t T, int64_t K, int64_t L, int32_t diag, double alpha, double weight_floor, double var_floor,
                              int32_t dtype, void* w, void* mu, void* sigma, void* stream)
{
    const char* route = "";
    if (int rc = gmm_check(route, GMM_UPDATE, T, K, L, L, diag, dtype)) return rc;
    if (!(workspace && w && mu && sigma) || (!diag && !mask)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: null pointer");
    if (!(alpha >= 0 && alpha <= 1 && weight_floor >= 0 && var_floor >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: invalid options");
    if (alpha != 0 && !(ubm_w && ubm_mu && ubm_sigma)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: alpha needs the background model");
    const int rc = with_dtype(dtype, "gmm", [&](auto tag) {
        return gmm_update<decltype(tag)>(workspace, readback, ubm_w, ubm_mu, ubm_sigma, mask, T, K, L, diag, alpha, weight_floor, var_floor, w, mu, sigma,
                                         (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_gmm_regress(const void* sigma, int64_t K, int64_t L, int64_t Lx, int32_t dtype, void* M, void* stream)
{
    const char* route = "";
    if (int rc = gmm_check(route, GMM_REGRESS, 1, K, L, Lx, 0, dtype)) return rc;
    if (Lx >= L) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: invalid sizes");
    if (!(sigma && M)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: null pointer");
    return with_dtype(dtype, "gmm", [&](auto tag) {
        using T = decltype(tag);
        const size_t lds = (size_t)(2 * Lx * Lx + Lx) * sizeof(T);   // (below 64 KiB at every Lx inside the ceiling)
        hipLaunchKernelGGL((gmm_regress_kernel<T>), dim3((unsigned)K), dim3(256), lds, (hipStream_t)stream, (const T*)sigma, (int)L, (int)Lx, (T*)M);
        return check_launch(route);
    });
}

DSA_EXPORT int dsa_gmm_transform(const void* x, const void* posterior, const void* mu, const void* M, int64_t T, int64_t K, int64_t L, int64_t Lx,
                                 int32_t dtype, void* indices, void* y, void* stream)
{
    const char* route = "";
    if (int rc = gmm_check(route, GMM_TRANSFORM, T, K, L, Lx, 0, dtype)) return rc;
    if (!(posterior && indices) || (y && !(x && mu && M)) || (y && Lx >= L)) return fail(DSA_ERR_INVALID_ARGUMENT, "gmm: null pointer");
    const dim3 grid((unsigned)((T + 255) / 256));
    return with_dtype(dtype, "gmm", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's row count)
        hipLaunchKernelGGL((gmm_transform_kernel<V>), grid, dim3(256), 0, (hipStream_t)stream, (const V*)x, (const V*)posterior, (const V*)mu, (const V*)M,
                           (long)T, (int)K, (int)L, (int)Lx, (int64_t*)indices, (V*)y);
        return check_launch(route);
    });
}
