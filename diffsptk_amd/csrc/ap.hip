// Band aperiodicity by TANDEM-STRAIGHT (include/diffsptk_amd.h, section a25): AperiodicityExtractionByTANDEM.forward, ap.py:294-374, with the
// clip and the output format of Aperiodicity.forward, ap.py:166-167.  (There: per band two padded strided convolutions, three gathers of
// (B, N, J + 2), an unfold, two batched matrix products, cholesky_ex in a loop with a host read per trial, cholesky_solve, two stds.)
//
//   qmf        one level of the pyramid, one thread per output sample: both stride-2 filters (41-tap high-pass, 37-tap low-pass, the same
//              centre) read the level's input once, the reflection pad is index arithmetic.  n_band - 1 launches, each half the last.
//              The band signals are float64 whatever the data's dtype, and the taps are this file's float64 constants: on a clean
//              periodic signal the aperiodicity IS the rounding noise of the bands, and float32 bands or float32 taps each moved a
//              float32 sinusoid's result by 1e-5 (the window in float32: 3e-9).
//   tandem     one workgroup per (utterance, frame), one wave per band.  The wave forms the decisions t0, index_bias and curr_pos in the data's
//              dtype (every product, quotient and sum rounded on its own, in the reference's order: they are truncated to integers), gathers
//              the three runs of J + 2 clamped samples into LDS, strides j over its 64 lanes for the 21 + 6 sums of R = H' W H and b = H' W X,
//              reduces them over the wave, factors R + eps m I in registers (m = 1, 10, ... 10^8 until every pivot is positive and finite:
//              the escalation is the fit's own), solves, and goes over the LDS-resident runs twice more: the means of sqrt(w) (X - H a) and
//              sqrt(w) X, then the centred squares.  The residual is formed sample by sample, never as X'WX - 2 a'b + a'Ra.  The sums, the
//              factorisation and the stds run in float64 for both dtypes.  After a barrier the workgroup writes its frame's output: the lowest
//              band doubled, the order reversed, the log-linear interpolation from the module's tables, the clip and the output format.
//   tandem vjp the same workgroup again, then the adjoint of the epilogue (each wave sums the bins that reach its band, in one order), of the
//              stds, the residual and the regularised solve (the regulariser a constant): per fit two scalars per j in LDS, from which the
//              cotangents of the three runs go to a scratch of (B, N, 3 sum(J + 2)); then one thread per band sample gathers the runs that
//              cover it -- curr_pos is monotone in n, so they are one range of frames, found by bisection -- in ascending (frame, run) order;
//              the clamped reads, which pile onto samples 0 and T_i - 1, are summed by a workgroup each.  No atomics.
//   qmf vjp    the transposed pair as a gather: an input sample sums the taps that read it, through its own position and through its two
//              possible reflections, in that order.
#include "common.h"

#include <limits.h>

namespace dsa {
namespace {

enum { AP_QMF = 0, AP_QMF_VJP = 1, AP_TANDEM = 2, AP_TANDEM_VJP = 3 };
const char* const kApRoutes[4][2] = {
    {"ap_qmf_f32", "ap_qmf_f64"}, {"ap_qmf_vjp_f32", "ap_qmf_vjp_f64"}, {"ap_tandem_f32", "ap_tandem_f64"}, {"ap_tandem_vjp_f32", "ap_tandem_vjp_f64"}};

constexpr int AP_THREADS = 256;    // the pyramid's and the overlap-add's workgroup
constexpr int AP_HP = 41, AP_LP = 37, AP_HALF = 20;   // ap.py:376-424; the low-pass sits two taps inside the high-pass
constexpr int AP_TRIALS = 9;       // ap.py:342-348: m = 10^0 .. 10^8 can succeed; the tenth trial raises either way
constexpr int AP_HEAD = 2 * DSA_AP_MAX_BANDS;   // float64 words in front of the runs: the band values, the block reductions' exchange

// The QMF pair of TANDEM-STRAIGHT's band splitting (ap.py:376-424: the values WORLD's first aperiodicity estimator ships).  Both filters are
// symmetric: the first half and the centre tap.
__device__ const double kApHigh[AP_HALF + 1] = {
    +0.00041447996898231424, +0.00078125051417292477, -0.0010917236836275842, -0.0019867925675967589, +0.0020903896961562292,
    +0.0040940570272849346,  -0.0034025808529816698,  -0.0074961541272056016, +0.0049722633399330637, +0.012738791249119802,
    -0.0066960326895749113,  -0.020694051570247052,   +0.0084324365650413451, +0.033074383758700532,  -0.010018936738799522,
    -0.054231361405808247,   +0.011293988915051487,   +0.10020081367388213,   -0.012120546202484579,  -0.31630021039095702,
    +0.51240682580627639};
__device__ const double kApLow[AP_HALF - 1] = {
    -0.00065488170077483048, +0.00007561994958159384, +0.0020408456937895227, -0.00074680535322030437, -0.0043502235688264931,
    +0.0025966428382642732,  +0.0076396022827566962,  -0.0064904118901497852, -0.011765804538954506,   +0.013649908479276255,
    +0.01636866479016021,    -0.026075976030529347,   -0.020910294856659444,  +0.048260725032316647,   +0.024767846611048111,
    -0.096178467583360641,   -0.027359756709866623,   +0.31488052161630042,   +0.52827343594055032};
__device__ __forceinline__ void ap_load_taps(double* sh, double* sl)
{
    if (threadIdx.x < AP_HP) sh[threadIdx.x] = kApHigh[threadIdx.x <= AP_HALF ? threadIdx.x : AP_HP - 1 - threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + AP_LP) {
        const int k = threadIdx.x - 64;
        sl[k] = kApLow[k <= AP_HALF - 2 ? k : AP_LP - 1 - k];
    }
    __syncthreads();
}

struct ApGeom {
    int n_band;
    int seg[DSA_AP_MAX_BANDS];     // J
    long off[DSA_AP_MAX_BANDS];    // the band's first column in a row of `bands`
    long len[DSA_AP_MAX_BANDS];    // T_i
    double fs[DSA_AP_MAX_BANDS];   // tmp_fs = 2 cutoff
    long runs;                     // sum of J + 2
};

template <typename T>
__device__ __forceinline__ long ap_trunc(T v)   // Tensor.int(); what no int32 holds is pinned, a NaN is 0: the indices are clamped anyway
{
    if (!(v == v)) return 0;
    return v < T(-2.0e9) ? -2000000000L : v > T(2.0e9) ? 2000000000L : (long)v;
}

__device__ __forceinline__ long ap_reflect(long i, long T) { return i < 0 ? -i : i >= T ? 2 * (T - 1) - i : i; }

// ---------------------------------------------------------------------------------------------------------------- pyramid
template <typename T>
__global__ __launch_bounds__(AP_THREADS) void ap_qmf_kernel(const T* __restrict__ x, long Tin, long ldx, long Tout, double* __restrict__ hp,
                                                            long ldhp, double* __restrict__ lp, long ldlp)
{
    __shared__ double sh[AP_HP], sl[AP_LP];
    ap_load_taps(sh, sl);
    const long o = (long)blockIdx.x * AP_THREADS + threadIdx.x, b = blockIdx.y;
    if (o >= Tout) return;
    const T* row = x + b * ldx;
    double ah = 0, al = 0;
    for (int k = 0; k < AP_HP; ++k) {
        const double v = (double)row[ap_reflect(2 * o - AP_HALF + k, Tin)];
        ah += sh[k] * v;
        if (k >= 2 && k < 2 + AP_LP) al += sl[k - 2] * v;
    }
    hp[b * ldhp + o] = ah;
    lp[b * ldlp + o] = al;
}

template <typename T>
__global__ __launch_bounds__(AP_THREADS) void ap_qmf_vjp_kernel(const double* __restrict__ ghp, long ldgh, const double* __restrict__ glp,
                                                                long ldgl, long Tin, long Tout, T* __restrict__ gx, long ldgx)
{
    __shared__ double sh[AP_HP], sl[AP_LP];
    ap_load_taps(sh, sl);
    const long j = (long)blockIdx.x * AP_THREADS + threadIdx.x, b = blockIdx.y;
    if (j >= Tin) return;
    const double* gh = ghp + b * ldgh;
    const double* gl = glp + b * ldgl;
    // the padded positions that read sample j: itself, its mirror at the head, its mirror at the tail
    const long pos[3] = {j, (j >= 1 && j <= AP_HALF) ? -j : LONG_MIN, (j < Tin - 1 && j >= Tin - 1 - AP_HALF) ? 2 * (Tin - 1) - j : LONG_MIN};
    double acc = 0;
    for (int s = 0; s < 3; ++s) {
        const long p = pos[s];
        if (p == LONG_MIN) continue;
        long lo = (p - AP_HALF + 1) >> 1, hi = (p + AP_HALF) >> 1;   // ceil and floor of the halves
        lo = lo < 0 ? 0 : lo;
        hi = hi > Tout - 1 ? Tout - 1 : hi;
        for (long o = lo; o <= hi; ++o) {
            const int k = (int)(p - 2 * o + AP_HALF);
            acc += sh[k] * gh[o];
            if (k >= 2 && k < 2 + AP_LP) acc += sl[k - 2] * gl[o];
        }
    }
    gx[b * ldgx + j] = (T)acc;
}

// ---------------------------------------------------------------------------------------------------------------- the fit
__device__ __forceinline__ constexpr int ap_q(int r, int c) { return r * (r + 1) / 2 + c; }   // the packed lower triangle

// the factor Lm of L L' = R + lam I; false when a pivot is not positive and finite (the later entries are then meaningless)
__device__ __forceinline__ bool ap_cholesky(const double (&R)[21], double lam, double (&Lm)[21])
{
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double s = R[ap_q(r, c)] + (r == c ? lam : 0.0);
#pragma unroll
            for (int k = 0; k < c; ++k) s -= Lm[ap_q(r, k)] * Lm[ap_q(c, k)];
            if (r == c) {
                ok = ok && s > 0.0 && s <= 1.7976931348623157e308;
                Lm[ap_q(r, r)] = sqrt(s);
            } else {
                Lm[ap_q(r, c)] = s / Lm[ap_q(c, c)];
            }
        }
    }
    return ok;
}

__device__ __forceinline__ void ap_solve(const double (&Lm)[21], const double (&rhs)[6], double (&out)[6])
{
    double t[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = rhs[r];
#pragma unroll
        for (int k = 0; k < r; ++k) s -= Lm[ap_q(r, k)] * t[k];
        t[r] = s / Lm[ap_q(r, r)];
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = t[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s -= Lm[ap_q(k, r)] * out[k];
        out[r] = s / Lm[ap_q(r, r)];
    }
}

// the value of output bin k before the clip, from the band values; idx0 / wgt: the pair it reads and the upper weight
template <typename T>
__device__ __forceinline__ double ap_bin(const double* vals, int n_band, const int64_t* __restrict__ iidx, const T* __restrict__ iw, int k,
                                         int& d0, double& wgt, bool& dead)
{
    if (!iidx) {
        d0 = k;
        wgt = 0;
        const double v = vals[k == 0 ? n_band - 1 : n_band - k];
        dead = false;
        return v;
    }
    long i = iidx[k];
    i = i < 0 ? 0 : i > n_band - 1 ? n_band - 1 : i;
    d0 = (int)i;
    wgt = (double)iw[k];
    const double v0 = vals[d0 == 0 ? n_band - 1 : n_band - d0], v1 = vals[n_band - (d0 + 1)];
    dead = v0 == 0.0 || v1 == 0.0;   // an exactly silent band: the bins it reaches are 0 before the clip
    if (dead) return 0.0;
    const double y0 = log(v0);
    return exp((log(v1) - y0) * wgt + y0);
}

__device__ __forceinline__ double ap_clip(double v, double lo, double hi) { return v < lo ? lo : v > hi ? hi : v; }   // a NaN stays

template <typename T, bool VJP>
__global__ __launch_bounds__(64 * DSA_AP_MAX_BANDS) void ap_tandem_kernel(
    const double* __restrict__ bands, long ldb, const T* __restrict__ f0, long N, const T* __restrict__ window, const T* __restrict__ wsqrt, long ldw,
    const int64_t* __restrict__ iidx, const T* __restrict__ iw, int K, ApGeom g, T step, T eps, double lo, double hi, int fmt,
    T* __restrict__ y, const T* __restrict__ gy, T* __restrict__ gruns, int64_t* __restrict__ starts)
{
    extern __shared__ double lds[];
    constexpr int NRUN = VJP ? 5 : 3;
    const int band = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long n = blockIdx.x, b = blockIdx.y;
    double* vals = lds;
    long before = 0;
    for (int i = 0; i < band; ++i) before += g.seg[i] + 2;
    const int J = g.seg[band], R = J + 2;
    double* ra = lds + AP_HEAD + NRUN * before;
    double* rb = ra + R;
    double* rg = rb + R;

    // the decisions (ap.py:295-317), in the data's dtype
    T f = f0[b * N + n];
    if (f <= T(32)) f = T(150);
    const T fs = (T)g.fs[band];
    const T pitch = rn_div(fs, f);
    const long t0 = ap_trunc(rn_add(pitch, T(0.5)));
    const long bias = ap_trunc(rn_add(rn_mul(pitch, T(0.5)), T(0.5)));
    const long cpos = ap_trunc(rn_add(rn_mul(rn_mul((T)n, step), fs), T(1.5)));
    const long origin = cpos - bias;
    const long sa = origin - t0 - 1, sb = origin + t0 - 1, sg = origin - 1;
    const long last = g.len[band] - 1;
    const double* row = bands + b * ldb + g.off[band];
    for (int p = lane; p < R; p += 64) {
        const long ia = sa + p, ib = sb + p, ig = sg + p;
        ra[p] = row[ia < 0 ? 0 : ia > last ? last : ia];
        rb[p] = row[ib < 0 ? 0 : ib > last ? last : ib];
        rg[p] = row[ig < 0 ? 0 : ig > last ? last : ig];
    }
    if (VJP && lane == 0) {
        int64_t* s = starts + ((b * N + n) * g.n_band + band) * DSA_AP_START_WORDS;
        s[0] = sa, s[1] = sb, s[2] = sg, s[3] = cpos;
    }
    __syncthreads();

    const T* w = window + band * ldw;
    const T* ws = wsqrt + band * ldw;
    double Rm[21], bv[6];
#pragma unroll
    for (int q = 0; q < 21; ++q) Rm[q] = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) bv[q] = 0;
    for (int j = lane; j < J; j += 64) {
        const double h[6] = {ra[j], ra[j + 1], ra[j + 2], rb[j], rb[j + 1], rb[j + 2]};
        const double x = rg[j + 1], wj = (double)w[j];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double wh = wj * h[r];
#pragma unroll
            for (int c = 0; c <= r; ++c) Rm[ap_q(r, c)] += wh * h[c];
            bv[r] += wh * x;
        }
    }
#pragma unroll
    for (int q = 0; q < 21; ++q) Rm[q] = wave_sum(Rm[q]);
#pragma unroll
    for (int q = 0; q < 6; ++q) bv[q] = wave_sum(bv[q]);

    double Lm[21], a[6];
    bool ok = false;
    T m = 1;
    int trials = 0;   // the failed ones: m = 10^trials is the factor's; AP_TRIALS when none factors
    for (; trials < AP_TRIALS; ++trials, m = rn_mul(m, T(10))) {
        ok = ap_cholesky(Rm, (double)rn_mul(eps, m), Lm);
        if (ok) break;
    }
    if (VJP && lane == 0) starts[((b * N + n) * g.n_band + band) * DSA_AP_START_WORDS + 4] = trials;
    if (ok) {
        ap_solve(Lm, bv, a);
    } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) a[q] = 0;
    }

    // the two stds (ap.py:354-359): means, then centred squares
    double sv = 0, su = 0;
    for (int j = lane; j < J; j += 64) {
        const double x = rg[j + 1], s = (double)ws[j];
        const double r = x - (ra[j] * a[0] + ra[j + 1] * a[1] + ra[j + 2] * a[2] + rb[j] * a[3] + rb[j + 1] * a[4] + rb[j + 2] * a[5]);
        sv += s * r;
        su += s * x;
    }
    const double mv = wave_sum(sv) / J, mu = wave_sum(su) / J;
    sv = su = 0;
    for (int j = lane; j < J; j += 64) {
        const double x = rg[j + 1], s = (double)ws[j];
        const double r = x - (ra[j] * a[0] + ra[j + 1] * a[1] + ra[j + 2] * a[2] + rb[j] * a[3] + rb[j + 1] * a[4] + rb[j + 2] * a[5]);
        const double dv = s * r - mv, du = s * x - mu;
        sv += dv * dv;
        su += du * du;
    }
    const double numer = sqrt(wave_sum(sv) / (J - 1)), denom = sqrt(wave_sum(su) / (J - 1));
    const double A = ok ? numer / (denom + 1e-16) : hi;   // a fit that no trial factors: the upper bound, and no gradient
    if (lane == 0) vals[band] = A;
    __syncthreads();

    if (!VJP) {
        T* out = y + (b * N + n) * (long)K;
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            int d0;
            double wgt;
            bool dead;
            const double c = ap_clip(ap_bin(vals, g.n_band, iidx, iw, k, d0, wgt, dead), lo, hi);
            out[k] = (T)(fmt == 0 ? c : fmt == 1 ? 1 - c : fmt == 2 ? c / (1 - c) : (1 - c) / c);
        }
        return;
    }

    // ---- the adjoint.  The cotangent of this wave's band value: the bins that reach position d = n_band - band (and 0, for the lowest)
    const T* gout = gy + (b * N + n) * (long)K;
    double gA = 0;
    const int mine = g.n_band - band;
    for (int k = lane; k < K; k += 64) {
        int d0;
        double wgt;
        bool dead;
        const double v = ap_bin(vals, g.n_band, iidx, iw, k, d0, wgt, dead);
        if (dead || !(v >= lo && v <= hi)) continue;   // clipped, silent or NaN: nothing passes
        const double gc = (double)gout[k] * (fmt == 0 ? 1.0 : fmt == 1 ? -1.0 : fmt == 2 ? 1.0 / ((1 - v) * (1 - v)) : -1.0 / (v * v));
        if (!iidx) {
            if (d0 == mine || (d0 == 0 && band == g.n_band - 1)) gA += gc;
            continue;
        }
        const double gv = gc * v;   // onto the interpolated logarithm
        const int d1 = d0 + 1;
        if (d0 == mine || (d0 == 0 && band == g.n_band - 1)) gA += gv * (1 - wgt) / A;
        if (d1 == mine) gA += gv * wgt / A;
    }
    gA = wave_sum(gA);
    const bool live = ok && denom > 0.0;   // a zero-variance denominator: no gradient
    const double dn = denom + 1e-16;
    const double cn = live && numer > 0.0 ? gA / dn / ((J - 1) * numer) : 0.0;
    const double cd = live ? -gA * numer / (dn * dn) / ((J - 1) * denom) : 0.0;

    double ga[6], z[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) ga[q] = 0;
    for (int j = lane; j < J; j += 64) {
        const double h[6] = {ra[j], ra[j + 1], ra[j + 2], rb[j], rb[j + 1], rb[j + 2]};
        const double x = rg[j + 1], s = (double)ws[j];
        const double r = x - (h[0] * a[0] + h[1] * a[1] + h[2] * a[2] + h[3] * a[3] + h[4] * a[4] + h[5] * a[5]);
        const double gr = cn != 0.0 ? s * cn * (s * r - mv) : 0.0;   // (a fit that did not factor may hold NaN: 0 NaN is not 0)
#pragma unroll
        for (int q = 0; q < 6; ++q) ga[q] -= h[q] * gr;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) ga[q] = wave_sum(ga[q]);
    if (ok) {
        ap_solve(Lm, ga, z);
    } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) z[q] = 0;
    }
    // per j: g_H[j][c] = al[j] a[c] + be[j] z[c];  g_X[j] to the third run's cotangent
    double* al = rg + R;
    double* be = al + R;
    T* grow = gruns + ((b * N + n) * g.runs + before) * 3;
    for (int j = lane; j < J; j += 64) {
        const double h[6] = {ra[j], ra[j + 1], ra[j + 2], rb[j], rb[j + 1], rb[j + 2]};
        const double x = rg[j + 1], s = (double)ws[j], wj = (double)w[j];
        const double r = x - (h[0] * a[0] + h[1] * a[1] + h[2] * a[2] + h[3] * a[3] + h[4] * a[4] + h[5] * a[5]);
        const double gr = cn != 0.0 ? s * cn * (s * r - mv) : 0.0;
        const double hz = h[0] * z[0] + h[1] * z[1] + h[2] * z[2] + h[3] * z[3] + h[4] * z[4] + h[5] * z[5];
        al[j] = ok ? -gr - wj * hz : 0.0;
        be[j] = ok ? wj * r : 0.0;
        grow[2 * R + j + 1] = ok ? (T)((cd != 0.0 ? s * cd * (s * x - mu) : 0.0) + gr + wj * hz) : T(0);
    }
    if (lane == 0) grow[2 * R] = T(0), grow[2 * R + R - 1] = T(0);
    __syncthreads();
    for (int p = lane; p < R; p += 64) {
        double s0 = 0, s1 = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int j = p - c;
            if (j >= 0 && j < J) {
                s0 += al[j] * a[c] + be[j] * z[c];
                s1 += al[j] * a[3 + c] + be[j] * z[3 + c];
            }
        }
        grow[p] = (T)s0;
        grow[R + p] = (T)s1;
    }
}

// the runs' cotangents back onto the band samples: grid (blocks + 2, band, utterance); the last two workgroups take samples 0 and T_i - 1
template <typename T>
__global__ __launch_bounds__(AP_THREADS) void ap_overlap_kernel(const T* __restrict__ gruns, const int64_t* __restrict__ starts, long N, ApGeom g,
                                                                unsigned blocks, double* __restrict__ gbands, long ldg)
{
    __shared__ double red[AP_THREADS / 64];
    const int band = blockIdx.y;
    const long b = blockIdx.z, len = g.len[band];
    const int J = g.seg[band], R = J + 2;
    long before = 0;
    for (int i = 0; i < band; ++i) before += g.seg[i] + 2;
    // |start - curr_pos| of any run: index_bias + t0 + 1 below, t0 - 1 above, with pitch <= tmp_fs / 32 (F0 above 32 Hz, or 150)
    const long t0max = (long)(g.fs[band] / 32) + 2, below = t0max + (long)(g.fs[band] / 64) + 3, above = t0max;
    const int64_t* st = starts + (b * N * g.n_band + band) * DSA_AP_START_WORDS;   // frame n: st[n * stride + r]; curr_pos at r = 3, non-decreasing in n
    const long stride = (long)g.n_band * DSA_AP_START_WORDS;
    const T* gr = gruns + (b * N * g.runs + before) * 3;          // frame n: gr[n * g.runs * 3 + r * R + p]
    const long gstride = g.runs * 3;
    double* out = gbands + b * ldg + g.off[band];
    auto first_at_least = [&](long v) {   // the first frame with curr_pos >= v, N if none
        long a = 0, c = N;
        while (a < c) {
            const long mid = (a + c) >> 1;
            if (st[mid * stride + 3] >= v) c = mid; else a = mid + 1;
        }
        return a;
    };
    if (blockIdx.x < blocks) {
        const long q = (long)blockIdx.x * AP_THREADS + threadIdx.x;
        if (q <= 0 || q >= len - 1) return;
        const long n0 = first_at_least(q - above - R), n1 = first_at_least(q + below + 1);
        double acc = 0;
        for (long n = n0; n < n1; ++n)
            for (int r = 0; r < 3; ++r) {
                const long p = q - st[n * stride + r];
                if (p >= 0 && p < R) acc += (double)gr[n * gstride + r * R + p];
            }
        out[q] = acc;
        return;
    }
    const bool head = blockIdx.x == blocks;
    const long n0 = head ? 0 : first_at_least(len - 1 - above - R), n1 = head ? first_at_least(below + 1) : N;
    const long items = (n1 - n0) * 3 * R;
    double acc = 0;
    for (long i = threadIdx.x; i < items; i += AP_THREADS) {
        const long n = n0 + i / (3 * R);
        const int r = (int)(i / R % 3), p = (int)(i % R);
        const long at = st[n * stride + r] + p;
        if (head ? at <= 0 : at >= len - 1) acc += (double)gr[n * gstride + r * R + p];
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[head ? 0 : len - 1] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- host
int ap_check_qmf(int64_t B, int64_t T, int32_t dtype)
{
    if (!(B >= 0 && T >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: unknown dtype");
    if (B > 65535 || T > INT64_MAX / 16 / (B > 0 ? B : 1)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes");
    return DSA_OK;
}

// the bands of ap.py:232-238, 264-266 and 304-310 for an utterance of T samples
int ap_geometry(ApGeom& g, int64_t B, int64_t N, int64_t T, int32_t P, int32_t sr, double wms, int32_t K, bool interp, int32_t fmt, int32_t dtype)
{
    if (!(B >= 0 && N >= 0 && T >= 0 && K >= 1)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: unknown dtype");
    if (!(P >= 1 && sr >= 1200 && wms > 0 && fmt >= 0 && fmt <= 3)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid options");
    int nb = 0;
    while (600LL << (nb + 1) <= (long long)sr) ++nb;   // int(log2(sr / 600))
    if (nb > DSA_AP_MAX_BANDS) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: more than DSA_AP_MAX_BANDS (8) bands");
    g.n_band = nb;
    g.runs = 0;
    int64_t level = T, off = 0, S = 0;
    for (int i = 0; i < nb; ++i) {
        const double cutoff = (double)sr / (double)(1LL << (i + 2 > nb ? nb : i + 2));
        const double J = cutoff * wms / 500 + 1.5;
        if (!(J >= 2)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: window_length_ms gives a segment shorter than 2 samples");
        if (!(J < 1e6))
            return fail(DSA_ERR_INVALID_ARGUMENT,
                        "ap: DSA_AP_LDS_BYTES(sum(J), n_band) exceed DSA_AP_MAX_LDS_BYTES (163840 bytes per workgroup): a segment of 10^6 samples or more");
        g.seg[i] = (int)J;
        g.fs[i] = 2 * cutoff;
        if (i < nb - 1) level = level > 0 ? (level - 1) / 2 + 1 : 0;
        g.len[i] = level;
        g.off[i] = off;
        off += level;
        S += g.seg[i];
        g.runs += g.seg[i] + 2;
    }
    if (DSA_AP_LDS_BYTES(S, nb) > DSA_AP_MAX_LDS_BYTES)
        return fail(DSA_ERR_INVALID_ARGUMENT,
                    "ap: DSA_AP_LDS_BYTES(sum(J), n_band) = 40 (sum(J) + 2 n_band) + 128 bytes exceed DSA_AP_MAX_LDS_BYTES (163840 bytes per workgroup)");
    if (!interp && K != nb + 1) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: without the interpolation tables the output has n_band + 1 values");
    if (B > 65535 || N > INT32_MAX || (dtype == DSA_F32 && N > (1 << 24)) || (N > 0 && B > INT64_MAX / 64 / N / (g.runs > K ? g.runs : K)) ||
        T > INT64_MAX / 16 / (B > 0 ? B : 1))
        return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes (a float32 frame index is exact up to 2^24)");
    return DSA_OK;
}

template <typename T, bool VJP>
int ap_launch_tandem(const ApGeom& g, const void* bands, int64_t ldb, const void* f0, const void* window, const void* wsqrt, int64_t ldw,
                     const void* iidx, const void* iw, int64_t B, int64_t N, int32_t P, int32_t sr, int32_t K, double eps, double lo, double hi,
                     int32_t fmt, void* y, const void* gy, void* gruns, void* starts, hipStream_t st)
{
    const size_t lds = 8 * ((size_t)AP_HEAD + (VJP ? 5 : 3) * (size_t)g.runs);
    return launch_lds<ap_tandem_kernel<T, VJP>>(DSA_AP_MAX_LDS_BYTES, "ap: cannot raise the dynamic LDS limit", dim3((unsigned)N, (unsigned)B),
                                                dim3(64 * g.n_band), lds, st, (const double*)bands, (long)ldb, (const T*)f0, (long)N, (const T*)window,
                                                (const T*)wsqrt, (long)ldw, (const int64_t*)iidx, (const T*)iw, (int)K, g, (T)((double)P / (double)sr),
                                                (T)eps, lo, hi, (int)fmt, (T*)y, (const T*)gy, (T*)gruns, (int64_t*)starts);
}

template <typename T>
void ap_launch_overlap(const ApGeom& g, const void* gruns, const void* starts, int64_t B, int64_t N, void* gbands, int64_t ldg, hipStream_t st)
{
    const unsigned blocks = (unsigned)((g.len[0] + AP_THREADS - 1) / AP_THREADS);   // band 0 is the longest
    hipLaunchKernelGGL((ap_overlap_kernel<T>), dim3(blocks + 2, (unsigned)g.n_band, (unsigned)B), dim3(AP_THREADS), 0, st, (const T*)gruns,
                       (const int64_t*)starts, (long)N, g, blocks, (double*)gbands, (long)ldg);
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_ap_qmf(const void* x, int64_t B, int64_t T, int64_t ldx, int32_t dtype, void* hp, int64_t ldhp, void* lp, int64_t ldlp, void* stream)
{
    if (int rc = ap_check_qmf(B, T, dtype)) return rc;
    if (B == 0 || T == 0) return DSA_OK;
    const int64_t To = (T - 1) / 2 + 1;
    if (T <= AP_HALF) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: a level of the pyramid needs at least 21 samples (the reflection pad of 20)");
    if (!(ldx >= T && ldhp >= To && ldlp >= To && To <= (int64_t)INT32_MAX * AP_THREADS)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes");
    if (!(x && hp && lp)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: null pointer");
    const dim3 grid((unsigned)((To + AP_THREADS - 1) / AP_THREADS), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "ap", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        hipLaunchKernelGGL((ap_qmf_kernel<V>), grid, dim3(AP_THREADS), 0, st, (const V*)x, (long)T, (long)ldx, (long)To, (double*)hp, (long)ldhp,
                           (double*)lp, (long)ldlp);
        return check_launch(kApRoutes[AP_QMF][dtype == DSA_F64]);
    });
}

DSA_EXPORT int dsa_ap_qmf_vjp(const void* ghp, int64_t ldghp, const void* glp, int64_t ldglp, int64_t B, int64_t T, int32_t dtype, void* gx, int64_t ldgx,
                              void* stream)
{
    if (int rc = ap_check_qmf(B, T, dtype)) return rc;
    if (B == 0 || T == 0) return DSA_OK;
    const int64_t To = (T - 1) / 2 + 1;
    if (T <= AP_HALF) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: a level of the pyramid needs at least 21 samples (the reflection pad of 20)");
    if (!(ldgx >= T && ldghp >= To && ldglp >= To && T <= (int64_t)INT32_MAX * AP_THREADS)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes");
    if (!(ghp && glp && gx)) return fail(DSA_ERR_INVALID_ARGUMENT, "ap: null pointer");
    const dim3 grid((unsigned)((T + AP_THREADS - 1) / AP_THREADS), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(dtype, "ap", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        hipLaunchKernelGGL((ap_qmf_vjp_kernel<V>), grid, dim3(AP_THREADS), 0, st, (const double*)ghp, (long)ldghp, (const double*)glp, (long)ldglp,
                           (long)T, (long)To, (V*)gx, (long)ldgx);
        return check_launch(kApRoutes[AP_QMF_VJP][dtype == DSA_F64]);
    });
}

DSA_EXPORT int dsa_ap_tandem(const void* bands, int64_t ldb, const void* f0, const void* window, const void* window_sqrt, int64_t ldw,
                             const void* interp_indices, const void* interp_weights, int64_t B, int64_t N, int64_t T, int32_t P, int32_t sample_rate,
                             double window_length_ms, int32_t K, double eps, double lower_bound, double upper_bound, int32_t out_format, int32_t dtype,
                             void* y, void* stream)
{
    ApGeom g;
    const bool interp = interp_indices || interp_weights;
    if (int rc = ap_geometry(g, B, N, T, P, sample_rate, window_length_ms, K, interp, out_format, dtype)) return rc;
    if (B == 0 || N == 0) return DSA_OK;
    if (g.len[g.n_band - 1] < 2 || ldb < g.off[g.n_band - 1] + g.len[g.n_band - 1] || ldw < g.seg[0])
        return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes (the bands of T samples do not fit their rows, or a band has fewer than 2 samples)");
    if (!(bands && f0 && window && window_sqrt && y) || (interp && !(interp_indices && interp_weights)))
        return fail(DSA_ERR_INVALID_ARGUMENT, "ap: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = with_dtype(dtype, "ap", [&](auto tag) {
        return ap_launch_tandem<decltype(tag), false>(g, bands, ldb, f0, window, window_sqrt, ldw, interp_indices, interp_weights, B, N, P, sample_rate, K,
                                                      eps, lower_bound, upper_bound, out_format, y, nullptr, nullptr, nullptr, st);
    });
    return rc ? rc : check_launch(kApRoutes[AP_TANDEM][dtype == DSA_F64]);
}

DSA_EXPORT int dsa_ap_tandem_vjp(const void* gy, const void* bands, int64_t ldb, const void* f0, const void* window, const void* window_sqrt, int64_t ldw,
                                 const void* interp_indices, const void* interp_weights, int64_t B, int64_t N, int64_t T, int32_t P, int32_t sample_rate,
                                 double window_length_ms, int32_t K, double eps, double lower_bound, double upper_bound, int32_t out_format,
                                 int32_t dtype, void* gruns, void* starts, void* gbands, int64_t ldg, void* stream)
{
    ApGeom g;
    const bool interp = interp_indices || interp_weights;
    if (int rc = ap_geometry(g, B, N, T, P, sample_rate, window_length_ms, K, interp, out_format, dtype)) return rc;
    if (B == 0 || T == 0) return DSA_OK;
    const int64_t cols = g.off[g.n_band - 1] + g.len[g.n_band - 1];
    if (g.len[g.n_band - 1] < 2 || ldb < cols || ldg < cols || ldw < g.seg[0] || g.len[0] > (int64_t)INT32_MAX * AP_THREADS / 2)
        return fail(DSA_ERR_INVALID_ARGUMENT, "ap: invalid sizes (the bands of T samples do not fit their rows, or a band has fewer than 2 samples)");
    if (!(gbands && (N == 0 || (gy && bands && f0 && window && window_sqrt && gruns && starts))) || (interp && !(interp_indices && interp_weights)))
        return fail(DSA_ERR_INVALID_ARGUMENT, "ap: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (N > 0) {
        const int rc = with_dtype(dtype, "ap", [&](auto tag) {
            return ap_launch_tandem<decltype(tag), true>(g, bands, ldb, f0, window, window_sqrt, ldw, interp_indices, interp_weights, B, N, P, sample_rate,
                                                         K, eps, lower_bound, upper_bound, out_format, nullptr, gy, gruns, starts, st);
        });
        if (rc) return rc;
        if (int rc2 = check_launch(kApRoutes[AP_TANDEM_VJP][dtype == DSA_F64])) return rc2;
    }
    return with_dtype(dtype, "ap", [&](auto tag) {
        ap_launch_overlap<decltype(tag)>(g, gruns, starts, B, N, gbands, ldg, st);
        return check_launch(kApRoutes[AP_TANDEM_VJP][dtype == DSA_F64]);
    });
}
