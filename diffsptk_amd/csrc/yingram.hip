// Yingram (include/diffsptk_amd.h, section a22): YIN's cumulative-mean-normalised difference function on a semitone grid,
// Yingram._forward, yingram.py:167-194.  (There: a dozen torch operators over (frames, L) tensors -- a padded copy, a cumulative sum, two
// slices, an autocorrelation through rfft / irfft, a second cumulative sum, a padded copy and two gathers.)  Per frame x[0 .. L-1]:
//   1  d[tau]  = sum_{j < L - tau} (x[j] - x[j + tau])^2,  tau = 1 .. K - 1  (K = lag_max)
//   2  d'[tau] = tau d[tau] / (S_tau + 1e-7),  S_tau = sum_{k <= tau} d[k];  d'[0] = 1
//   3  y[m]    = d'[floor_m] + (lags_m - floor_m) (d'[ceil_m] - d'[floor_m])
// One launch forward, one backward; nothing but x, the tables and y (or gy, x and gx) touches memory.  Two routes:
//   direct  the lag sums as they are written, one lag per thread over x in LDS, every square added in float64: no cancellation.  A frame
//           belongs to a team of 64, 128 or 256 threads, so a workgroup of 256 holds up to four short frames.
//   fft     d[tau] = c[L - tau] + c[L] - c[tau] - 2 r[tau] with c the float64 prefix sums of x^2 and r the autocorrelation through the
//           shared LDS transform (lds_fft.h): the N >= L + K real points packed as N / 2 complex ones, the power spectrum unpacked,
//           packed again and transformed back, all in place.  One frame per workgroup.
// The scan of step 2 (float64, chunk per thread, one exchange through LDS) and the gather of step 3 run in the same workgroup.
// The backward is the adjoint in the same order: the cotangent of d' gathered per lag (the tables are monotone, so a lag's bins are
// one run found by bisection: no atomics), the reverse scan of step 2, and step 1 either as written (direct) or as the correlation of
// the lag cotangents with x through three more transforms (fft).  The fused entry is the forward with a loader that frames on the fly.
#include "common.h"
#include "lds_fft.h"

namespace dsa {
namespace {

// dsa_last_kernel() of the three entries: [entry][route][dtype]
enum { YIN_FWD = 0, YIN_VJP = 1, YIN_FRAME = 2 };
enum { YIN_DIRECT = 0, YIN_FFT = 1 };
const char* const kYinRoutes[3][2][2] = {
    {{"yingram_direct_f32", "yingram_direct_f64"}, {"yingram_fft_f32", "yingram_fft_f64"}},
    {{"yingram_vjp_direct_f32", "yingram_vjp_direct_f64"}, {"yingram_vjp_fft_f32", "yingram_vjp_fft_f64"}},
    {{"frame_yingram_direct_f32", "frame_yingram_direct_f64"}, {"frame_yingram_fft_f32", "frame_yingram_fft_f64"}},
};

constexpr int YIN_DIRECT_THREADS = 256;
constexpr int YIN_FFT_MAX_THREADS = 512;
constexpr int YIN_RED = 16;   // float64 slots of a team's scan exchange: one per wave, at most 8 waves
constexpr double YIN_EPS = 1e-7;

// where a frame's samples come from: row f of (F, L) frames, or frame n of utterance b of a (B, T) waveform, zero outside it
template <typename T>
struct YinRow {
    const T* base;
    long start, len;
    __device__ __forceinline__ T at(int j) const
    {
        const long i = start + j;
        return i >= 0 && i < len ? base[i] : T(0);
    }
};
template <typename T>
struct YinSource {
    const T* x;
    long Tlen, N;
    int L, P, left, framed;
    __device__ __forceinline__ YinRow<T> row(long f) const
    {
        if (!framed) return YinRow<T>{x + f * L, 0, (long)L};
        const long b = f / N, n = f - b * N;
        return YinRow<T>{x + b * Tlen, n * P - left, Tlen};
    }
};

// (prefix sums over a team's threads: team_scan_excl, common.h; red: the team's YIN_RED slots)
// step 2 in place: d[1 .. K-1] -> d'[1 .. K-1], d'[0] = 1.  Thread t owns the lags [lo, hi).
template <typename T>
__device__ __forceinline__ void yin_normalise(T* d, int K, double* red, int t, int team)
{
    const int per = (K - 1 + team - 1) / team;
    const int lo = min(K, 1 + t * per), hi = min(K, lo + per);
    double s = 0;
    for (int k = lo; k < hi; ++k) s += (double)d[k];
    double total;
    double run = team_scan_excl(s, red, t, team, total);
    for (int k = lo; k < hi; ++k) {
        const double v = (double)d[k];
        run += v;
        d[k] = (T)((double)k * v / (run + YIN_EPS));
    }
    if (t == 0) d[0] = T(1);
}

// step 3
template <typename T>
__device__ __forceinline__ void yin_gather(const T* dn, int K, int M, const T* __restrict__ lags, const int64_t* __restrict__ fl,
                                           const int64_t* __restrict__ ce, T* __restrict__ y, int t, int team)
{
    for (int m = t; m < M; m += team) {
        const int64_t f = fl[m], c = ce[m];
        const T a = dn[(int)min(max(f, (int64_t)0), (int64_t)(K - 1))], b = dn[(int)min(max(c, (int64_t)0), (int64_t)(K - 1))];
        const T w = lags[m] - (T)f;
        y[m] = a + w * (b - a);
    }
}

// the first m with a[m] <= v of a non-increasing table
__device__ __forceinline__ int yin_first_le(const int64_t* __restrict__ a, int M, int64_t v)
{
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// the adjoint of step 3 for one lag: the bins whose floor is tau weigh 1 - w, those whose ceiling is tau weigh w (w = 0 where both are)
template <typename T>
__device__ __forceinline__ double yin_cotangent(const T* __restrict__ gy, int M, const T* __restrict__ lags, const int64_t* __restrict__ fl,
                                                const int64_t* __restrict__ ce, int tau)
{
    double s = 0;
    for (int m = yin_first_le(fl, M, tau); m < M && fl[m] == tau; ++m) s += (double)gy[m] * (1.0 - (double)(lags[m] - (T)fl[m]));
    for (int m = yin_first_le(ce, M, tau); m < M && ce[m] == tau; ++m) s += (double)gy[m] * (double)(lags[m] - (T)fl[m]);
    return s;
}

// the adjoint of step 2 in place: g[k] the cotangent of d'[k] -> the cotangent of d[k],
//   g[k] k / (S_k + eps) - sum_{j >= k} g[j] j d[j] / (S_j + eps)^2,  k = 1 .. K-1; g[0] is not read (d'[0] is a constant).
template <typename T>
__device__ __forceinline__ void yin_normalise_adjoint(const T* d, T* g, int K, double* red, int t, int team)
{
    const int per = (K - 1 + team - 1) / team;
    const int lo = min(K, 1 + t * per), hi = min(K, lo + per);
    double s = 0;
    for (int k = lo; k < hi; ++k) s += (double)d[k];
    double total;
    const double s0 = team_scan_excl(s, red, t, team, total);
    double run = s0, qs = 0;
    for (int k = lo; k < hi; ++k) {
        const double v = (double)d[k];
        run += v;
        const double den = run + YIN_EPS;
        qs += (double)g[k] * (double)k * v / (den * den);
    }
    double qall;
    double before = team_scan_excl(qs, red, t, team, qall);
    run = s0;
    for (int k = lo; k < hi; ++k) {
        const double v = (double)d[k];
        run += v;
        const double den = run + YIN_EPS, gk = (double)g[k];
        g[k] = (T)(gk * (double)k / den - (qall - before));
        before += gk * (double)k * v / (den * den);
    }
}

// ---------------------------------------------------------------------------------------------------------------- direct route
// LDS: per team YIN_RED float64, then per team x (L) and d (K)
template <typename T>
__global__ __launch_bounds__(YIN_DIRECT_THREADS) void yin_direct_kernel(YinSource<T> src, long F, int L, int K, int M,
                                                                          const T* __restrict__ lags, const int64_t* __restrict__ fl,
                                                                          const int64_t* __restrict__ ce, int team, T* __restrict__ y)
{
    extern __shared__ __align__(16) unsigned char yin_lds[];
    const int G = YIN_DIRECT_THREADS / team, g = threadIdx.x / team, t = threadIdx.x - g * team;
    double* red = reinterpret_cast<double*>(yin_lds) + g * YIN_RED;
    T* xs = reinterpret_cast<T*>(reinterpret_cast<double*>(yin_lds) + G * YIN_RED) + (long)g * (L + K);
    T* ds = xs + L;
    const long f = (long)blockIdx.x * G + g;
    const bool live = f < F;
    const YinRow<T> row = src.row(live ? f : 0);
    for (int j = t; j < L; j += team) xs[j] = live ? row.at(j) : T(0);
    __syncthreads();
    for (int tau = 1 + t; tau < K; tau += team) {
        double acc = 0;
        for (int j = 0; j < L - tau; ++j) {
            const double dl = (double)(xs[j] - xs[j + tau]);
            acc += dl * dl;
        }
        ds[tau] = (T)acc;
    }
    __syncthreads();
    yin_normalise(ds, K, red, t, team);
    __syncthreads();
    if (live) yin_gather(ds, K, M, lags, fl, ce, y + f * M, t, team);
}

// LDS: per team YIN_RED float64, then per team x (L), d (K) and g (K)
template <typename T>
__global__ __launch_bounds__(YIN_DIRECT_THREADS) void yin_vjp_direct_kernel(const T* __restrict__ x, const T* __restrict__ gy, long F, int L,
                                                                              int K, int M, const T* __restrict__ lags,
                                                                              const int64_t* __restrict__ fl, const int64_t* __restrict__ ce,
                                                                              int team, T* __restrict__ gx)
{
    extern __shared__ __align__(16) unsigned char yin_lds[];
    const int G = YIN_DIRECT_THREADS / team, g = threadIdx.x / team, t = threadIdx.x - g * team;
    double* red = reinterpret_cast<double*>(yin_lds) + g * YIN_RED;
    T* xs = reinterpret_cast<T*>(reinterpret_cast<double*>(yin_lds) + G * YIN_RED) + (long)g * (L + 2 * K);
    T* ds = xs + L;
    T* gs = ds + K;
    const long f = (long)blockIdx.x * G + g;
    const bool live = f < F;
    const T* xf = x + (live ? f : 0) * L;
    const T* gyf = gy + (live ? f : 0) * M;
    for (int j = t; j < L; j += team) xs[j] = live ? xf[j] : T(0);
    __syncthreads();
    for (int tau = 1 + t; tau < K; tau += team) {
        double acc = 0;
        for (int j = 0; j < L - tau; ++j) {
            const double dl = (double)(xs[j] - xs[j + tau]);
            acc += dl * dl;
        }
        ds[tau] = (T)acc;
        gs[tau] = live ? (T)yin_cotangent(gyf, M, lags, fl, ce, tau) : T(0);
    }
    __syncthreads();
    yin_normalise_adjoint(ds, gs, K, red, t, team);
    __syncthreads();
    if (!live) return;
    for (int i = t; i < L; i += team) {   // the adjoint of step 1 as it is written
        const T xi = xs[i];
        double acc = 0;
        const int up = min(K - 1, L - 1 - i), down = min(K - 1, i);
        for (int tau = 1; tau <= up; ++tau) acc += (double)gs[tau] * (double)(xi - xs[i + tau]);
        for (int tau = 1; tau <= down; ++tau) acc += (double)gs[tau] * (double)(xi - xs[i - tau]);
        gx[f * L + i] = (T)(2.0 * acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------- fft route
enum { YIN_POWER = 0, YIN_REAL = 1, YIN_MULT = 2 };

template <typename T>
__device__ __forceinline__ void yin_unscramble(T* re, T* im, int H, int lg)
{   // the transform leaves X[k] at the bit-reversed index: swap it home, every pair by its lower index
    for (int i = threadIdx.x; i < H; i += blockDim.x) {
        const int j = fft_brev(i, lg);
        if (i < j) {
            const T a = re[i], b = im[i];
            re[i] = re[j];
            im[i] = im[j];
            re[j] = a;
            im[j] = b;
        }
    }
    __syncthreads();
}

// re/im: Z = the H-point transform of z[n] = v[2n] + i v[2n+1], natural order; X[k], k = 0 .. H, the 2H-point transform of the real v:
//   X[k] = E + W^k O,  X[H-k] = conj(E - W^k O),  E = (Z[k] + conj Z[H-k]) / 2,  O = (Z[k] - conj Z[H-k]) / 2i,  W = exp(-2 pi i / 2H).
// YIN_REAL   buf[k] = Re X[k] (the whole spectrum of an even v); re/im are left alone.
// YIN_POWER  U = |X[k]|^2, V = |X[H-k]|^2;  YIN_MULT  U = X[k] buf[k], V = conj(X[H-k]) buf[H-k]: the Hermitian spectrum Y whose real
//            inverse is wanted.  re/im[k] = conj(S + iQ), re/im[H-k] = S - iQ with S = U + V, Q = conj(W)^k (U - V): the conjugate of the
//            packed spectrum, so that the FORWARD transform of re/im is conj(v'[2n] + i v'[2n+1]) 2H of the inverse v'.
template <typename T, int MODE>
__device__ __forceinline__ void yin_spectrum(T* re, T* im, T* buf, int H, const T* __restrict__ tw)
{
    for (int k = threadIdx.x; k <= (H >> 1); k += blockDim.x) {
        const int m = k ? H - k : 0;
        const T zkr = re[k], zki = im[k], zmr = re[m], zmi = im[m];
        if (k == 0) {
            const T x0 = zkr + zki, xh = zkr - zki;   // X[0] and X[H], both real
            if (MODE == YIN_REAL) {
                buf[0] = x0;
                buf[H] = xh;
            } else {
                const T u = MODE == YIN_POWER ? x0 * x0 : x0 * buf[0], v = MODE == YIN_POWER ? xh * xh : xh * buf[H];
                re[0] = u + v;
                im[0] = -(u - v);
            }
            continue;
        }
        const T c = tw[2 * k], w1 = tw[2 * k + 1];
        const T er = T(0.5) * (zkr + zmr), ei = T(0.5) * (zki - zmi);
        const T pr = T(0.5) * (zki + zmi), pi = T(-0.5) * (zkr - zmr);
        const T t2r = c * pr - w1 * pi, t2i = c * pi + w1 * pr;
        const T ar = er + t2r, ai = ei + t2i;   // X[k]
        const T br = er - t2r, bi = ei - t2i;   // conj(X[H-k])
        if (MODE == YIN_REAL) {
            buf[k] = ar;
            buf[m] = br;
            continue;
        }
        T ur, ui, vr, vi;
        if (MODE == YIN_POWER) {
            ur = ar * ar + ai * ai;
            vr = br * br + bi * bi;
            ui = vi = T(0);
        } else {
            const T hk = buf[k], hm = buf[m];
            ur = ar * hk;
            ui = ai * hk;
            vr = br * hm;
            vi = bi * hm;
        }
        if (2 * k == H) {   // its own partner: conj(S + iQ) = 2 U
            re[k] = T(2) * ur;
            im[k] = T(2) * ui;
            continue;
        }
        const T sr = ur + vr, si = ui + vi, dr = ur - vr, di = ui - vi;
        const T sn = -w1;
        const T qr = c * dr - sn * di, qi = c * di + sn * dr;
        re[k] = sr - qi;
        im[k] = -(si + qr);
        re[m] = sr + qi;
        im[m] = si - qr;
    }
    __syncthreads();
}

// element n of the real sequence whose conjugated packed transform the last lds_fft_pow2 left in re/im (bit-reversed), times 2H
template <typename T>
__device__ __forceinline__ T yin_unpacked(const T* re, const T* im, int n, int lg)
{
    const int p = fft_brev(n >> 1, lg);
    return n & 1 ? -im[p] : re[p];
}

// d[1 .. K-1] of one frame into buf, by the whole workgroup.  cs: L + 1 float64.  Leaves re/im dead.
template <typename T>
__device__ __forceinline__ void yin_fft_differences(const YinRow<T>& row, int L, int K, int H, int lg, const T* __restrict__ tw, T* re, T* im,
                                                    T* buf, double* cs, double* red)
{
    const int t = threadIdx.x, nt = blockDim.x;
    for (int j = t; j < H; j += nt) {
        re[j] = 2 * j < L ? row.at(2 * j) : T(0);
        im[j] = 2 * j + 1 < L ? row.at(2 * j + 1) : T(0);
    }
    __syncthreads();
    {   // c[n] = sum_{j < n} x[j]^2 in float64
        const int per = (L + nt - 1) / nt;
        const int lo = min(L, t * per), hi = min(L, lo + per);
        double s = 0;
        for (int j = lo; j < hi; ++j) {
            const double v = (double)(j & 1 ? im[j >> 1] : re[j >> 1]);
            s += v * v;
        }
        double total;
        double run = team_scan_excl(s, red, t, nt, total);
        for (int j = lo; j < hi; ++j) {
            const double v = (double)(j & 1 ? im[j >> 1] : re[j >> 1]);
            run += v * v;
            cs[j + 1] = run;
        }
        if (t == 0) cs[0] = 0;
    }
    __syncthreads();   // the transform has no barrier on entry and overwrites, in its first pass, what other waves' chunks above still read
    lds_fft_pow2(re, im, H, lg, tw, 2);
    yin_unscramble(re, im, H, lg);
    yin_spectrum<T, YIN_POWER>(re, im, buf, H, tw);
    lds_fft_pow2(re, im, H, lg, tw, 2);
    const double scale = 1.0 / (2.0 * H);
    for (int tau = 1 + t; tau < K; tau += nt)
        buf[tau] = (T)(cs[L - tau] + cs[L] - cs[tau] - 2.0 * scale * (double)yin_unpacked(re, im, tau, lg));
    __syncthreads();
}

// LDS: cs (L + 1 float64), YIN_RED float64, re, im (H), buf (H + 1)
template <typename T>
struct YinFftLds {
    double *cs, *red;
    T *re, *im, *buf;
    __device__ __forceinline__ YinFftLds(unsigned char* p, int L, int H)
    {
        cs = reinterpret_cast<double*>(p);
        red = cs + L + 1;
        re = reinterpret_cast<T*>(red + YIN_RED);
        im = re + H;
        buf = im + H;
    }
};

template <typename T>
__global__ __launch_bounds__(YIN_FFT_MAX_THREADS) void yin_fft_kernel(YinSource<T> src, int L, int K, int M, int H, int lg,
                                                                        const T* __restrict__ tw, const T* __restrict__ lags,
                                                                        const int64_t* __restrict__ fl, const int64_t* __restrict__ ce,
                                                                        T* __restrict__ y)
{
    extern __shared__ __align__(16) unsigned char yin_lds[];
    const YinFftLds<T> s(yin_lds, L, H);
    const long f = blockIdx.x;
    yin_fft_differences(src.row(f), L, K, H, lg, tw, s.re, s.im, s.buf, s.cs, s.red);
    yin_normalise(s.buf, K, s.red, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    yin_gather(s.buf, K, M, lags, fl, ce, y + f * M, (int)threadIdx.x, (int)blockDim.x);
}

template <typename T>
__global__ __launch_bounds__(YIN_FFT_MAX_THREADS) void yin_vjp_fft_kernel(const T* __restrict__ x, const T* __restrict__ gy, int L, int K, int M,
                                                                            int H, int lg, const T* __restrict__ tw, const T* __restrict__ lags,
                                                                            const int64_t* __restrict__ fl, const int64_t* __restrict__ ce,
                                                                            T* __restrict__ gx)
{
    extern __shared__ __align__(16) unsigned char yin_lds[];
    const YinFftLds<T> s(yin_lds, L, H);
    const int t = threadIdx.x, nt = blockDim.x;
    const long f = blockIdx.x;
    const YinRow<T> row{x + f * L, 0, (long)L};
    const T* gyf = gy + f * M;
    yin_fft_differences(row, L, K, H, lg, tw, s.re, s.im, s.buf, s.cs, s.red);
    T* g = s.re;   // (K <= H: the transform's arrays are free until the next one is packed)
    for (int tau = 1 + t; tau < K; tau += nt) g[tau] = (T)yin_cotangent(gyf, M, lags, fl, ce, tau);
    __syncthreads();
    yin_normalise_adjoint(s.buf, g, K, s.red, t, nt);
    __syncthreads();
    // gx[i] = 2 x[i] (G[min(K-1, L-1-i)] + G[min(K-1, i)]) - 2 sum_tau g[tau] (x[i + tau] + x[i - tau]),  G the prefix sums of g
    for (int tau = 1 + t; tau < K; tau += nt) s.buf[tau] = g[tau];
    if (t == 0) s.buf[0] = T(0);
    __syncthreads();
    double* G = s.cs;
    {
        const int per = (K - 1 + nt - 1) / nt;
        const int lo = min(K, 1 + t * per), hi = min(K, lo + per);
        double sum = 0;
        for (int k = lo; k < hi; ++k) sum += (double)s.buf[k];
        double total;
        double run = team_scan_excl(sum, s.red, t, nt, total);
        for (int k = lo; k < hi; ++k) {
            run += (double)s.buf[k];
            G[k] = run;
        }
        if (t == 0) G[0] = 0;
    }
    // the even sequence h[n] = h[2H - n] = g[n], h[0] = 0, packed; its spectrum is real
    const int N = 2 * H;
    for (int j = t; j < H; j += nt) {
        const int a = 2 * j, b = 2 * j + 1;
        const int ia = a < K ? a : N - a < K ? N - a : 0, ib = b < K ? b : N - b < K ? N - b : 0;   // (index 0 holds the zero)
        s.re[j] = s.buf[ia];
        s.im[j] = s.buf[ib];
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, H, lg, tw, 2);
    yin_unscramble(s.re, s.im, H, lg);
    yin_spectrum<T, YIN_REAL>(s.re, s.im, s.buf, H, tw);
    for (int j = t; j < H; j += nt) {
        s.re[j] = 2 * j < L ? row.at(2 * j) : T(0);
        s.im[j] = 2 * j + 1 < L ? row.at(2 * j + 1) : T(0);
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, H, lg, tw, 2);
    yin_unscramble(s.re, s.im, H, lg);
    yin_spectrum<T, YIN_MULT>(s.re, s.im, s.buf, H, tw);
    lds_fft_pow2(s.re, s.im, H, lg, tw, 2);
    const double scale = 1.0 / (2.0 * H);
    for (int i = t; i < L; i += nt) {
        const double corr = scale * (double)yin_unpacked(s.re, s.im, i, lg);
        const double sums = G[min(K - 1, L - 1 - i)] + G[min(K - 1, i)];
        gx[f * L + i] = (T)(2.0 * ((double)row.at(i) * sums - corr));
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
inline int64_t yin_pow2_at_least(int64_t n)
{
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// what the fft route holds in LDS at the longest lag range a frame length allows, lag_max = L - 1: the ceiling's formula
inline int64_t yin_lds_bytes(int64_t L, int64_t size) { return DSA_YINGRAM_LDS_BYTES(yin_pow2_at_least(2 * L - 1) / 2, L, size); }

int yin_check(const char*& route, int& fft, int entry, int64_t F, int64_t L, int64_t K, int64_t M, int32_t algo, int32_t dtype)
{
    if (!(F >= 0 && L >= 2 && K >= 1 && K < L && M >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: unknown dtype");
    if (algo != DSA_ALGO_AUTO && algo != DSA_ALGO_GENERIC && algo != DSA_ALGO_TUNED) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: unknown algo");
    const int64_t size = dtype == DSA_F32 ? 4 : 8;
    if (L > DSA_YINGRAM_MAX_LDS_BYTES || yin_lds_bytes(L, size) > DSA_YINGRAM_MAX_LDS_BYTES)
        return fail(DSA_ERR_INVALID_ARGUMENT,
                    "yingram: (3 H + 1) sizeof(dtype) + 8 (L + 1) + 128 bytes, 2 H the power of two from 2 L - 1 on, exceed "
                    "DSA_YINGRAM_MAX_LDS_BYTES (163840 bytes per workgroup)");
    // every tensor's byte offset is an int64, every launch dimension an int32: F L, F M, F workgroups
    if (F > INT32_MAX || M > ((int64_t)1 << 24)) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: invalid sizes");
    fft = algo == DSA_ALGO_TUNED || (algo == DSA_ALGO_AUTO && L >= DSA_YINGRAM_FFT_MIN_FRAME_LENGTH);
    route = kYinRoutes[entry][fft][dtype == DSA_F64];
    return DSA_OK;
}

inline int yin_team(int64_t K) { return K - 1 <= 64 ? 64 : K - 1 <= 128 ? 128 : 256; }

struct YinFftPlan {
    int H, lg, threads;
    size_t lds;
};
inline YinFftPlan yin_fft_plan(int64_t L, int64_t K, size_t size)
{
    YinFftPlan p;
    const int64_t N = yin_pow2_at_least(L + K < 4 ? 4 : L + K);
    p.H = (int)(N / 2);
    p.lg = 0;
    while ((1 << p.lg) < p.H) ++p.lg;
    p.threads = p.H / 4 < 64 ? 64 : p.H / 4 > YIN_FFT_MAX_THREADS ? YIN_FFT_MAX_THREADS : p.H / 4;
    p.lds = (size_t)DSA_YINGRAM_LDS_BYTES(p.H, L, size);
    return p;
}

constexpr const char* kYinLdsError = "yingram: cannot raise the dynamic LDS limit";

template <typename T>
int yin_forward(const YinSource<T>& src, int64_t F, int64_t L, int64_t K, int64_t M, const void* lags, const void* fl, const void* ce,
                const void* tw, int fft, void* y, hipStream_t st)
{
    if (fft) {
        const YinFftPlan p = yin_fft_plan(L, K, sizeof(T));
        return launch_lds<yin_fft_kernel<T>>(DSA_YINGRAM_MAX_LDS_BYTES, kYinLdsError, dim3((unsigned)F), dim3(p.threads), p.lds, st,
                                             src, (int)L, (int)K, (int)M, p.H, p.lg, (const T*)tw, (const T*)lags, (const int64_t*)fl, (const int64_t*)ce,
                                             (T*)y);
    }
    const int team = yin_team(K), G = YIN_DIRECT_THREADS / team;
    const size_t lds = (size_t)G * (YIN_RED * 8 + (size_t)(L + K) * sizeof(T));
    return launch_lds<yin_direct_kernel<T>>(DSA_YINGRAM_MAX_LDS_BYTES, kYinLdsError, dim3((unsigned)((F + G - 1) / G)),
                                            dim3(YIN_DIRECT_THREADS), lds, st, src, (long)F, (int)L, (int)K, (int)M, (const T*)lags, (const int64_t*)fl,
                                            (const int64_t*)ce, team, (T*)y);
}

template <typename T>
int yin_backward(const void* gy, const void* x, int64_t F, int64_t L, int64_t K, int64_t M, const void* lags, const void* fl, const void* ce,
                 const void* tw, int fft, void* gx, hipStream_t st)
{
    if (fft) {
        const YinFftPlan p = yin_fft_plan(L, K, sizeof(T));
        return launch_lds<yin_vjp_fft_kernel<T>>(DSA_YINGRAM_MAX_LDS_BYTES, kYinLdsError, dim3((unsigned)F), dim3(p.threads), p.lds,
                                                 st, (const T*)x, (const T*)gy, (int)L, (int)K, (int)M, p.H, p.lg, (const T*)tw, (const T*)lags,
                                                 (const int64_t*)fl, (const int64_t*)ce, (T*)gx);
    }
    const int team = yin_team(K), G = YIN_DIRECT_THREADS / team;
    const size_t lds = (size_t)G * (YIN_RED * 8 + (size_t)(L + 2 * K) * sizeof(T));
    return launch_lds<yin_vjp_direct_kernel<T>>(DSA_YINGRAM_MAX_LDS_BYTES, kYinLdsError, dim3((unsigned)((F + G - 1) / G)),
                                                dim3(YIN_DIRECT_THREADS), lds, st, (const T*)x, (const T*)gy, (long)F, (int)L, (int)K, (int)M,
                                                (const T*)lags, (const int64_t*)fl, (const int64_t*)ce, team, (T*)gx);
}

template <typename T>
YinSource<T> yin_source(const void* x, int64_t Tlen, int64_t N, int64_t L, int64_t P, int left, int framed)
{
    return YinSource<T>{(const T*)x, (long)Tlen, (long)N, (int)L, (int)P, left, framed};
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_yingram(const void* x, int64_t F, int32_t L, int32_t lag_max, const void* lags, const void* lags_floor,
                               const void* lags_ceil, int32_t M, const void* twiddle, int32_t algo, int32_t dtype, void* y, void* stream)
{
    const char* route = "";
    int fft = 0;
    if (int rc = yin_check(route, fft, YIN_FWD, F, L, lag_max, M, algo, dtype)) return rc;
    if (F == 0 || M == 0) return DSA_OK;
    if (!(x && lags && lags_floor && lags_ceil && y) || (fft && !twiddle)) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: null pointer");
    const int rc = with_dtype(dtype, "yingram", [&](auto tag) {
        using T = decltype(tag);
        return yin_forward<T>(yin_source<T>(x, 0, 1, L, 1, 0, 0), F, L, lag_max, M, lags, lags_floor, lags_ceil, twiddle, fft, y, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_yingram_vjp(const void* gy, const void* x, int64_t F, int32_t L, int32_t lag_max, const void* lags, const void* lags_floor,
                               const void* lags_ceil, int32_t M, const void* twiddle, int32_t algo, int32_t dtype, void* gx, void* stream)
{
    const char* route = "";
    int fft = 0;
    if (int rc = yin_check(route, fft, YIN_VJP, F, L, lag_max, M, algo, dtype)) return rc;
    if (F == 0) return DSA_OK;
    if (!(x && gx) || (M > 0 && !(gy && lags && lags_floor && lags_ceil)) || (fft && !twiddle))
        return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: null pointer");
    const int rc = with_dtype(dtype, "yingram", [&](auto tag) {
        return yin_backward<decltype(tag)>(gy, x, F, L, lag_max, M, lags, lags_floor, lags_ceil, twiddle, fft, gx, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_frame_yingram(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t center, int32_t lag_max,
                                     const void* lags, const void* lags_floor, const void* lags_ceil, int32_t M, const void* twiddle,
                                     int32_t algo, int32_t dtype, void* y, void* stream)
{
    const char* route = "";
    int fft = 0;
    if (!(B >= 0 && T >= 0 && P >= 1)) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: invalid sizes");
    const int64_t N = dsa_num_frames(T, P);
    if (N > 0 && B > INT32_MAX / N) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: invalid sizes");
    const int64_t F = B * N;
    if (int rc = yin_check(route, fft, YIN_FRAME, F, L, lag_max, M, algo, dtype)) return rc;
    if (F == 0 || M == 0) return DSA_OK;
    if (!(x && lags && lags_floor && lags_ceil && y) || (fft && !twiddle)) return fail(DSA_ERR_INVALID_ARGUMENT, "yingram: null pointer");
    const int left = center ? L / 2 : 0;
    const int rc = with_dtype(dtype, "yingram", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's signal length)
        return yin_forward<V>(yin_source<V>(x, T, N, L, P, left, 1), F, L, lag_max, M, lags, lags_floor, lags_ceil, twiddle, fft, y, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}
