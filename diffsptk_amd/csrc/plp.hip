// Perceptual linear prediction after the filter bank: PerceptualLinearPredictiveCoefficientsAnalysis._forward, plp.py:313-320
// from `y, E = fbank(x)` on, with levdur.py:114-127 (eps = 0) and mgc2mgc.py:207-300 (lpc2c: in_gamma = -1, in_norm, in_mul ->
// gamma 0).  y:(F,C) log filter-bank outputs, E:(F) log energy:
//   v_c = (exp(y_c) q_c)^cf,  u = [v_0, v_0 .. v_{C-1}, v_{C-1}]                   (equal loudness, compression, replicate1)
//   r_k = sum_n u_n Q[n][k],  k = 0..M                                             (hfft(u, norm="forward")[:M+1])
//   [K, a] = levdur(r):  toeplitz(r[:M]) a = -r[1:],  K = sqrt(r_0 + r[1:].a)
//   c_0 = log K,  c_m = sum_{j=0..N/2} w_j log|A_j| cos(2 pi j m / N),  A_j = 1 + sum_m a_m e^{-2 pi i j m / N}   (the aliased
//   N-point sum of mgc2mgc, folded onto the half spectrum; w_j = -(2/N) {1, 2, .., 2, (1)})
//   c *= lifter,  out = [c_1 .. c_M] (+ c_0) (+ E)                                  (out_format y / yE / yc / ycE)
// The adjoint runs the chain backwards from the saved [K, a]: lifter, gK = gc_0 / K, g log|A_j|, ga_m, the Levinson adjoint
// (R v = abar solved by Levinson's recursion for a general right-hand side: the Toeplitz system's own O(M^2) solver), the transposed
// hfft table, replicate1's adjoint and g y_c = gv_c cf v_c.
//
// One wave per frame.  Lanes run over channels, lags, and the half spectrum in chunks of 64; every per-frame vector lives in the
// wave's own LDS slice (wave-private: __builtin_amdgcn_wave_barrier orders it, LDS operations of a wave run in order), the tables
// are read from memory (one row per m: the lanes of a chunk read consecutive j).  The Levinson recursions run in float64 with one
// lag per lane and cross-lane shuffles.  Every reduction has a fixed order inside the frame's wave: a frame's bits do not depend on
// F.  Kernel and launch geometry depend on (C, M, N, dtype) only.
#include "common.h"

#include <atomic>
#include <climits>

namespace dsa {
namespace {

constexpr int kPlpWaves = 4;   // waves (frames) per block when the LDS slices fit in 64 KiB

// the packed table (utils/tables.py: plp_table), in the dtype of the data
template <typename T>
struct PlpTable {
    const T* q;     // (C)
    const T* Q;     // (C+2, M+1)
    const T* cs;    // (M+1, J)
    const T* sn;    // (M+1, J)
    const T* w;     // (J)
    const T* lift;  // (M+1)
    __device__ PlpTable(const T* tab, int C, int M, int J)
        : q(tab), Q(tab + C), cs(Q + (long)(C + 2) * (M + 1)), sn(cs + (long)(M + 1) * J), w(sn + (long)(M + 1) * J),
          lift(w + J)
    {
    }
};

// bytes of one wave's LDS slice: doubles u (C+2), a, v, gr (64 each); T a, gc (64 each), 2J spectral values
template <typename T>
__host__ __device__ inline long plp_slice_bytes(int C, int J)
{
    long b = 8L * (C + 2 + 3 * 64) + (long)sizeof(T) * (2 * 64 + 2L * J);
    return (b + 15) & ~15L;
}

template <typename T>
struct PlpSlice {
    double* u;
    double* ad;
    double* vd;
    double* grd;
    T* at;
    T* gct;
    T* buf;
    __device__ PlpSlice(unsigned char* base, int C)
    {
        u = reinterpret_cast<double*>(base);
        ad = u + (C + 2);
        vd = ad + 64;
        grd = vd + 64;
        at = reinterpret_cast<T*>(grd + 64);
        gct = at + 64;
        buf = gct + 64;
    }
};

__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }

// u into LDS (float64), then r_k on lane k (k <= M; 0 elsewhere).  plp.py:315-317.
template <typename T>
__device__ __forceinline__ double plp_autocorrelation(const T* __restrict__ y, long f, int C, int M, double cf,
                                                      const PlpTable<T>& tb, double* u, int lane)
{
    for (int c = lane; c < C; c += 64) {
        const T v = dsa_pow(dsa_exp(y[f * C + c]) * tb.q[c], (T)cf);
        u[c + 1] = (double)v;
        if (c == 0) u[0] = (double)v;
        if (c == C - 1) u[C + 1] = (double)v;
    }
    wave_sync();
    double r = 0.0;
    if (lane <= M)
        for (int n = 0; n < C + 2; ++n) r += u[n] * (double)tb.Q[(long)n * (M + 1) + lane];
    wave_sync();
    return r;
}

// levdur.py:114-127 with eps = 0 on r (lag k on lane k): a_lane on lanes 1..M, returns K on every lane.
__device__ __forceinline__ double plp_levinson(double r_lane, int M, double& a, int lane)
{
    const double r0 = __shfl(r_lane, 0, 64);
    a = 0.0;
    double E = r0;
    for (int m = 1; m <= M; ++m) {
        const bool inner = lane >= 1 && lane < m;
        const double rmj = __shfl(r_lane, (m - lane) & 63, 64);   // r[m-j] on lane j
        const double acc = wave_sum(inner ? a * rmj : 0.0);
        const double k = -(__shfl(r_lane, m, 64) + acc) / E;
        const double amj = __shfl(a, (m - lane) & 63, 64);        // a[m-j] on lane j
        if (inner) a += k * amj;
        if (lane == m) a = k;
        E *= (1.0 - k * k);
    }
    return sqrt(wave_sum((lane >= 1 && lane <= M) ? r_lane * a : 0.0) + r0);
}

// Re and Im of A_j = 1 + sum_m a_m e^{-2 pi i j m / N} (a_m = at[m - 1])
template <typename T>
__device__ __forceinline__ void plp_spectrum(const PlpTable<T>& tb, const T* at, int M, int J, int j, T& re, T& im)
{
    re = T(1);
    im = T(0);
    for (int m = 1; m <= M; ++m) {
        const T am = at[m - 1];
        re += am * tb.cs[(long)m * J + j];
        im -= am * tb.sn[(long)m * J + j];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void plp_fwd_kernel(const T* __restrict__ y, const T* __restrict__ E, long F, int C, int M,
                                                      int N, double cf, int fmt, const T* __restrict__ tab, T* __restrict__ out,
                                                      T* __restrict__ save)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char plp_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * (blockDim.x >> 6) + wave;
    if (f >= F) return;
    const int J = N / 2 + 1;
    const PlpTable<T> tb(tab, C, M, J);
    PlpSlice<T> s(plp_smem + plp_slice_bytes<T>(C, J) * wave, C);

    const double r = plp_autocorrelation(y, f, C, M, cf, tb, s.u, lane);
    double a;
    const double K = plp_levinson(r, M, a, lane);
    const T Kt = (T)K, at = (T)a;
    if (lane >= 1 && lane <= M) s.at[lane - 1] = at;
    if (save != nullptr && lane <= M) save[f * (M + 1) + lane] = lane == 0 ? Kt : at;
    wave_sync();

    // w_j log|A_j| over the half spectrum (plp.py:318, mgc2mgc.py:207-300)
    for (int j0 = 0; j0 < J; j0 += 64) {
        const int j = j0 + lane;
        if (j < J) {
            T re, im;
            plp_spectrum(tb, s.at, M, J, j, re, im);
            s.buf[j] = tb.w[j] * (T(0.5) * dsa_log(re * re + im * im));
        }
    }
    wave_sync();
    T c = T(0);
    for (int m = 1; m <= M; ++m) {
        T acc = T(0);
        for (int j = lane; j < J; j += 64) acc += s.buf[j] * tb.cs[(long)m * J + j];
        acc = wave_sum(acc);
        if (lane == m) c = acc;
    }
    if (lane == 0) c = dsa_log(Kt);
    if (lane <= M) c *= tb.lift[lane];   // plp.py:318
    // plp.py:319-320 and the formatter of plp.py:230-239
    const int Mo = M + (fmt & 1) + (fmt >> 1);
    const int src = lane < M ? lane + 1 : 0;   // lane M: c_0 (yc, ycE); E overwrites the last column
    T o = __shfl(c, src, 64);
    if ((fmt & 1) && lane == Mo - 1) o = E[f];
    if (lane < Mo) out[f * Mo + lane] = o;
}

template <typename T>
__global__ __launch_bounds__(256) void plp_bwd_kernel(const T* __restrict__ gout, const T* __restrict__ y, const T* __restrict__ save,
                                                      long F, int C, int M, int N, double cf, int fmt, const T* __restrict__ tab,
                                                      T* __restrict__ gy, T* __restrict__ gE)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char plp_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * (blockDim.x >> 6) + wave;
    if (f >= F) return;
    const int J = N / 2 + 1;
    const PlpTable<T> tb(tab, C, M, J);
    PlpSlice<T> s(plp_smem + plp_slice_bytes<T>(C, J) * wave, C);
    const int Mo = M + (fmt & 1) + (fmt >> 1);

    const double r = plp_autocorrelation(y, f, C, M, cf, tb, s.u, lane);   // lag k on lane k
    const T Kt = save[f * (M + 1)];
    const double K = (double)Kt;
    const T at = (lane >= 1 && lane <= M) ? save[f * (M + 1) + lane] : T(0);
    // cotangent of the liftered cepstrum (the formatter and plp.py:318 transposed)
    T gc = T(0);
    if (lane >= 1 && lane <= M) gc = gout[f * Mo + lane - 1] * tb.lift[lane];
    if (lane == 0 && (fmt & 2)) gc = gout[f * Mo + M] * tb.lift[0];
    if (lane == 0 && gE != nullptr) gE[f] = (fmt & 1) ? gout[f * Mo + Mo - 1] : T(0);
    if (lane >= 1 && lane <= M) {
        s.at[lane - 1] = at;
        s.gct[lane - 1] = gc;
    }
    wave_sync();

    // g log|A_j| = w_j sum_m gc_m cos_mj;  d log|A_j| / d a_m = (Re_j cos_mj - Im_j sin_mj) / |A_j|^2
    for (int j0 = 0; j0 < J; j0 += 64) {
        const int j = j0 + lane;
        if (j < J) {
            T re, im;
            plp_spectrum(tb, s.at, M, J, j, re, im);
            T gl = T(0);
            for (int m = 1; m <= M; ++m) gl += s.gct[m - 1] * tb.cs[(long)m * J + j];
            const T g = tb.w[j] * gl / (re * re + im * im);
            s.buf[j] = g * re;
            s.buf[J + j] = g * im;
        }
    }
    wave_sync();
    double ga = 0.0;
    for (int m = 1; m <= M; ++m) {
        T acc = T(0);
        for (int j = lane; j < J; j += 64) acc += s.buf[j] * tb.cs[(long)m * J + j] - s.buf[J + j] * tb.sn[(long)m * J + j];
        acc = wave_sum(acc);
        if (lane == m) ga = (double)acc;
    }

    // Levinson adjoint (levdur_bwd_kernel's maths, lpc.hip): K = sqrt(r_0 + p.a), R a = -p, p = r[1:], R = toeplitz(r[:M]).
    //   sbar = gK / (2K) with gK = gc_0 / K;  abar = ga + sbar p;  v = R^{-1} abar;
    //   gr_0 = sbar - sum_i v_i a_i - ...;  gr_m = sbar a_m - v_{m-1} - sum_{|i-j| = m} v_i a_j  (the Toeplitz scatter of -v a^T)
    const double sbar = (double)__shfl(gc, 0, 64) / (2.0 * K * K);
    const double abar_hi = ga + sbar * r;                     // abar_{lane-1} on lanes 1..M
    const double b = __shfl(abar_hi, (lane + 1) & 63, 64);  // abar_i on lane i (0..M-1)
    // R v = b by Levinson's recursion: T_n f = e_1, backward vector = reverse(f), x_n solves the leading n x n system
    const double t0 = __shfl(r, 0, 64);
    double fv = lane == 0 ? 1.0 / t0 : 0.0;
    double xv = lane == 0 ? __shfl(b, 0, 64) / t0 : 0.0;
    for (int n = 1; n < M; ++n) {
        const double tni = __shfl(r, (n - lane) & 63, 64);   // t_{n-i} on lane i
        const double ef = wave_sum(lane < n ? tni * fv : 0.0);
        const double ex = wave_sum(lane < n ? tni * xv : 0.0);
        const double fr = __shfl(fv, (n - lane) & 63, 64);   // f_{n-i}: [0; backward vector] at i
        const double fn = ((lane < n ? fv : 0.0) - ef * ((lane >= 1 && lane <= n) ? fr : 0.0)) / (1.0 - ef * ef);
        const double bn = __shfl(fn, (n - lane) & 63, 64);   // the new backward vector
        const double bsc = __shfl(b, n, 64) - ex;
        fv = lane <= n ? fn : 0.0;
        xv = lane <= n ? (lane < n ? xv : 0.0) + bsc * bn : 0.0;
    }
    const T a_lo = __shfl(at, (lane + 1) & 63, 64);          // a_{i+1} on lane i
    if (lane < M) {
        s.vd[lane] = xv;
        s.ad[lane] = (double)a_lo;
    }
    wave_sync();
    if (lane <= M) {
        double acc = 0.0;
        for (int i = 0; i + lane < M; ++i) {
            acc -= s.vd[i] * s.ad[i + lane];
            if (lane > 0) acc -= s.vd[i + lane] * s.ad[i];
        }
        if (lane >= 1) acc += sbar * s.ad[lane - 1] - s.vd[lane - 1];
        if (lane == 0) acc += sbar;
        s.grd[lane] = acc;
    }
    wave_sync();

    // the transposed hfft table, replicate1's adjoint, and the compression / equal-loudness / exp chain
    for (int c = lane; c < C; c += 64) {
        double gv = 0.0;
        const T* Qn = tb.Q + (long)(c + 1) * (M + 1);
        for (int k = 0; k <= M; ++k) gv += s.grd[k] * (double)Qn[k];
        if (c == 0)
            for (int k = 0; k <= M; ++k) gv += s.grd[k] * (double)tb.Q[k];
        if (c == C - 1) {
            const T* Ql = tb.Q + (long)(C + 1) * (M + 1);
            for (int k = 0; k <= M; ++k) gv += s.grd[k] * (double)Ql[k];
        }
        gy[f * C + c] = (T)(gv * cf * s.u[c + 1]);
    }
}

// waves per block and dynamic LDS bytes from (C, N, dtype) only; 0 when one wave's slice exceeds the CU's LDS
template <typename T>
int plp_geometry(int C, int N, long& lds)
{
    const long slice = plp_slice_bytes<T>(C, N / 2 + 1);
    for (int w = kPlpWaves; w >= 1; w >>= 1)
        if (slice * w <= 64 * 1024 || w == 1) {
            lds = slice * w;
            return lds <= 160 * 1024 ? w : 0;
        }
    return 0;
}

template <typename T>
int plp_launch_fwd(const void* y, const void* E, int64_t F, int C, int M, int N, double cf, int fmt, const void* tab, void* out,
                   void* save, hipStream_t st)
{
    long lds = 0;
    const int waves = plp_geometry<T>(C, N, lds);
    if (waves == 0) return fail(DSA_ERR_UNSUPPORTED, "plp: n_channel / n_fft too large for one wave's LDS%s");
    if (int rc = launch_lds<plp_fwd_kernel<T>>(lds > 64 * 1024 ? 160 * 1024 : 0, "plp: cannot raise the LDS limit%s",
                                               dim3((unsigned)((F + waves - 1) / waves)), dim3(64 * waves), (unsigned)lds, st, (const T*)y, (const T*)E,
                                               (long)F, C, M, N, cf, fmt, (const T*)tab, (T*)out, (T*)save))
        return rc;
    return check_launch("plp_fwd");
}

template <typename T>
int plp_launch_bwd(const void* gout, const void* y, const void* save, int64_t F, int C, int M, int N, double cf, int fmt,
                   const void* tab, void* gy, void* gE, hipStream_t st)
{
    long lds = 0;
    const int waves = plp_geometry<T>(C, N, lds);
    if (waves == 0) return fail(DSA_ERR_UNSUPPORTED, "plp_bwd: n_channel / n_fft too large for one wave's LDS%s");
    if (int rc = launch_lds<plp_bwd_kernel<T>>(lds > 64 * 1024 ? 160 * 1024 : 0, "plp_bwd: cannot raise the LDS limit%s",
                                               dim3((unsigned)((F + waves - 1) / waves)), dim3(64 * waves), (unsigned)lds, st, (const T*)gout,
                                               (const T*)y, (const T*)save, (long)F, C, M, N, cf, fmt, (const T*)tab, (T*)gy, (T*)gE))
        return rc;
    return check_launch("plp_bwd");
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_plp_fwd(const void* y, const void* E, int64_t F, int32_t C, int32_t M, int32_t N, double compression_factor,
                           int32_t out_format, const void* table, int32_t dtype, void* out, void* save, void* stream)
{
    DSA_REQUIRE(F >= 0 && M >= 0 && M <= DSA_PLP_MAX_ORDER && C > M && N > M + 1 && out_format >= 0 && out_format <= 3,
                "plp: invalid sizes");
    DSA_REQUIRE(F <= (int64_t)INT32_MAX, "plp: too many frames");
    if (F == 0) return DSA_OK;
    DSA_REQUIRE(y && table && out, "plp: null pointer");
    DSA_REQUIRE(E || !(out_format & 1), "plp: out_format with E needs E");
    return with_dtype(dtype, "plp", [&](auto tag) {
        return plp_launch_fwd<decltype(tag)>(y, E, F, C, M, N, compression_factor, out_format, table, out, save, (hipStream_t)stream);
    });
}

DSA_EXPORT int dsa_plp_bwd(const void* gout, const void* y, const void* save, int64_t F, int32_t C, int32_t M, int32_t N,
                           double compression_factor, int32_t out_format, const void* table, int32_t dtype, void* gy, void* gE,
                           void* stream)
{
    DSA_REQUIRE(F >= 0 && M >= 0 && M <= DSA_PLP_MAX_ORDER && C > M && N > M + 1 && out_format >= 0 && out_format <= 3,
                "plp_bwd: invalid sizes");
    DSA_REQUIRE(F <= (int64_t)INT32_MAX, "plp_bwd: too many frames");
    if (F == 0) return DSA_OK;
    DSA_REQUIRE(gout && y && save && table && gy, "plp_bwd: null pointer");
    return with_dtype(dtype, "plp_bwd", [&](auto tag) {
        return plp_launch_bwd<decltype(tag)>(gout, y, save, F, C, M, N, compression_factor, out_format, table, gy, gE, (hipStream_t)stream);
    });
}
