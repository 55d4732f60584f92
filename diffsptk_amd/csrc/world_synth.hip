// WORLD synthesis (include/diffsptk_amd.h, section a24): WorldSynthesis.forward, world_synth.py:166-321, with get_minimum_phase_spectrum and
// interp1 of third_party/world/common.py:73-84, 141-163.  (There: about sixty torch operators over (pulses, L) tensors -- a nonzero, boolean
// gathers, two irfft -> rfft -> exp chains, two hfft with flips and fftshifts, and a flat scatter_add_.)  Three launches forward, two backward.
//
//   pulses     one workgroup per utterance.  Per sample i < N P, in the data's dtype and with every product and sum rounded on its own (the
//              decisions below are discontinuous in this arithmetic, so it follows the reference operation by operation):
//                t_i = i / sr;  x_n = n (P / sr);  idx = the first n with x_n >= t_i (searchsorted, right = False);
//                m = (y_idx - y_(idx-1)) / (x_idx - x_(idx-1)),  b = y_(idx-1) - m x_(idx-1),  value = m t_i + b   (y_0 / y_(N-1) at the ends)
//              for y = F0 (0 below sr / L + 1) and for y = the voicing flag; voiced_i = 1/2 < flag; f_i = voiced ? F0_i : default_f0;
//              phase_i = (dtype) sum_{j <= i} (tau / sr) (double) f_j;  wrap_i = fmod(phase_i, tau);  a pulse at i where pi < |wrap_(i+1) - wrap_i|.
//              The float64 sum is the SEQUENTIAL one of torch.cumsum: the terms are formed by all threads, 2048 at a time into LDS, and
//              added in order by one lane (a parallel scan moves the last place of the phase, which moved the fractional shift of
//              a float64 pulse by 4e-12 of a sample: more than a unit in the last place of every input does).
//              Pulses are counted per thread, the counts scanned, and the records written in time order.
//   responses  one workgroup per pulse, everything between the input rows and the L response values in LDS: the two rows of sp and ap
//              interpolated and clipped, both minimum-phase spectra, the fractional shift, the noise spectrum and the two inverse
//              transforms, as FOUR complex L-point transforms (lds_fft.h), each carrying two real sequences:
//                1  z = (log S1) / 2 + i (log S2) / 2, both real and even  ->  Z = L c1 + i L c2, the two cepstra;
//                2  z = fold(c1) + i fold(c2)  ->  A1, A2 by the Hermitian split; M = exp(A);
//                3  z = the masked, centred noise  ->  its spectrum;
//                4  W = full(M1 e^(-i k coef)) + i full(M2 noise spectrum), both Hermitian  ->  the forward transform of W read at
//                   (L/2 - n) mod L: the reversal of hfft's output and the fftshift are that index; real part periodic, imaginary aperiodic;
//              then the DC removal, the voiced mask and the sqrt(noise_size) / L scaling.
//   overlap    one thread per output sample: the pulses whose response covers it are one run of its utterance's sorted indices, found by
//              bisection, and added in ascending order.  No atomics; the narrow(L / 2, T) is an offset.
//   vjp pulses one workgroup per pulse: transforms 1 to 3 again, which leave X = M1 e^(-i k coef) and Y = M2 noise spectrum; the cotangent
//              read from gy; then the adjoint with three more transforms: the spectra of the two response cotangents (g_X, g_Y; then
//              g_A = g conj(X or Y), because d exp(A) = exp(A) dA), back to the folded cepstra, and on to the log spectra.
//   vjp frames one workgroup per frame: the pulses whose floor or ceil frame it is are one run, added in pulse order with the lower / upper
//              weights, and zero where the input was clipped.
#include "common.h"
#include "lds_fft.h"

namespace dsa {
namespace {

// dsa_last_kernel() of the five entries: [entry][dtype]
enum { WS_PULSES = 0, WS_RESPONSES = 1, WS_OVERLAP_ADD = 2, WS_VJP_PULSES = 3, WS_VJP_FRAMES = 4 };
const char* const kWsRoutes[5][2] = {
    {"world_synth_pulses_f32", "world_synth_pulses_f64"},           {"world_synth_responses_f32", "world_synth_responses_f64"},
    {"world_synth_overlap_add_f32", "world_synth_overlap_add_f64"}, {"world_synth_vjp_pulses_f32", "world_synth_vjp_pulses_f64"},
    {"world_synth_vjp_frames_f32", "world_synth_vjp_frames_f64"},
};

constexpr int WS_THREADS = 256;        // the time-base workgroup, and the overlap-add's
constexpr int WS_CHUNK = 2048;         // samples of the time base in LDS at a time: eight per thread
constexpr int WS_MAX_THREADS = 1024;   // the per-pulse workgroup: L / 4, between 64 and this
constexpr int WS_RED_BYTES = 256;      // the reductions' exchange at the head of the per-pulse LDS
constexpr double kWsEps = 1e-6;        // world_synth.py:189

// ---------------------------------------------------------------------------------------------------------------- time base
template <typename T>
struct WsTimeBase {
    const T* f0;   // the utterance's N values
    long N;
    int P;
    T step, sr, fmin, deflt;   // (dtype)(P / sr), (dtype) sr, (dtype)(sr / L + 1), (dtype) default_f0
    double dphase;             // tau / sr

    __device__ __forceinline__ T x(long n) const { return rn_mul((T)n, step); }
    __device__ __forceinline__ T y(long n) const
    {
        const T v = f0[n];
        return v < fmin ? T(0) : v;
    }
    __device__ __forceinline__ T time(long i) const { return (T)i / sr; }
    // interp1 of one query: m t + b on the segment that searchsorted(right = False) picks
    __device__ __forceinline__ void at(long i, T& f, bool& voiced) const
    {
        const T t = time(i);
        long k = i / P;
        if (k > N) k = N;
        while (k < N && x(k) < t) ++k;
        while (k > 0 && !(x(k - 1) < t)) --k;
        T vf, vv;
        if (k == 0 || k == N) {   // the padded ends: slope 0, intercept the end value
            vf = y(k == 0 ? 0 : N - 1);
            vv = T(0) < vf ? T(1) : T(0);
        } else {
            const T x0 = x(k - 1), dx = rn_sub(x(k), x0);
            const T y0 = y(k - 1), y1 = y(k);
            const T v0 = T(0) < y0 ? T(1) : T(0), v1 = T(0) < y1 ? T(1) : T(0);
            const T mf = rn_sub(y1, y0) / dx, mv = rn_sub(v1, v0) / dx;
            vf = rn_add(rn_mul(mf, t), rn_sub(y0, rn_mul(mf, x0)));
            vv = rn_add(rn_mul(mv, t), rn_sub(v0, rn_mul(mv, x0)));
        }
        voiced = T(0.5) < vv;
        f = voiced ? vf : deflt;
    }
    __device__ __forceinline__ double term(long i, bool& voiced) const
    {
        T f;
        at(i, f, voiced);
        return rn_mul(dphase, (double)f);
    }
};

// irec: (pulses, 4) int64 = sample index, utterance, floor frame, ceil frame; frec: (pulses, 3) of the dtype = the fractional time shift in
// seconds, the upper weight frame - floor, the voiced flag.  Both NULL: only counts[b] is written.
// WS_CHUNK samples at a time: every thread forms its samples' terms (tau / sr) f_i into LDS, ONE lane adds them up in order -- the float64
// sum is then the sequential sum of torch.cumsum bit for bit, whatever the utterance's length, at eight adds per thread's worth of
// terms --, and every thread looks at its eight neighbouring pairs; the pulses found are counted, the counts scanned, the records written.
template <typename T>
__global__ __launch_bounds__(WS_THREADS) void ws_pulses_kernel(const T* __restrict__ f0, long N, int P, T step, T sr, T fmin, T deflt, T rate,
                                                               double dphase, const int64_t* __restrict__ offsets, int64_t* __restrict__ counts,
                                                               int64_t* __restrict__ irec, T* __restrict__ frec)
{
    __shared__ double ph[WS_CHUNK + 1];   // ph[0]: the phase of the sample before the chunk; ph[1 + j]: of the chunk's sample j
    __shared__ int ired[8];
    const int t = threadIdx.x;
    const long b = blockIdx.x, Tn = N * (long)P;
    const WsTimeBase<T> tb{f0 + b * N, N, P, step, sr, fmin, deflt, dphase};
    const T tau = (T)kTau, pi = (T)kPi;
    constexpr int PER = WS_CHUNK / WS_THREADS;
    long at = irec ? offsets[b] : 0;
    const long end = irec ? offsets[b + 1] : 0;
    long found = 0;
    double carry = 0.0;   // lane 0's: the phase of the last sample of the chunk before
    for (long c0 = 0; c0 < Tn; c0 += WS_CHUNK) {
        const int n = (int)(Tn - c0 < WS_CHUNK ? Tn - c0 : WS_CHUNK);
        bool voiced;
        if (t == 0) ph[0] = carry;
        for (int j = t; j < n; j += WS_THREADS) ph[1 + j] = tb.term(c0 + j, voiced);
        __syncthreads();
        if (t == 0) {
            double run = carry;
#pragma unroll 8
            for (int j = 0; j < n; ++j) {
                run += ph[1 + j];
                ph[1 + j] = run;
            }
            carry = run;
        }
        __syncthreads();
        // the pairs (s - 1, s) of this thread's samples s = c0 + j, s >= 1: a pulse at s - 1
        const int j0 = t * PER, j1 = min(n, j0 + PER);
        unsigned hits = 0;
        for (int j = j0; j < j1; ++j) {
            if (c0 + j == 0) continue;
            const T w0 = dsa_fmod((T)ph[j], tau), w1 = dsa_fmod((T)ph[1 + j], tau);
            if (pi < dsa_abs(rn_sub(w1, w0))) hits |= 1u << (j - j0);
        }
        int all;
        const int before = team_scan_excl((int)__popc(hits), ired, t, WS_THREADS, all);
        if (irec) {
            long row = at + before;
            for (int j = j0; j < j1; ++j) {
                if (!(hits >> (j - j0) & 1u) || row >= end) continue;
                const long i = c0 + j - 1;
                const T w0 = dsa_fmod((T)ph[j], tau), w1 = dsa_fmod((T)ph[1 + j], tau);
                T f;
                tb.at(i, f, voiced);
                const T y1 = rn_sub(w0, tau);
                const T shift = (-y1 / rn_sub(w1, y1)) / sr;
                const T frame = rn_mul(tb.time(i), rate);
                const long fl = min((long)dsa_floor(frame), N - 1), ce = min((long)dsa_ceil(frame), N - 1);
                irec[row * 4 + 0] = i;
                irec[row * 4 + 1] = b;
                irec[row * 4 + 2] = fl;
                irec[row * 4 + 3] = ce;
                frec[row * 3 + 0] = shift;
                frec[row * 3 + 1] = rn_sub(frame, (T)fl);
                frec[row * 3 + 2] = voiced ? T(1) : T(0);
                ++row;
            }
        }
        at += all;
        found += all;
        __syncthreads();   // every pair has been read before the next chunk's terms replace them
    }
    if (t == 0) counts[b] = found;
}

// ---------------------------------------------------------------------------------------------------------------- one pulse
template <typename T>
struct WsLds {
    double* red;
    T *re, *im, *a0, *a1, *a2, *a3;
    __device__ __forceinline__ WsLds(unsigned char* p, int L)
    {
        red = reinterpret_cast<double*>(p);
        re = reinterpret_cast<T*>(p + WS_RED_BYTES);
        im = re + L;
        a0 = im + L;
        a1 = a0 + (L / 2 + 1);
        a2 = a1 + (L / 2 + 1);
        a3 = a2 + (L / 2 + 1);
    }
};

// torch.sqrt of the int64 noise_size (world_synth.py:298) is a FLOAT32 tensor whatever the data's dtype: the float64 reference scales its
// periodic response by a square root rounded to 24 bits, and so does this
template <typename T>
__device__ __forceinline__ T ws_root(long noise_size) { return (T)sqrtf((float)noise_size); }

template <typename T>
struct WsPulse {
    long index, b, fl, ce, noise_size;
    T shift, upper, lower;
    bool voiced;
    const T *spf, *spc, *apf, *apc;   // the two rows of each input
};

template <typename T>
__device__ __forceinline__ WsPulse<T> ws_pulse(long p, const int64_t* __restrict__ irec, const T* __restrict__ frec, const int64_t* __restrict__ offsets,
                                               const T* __restrict__ ap, const T* __restrict__ sp, long B, long N, int D)
{
    WsPulse<T> q;
    q.index = irec[p * 4 + 0];
    q.b = min(max(irec[p * 4 + 1], (int64_t)0), (int64_t)(B - 1));
    q.fl = min(max(irec[p * 4 + 2], (int64_t)0), (int64_t)(N - 1));
    q.ce = min(max(irec[p * 4 + 3], (int64_t)0), (int64_t)(N - 1));
    q.noise_size = p + 1 < offsets[q.b + 1] ? max(irec[(p + 1) * 4] - q.index, (int64_t)0) : 0;   // 0 for an utterance's last pulse
    q.shift = frec[p * 3 + 0];
    q.upper = frec[p * 3 + 1];
    q.lower = T(1) - q.upper;
    q.voiced = T(0.5) < frec[p * 3 + 2];
    q.spf = sp + (q.b * N + q.fl) * D;
    q.spc = sp + (q.b * N + q.ce) * D;
    q.apf = ap + (q.b * N + q.fl) * D;
    q.apc = ap + (q.b * N + q.ce) * D;
    return q;
}

// the interpolated rows at bin k: the envelope, the aperiodicity before squaring, and the two spectra whose minimum phase is taken
template <typename T>
__device__ __forceinline__ void ws_rows(const WsPulse<T>& q, int k, T& se, T& qa, T& wv, T& S1, T& S2)
{
    const T eps = (T)kWsEps, top = (T)(1.0 - kWsEps);
    const T sf = max(q.spf[k], eps), sc = max(q.spc[k], eps);
    const T af = min(max(q.apf[k], eps), top), ac = min(max(q.apc[k], eps), top);
    se = q.lower * sf + q.upper * sc;
    qa = q.lower * af + q.upper * ac;
    const T ar = qa * qa;
    wv = q.voiced ? ar : T(1);
    S1 = (T(1) - ar) * se;
    S2 = wv * se;
}

// transforms 1 to 3: on return a0 + i a1 = X[k] = M1[k] e^(-i k coef) and a2 + i a3 = Y[k] = M2[k] N[k], k = 0 .. L/2; re / im are dead
template <typename T>
__device__ __forceinline__ void ws_spectra(const WsPulse<T>& q, const WsLds<T>& s, const T* __restrict__ noise_row, int L, int lg, T coef,
                                           const T* __restrict__ tw)
{
    const int H = L >> 1, t = threadIdx.x, nt = blockDim.x;
    for (int k = t; k <= H; k += nt) {
        T se, qa, wv, S1, S2;
        ws_rows(q, k, se, qa, wv, S1, S2);
        const T l1 = T(0.5) * dsa_log(S1), l2 = T(0.5) * dsa_log(S2);
        s.re[k] = l1;
        s.im[k] = l2;
        if (k > 0 && k < H) {
            s.re[L - k] = l1;
            s.im[L - k] = l2;
        }
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, L, lg, tw);
    const T inv = T(1) / (T)L;
    for (int n = t; n <= H; n += nt) {   // the cepstra, folded
        const int p = fft_brev(n, lg);
        const T f = n == 0 || n == H ? inv : T(2) * inv;
        s.a0[n] = f * s.re[p];
        s.a2[n] = f * s.im[p];
    }
    __syncthreads();
    for (int n = t; n < L; n += nt) {
        s.re[n] = n <= H ? s.a0[n] : T(0);
        s.im[n] = n <= H ? s.a2[n] : T(0);
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, L, lg, tw);
    for (int k = t; k <= H; k += nt) {   // A1 = (Z[k] + conj Z[L-k]) / 2, A2 = (Z[k] - conj Z[L-k]) / 2i; M = exp(A)
        const int pk = fft_brev(k, lg), pm = fft_brev((L - k) & (L - 1), lg);
        const T zkr = s.re[pk], zki = s.im[pk], zmr = s.re[pm], zmi = s.im[pm];
        const T a1r = T(0.5) * (zkr + zmr), a1i = T(0.5) * (zki - zmi);
        const T a2r = T(0.5) * (zki + zmi), a2i = T(-0.5) * (zkr - zmr);
        const T e1 = dsa_exp(a1r), e2 = dsa_exp(a2r);
        s.a0[k] = e1 * dsa_cos(a1i);
        s.a1[k] = e1 * dsa_sin(a1i);
        s.a2[k] = e2 * dsa_cos(a2i);
        s.a3[k] = e2 * dsa_sin(a2i);
    }
    // the noise: masked to noise_size values, centred on sum / noise_size, masked again
    const long ns = q.noise_size;
    double part = 0.0;
    for (int n = t; n < L; n += nt)
        if (n < ns) part += (double)noise_row[n];
    const double sum = block_sum(part, s.red);   // (its barriers also end the reads of re / im above)
    const T avg = ns > 0 ? (T)sum / (T)ns : T(0);
    for (int n = t; n < L; n += nt) {
        s.re[n] = n < ns ? noise_row[n] - avg : T(0);
        s.im[n] = T(0);
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, L, lg, tw);
    for (int k = t; k <= H; k += nt) {
        const int pk = fft_brev(k, lg);
        const T nr = s.re[pk], ni = s.im[pk];
        const T ang = (T)k * coef;
        const T c = dsa_cos(ang), sn = -dsa_sin(ang);
        const T m1r = s.a0[k], m1i = s.a1[k], m2r = s.a2[k], m2i = s.a3[k];
        s.a0[k] = m1r * c - m1i * sn;
        s.a1[k] = m1r * sn + m1i * c;
        s.a2[k] = m2r * nr - m2i * ni;
        s.a3[k] = m2r * ni + m2i * nr;
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(WS_MAX_THREADS) void ws_responses_kernel(const T* __restrict__ ap, const T* __restrict__ sp, const T* __restrict__ noise,
                                                                      const int64_t* __restrict__ irec, const T* __restrict__ frec,
                                                                      const int64_t* __restrict__ offsets, const T* __restrict__ remover,
                                                                      const T* __restrict__ tw, long B, long N, int L, int lg, T coef_scale,
                                                                      T* __restrict__ response)
{
    extern __shared__ __align__(16) unsigned char ws_lds[];
    const WsLds<T> s(ws_lds, L);
    const int H = L >> 1, t = threadIdx.x, nt = blockDim.x;
    const long p = blockIdx.x;
    const WsPulse<T> q = ws_pulse(p, irec, frec, offsets, ap, sp, B, N, H + 1);
    ws_spectra(q, s, noise + p * L, L, lg, coef_scale * q.shift, tw);
    // W = full(X) + i full(Y); the imaginary parts of X and Y at 0 and L/2 are not part of a Hermitian spectrum (irfft drops them)
    for (int k = t; k <= H; k += nt) {
        const T xr = s.a0[k], xi = s.a1[k], yr = s.a2[k], yi = s.a3[k];
        if (k == 0 || k == H) {
            s.re[k] = xr;
            s.im[k] = yr;
        } else {
            s.re[k] = xr - yi;
            s.im[k] = xi + yr;
            s.re[L - k] = xr + yi;
            s.im[L - k] = yr - xi;
        }
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, L, lg, tw);
    // sample n of the shifted responses is the transform at (L/2 - n) mod L
    double part = 0.0;
    for (int n = H + t; n < L; n += nt) part += (double)s.re[fft_brev((H - n) & (L - 1), lg)];
    const T dc = (T)block_sum(part, s.red);
    const T root = ws_root<T>(q.noise_size), fL = (T)L;
    T* out = response + p * L;
    for (int n = t; n < L; n += nt) {
        const int pos = fft_brev((H - n) & (L - 1), lg);
        const T dd = -dc * remover[n];
        const T periodic = q.voiced ? (n < H ? dd : s.re[pos] + dd) : T(0);
        out[n] = (periodic * root + s.im[pos]) / fL;
    }
}

// y[b, j] = the sum over the utterance's pulses with index <= j + L/2 < index + L, ascending
template <typename T>
__global__ __launch_bounds__(WS_THREADS) void ws_overlap_kernel(const T* __restrict__ response, const int64_t* __restrict__ irec,
                                                                const int64_t* __restrict__ offsets, long Tout, int L, T* __restrict__ y)
{
    const long b = blockIdx.y;
    const long first = offsets[b], last = offsets[b + 1];
    const long j = (long)blockIdx.x * WS_THREADS + threadIdx.x;
    if (j < Tout) {
        const long pos = j + (L >> 1);
        long lo = first, hi = last;   // the first pulse with index > pos - L
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (irec[mid * 4] > pos - L)
                hi = mid;
            else
                lo = mid + 1;
        }
        T acc = T(0);
        for (long p = lo; p < last; ++p) {
            const long at = pos - irec[p * 4];
            if (at < 0) break;
            if (at < L) acc += response[p * L + at];
        }
        y[b * Tout + j] = acc;
    }
}

// grows: (pulses, 2, L/2 + 1) -- the cotangents of the interpolated envelope row and of the interpolated aperiodicity row (before squaring)
template <typename T>
__global__ __launch_bounds__(WS_MAX_THREADS) void ws_vjp_pulses_kernel(const T* __restrict__ gy, const T* __restrict__ ap, const T* __restrict__ sp,
                                                                       const T* __restrict__ noise, const int64_t* __restrict__ irec,
                                                                       const T* __restrict__ frec, const int64_t* __restrict__ offsets,
                                                                       const T* __restrict__ remover, const T* __restrict__ tw, long B, long N,
                                                                       long Tout, int L, int lg, T coef_scale, T* __restrict__ grows)
{
    extern __shared__ __align__(16) unsigned char ws_lds[];
    const WsLds<T> s(ws_lds, L);
    const int H = L >> 1, t = threadIdx.x, nt = blockDim.x;
    const long p = blockIdx.x;
    const WsPulse<T> q = ws_pulse(p, irec, frec, offsets, ap, sp, B, N, H + 1);
    ws_spectra(q, s, noise + p * L, L, lg, coef_scale * q.shift, tw);
    // the response's cotangent straight from gy, zero outside the waveform
    const T* g = gy + q.b * Tout;
    const long base = q.index - H;
    const T fL = (T)L, root = q.voiced ? ws_root<T>(q.noise_size) : T(0);
    double part = 0.0;
    for (int n = t; n < L; n += nt) {
        const long j = base + n;
        const T gn = j >= 0 && j < Tout ? g[j] / fL : T(0);
        part += (double)(gn * root) * (double)remover[n];
    }
    const T gdc = -(T)block_sum(part, s.red);
    for (int n = t; n < L; n += nt) {   // G[(n + L/2) mod L] = the periodic cotangent + i the aperiodic one
        const long j = base + n;
        const T gn = j >= 0 && j < Tout ? g[j] / fL : T(0);
        const int m = (n + H) & (L - 1);
        s.re[m] = n >= H ? gn * root + gdc : T(0);
        s.im[m] = gn;
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, L, lg, tw);
    for (int k = t; k <= H; k += nt) {   // g_X = w R1, g_Y = w R2 (real at the ends); g_A = g conj(X or Y)
        const int pk = fft_brev(k, lg), pm = fft_brev((L - k) & (L - 1), lg);
        const T zkr = s.re[pk], zki = s.im[pk], zmr = s.re[pm], zmi = s.im[pm];
        const bool edge = k == 0 || k == H;
        const T w = edge ? T(0.5) : T(1);   // (the split's 1/2 times the weight)
        const T r1r = w * (zkr + zmr), r1i = edge ? T(0) : w * (zki - zmi);
        const T r2r = w * (zki + zmi), r2i = edge ? T(0) : -w * (zkr - zmr);
        const T xr = s.a0[k], xi = s.a1[k], yr = s.a2[k], yi = s.a3[k];
        s.a0[k] = r1r * xr + r1i * xi;
        s.a1[k] = r1i * xr - r1r * xi;
        s.a2[k] = r2r * yr + r2i * yi;
        s.a3[k] = r2i * yr - r2r * yi;
    }
    __syncthreads();
    // the adjoint of rfft: Re sum_{k <= L/2} g_A[k] e^(+i theta k n), both at once through the Hermitian parts
    for (int k = t; k <= H; k += nt) {
        const T u1r = s.a0[k], u1i = s.a1[k], u2r = s.a2[k], u2i = s.a3[k];
        if (k == 0 || k == H) {
            s.re[k] = u1r;
            s.im[k] = u2r;
        } else {
            s.re[k] = T(0.5) * (u1r - u2i);
            s.im[k] = T(0.5) * (u1i + u2r);
            s.re[L - k] = T(0.5) * (u1r + u2i);
            s.im[L - k] = T(0.5) * (u2r - u1i);
        }
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, L, lg, tw);
    for (int n = t; n <= H; n += nt) {   // the fold's adjoint; the inverse transform sits at (L - n) mod L
        const int pos = fft_brev((L - n) & (L - 1), lg);
        const T f = n == 0 || n == H ? T(1) : T(2);
        s.a0[n] = f * s.re[pos];
        s.a2[n] = f * s.im[pos];
    }
    __syncthreads();
    for (int n = t; n < L; n += nt) {
        s.re[n] = n <= H ? s.a0[n] : T(0);
        s.im[n] = n <= H ? s.a2[n] : T(0);
    }
    __syncthreads();
    lds_fft_pow2(s.re, s.im, L, lg, tw);
    T* out = grows + p * 2 * (long)(H + 1);
    for (int k = t; k <= H; k += nt) {   // the adjoint of irfft on a real spectrum: (w_k / L) Re of the transform
        const int pk = fft_brev(k, lg), pm = fft_brev((L - k) & (L - 1), lg);
        const T w = (k == 0 || k == H ? T(0.5) : T(1)) / fL;
        const T g1 = w * (s.re[pk] + s.re[pm]), g2 = w * (s.im[pk] + s.im[pm]);   // of (log S1) / 2 and (log S2) / 2
        T se, qa, wv, S1, S2;
        ws_rows(q, k, se, qa, wv, S1, S2);
        const T gS1 = q.voiced ? T(0.5) * g1 / S1 : T(0), gS2 = T(0.5) * g2 / S2;   // (an unvoiced pulse has no periodic part: exactly zero)
        const T ar = qa * qa;
        const T gar = (q.voiced ? gS2 * se : T(0)) - gS1 * se;
        out[k] = gS1 * (T(1) - ar) + gS2 * wv;
        out[H + 1 + k] = T(2) * qa * gar;
    }
}

// gsp, gap: (B, N, D).  The floor and ceil frames do not decrease along an utterance's pulses: the pulses that touch frame n are one run.
template <typename T>
__global__ __launch_bounds__(WS_THREADS) void ws_vjp_frames_kernel(const T* __restrict__ grows, const T* __restrict__ ap, const T* __restrict__ sp,
                                                                   const int64_t* __restrict__ irec, const T* __restrict__ frec,
                                                                   const int64_t* __restrict__ offsets, long N, int D, T* __restrict__ gap,
                                                                   T* __restrict__ gsp)
{
    const long b = blockIdx.y, n = blockIdx.x;
    const long first = offsets[b], last = offsets[b + 1];
    long lo = first, hi = last;   // the first pulse whose ceil frame is >= n
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (irec[mid * 4 + 3] >= n)
            hi = mid;
        else
            lo = mid + 1;
    }
    const T eps = (T)kWsEps, top = (T)(1.0 - kWsEps);
    const long row = (b * N + n) * D;
    for (int k = threadIdx.x; k < D; k += WS_THREADS) {
        T as = T(0), aa = T(0);
        for (long p = lo; p < last && irec[p * 4 + 2] <= n; ++p) {
            const T upper = frec[p * 3 + 1], lower = T(1) - upper;
            const T gs = grows[p * 2 * (long)D + k], ga = grows[p * 2 * (long)D + D + k];
            if (irec[p * 4 + 2] == n) {
                as += lower * gs;
                aa += lower * ga;
            }
            if (irec[p * 4 + 3] == n) {
                as += upper * gs;
                aa += upper * ga;
            }
        }
        const T a = ap[row + k];
        gsp[row + k] = sp[row + k] >= eps ? as : T(0);
        gap[row + k] = a >= eps && a <= top ? aa : T(0);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct WsPlan {
    int lg, threads;
    size_t lds;
};

int ws_check(WsPlan& plan, int64_t B, int64_t N, int64_t pulses, int64_t L, int32_t dtype)
{
    if (!(B >= 0 && N >= 0 && pulses >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: unknown dtype");
    if (!(L >= 8 && L <= (1 << 24) && (L & (L - 1)) == 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: fft_length must be a power of two, at least 8");
    const int64_t size = dtype == DSA_F32 ? 4 : 8;
    if (DSA_WORLD_LDS_BYTES(L, size) > DSA_WORLD_MAX_LDS_BYTES)
        return fail(DSA_ERR_INVALID_ARGUMENT,
                    "world_synth: (4 L + 4) sizeof(dtype) + 256 bytes exceed DSA_WORLD_MAX_LDS_BYTES (163840 bytes per workgroup)");
    // every tensor's byte offset is an int64, every launch dimension an int32
    if (B > 65535 || N > INT32_MAX || pulses > INT32_MAX || (N > 0 && B > INT64_MAX / 16 / N / (L / 2 + 1)) || pulses > INT64_MAX / 16 / L)
        return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: invalid sizes");
    plan.lg = 0;
    while ((1 << plan.lg) < L) ++plan.lg;
    plan.threads = L / 4 < 64 ? 64 : L / 4 > WS_MAX_THREADS ? WS_MAX_THREADS : (int)(L / 4);
    plan.lds = (size_t)DSA_WORLD_LDS_BYTES(L, size);
    return DSA_OK;
}

template <typename T>
int ws_pulses(const void* f0, int64_t B, int64_t N, int32_t P, int32_t sr, int32_t L, double default_f0, const void* offsets, void* counts,
              void* irec, void* frec, hipStream_t st)
{
    hipLaunchKernelGGL((ws_pulses_kernel<T>), dim3((unsigned)B), dim3(WS_THREADS), 0, st, (const T*)f0, (long)N, (int)P, (T)((double)P / (double)sr),
                       (T)sr, (T)((double)sr / (double)L + 1.0), (T)default_f0, (T)((double)sr / (double)P), kTau / (double)sr,
                       (const int64_t*)offsets, (int64_t*)counts, (int64_t*)irec, (T*)frec);
    return DSA_OK;
}

template <typename T>
int ws_responses(const void* ap, const void* sp, const void* noise, const void* irec, const void* frec, const void* offsets, const void* remover,
                 const void* tw, int64_t B, int64_t N, int32_t sr, int32_t L, int64_t pulses, const WsPlan& plan, void* response, hipStream_t st)
{
    return launch_lds<ws_responses_kernel<T>>(DSA_WORLD_MAX_LDS_BYTES, "world_synth: cannot raise the dynamic LDS limit", dim3((unsigned)pulses),
                                              dim3(plan.threads), plan.lds, st, (const T*)ap, (const T*)sp, (const T*)noise, (const int64_t*)irec,
                                              (const T*)frec, (const int64_t*)offsets, (const T*)remover, (const T*)tw, (long)B, (long)N, (int)L,
                                              plan.lg, (T)(kTau * (double)sr / (double)L), (T*)response);
}

template <typename T>
int ws_vjp_pulses(const void* gy, const void* ap, const void* sp, const void* noise, const void* irec, const void* frec, const void* offsets,
                  const void* remover, const void* tw, int64_t B, int64_t N, int64_t Tout, int32_t sr, int32_t L, int64_t pulses, const WsPlan& plan,
                  void* grows, hipStream_t st)
{
    return launch_lds<ws_vjp_pulses_kernel<T>>(DSA_WORLD_MAX_LDS_BYTES, "world_synth: cannot raise the dynamic LDS limit", dim3((unsigned)pulses),
                                               dim3(plan.threads), plan.lds, st, (const T*)gy, (const T*)ap, (const T*)sp, (const T*)noise,
                                               (const int64_t*)irec, (const T*)frec, (const int64_t*)offsets, (const T*)remover, (const T*)tw, (long)B,
                                               (long)N, (long)Tout, (int)L, plan.lg, (T)(kTau * (double)sr / (double)L), (T*)grows);
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_world_synth_pulses(const void* f0, int64_t B, int64_t N, int32_t P, int32_t sample_rate, int32_t L, double default_f0,
                                      const void* offsets, int32_t dtype, void* counts, void* irec, void* frec, void* stream)
{
    WsPlan plan;
    if (int rc = ws_check(plan, B, N, 0, L, dtype)) return rc;
    if (!(P >= 1 && sample_rate >= 1) || (N > 0 && P > (1 << 24) / N && dtype == DSA_F32) || (N > 0 && P > INT32_MAX / N))
        return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: invalid sizes (a float32 time axis holds N P <= 2^24 samples exactly)");
    if (B == 0 || N == 0) return DSA_OK;
    if (!(f0 && counts) || ((irec || frec) && !(irec && frec && offsets))) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = with_dtype(dtype, "world_synth", [&](auto tag) {
        return ws_pulses<decltype(tag)>(f0, B, N, P, sample_rate, L, default_f0, offsets, counts, irec, frec, st);
    });
    return rc ? rc : check_launch(kWsRoutes[WS_PULSES][dtype == DSA_F64]);
}

DSA_EXPORT int dsa_world_synth_responses(const void* ap, const void* sp, const void* noise, const void* irec, const void* frec, const void* offsets,
                                         const void* dc_remover, const void* twiddle, int64_t B, int64_t N, int32_t sample_rate, int32_t L,
                                         int64_t pulses, int32_t dtype, void* response, void* stream)
{
    WsPlan plan;
    if (int rc = ws_check(plan, B, N, pulses, L, dtype)) return rc;
    if (sample_rate < 1) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: invalid sizes");
    if (B == 0 || N == 0 || pulses == 0) return DSA_OK;
    if (!(ap && sp && noise && irec && frec && offsets && dc_remover && twiddle && response))
        return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = with_dtype(dtype, "world_synth", [&](auto tag) {
        return ws_responses<decltype(tag)>(ap, sp, noise, irec, frec, offsets, dc_remover, twiddle, B, N, sample_rate, L, pulses, plan, response, st);
    });
    return rc ? rc : check_launch(kWsRoutes[WS_RESPONSES][dtype == DSA_F64]);
}

DSA_EXPORT int dsa_world_synth_overlap_add(const void* response, const void* irec, const void* offsets, int64_t B, int64_t T, int32_t L, int64_t pulses,
                                           int32_t dtype, void* y, void* stream)
{
    WsPlan plan;
    if (int rc = ws_check(plan, B, 0, pulses, L, dtype)) return rc;
    if (!(T >= 0 && T <= INT32_MAX)) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: invalid sizes");   // T / 256 workgroups per utterance
    if (B == 0 || T == 0) return DSA_OK;
    if (!(offsets && y) || (pulses > 0 && !(response && irec))) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((T + WS_THREADS - 1) / WS_THREADS), (unsigned)B);
    return with_dtype(dtype, "world_synth", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's length)
        hipLaunchKernelGGL((ws_overlap_kernel<V>), grid, dim3(WS_THREADS), 0, st, (const V*)response, (const int64_t*)irec, (const int64_t*)offsets,
                           (long)T, (int)L, (V*)y);
        return check_launch(kWsRoutes[WS_OVERLAP_ADD][dtype == DSA_F64]);
    });
}

DSA_EXPORT int dsa_world_synth_vjp_pulses(const void* gy, const void* ap, const void* sp, const void* noise, const void* irec, const void* frec,
                                          const void* offsets, const void* dc_remover, const void* twiddle, int64_t B, int64_t N, int64_t T,
                                          int32_t sample_rate, int32_t L, int64_t pulses, int32_t dtype, void* grows, void* stream)
{
    WsPlan plan;
    if (int rc = ws_check(plan, B, N, pulses, L, dtype)) return rc;
    if (!(sample_rate >= 1 && T >= 0 && T <= INT64_MAX / 16 / (B > 0 ? B : 1))) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: invalid sizes");
    if (B == 0 || N == 0 || pulses == 0) return DSA_OK;
    if (!(ap && sp && noise && irec && frec && offsets && dc_remover && twiddle && grows) || (T > 0 && !gy))
        return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = with_dtype(dtype, "world_synth", [&](auto tag) {
        return ws_vjp_pulses<decltype(tag)>(gy, ap, sp, noise, irec, frec, offsets, dc_remover, twiddle, B, N, T, sample_rate, L, pulses, plan, grows, st);
    });
    return rc ? rc : check_launch(kWsRoutes[WS_VJP_PULSES][dtype == DSA_F64]);
}

DSA_EXPORT int dsa_world_synth_vjp_frames(const void* grows, const void* ap, const void* sp, const void* irec, const void* frec, const void* offsets,
                                          int64_t B, int64_t N, int32_t L, int64_t pulses, int32_t dtype, void* gap, void* gsp, void* stream)
{
    WsPlan plan;
    if (int rc = ws_check(plan, B, N, pulses, L, dtype)) return rc;
    if (B == 0 || N == 0) return DSA_OK;
    if (!(ap && sp && offsets && gap && gsp) || (pulses > 0 && !(grows && irec && frec))) return fail(DSA_ERR_INVALID_ARGUMENT, "world_synth: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)N, (unsigned)B);
    const int D = L / 2 + 1;
    return with_dtype(dtype, "world_synth", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((ws_vjp_frames_kernel<T>), grid, dim3(WS_THREADS), 0, st, (const T*)grows, (const T*)ap, (const T*)sp, (const int64_t*)irec,
                           (const T*)frec, (const int64_t*)offsets, (long)N, D, (T*)gap, (T*)gsp);
        return check_launch(kWsRoutes[WS_VJP_FRAMES][dtype == DSA_F64]);
    });
}
