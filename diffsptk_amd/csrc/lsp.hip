// Line spectral pairs (include/diffsptk_amd.h, section a15):
//   lpc2lsp   LinearPredictiveCoefficientsToLineSpectralPairs._forward, lpc2lsp.py:169-197   (two companion-matrix eigenproblems there)
//   lsp2lpc   LineSpectralPairsToLinearPredictiveCoefficients._forward, lsp2lpc.py:171-195   (a complex product of roots there)
//   lspcheck  LineSpectralPairsStabilityCheck._forward, lspcheck.py:115-145                   (a Python double loop there)
// each forward and adjoint in one launch, float64 arithmetic whatever the data's dtype, one rounding at the store.
//
// Rows are [K, c_1 .. c_M], N = M + 1, a_0 = 1.  With P(z) = A(z) - z^-N A(1/z) and Q(z) = A(z) + z^-N A(1/z), on the unit circle
//   Q = 2 e^{-jNw/2} Gq(w),  Gq(w) = sum_k a_k cos((N/2 - k) w)        P = 2j e^{-jNw/2} Gp(w),  Gp(w) = sum_k a_k sin((N/2 - k) w)
// and the LSPs are the zeros of Gq and Gp in (0, pi): w_1 < w_3 < .. belong to Gq, w_2 < w_4 < .. to Gp.  The trivial factors are
//   M even:  Q = Q' (1 + z^-1),  P = P' (1 - z^-1)         M odd:  Q = Q',  P = P' (1 - z^-2)
// and Q', P' are symmetric of even degree 2 Dq, 2 Dp (Dq = ceil(M / 2), Dp = floor(M / 2)): on the unit circle each is a Chebyshev
// series sum_n c_n T_n(x) in x = cos w, c_0 = g'_D, c_n = 2 g'_{D-n}, which is evaluated as sum_n c_n cos(n w) with cos(n w) and
// sin(n w) from the rotation recurrence -- the value and the derivative with respect to w in one pass, and no acos at the end.
//
// lpc2lsp forward (Kabal & Ramachandran 1986): ONE WAVE PER FRAME, the lanes are grid points.  Lane l owns [l, l + 1] pi / 64, cut in
// 2^r cells at level r; a sign change between two cell ends is a bracket.  Level 0 is tried first and the step is halved, at most
// LS_LEVELS - 1 times (down to pi / 4096 = 7.7e-4 rad), until Dq + Dp = M brackets are found: a wave-uniform decision.  The brackets
// are listed in LDS in ascending order (a wave scan of the lanes' counts) and lane j refines root j + 1 with a FIXED number of
// steps: LS_BISECT bisections, then LS_NEWTON Newton steps that are kept inside the bracket.  A row whose M roots are not found, or
// whose roots do not interlace (a predictor that is not minimum phase, NaN input), gets NaN in w_1 .. w_M.
// lpc2lsp backward: one wave per frame too, lane i owns root w_i.  dw_i / da_k = -(dG / da_k) / (dG / dw) at w_i (G = Gq or Gp by the
// parity of i): no root finder.  The sum over i is a wave reduction per k; the sines and cosines come from the rotation recurrence.
//
// lsp2lpc and lspcheck: ONE FRAME PER LANE as parcor.hip; 64 rows are one contiguous stretch of memory that goes through LDS with
// coalesced loads and stores.  Per-lane arrays live in LDS as [index][lane]: the loops are uniform in the order M, so the 64 lanes
// touch 64 consecutive doubles and there is no bank conflict and no register array with a variable index.
//   lsp2lpc fwd   the products of the real sections 1 - 2 cos w_i z^-1 + z^-2 over the odd- and the even-indexed LSPs; a product of
//                 d sections is symmetric of degree 2 d, so only d + 1 coefficients are kept.  Never a complex number.  The
//                 sections are multiplied in bit-reversed order of frequency (ls_sections): no cancellation between partial products.
//   lsp2lpc bwd   d p' / d b_i = z^-1 p' / section_i: the quotient by synthetic division (its first half, streamed through the
//                 dot product with the folded cotangent), O(M^2) per frame, no workspace.
//   lspcheck      the Gauss-Seidel sweeps on the row in LDS; the backward replays the forward from the input to regenerate the masks
//                 of sweep t (two 64-bit words in registers) for t descending: O(n^2 M) for a row that ran n sweeps, no workspace.
#include "common.h"

namespace dsa {
namespace {

constexpr int LS_LEVELS = 7;    // grid steps pi / 64 .. pi / 4096
constexpr int LS_BISECT = 16;   // a level-0 bracket of 4.9e-2 rad shrinks to 7.5e-7 before the first Newton step
constexpr int LS_NEWTON = 6;
constexpr int LS_HALF = DSA_LSP_MAX_ORDER / 2 + 2;
constexpr int LS_MAX_LDS = 112 * 1024;

enum { LS_LSP2LPC_FWD = 0, LS_LSP2LPC_BWD, LS_CHECK_FWD, LS_CHECK_BWD };
const char* const kLsLaneNames[] = {"lsp_lsp2lpc_fwd", "lsp_lsp2lpc_bwd", "lsp_lspcheck_fwd", "lsp_lspcheck_bwd"};

// ---------------------------------------------------------------------------------------------- lpc2lsp: one wave per frame
// both deflated series at w; cp is padded with zeros up to D
__device__ __forceinline__ void ls_eval2(const double* cq, const double* cp, int D, double w, double& fq, double& fp)
{
    double s, c;
    sincos(w, &s, &c);
    double C = 1.0, S = 0.0;
    fq = cq[0];
    fp = cp[0];
    for (int n = 1; n <= D; ++n) {
        const double C2 = fma(C, c, -S * s), S2 = fma(S, c, C * s);
        C = C2;
        S = S2;
        fq = fma(cq[n], C, fq);
        fp = fma(cp[n], C, fp);
    }
}
// one series and its derivative with respect to w
__device__ __forceinline__ void ls_eval_d(const double* cf, int D, double w, double& f, double& df)
{
    double s, c;
    sincos(w, &s, &c);
    double C = 1.0, S = 0.0;
    f = cf[0];
    df = 0.0;
    for (int n = 1; n <= D; ++n) {
        const double C2 = fma(C, c, -S * s), S2 = fma(S, c, C * s);
        C = C2;
        S = S2;
        f = fma(cf[n], C, f);
        df = fma(-(double)n * cf[n], S, df);
    }
}
// the lane's stretch in S cells of width h: the sign changes of both series; with `put`, the cells go to the lists from oq / op on
__device__ __forceinline__ void ls_walk(const double* cq, const double* cp, int D, int S, double h, int& nq, int& np, bool put, int* lq,
                                        int* lp, int oq, int op)
{
    const int i0 = (int)threadIdx.x * S;
    double fq, fp;
    ls_eval2(cq, cp, D, (double)i0 * h, fq, fp);
    bool sq = fq >= 0.0, sp = fp >= 0.0;
    nq = np = 0;
    for (int s = 1; s <= S; ++s) {
        ls_eval2(cq, cp, D, (double)(i0 + s) * h, fq, fp);   // the same expression in the lane that starts here: the same bits
        const bool tq = fq >= 0.0, tp = fp >= 0.0;
        if (tq != sq) {
            if (put && oq + nq < LS_HALF) lq[oq + nq] = i0 + s - 1;
            ++nq;
        }
        if (tp != sp) {
            if (put && op + np < LS_HALF) lp[op + np] = i0 + s - 1;
            ++np;
        }
        sq = tq;
        sp = tp;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void lsp_lpc2lsp_fwd_kernel(const T* __restrict__ a, long F, int M, int log_gain, double unit,
                                                             T* __restrict__ out, int* __restrict__ failed)
{
    __shared__ double row[DSA_LSP_MAX_ORDER + 2];   // 1, a_1 .. a_M, 0
    __shared__ double cq[LS_HALF], cp[LS_HALF];
    __shared__ int lq[LS_HALF], lp[LS_HALF];
    const int lane = threadIdx.x, N = M + 1;
    const int Dq = (M + 1) / 2, Dp = M / 2;
    for (long f = blockIdx.x; f < F; f += gridDim.x) {
        const long base = f * N;
        __syncthreads();
        for (int j = lane; j <= M; j += 64) row[j] = j ? (double)a[base + j] : 1.0;
        if (lane == 0) row[N] = 0.0;
        __syncthreads();
        if (lane == 0) {   // q_k = a_k + a_{N-k}, p_k = a_k - a_{N-k}, the trivial factors divided out, as Chebyshev coefficients
            double q1 = 0.0, p1 = 0.0, p2 = 0.0;
            for (int k = 0; k <= Dq; ++k) {
                const double o = row[N - k];
                double q = row[k] + o, p = row[k] - o;
                if (M & 1) {
                    p += p2;
                } else {
                    q -= q1;
                    p += p1;
                }
                p2 = p1;
                p1 = p;
                q1 = q;
                cq[Dq - k] = k == Dq ? q : 2.0 * q;
                if (k <= Dp) cp[Dp - k] = k == Dp ? p : 2.0 * p;
            }
            for (int n = Dp + 1; n <= Dq; ++n) cp[n] = 0.0;
        }
        __syncthreads();

        bool found = M == 0;
        int nq = 0, np = 0, level = 0;
        for (int r = 0; !found && r < LS_LEVELS; ++r) {
            ls_walk(cq, cp, Dq, 1 << r, kPi / (double)(64 << r), nq, np, false, lq, lp, 0, 0);
            found = wave_sum(nq) == Dq && wave_sum(np) == Dp;
            level = r;
        }
        double x = __builtin_nan("");
        if (found && M > 0) {
            const double h = kPi / (double)(64 << level);
            ls_walk(cq, cp, Dq, 1 << level, h, nq, np, true, lq, lp, wave_scan_incl(nq, lane) - nq, wave_scan_incl(np, lane) - np);
            __syncthreads();
            if (lane < M) {
                const bool isq = !(lane & 1);
                const double* cf = isq ? cq : cp;
                const int cell = isq ? lq[lane >> 1] : lp[lane >> 1];
                double lo = (double)cell * h, hi = (double)(cell + 1) * h, fv, dv;
                ls_eval_d(cf, Dq, lo, fv, dv);
                const bool slo = fv >= 0.0;
                for (int it = 0; it < LS_BISECT; ++it) {
                    const double m = 0.5 * (lo + hi);
                    ls_eval_d(cf, Dq, m, fv, dv);
                    if ((fv >= 0.0) == slo) lo = m;
                    else hi = m;
                }
                x = 0.5 * (lo + hi);
                for (int it = 0; it < LS_NEWTON; ++it) {
                    ls_eval_d(cf, Dq, x, fv, dv);
                    if ((fv >= 0.0) == slo) lo = x;
                    else hi = x;
                    const double xn = x - fv / dv;
                    x = (xn >= lo && xn <= hi) ? xn : 0.5 * (lo + hi);
                }
            }
            const double prev = __shfl_up(x, 1, 64);
            const bool bad = lane < M && !(x > (lane ? prev : 0.0) && x < kPi);   // the roots of Q' and P' interlace, or A is not minimum phase
            if (__ballot(bad)) found = false;
        }
        if (lane < M) out[base + 1 + lane] = found ? (T)(x / unit) : (T)__builtin_nan("");
        if (lane == 0) {
            const T K = a[base];
            out[base] = log_gain ? (T)log((double)K) : K;
            if (!found && failed) *failed = 1;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64) void lsp_lpc2lsp_bwd_kernel(const T* __restrict__ gw, const T* __restrict__ a, const T* __restrict__ w, long F,
                                                             int M, int log_gain, double unit, T* __restrict__ ga)
{
    __shared__ double row[DSA_LSP_MAX_ORDER + 1];   // 1, a_1 .. a_M
    const int lane = threadIdx.x, N = M + 1;
    const double half_n = 0.5 * (double)N;
    for (long f = blockIdx.x; f < F; f += gridDim.x) {
        const long base = f * N;
        __syncthreads();
        for (int j = lane; j <= M; j += 64) row[j] = j ? (double)a[base + j] : 1.0;
        __syncthreads();
        const bool live = lane < M, isq = !(lane & 1);
        const double th = live ? (double)w[base + 1 + lane] * unit : 0.0;
        const double g = live ? (double)gw[base + 1 + lane] : 0.0;
        double s, c, S0, C0;
        sincos(th, &s, &c);
        sincos(half_n * th, &S0, &C0);
        double C = C0, S = S0, d = 0.0;   // dG / dw at w_i: Gq' = -sum a_j (N/2 - j) sin((N/2 - j) w), Gp' = sum a_j (N/2 - j) cos((N/2 - j) w)
        for (int j = 0; j <= M; ++j) {
            d = fma(row[j] * (half_n - (double)j), isq ? -S : C, d);
            const double C2 = fma(C, c, S * s), S2 = fma(S, c, -C * s);   // the angle goes down by w
            C = C2;
            S = S2;
        }
        const double sc = live ? -g / (unit * d) : 0.0;
        C = C0;
        S = S0;
        double mine = 0.0;
        for (int k = 1; k <= M; ++k) {   // ga_k = sum_i sc_i cos or sin((N/2 - k) w_i)
            const double C2 = fma(C, c, S * s), S2 = fma(S, c, -C * s);
            C = C2;
            S = S2;
            const double t = wave_sum(sc * (isq ? C : S));
            if (lane == k - 1) mine = t;
        }
        if (live) ga[base + 1 + lane] = (T)mine;
        if (lane == 0) ga[base] = log_gain ? (T)((double)gw[base] / (double)a[base]) : gw[base];
    }
}

// ---------------------------------------------------------------------------------------------- one frame per lane
// (tiles of rows travel between global memory and LDS rows of stride S by wave_tile_in / wave_tile_out, common.h)
// per-lane arrays in LDS: element k of the lane's array is v[64 k]
#define LS_AT(v, k) (v)[(k) << 6]

// the product of the sections 1 + b_i z^-1 + z^-2, b_i = -2 cos(unit w_i), over i = first, first + 2, .. <= M: the first half
// c_0 .. c_d of its 2 d + 1 symmetric coefficients.  th, when given, receives unit w_i at element i - 1.
// The sections are NOT taken in ascending frequency: the partial product of the d lowest sections has its roots in one arc and
// coefficients like those of (1 - z^-1)^(2 d), 4^d at the centre, which the remaining sections cancel again -- at M = 64 that loses
// 14 of float64's 16 digits (the reference's complex product loses them the same way).  In bit-reversed order (0, n/2, n/4, 3n/4, ..)
// every partial product has its roots spread round the circle and its coefficients stay below 1e3 for the LPC of windowed frames.
template <typename T>
__device__ __forceinline__ void ls_sections(double* c, const T* wrow, int first, int M, double unit, double* th)
{
    LS_AT(c, 0) = 1.0;
    const int D = M >= first ? (M - first) / 2 + 1 : 0;   // sections
    int bits = 0;
    while ((1 << bits) < D) ++bits;
    int d = 0;
    for (int t = 0; D > 0 && t < (1 << bits); ++t) {
        const int j = bits ? fft_brev(t, bits) : 0;
        if (j >= D) continue;
        const int i = first + 2 * j;
        const double a = (double)wrow[i] * unit;
        if (th) LS_AT(th, i - 1) = a;
        const double b = -2.0 * cos(a);
        LS_AT(c, d + 1) = fma(b, LS_AT(c, d), d >= 1 ? 2.0 * LS_AT(c, d - 1) : 0.0);   // the new centre: c_{d+1} was c_{d-1}
        for (int k = d; k >= 1; --k) LS_AT(c, k) = fma(b, LS_AT(c, k - 1), LS_AT(c, k)) + (k >= 2 ? LS_AT(c, k - 2) : 0.0);
        ++d;
    }
}
// coefficient k of the symmetric polynomial of degree 2 D whose first half is c
__device__ __forceinline__ double ls_full(const double* c, int D, int k)
{
    if (k < 0 || k > 2 * D) return 0.0;
    return LS_AT(c, k <= D ? k : 2 * D - k);
}

// one Gauss-Seidel sweep and the clip of lspcheck.py:133-139 on w_1 .. w_M (w[0 .. M-1] here); returns the row's exit test
// (lspcheck.py:140-141).  pm / cm: the masks of torch.clip's gradient (1 on the bound) -- the pairs that moved, the values not clipped.
__device__ __forceinline__ bool ls_sweep(double* w, int M, double d, double lo, double hi, double thr, unsigned long long& pm,
                                         unsigned long long& cm)
{
    pm = cm = 0ull;
    if (M < 1) return true;
    double cur = LS_AT(w, 0);
    for (int m = 0; m + 1 < M; ++m) {
        const double nxt = LS_AT(w, m + 1);
        const double x = d - (nxt - cur);
        const double st = 0.5 * (x < 0.0 ? 0.0 : x);   // NaN passes, as torch.clip
        if (x >= 0.0) pm |= 1ull << m;
        LS_AT(w, m) = cur - st;
        cur = nxt + st;
    }
    LS_AT(w, M - 1) = cur;
    bool conv = true;
    double prev = 0.0;
    for (int j = 0; j < M; ++j) {
        double v = LS_AT(w, j);
        if (v >= lo && v <= hi) cm |= 1ull << j;
        v = v < lo ? lo : (v > hi ? hi : v);
        LS_AT(w, j) = v;
        if (j) conv = conv && (v - prev >= thr);
        prev = v;
    }
    return conv;
}

// in0 / in1 / p / q per OP:
//   LSP2LPC_FWD w  -  unit   log_gain          LSP2LPC_BWD ga   w  unit    log_gain
//   CHECK_FWD   w  -  min_distance  n_iter     CHECK_BWD   gout w  min_distance  n_iter
template <typename T, int OP>
__global__ __launch_bounds__(64) void lsp_lane_kernel(const T* __restrict__ in0, const T* __restrict__ in1, long F, int M, double p, int q,
                                                      int W, T* __restrict__ out0, int* __restrict__ unstable)
{
    extern __shared__ double ls_smem[];
    const int M1 = M + 1, S = M1 | 1, lane = threadIdx.x;
    double* work = ls_smem + lane;          // W arrays' worth of doubles per lane, [index][lane]
    T* rows = (T*)(ls_smem + 64 * W);       // 64 rows of stride S
    T* mine = rows + lane * S;
    const long f0 = (long)blockIdx.x * 64;
    const int n = (int)(F - f0 < 64 ? F - f0 : 64);
    const int cnt = n * M1;
    const long base = f0 * M1;
    const bool live = lane < n;
    const int Dq = (M + 1) / 2, Dp = M / 2, HP = Dq + 1;

    if (OP == LS_LSP2LPC_FWD) {
        double *cq = work, *cp = work + 64 * HP;
        wave_tile_in(rows, in0, base, cnt, M1, S);
        __syncthreads();
        if (live) {   // (a lane beyond the last row has no row in LDS)
            const T k0 = mine[0];
            ls_sections(cq, mine, 1, M, p, (double*)nullptr);
            ls_sections(cp, mine, 2, M, p, (double*)nullptr);
            mine[0] = q ? (T)exp((double)k0) : k0;
            for (int k = 1; k <= M; ++k) {   // a = (P + Q) / 2 with the trivial factors of lsp2lpc.py:148-153
                const double v = (M & 1) ? ls_full(cp, Dp, k) - ls_full(cp, Dp, k - 2) + ls_full(cq, Dq, k)
                                         : (ls_full(cp, Dp, k) - ls_full(cp, Dp, k - 1)) + (ls_full(cq, Dq, k) + ls_full(cq, Dq, k - 1));
                mine[k] = (T)(0.5 * v);
            }
        }
    } else if (OP == LS_LSP2LPC_BWD) {
        double *cq = work, *cp = work + 64 * HP, *th = work + 128 * HP;
        wave_tile_in(rows, in1, base, cnt, M1, S);
        __syncthreads();
        const T k0 = live ? mine[0] : T(0);
        if (live) {
            ls_sections(cq, mine, 1, M, p, th);
            ls_sections(cp, mine, 2, M, p, th);
        }
        __syncthreads();
        wave_tile_in(rows, in0, base, cnt, M1, S);
        __syncthreads();
        for (int i = 1; live && i <= M; ++i) {
            const bool isq = i & 1;
            const double* c = isq ? cq : cp;
            const int D = isq ? Dq : Dp;
            double sn, cs;
            sincos(LS_AT(th, i - 1), &sn, &cs);
            const double b = -2.0 * cs;
            double r1 = 0.0, r2 = 0.0, acc = 0.0;   // r = p' / section_i by synthetic division; gb_i = sum_m h_m r_m
            for (int m = 0; m < D; ++m) {
                const double r = LS_AT(c, m) - fma(b, r1, r2);
                r2 = r1;
                r1 = r;
                double h = 0.0;   // the cotangent of coefficients m + 1 and 2 D - 1 - m of the full polynomial (one and the same at the centre)
                for (int e = 0; e < (m == D - 1 ? 1 : 2); ++e) {
                    const int j = e ? 2 * D - 1 - m : m + 1;
                    const int j2 = (M & 1) ? j + 2 : j + 1;
                    const double g1 = (j >= 1 && j <= M) ? (double)mine[j] : 0.0, g2 = (j2 >= 1 && j2 <= M) ? (double)mine[j2] : 0.0;
                    h += isq ? ((M & 1) ? g1 : g1 + g2) : g1 - g2;
                }
                acc = fma(0.5 * h, r, acc);
            }
            LS_AT(th, i - 1) = acc * 2.0 * sn * p;   // b_i = -2 cos(unit w_i)
        }
        if (live && q) mine[0] = (T)((double)mine[0] * exp((double)k0));
        for (int i = 1; live && i <= M; ++i) mine[i] = (T)LS_AT(th, i - 1);
    } else if (OP == LS_CHECK_FWD) {
        double* w = work;
        const double d = (double)(T)p, lo = d, hi = (double)(T)(kPi - p), thr = (double)(T)(p - 1e-16), pi_t = (double)(T)kPi;
        wave_tile_in(rows, in0, base, cnt, M1, S);
        __syncthreads();
        bool bad = false;
        double prev = 0.0;
        for (int j = 0; live && j <= M; ++j) {
            const double v = (double)mine[j];
            bad = bad || v <= 0.0 || pi_t <= v || (j >= 2 && v <= prev);   // lspcheck.py:121: the whole row, K included
            prev = v;
            if (j) LS_AT(w, j - 1) = v;
        }
        if (unstable && bad) *unstable = 1;
        bool done = !live;
        unsigned long long pm, cm;
        for (int it = 0; it < q; ++it) {
            if (!done) done = ls_sweep(w, M, d, lo, hi, thr, pm, cm);
            if (!__ballot(!done)) break;
        }
        for (int j = 1; live && j <= M; ++j) mine[j] = (T)LS_AT(w, j - 1);
    } else {
        double *w = work, *g = work + 64 * M;
        const double d = (double)(T)p, lo = d, hi = (double)(T)(kPi - p), thr = (double)(T)(p - 1e-16);
        wave_tile_in(rows, in0, base, cnt, M1, S);
        __syncthreads();
        const T gk = live ? mine[0] : T(0);
        for (int j = 1; live && j <= M; ++j) LS_AT(g, j - 1) = (double)mine[j];
        __syncthreads();
        wave_tile_in(rows, in1, base, cnt, M1, S);
        __syncthreads();
        unsigned long long pm, cm;
        int ran = 0;   // the sweeps this row ran
        if (live) {
            for (int j = 1; j <= M; ++j) LS_AT(w, j - 1) = (double)mine[j];
            bool done = false;
            for (int it = 0; it < q && !done; ++it) {
                done = ls_sweep(w, M, d, lo, hi, thr, pm, cm);
                ++ran;
            }
        }
        for (int t = wave_max(ran) - 1; t >= 0; --t) {
            if (t < ran) {
                for (int j = 1; j <= M; ++j) LS_AT(w, j - 1) = (double)mine[j];
                for (int it = 0; it <= t; ++it) ls_sweep(w, M, d, lo, hi, thr, pm, cm);   // pm, cm: those of sweep t
                for (int j = 0; j < M; ++j)
                    if (!((cm >> j) & 1ull)) LS_AT(g, j) = 0.0;
                for (int m = M - 2; m >= 0; --m)
                    if ((pm >> m) & 1ull) {
                        const double gm = LS_AT(g, m), gn = LS_AT(g, m + 1), hs = 0.5 * (gn - gm);
                        LS_AT(g, m) = gm + hs;
                        LS_AT(g, m + 1) = gn - hs;
                    }
            }
        }
        if (live) mine[0] = gk;
        for (int j = 1; live && j <= M; ++j) mine[j] = (T)LS_AT(g, j - 1);
    }
    __syncthreads();
    wave_tile_out(rows, out0, base, cnt, M1, S);
}
#undef LS_AT

template <typename T, int OP>
int lsp_lane_launch_t(const void* in0, const void* in1, int64_t F, int M, double p, int q, void* out0, void* unstable, hipStream_t st)
{
    const int HP = (M + 1) / 2 + 1;
    const int W = OP == LS_LSP2LPC_FWD ? 2 * HP : OP == LS_LSP2LPC_BWD ? 2 * HP + M : OP == LS_CHECK_FWD ? M : 2 * M;
    const size_t lds = 64 * (size_t)W * sizeof(double) + 64 * (size_t)((M + 1) | 1) * sizeof(T);
    if (launch_lds<lsp_lane_kernel<T, OP>>(LS_MAX_LDS, "%s: cannot reserve LDS", dim3((unsigned)((F + 63) / 64)), dim3(64), lds, st, (const T*)in0,
                                           (const T*)in1, (long)F, M, p, q, W, (T*)out0, (int*)unstable))
        return fail(DSA_ERR_LAUNCH, "%s: cannot reserve LDS", kLsLaneNames[OP]);   // (the message again, with the name in it)
    return check_launch(kLsLaneNames[OP]);
}

template <int OP>
int lsp_lane_launch(const char* what, const void* in0, const void* in1, bool two, int64_t F, int32_t M, double p, int32_t q, int32_t dtype,
                    void* out0, void* unstable, void* stream)
{
    if (!(F >= 0 && M >= 0 && M <= DSA_LSP_MAX_ORDER && q >= 0)) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: invalid sizes", what);
    if (F == 0) return DSA_OK;
    if (!(in0 && out0 && (!two || in1))) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    return with_dtype(dtype, what, [&](auto tag) {
        return lsp_lane_launch_t<decltype(tag), OP>(in0, in1, F, M, p, q, out0, unstable, (hipStream_t)stream);
    });
}

int lsp_wave_check(const char* what, int64_t F, int32_t M, bool pointers)
{
    if (!(F >= 0 && M >= 0 && M <= DSA_LSP_MAX_ORDER)) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: invalid sizes", what);
    if (F > 0 && !pointers) return fail(DSA_ERR_INVALID_ARGUMENT, "%s: null pointer", what);
    return DSA_OK;
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_lpc2lsp_fwd(const void* a, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype, void* w, int32_t* failed,
                               void* stream)
{
    if (int rc = lsp_wave_check("lpc2lsp_fwd", F, M, a && w)) return rc;
    if (F == 0) return DSA_OK;
    const dim3 grid((unsigned)(F < (1 << 20) ? F : (1 << 20)));
    return with_dtype(dtype, "lpc2lsp_fwd", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((lsp_lpc2lsp_fwd_kernel<T>), grid, dim3(64), 0, (hipStream_t)stream, (const T*)a, (long)F, M, log_gain, unit, (T*)w,
                           (int*)failed);
        return check_launch("lsp_lpc2lsp_fwd");
    });
}

DSA_EXPORT int dsa_lpc2lsp_bwd(const void* gw, const void* a, const void* w, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype,
                               void* ga, void* stream)
{
    if (int rc = lsp_wave_check("lpc2lsp_bwd", F, M, gw && a && w && ga)) return rc;
    if (F == 0) return DSA_OK;
    const dim3 grid((unsigned)(F < (1 << 20) ? F : (1 << 20)));
    return with_dtype(dtype, "lpc2lsp_bwd", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((lsp_lpc2lsp_bwd_kernel<T>), grid, dim3(64), 0, (hipStream_t)stream, (const T*)gw, (const T*)a, (const T*)w, (long)F, M,
                           log_gain, unit, (T*)ga);
        return check_launch("lsp_lpc2lsp_bwd");
    });
}

DSA_EXPORT int dsa_lsp2lpc_fwd(const void* w, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype, void* a, void* stream)
{
    return lsp_lane_launch<LS_LSP2LPC_FWD>("lsp2lpc_fwd", w, nullptr, false, F, M, unit, log_gain != 0, dtype, a, nullptr, stream);
}

DSA_EXPORT int dsa_lsp2lpc_bwd(const void* ga, const void* w, int64_t F, int32_t M, int32_t log_gain, double unit, int32_t dtype, void* gw,
                               void* stream)
{
    return lsp_lane_launch<LS_LSP2LPC_BWD>("lsp2lpc_bwd", ga, w, true, F, M, unit, log_gain != 0, dtype, gw, nullptr, stream);
}

DSA_EXPORT int dsa_lspcheck_fwd(const void* w, int64_t F, int32_t M, double min_distance, int32_t n_iter, int32_t dtype, void* out,
                                int32_t* unstable, void* stream)
{
    return lsp_lane_launch<LS_CHECK_FWD>("lspcheck_fwd", w, nullptr, false, F, M, min_distance, n_iter, dtype, out, unstable, stream);
}

DSA_EXPORT int dsa_lspcheck_bwd(const void* gout, const void* w, int64_t F, int32_t M, double min_distance, int32_t n_iter, int32_t dtype,
                                void* gw, void* stream)
{
    return lsp_lane_launch<LS_CHECK_BWD>("lspcheck_bwd", gout, w, true, F, M, min_distance, n_iter, dtype, gw, nullptr, stream);
}
