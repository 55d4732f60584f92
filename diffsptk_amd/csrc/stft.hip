// Fused STFT (a5) for gfx950: the tuned kernels and the entries dsa_stft_fwd / _bwd, dsa_istft_fwd, dsa_stft_fbank_fwd.
//
// Two kernel families:
//  * generic  -- any frame length / period / even fft length, float32 and float64, every
//                option of the reference.  One workgroup per frame, direct DFT against a
//                host-built twiddle table.  Correctness path for odd configurations and for
//                float64 (gradcheck); never the fast path.  Lives in spec.hip; reached
//                through stft_generic_fwd / stft_generic_bwd (common.h).
//  * tuned    -- nfft = 512, float32: the BASELINE configuration.  One workgroup handles 16
//                consecutive frames of one utterance: the waveform stretch they share is read
//                from HBM once into LDS (frames overlap there, not in HBM), each frame is
//                transformed by 16 lanes (4 frames per wave64) as a 256-point complex FFT =
//                radix-16 in registers -> twiddle -> 16x16 transpose through LDS -> radix-16,
//                and the real-FFT split + |.|^2 + eps + formatting is fused into the
//                coalesced write of the (frames x 257) tile.
//                Algorithmic HBM traffic: P*4 B read + 257*4 B written per frame.
//
// Reference semantics: diffsptk/modules/{stft,istft}.py (cited per kernel).
#include "common.h"
#include "stft_tile.h"

namespace dsa {

// =========================================================================== tuned rFFT-512 path

struct alignas(8) cf {   // 8-byte aligned: LDS accesses of a complex value become one ds_read_b64 / ds_write_b64 (not read2_b32 pairs)
    float re, im;
};
__device__ __forceinline__ cf operator+(cf a, cf b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cf operator-(cf a, cf b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cf cmul(cf a, cf b)
{
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// 4-point DFT in place, forward (W4 = -i); INV conjugates the kernel.
template <bool INV>
__device__ __forceinline__ void dft4(cf& a0, cf& a1, cf& a2, cf& a3)
{
    cf s02 = a0 + a2, d02 = a0 - a2, s13 = a1 + a3, d13 = a1 - a3;
    a0 = s02 + s13;
    a2 = s02 - s13;
    if (!INV) {
        a1 = {d02.re + d13.im, d02.im - d13.re};  // d02 - i d13
        a3 = {d02.re - d13.im, d02.im + d13.re};  // d02 + i d13
    } else {
        a1 = {d02.re - d13.im, d02.im + d13.re};
        a3 = {d02.re + d13.im, d02.im - d13.re};
    }
}

// 16-point DFT in registers (radix 4 x 4).  Output order: X[k] sits in v[4*(k&3) + (k>>2)].
template <bool INV>
__device__ __forceinline__ void fft16(cf (&v)[16])
{
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R2 = 0.70710678118654752f;
    constexpr float sg = INV ? 1.f : -1.f;  // sign of the imaginary part of W16^e
#pragma unroll
    for (int n0 = 0; n0 < 4; ++n0) dft4<INV>(v[n0], v[n0 + 4], v[n0 + 8], v[n0 + 12]);
    // after the first pass v[n0 + 4q] = B[n0][q]; twiddle by W16^(n0*q)
    v[1 + 4 * 1] = cmul(v[1 + 4 * 1], cf{C1, sg * S1});   // e = 1
    v[1 + 4 * 2] = cmul(v[1 + 4 * 2], cf{R2, sg * R2});   // e = 2
    v[1 + 4 * 3] = cmul(v[1 + 4 * 3], cf{S1, sg * C1});   // e = 3
    v[2 + 4 * 1] = cmul(v[2 + 4 * 1], cf{R2, sg * R2});   // e = 2
    v[2 + 4 * 2] = cf{-sg * v[2 + 4 * 2].im, sg * v[2 + 4 * 2].re};   // e = 4: (0, sg) * v
    v[2 + 4 * 3] = cmul(v[2 + 4 * 3], cf{-R2, sg * R2});  // e = 6
    v[3 + 4 * 1] = cmul(v[3 + 4 * 1], cf{S1, sg * C1});   // e = 3
    v[3 + 4 * 2] = cmul(v[3 + 4 * 2], cf{-R2, sg * R2});  // e = 6
    v[3 + 4 * 3] = cmul(v[3 + 4 * 3], cf{-C1, -sg * S1}); // e = 9
#pragma unroll
    for (int q = 0; q < 4; ++q) dft4<INV>(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
#define FFT16_OUT(k) (4 * ((k)&3) + ((k) >> 2))

#ifdef DSA_STFT_TIMING
__device__ unsigned long long g_stft_stamps[16];
#define STFT_STAMP(i)                                                                 \
    do {                                                                              \
        if (wid == 0 && lane == 0 && c == nw)                                         \
            g_stft_stamps[i] = __builtin_readcyclecounter();                          \
    } while (0)
#else
#define STFT_STAMP(i)
#endif

// ShortTimeFourierTransform._forward stft.py:237-241 for nfft = 512, float32.
// One wave64 per workgroup, autonomous (no inter-wave barriers): it owns kFPW = 4 consecutive
// frames of one utterance per pass -- the 3P + L samples they share are read from HBM once into
// LDS -- and writes their 4 x 257 output rows as one contiguous, 16-byte aligned run of float4.
// LDS is kept to ~10 KB per wave so that 12+ waves fit a CU (the pass is a long dependent chain;
// throughput comes from waves in flight):
//   zbuf[kFPW][256] cf : (a) first the input stretch (3P + L floats), (b) then the 16 x 16
//                        transpose tiles (row stride 17: element (k1, j) at k1*17 + j),
//                        (c) then the spectra Z in natural order, (d) finally the staged 4 x 257
//                        output tile -- each use is dead before the next begins;
//   t256[16][16] cf    : W256^(j k1), shared by the 4 frames;   fmax[kFPW].
// (kFPW, the tile stride kZS and DSA_WAVE_SYNC, the fence between the phases: stft_tile.h)
// PLAIN: power format, no relative floor, constant padding, fixed at compile time (the bench path): the format
// branches and the per-frame maxima leave the register allocation.
// LC: frame length fixed at compile time (0 = runtime).  With LC = 400 the selects that cut a lane's 32 samples at
// the frame end fold away for 15 of the 16 sample pairs, and the three pairs past the frame are constant zeros
// that the compiler propagates through the first FFT stage.
// The PLAIN instantiations need < 128 registers (stft.hip is built without packed-float32 selection), so four
// waves fit a SIMD; LDS is what limits them then, so two waves share a workgroup and with it the 2 KB twiddle table
// (8 workgroups x 19.5 KB per CU).  The waves stay autonomous: each fills the whole table itself (identical values)
// before its first use, and no barrier is ever needed.
template <bool ZMEAN, bool PLAIN = false, int LC = 0>
__global__ __launch_bounds__(128, 4) void stft512_fwd_kernel(
    const float* __restrict__ x, long Tlen, long N, int L, int P, int left, int mode_arg,
    const float* __restrict__ w, const float* __restrict__ twiddle, float eps, int use_floor_arg,
    float floor_lin, int fmt_arg, float* __restrict__ y, long total_chunks, int chunks_per_utt,
    int io_floats)
{
    const int use_floor = PLAIN ? 0 : use_floor_arg;
    const int fmt = PLAIN ? (int)DSA_SPEC_POWER : fmt_arg;
    const int mode = PLAIN ? (int)DSA_PAD_CONSTANT : mode_arg;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int WPB = 2;   // waves per workgroup
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    cf* zbuf = reinterpret_cast<cf*>(smem_raw) + wv * kFPW * kZS;
    float* io_buf = reinterpret_cast<float*>(zbuf);  // aliases zbuf (see above)
    cf* t256 = reinterpret_cast<cf*>(smem_raw) + WPB * kFPW * kZS;
    float* fmax = reinterpret_cast<float*>(t256 + 256) + wv * kFPW;
    (void)io_floats;
    const long wid = (long)blockIdx.x * WPB + wv, nw = (long)gridDim.x * WPB;   // this wave, all waves

    const int lane = threadIdx.x & 63;
    const int j = lane & 15;   // lane within the frame group
    const int fl = lane >> 4;  // frame slot within the pass (0..3)

    // per-wave constants: per-lane window, W256^(j*k1) table, split twiddles of this lane's bins
    float wreg[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        int l = 2 * j + 32 * (r >> 1) + (r & 1);
        wreg[r] = l < L ? w[l] : 0.f;
    }
    for (int i = lane; i < 256; i += 64) {
        int m = 2 * (i & 15) * (i >> 4);  // entry [k1 = i >> 4][j = i & 15]: W256^(j k1) = W512^(2 j k1)
        // HALVED: the factor 1/2 of the real-FFT split X[k] = (S + ...) / 2 rides on the twiddle (exact: a power of two)
        t256[i] = cf{0.5f * twiddle[2 * m], 0.5f * twiddle[2 * m + 1]};
    }
    const cf twA = cf{twiddle[2 * (lane + 1)], twiddle[2 * (lane + 1) + 1]};    // W512^(lane+1)
    const cf twB = cf{twiddle[2 * (lane + 65)], twiddle[2 * (lane + 65) + 1]};  // W512^(lane+65)
    const float inv_L = 1.f / (float)L;
    const int K = 257;
    const bool complex_out = fmt == DSA_SPEC_COMPLEX || fmt == DSA_SPEC_COMPLEX_INV;
    // DSA_SPEC_COMPLEX_INV as a FORWARD format: the complex spectrum times c_k / 512 (the adjoint of the inverse
    // transform's weights: the backward of dsa_istft_fwd)
    const float osc = fmt == DSA_SPEC_COMPLEX_INV ? 2.f / 512.f : 1.f, osc_edge = fmt == DSA_SPEC_COMPLEX_INV ? 1.f / 512.f : 1.f;
    cf* zf = zbuf + fl * kZS;

    // (utterance, chunk) of pass c advance incrementally: one 64-bit division per wave instead of one per pass
    long b = wid / chunks_per_utt;
    int ci = (int)(wid - b * chunks_per_utt);
    const long b_step = nw / chunks_per_utt;
    const int ci_step = (int)(nw - b_step * chunks_per_utt);
    // PLAIN: the NEXT pass's stretch is fetched into registers (3 x float4 per lane) while this pass computes, so
    // the HBM round trip leaves the dependent chain of a pass; possible because this instantiation does not spill.
    float4 pre0 = make_float4(0.f, 0.f, 0.f, 0.f), pre1 = pre0, pre2 = pre0;
    bool pre_ok = false;
    for (long c = wid; c < total_chunks; c += nw, b += b_step, ci += ci_step) {
        if (ci >= chunks_per_utt) {
            ci -= chunks_per_utt;
            ++b;
        }
        const long frame0 = (long)ci * kFPW;
        const int nvalid = (int)((N - frame0) < kFPW ? (N - frame0) : kFPW);
        const float* xb = x + b * Tlen;
        DSA_WAVE_SYNC();  // previous pass is done with the LDS tile (single-wave workgroup)
        STFT_STAMP(0);
        // ---- stage the shared waveform stretch (each sample read from HBM once) ----
        {
            const long g0 = frame0 * P - left;
            const int need = (nvalid - 1) * P + L;  // samples the valid frames touch
            const bool interior = g0 >= 0 && g0 + need <= Tlen;
            if (PLAIN && pre_ok) {
                float4* dst4 = reinterpret_cast<float4*>(io_buf);
                const int n4 = need >> 2;
                if (lane < n4) dst4[lane] = pre0;
                if (lane + 64 < n4) dst4[lane + 64] = pre1;
                if (lane + 128 < n4) dst4[lane + 128] = pre2;
            } else if (interior && (((size_t)(xb + g0)) & 15) == 0) {
                const float4* src4 = reinterpret_cast<const float4*>(xb + g0);
                float4* dst4 = reinterpret_cast<float4*>(io_buf);
                const int n4 = need >> 2;
                for (int s = lane; s < n4; s += 64) dst4[s] = src4[s];
                for (int s = (n4 << 2) + lane; s < need; s += 64) io_buf[s] = xb[g0 + s];
            } else {
                for (int s = lane; s < need; s += 64) io_buf[s] = load_padded(xb, g0 + s, Tlen, mode);
            }
        }
        DSA_WAVE_SYNC();
        STFT_STAMP(1);
        if (PLAIN) {   // issue the next pass's loads (no wait here)
            long b2 = b + b_step;
            int ci2 = ci + ci_step;
            if (ci2 >= chunks_per_utt) {
                ci2 -= chunks_per_utt;
                ++b2;
            }
            pre_ok = false;
            if (c + nw < total_chunks) {
                const long fr2 = (long)ci2 * kFPW;
                const int nv2 = (int)((N - fr2) < kFPW ? (N - fr2) : kFPW);
                const long g2 = fr2 * P - left;
                const int need2 = (nv2 - 1) * P + L;
                const float* xb2 = x + b2 * Tlen;
                if (g2 >= 0 && g2 + need2 <= Tlen && (((size_t)(xb2 + g2)) & 15) == 0 && (need2 & 3) == 0 && need2 <= 768) {
                    const float4* src4 = reinterpret_cast<const float4*>(xb2 + g2);
                    const int n4 = need2 >> 2;
                    pre0 = src4[lane < n4 ? lane : n4 - 1];
                    pre1 = src4[lane + 64 < n4 ? lane + 64 : n4 - 1];
                    pre2 = src4[lane + 128 < n4 ? lane + 128 : n4 - 1];
                    pre_ok = true;
                }
            }
        }
        // ---- per frame: window, 256-point complex FFT (16 lanes x 16 points) ----
        cf v[16];
        {
            const float* src = io_buf + fl * P + 2 * j;
            int lim = (LC ? LC : L) - 2 * j;  // element (m1, c) belongs to the frame iff 32 m1 + c < lim
            // recomputed per pass on purpose: hoisted out of the pass loop, the 32 lane masks of the selects below
            // occupy 64 scalar registers for the whole kernel and push the loop's scalars into spills
            if (!LC) asm volatile("" : "+v"(lim));
            float sum = 0.f;
            // all 16 LDS reads are issued back to back (reading past the frame stays inside the tile);
            // samples past the frame are then selected away, never multiplied: zero padding is exact
            // and non-finite neighbours stay out of frames that do not contain them
            float2 raw[16];
#pragma unroll
            for (int m1 = 0; m1 < 16; ++m1) raw[m1] = make_float2(src[32 * m1], src[32 * m1 + 1]);
#pragma unroll
            for (int m1 = 0; m1 < 16; ++m1) {
                const float a0 = 32 * m1 < lim ? raw[m1].x : 0.f;
                const float a1 = 32 * m1 + 1 < lim ? raw[m1].y : 0.f;
                v[m1] = cf{a0, a1};
                if (ZMEAN) sum += a0 + a1;
            }
            float mean = 0.f;
            if (ZMEAN) {  // frame.py:139-140: mean over the L samples of the frame
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
                mean = sum * inv_L;
            }
#pragma unroll
            for (int m1 = 0; m1 < 16; ++m1) {
                float a0 = v[m1].re, a1 = v[m1].im;
                if (ZMEAN) {
                    a0 = 32 * m1 < lim ? a0 - mean : 0.f;
                    a1 = 32 * m1 + 1 < lim ? a1 - mean : 0.f;
                }
                v[m1] = cf{a0 * wreg[2 * m1], a1 * wreg[2 * m1 + 1]};  // window.py:190 (wreg = 0 past L)
            }
        }
        DSA_WAVE_SYNC();  // every lane has its samples: the stretch may be overwritten
        STFT_STAMP(2);
        fft16<false>(v);
        STFT_STAMP(3);
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1)  // twiddle, then transposed store: (k1, j) -> k1*17 + j (row stride 17: every
            zf[k1 * 17 + j] = cmul(v[FFT16_OUT(k1)], t256[k1 * 16 + j]);   // address is lane base + immediate, no XOR math)
        DSA_WAVE_SYNC();
        STFT_STAMP(4);
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = zf[j * 17 + i];  // lane k1 = j reads A[i][k1]: 34 j floats apart, 16 distinct bank pairs
        DSA_WAVE_SYNC();
        STFT_STAMP(5);
        fft16<false>(v);
        STFT_STAMP(6);
#pragma unroll
        for (int k0 = 0; k0 < 16; ++k0) zf[j + 16 * k0] = v[FFT16_OUT(k0)];  // Z[k1 + 16 k0], natural order
        DSA_WAVE_SYNC();
        STFT_STAMP(7);
        // ---- real-FFT split, two bins (k, 256-k) per lane from one pair (Z[k], Z[256-k]) ----
        //   S = a + conj(b), Dd = a - conj(b), Pp = W Dd:
        //   2 X[k] = (S.re + Pp.im, S.im - Pp.re),  2 X[256-k] = (S.re - Pp.im, -S.im - Pp.re)
        // All pairs are read before anything is written: the staged tile reuses the same LDS.
        const long row0 = b * N + frame0;
        const long out0 = row0 * K;
        float* stage = io_buf;
        float2* y2 = reinterpret_cast<float2*>(y);
        // pairs (k, 256 - k) for k = 1..128: part 0 -> k = lane + 1, part 1 -> k = lane + 65 (lane 63
        // gets the self-pair k = 128); bins 0 and 256 come from Z[0] alone: X[0] = re + im, X[256] = re - im
        cf pa[kFPW][2], pb[kFPW][2], z0[kFPW];
#pragma unroll
        for (int f = 0; f < kFPW; ++f) {
            const cf* z = zbuf + f * kZS;
            pa[f][0] = z[lane + 1];
            pb[f][0] = z[255 - lane];
            pa[f][1] = z[lane + 65];
            pb[f][1] = z[191 - lane];
            z0[f] = z[0];
        }
        DSA_WAVE_SYNC();
        float fm[kFPW] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < kFPW; ++f) {
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const int k = part == 0 ? lane + 1 : lane + 65;
                const cf W = part == 0 ? twA : twB;
                const cf a = pa[f][part], bq = pb[f][part];
                const cf S = {a.re + bq.re, a.im - bq.im};
                const cf Dd = {a.re - bq.re, a.im + bq.im};
                const cf Pp = cmul(W, Dd);
                const cf X1 = {S.re + Pp.im, S.im - Pp.re};     // Z arrives halved (see t256)
                const cf X2 = {S.re - Pp.im, -S.im - Pp.re};
                if (complex_out) {
                    if (f < nvalid) {
                        y2[out0 + f * K + k] = make_float2(X1.re * osc, X1.im * osc);
                        y2[out0 + f * K + 256 - k] = make_float2(X2.re * osc, X2.im * osc);
                    }
                } else {
                    const float s1 = X1.re * X1.re + X1.im * X1.im + eps;  // spec.py:173
                    const float s2 = X2.re * X2.re + X2.im * X2.im + eps;
                    stage[f * K + k] = s1;
                    stage[f * K + 256 - k] = s2;
                    if (use_floor) {
                        const float mx = s1 > s2 ? s1 : s2;
                        fm[f] = mx > fm[f] ? mx : fm[f];
                    }
                }
            }
            // the two real-valued end bins
            const float x0 = 2.f * (z0[f].re + z0[f].im), x256 = 2.f * (z0[f].re - z0[f].im);   // these two take Z[0] whole
            if (complex_out) {
                if (f < nvalid && lane == 0) {
                    y2[out0 + f * K] = make_float2(x0 * osc_edge, 0.f);
                    y2[out0 + f * K + 256] = make_float2(x256 * osc_edge, 0.f);
                }
            } else {
                const float s0 = x0 * x0 + eps, s256 = x256 * x256 + eps;
                if (lane == 0) {
                    stage[f * K] = s0;
                    stage[f * K + 256] = s256;
                }
                if (use_floor) {
                    const float mx = s0 > s256 ? s0 : s256;
                    fm[f] = mx > fm[f] ? mx : fm[f];
                }
            }
        }
        if (complex_out) continue;
        if (use_floor) {  // per-frame maximum for the relative floor (spec.py:174-176)
#pragma unroll
            for (int f = 0; f < kFPW; ++f) {
                float m = wave_max(fm[f]);
                if (lane == 0) fmax[f] = m;
            }
        }
        DSA_WAVE_SYNC();
        STFT_STAMP(8);
        // ---- formatter + coalesced write of the staged tile ----
        const bool plain = !use_floor && fmt == DSA_SPEC_POWER;
        if (nvalid == kFPW && (row0 & 3) == 0) {
            // 4 rows x 257 floats = 257 float4, 16-byte aligned because row0 % 4 == 0
            float4* y4 = reinterpret_cast<float4*>(y + out0);
            const float4* s4 = reinterpret_cast<const float4*>(stage);
#pragma unroll
            for (int jj = 0; jj < 5; ++jj) {
                const int t = lane + 64 * jj;
                if (t < K) {
                    float4 q = s4[t];
                    if (!plain) {
                        float o4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            const int idx = 4 * t + cc;
                            float sv = o4[cc];
                            if (use_floor) {
                                const int f = idx >= 3 * K ? 3 : (idx >= 2 * K ? 2 : (idx >= K ? 1 : 0));
                                const float flv = fmax[f] * floor_lin;
                                sv = sv > flv ? sv : flv;
                            }
                            o4[cc] = spec_format(sv, fmt);
                        }
                        q = make_float4(o4[0], o4[1], o4[2], o4[3]);
                    }
                    y4[t] = q;
                }
            }
        } else {
            const int total = nvalid * K;
            for (int idx = lane; idx < total; idx += 64) {
                float sv = stage[idx];
                if (use_floor) {
                    const int f = idx >= 3 * K ? 3 : (idx >= 2 * K ? 2 : (idx >= K ? 1 : 0));
                    const float flv = fmax[f] * floor_lin;
                    sv = sv > flv ? sv : flv;
                }
                y[out0 + idx] = spec_format(sv, fmt);
            }
        }
        STFT_STAMP(9);
    }
}

}  // namespace dsa
#include "stft_pk.h"
#include "stft_bwd_pk.h"
#include "stft_pk_big.h"
#include "stft_bwd_pk_big.h"
namespace dsa {

// Backward of stft512_fwd_kernel (autograd of stft.py:237-241), same
// wave-per-pass structure and LDS tile.  Per pass of 4 frames:
//   recompute Z (stage, window, FFT-256) -> split into X[k] -> cotangent S[k] of the half spectrum
//   (power formats: gs[k] X[k] with gs = gy * format'(s);  complex: gy / 2) -> Hermitian-pack into a
//   256-point complex spectrum Zin[k] = (a + b) + i conj(W^k) (a - b), a = S[k], b = conj(S[256-k]) ->
//   inverse FFT-256 (same radix-16 x 16 code, conjugated twiddles) = cotangent of the windowed
//   frame -> times window (-> zmean adjoint) -> overlap-add of the 4 frames inside the pass ->
//   one contiguous partial span of 3P + L samples per pass, written to `part` (pass-major).
// A second kernel (stft_span_gather_kernel) adds the <= ceil((3P+L)/(4P)) partial spans that cover
// each waveform sample in a fixed order: deterministic, no atomics.
#ifndef DSA_STFT_BWD_WAVES
#define DSA_STFT_BWD_WAVES 3
#endif
// CPLX: the cotangent is complex (format "complex" or an inverse transform): X is not needed, so the
// input stretch is not staged and the forward FFT is skipped.
// PLAIN: power format with constant padding, fixed at compile time (the training path of the bench
// configuration): the format switch and the padding modes leave the register allocation.
template <bool ZMEAN, bool CPLX = false, bool PLAIN = false>
__global__ __launch_bounds__((PLAIN || CPLX) ? 128 : 64, (PLAIN || CPLX) ? 4 : DSA_STFT_BWD_WAVES) void stft512_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gy, long Tlen, long N, int L, int P, int left,
    int mode_arg, const float* __restrict__ w, const float* __restrict__ twiddle, float eps, int fmt_arg,
    float* __restrict__ part, long total_chunks, int chunks_per_utt, int span)
{
    const int fmt = PLAIN ? (int)DSA_SPEC_POWER : fmt_arg;
    const int mode = PLAIN ? (int)DSA_PAD_CONSTANT : mode_arg;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int WPB = (PLAIN || CPLX) ? 2 : 1;   // waves per workgroup (they share the twiddle table only, as in the forward)
    const int wv = WPB > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    cf* zbuf = reinterpret_cast<cf*>(smem_raw) + wv * kFPW * kZS;
    float* io_buf = reinterpret_cast<float*>(zbuf);
    cf* t256 = WPB > 1 ? reinterpret_cast<cf*>(smem_raw) + WPB * kFPW * kZS : zbuf + kFPW * 256;
    const long wid = (long)blockIdx.x * WPB + wv, nw = (long)gridDim.x * WPB;

    const int lane = threadIdx.x & 63;
    const int j = lane & 15, fl = lane >> 4;
    float wreg[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        int l = 2 * j + 32 * (r >> 1) + (r & 1);
        wreg[r] = l < L ? w[l] : 0.f;
    }
    for (int i = lane; i < 256; i += 64) {
        int m = 2 * (i & 15) * (i >> 4);
        t256[i] = cf{twiddle[2 * m], twiddle[2 * m + 1]};
    }
    const cf twA = cf{twiddle[2 * lane], twiddle[2 * lane + 1]};
    const cf twB = cf{twiddle[2 * (lane + 64)], twiddle[2 * (lane + 64) + 1]};
    const float inv_L = 1.f / (float)L;
    const int K = 257;
    const bool complex_out = fmt == DSA_SPEC_COMPLEX || fmt == DSA_SPEC_COMPLEX_INV;
    // complex cotangent: the adjoint takes g / 2 (g at the two real-valued bins); the inverse transform's
    // weights c_k / 512 on top of that make it g / 512 everywhere
    const float cot_scale = fmt == DSA_SPEC_COMPLEX_INV ? 1.f / 512.f : 0.5f;
    const float cot_edge = fmt == DSA_SPEC_COMPLEX_INV ? 1.f : 2.f;
    cf* zf = zbuf + fl * 256;
    const float2* gy2 = reinterpret_cast<const float2*>(gy);

    // (utterance, chunk) of pass c advance incrementally: one 64-bit division per wave instead of one per pass
    long b = wid / chunks_per_utt;
    int ci = (int)(wid - b * chunks_per_utt);
    const long b_step = nw / chunks_per_utt;
    const int ci_step = (int)(nw - b_step * chunks_per_utt);
    for (long c = wid; c < total_chunks; c += nw, b += b_step, ci += ci_step) {
        if (ci >= chunks_per_utt) {
            ci -= chunks_per_utt;
            ++b;
        }
        const long frame0 = (long)ci * kFPW;
        const int nvalid = (int)((N - frame0) < kFPW ? (N - frame0) : kFPW);
        const float* xb = x + b * Tlen;
        DSA_WAVE_SYNC();
        cf v[16];
        int lim = L - 2 * j;
        asm volatile("" : "+v"(lim));   // per pass on purpose: hoisted, the lane masks of the selects fill the scalar registers
        if constexpr (!CPLX) {
        {   // stage the input stretch
            const long g0 = frame0 * P - left;
            const int need = (nvalid - 1) * P + L;
            const bool interior = g0 >= 0 && g0 + need <= Tlen;
            if (interior && (((size_t)(xb + g0)) & 15) == 0) {
                const float4* src4 = reinterpret_cast<const float4*>(xb + g0);
                float4* dst4 = reinterpret_cast<float4*>(io_buf);
                const int n4 = need >> 2;
                for (int s = lane; s < n4; s += 64) dst4[s] = src4[s];
                for (int s = (n4 << 2) + lane; s < need; s += 64) io_buf[s] = xb[g0 + s];
            } else {
                for (int s = lane; s < need; s += 64) io_buf[s] = load_padded(xb, g0 + s, Tlen, mode);
            }
        }
        DSA_WAVE_SYNC();
        {
            const float* src = io_buf + fl * P + 2 * j;
            float sum = 0.f;
#pragma unroll
            for (int m1 = 0; m1 < 16; ++m1) {
                float a0 = 0.f, a1 = 0.f;
                if (32 * m1 + 32 <= L) {
                    a0 = src[32 * m1];
                    a1 = src[32 * m1 + 1];
                } else if (32 * m1 < L) {
                    a0 = 32 * m1 < lim ? src[32 * m1] : 0.f;
                    a1 = 32 * m1 + 1 < lim ? src[32 * m1 + 1] : 0.f;
                }
                v[m1] = cf{a0, a1};
                if (ZMEAN) sum += a0 + a1;
            }
            float mean = 0.f;
            if (ZMEAN) {
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 16);
                mean = sum * inv_L;
            }
#pragma unroll
            for (int m1 = 0; m1 < 16; ++m1) {
                float a0 = v[m1].re, a1 = v[m1].im;
                if (ZMEAN) {
                    a0 = 32 * m1 < lim ? a0 - mean : 0.f;
                    a1 = 32 * m1 + 1 < lim ? a1 - mean : 0.f;
                }
                v[m1] = cf{a0 * wreg[2 * m1], a1 * wreg[2 * m1 + 1]};
            }
        }
        DSA_WAVE_SYNC();
        fft16<false>(v);
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) zf[k1 * 16 + (j ^ k1)] = cmul(v[FFT16_OUT(k1)], t256[k1 * 16 + j]);
        DSA_WAVE_SYNC();
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = zf[j * 16 + (i ^ j)];
        DSA_WAVE_SYNC();
        fft16<false>(v);
#pragma unroll
        for (int k0 = 0; k0 < 16; ++k0) zf[j + 16 * k0] = v[FFT16_OUT(k0)];
        DSA_WAVE_SYNC();
        }
        // ---- split, cotangent, Hermitian packing (pairs read first, then written in place) ----
        const long out0 = (b * N + frame0) * K;
        cf pa[kFPW][3], pb[kFPW][3];
#pragma unroll
        for (int f = 0; f < kFPW; ++f) {
            const cf* z = zbuf + f * 256;
            if constexpr (CPLX) {
                pa[f][0] = pb[f][0] = pa[f][1] = pb[f][1] = pa[f][2] = pb[f][2] = cf{0.f, 0.f};
            } else {
                pa[f][0] = z[lane];
                pb[f][0] = z[(256 - lane) & 255];
                pa[f][1] = z[lane + 64];
                pb[f][1] = z[192 - lane];
                pa[f][2] = z[128];
                pb[f][2] = pa[f][2];
            }
        }
        DSA_WAVE_SYNC();
#pragma unroll
        for (int f = 0; f < kFPW; ++f) {
            cf* z = zbuf + f * 256;
            const bool fv = f < nvalid;
#pragma unroll
            for (int part_i = 0; part_i < 3; ++part_i) {
                const int k = part_i == 0 ? lane : (part_i == 1 ? lane + 64 : 128);
                const cf W = part_i == 0 ? twA : (part_i == 1 ? twB : cf{0.f, -1.f});
                const cf a = pa[f][part_i], bq = pb[f][part_i];
                const cf S = {a.re + bq.re, a.im - bq.im};
                const cf Dd = {a.re - bq.re, a.im + bq.im};
                const cf Pp = cmul(W, Dd);
                const cf X1 = {0.5f * (S.re + Pp.im), 0.5f * (S.im - Pp.re)};     // X[k]
                const cf X2 = {0.5f * (S.re - Pp.im), 0.5f * (-S.im - Pp.re)};    // X[256-k]
                // half-spectrum cotangents S1 = S[k], S2 = S[256-k]
                cf S1, S2;
                if (complex_out) {
                    const float2 g1 = fv ? gy2[out0 + f * K + k] : make_float2(0.f, 0.f);
                    const float2 g2 = fv ? gy2[out0 + f * K + 256 - k] : make_float2(0.f, 0.f);
                    S1 = cf{cot_scale * g1.x, cot_scale * g1.y};
                    S2 = cf{cot_scale * g2.x, cot_scale * g2.y};
                } else {
                    const float s1 = X1.re * X1.re + X1.im * X1.im + eps;
                    const float s2 = X2.re * X2.re + X2.im * X2.im + eps;
                    float g1 = fv ? gy[out0 + f * K + k] : 0.f;
                    float g2 = fv ? gy[out0 + f * K + 256 - k] : 0.f;
                    switch (fmt) {  // d format(s) / d s  (spec.py:123-132)
                    case DSA_SPEC_DB: g1 *= 4.342944819032518f / s1; g2 *= 4.342944819032518f / s2; break;
                    case DSA_SPEC_LOGMAG: g1 *= 0.5f / s1; g2 *= 0.5f / s2; break;
                    case DSA_SPEC_MAG: g1 *= 0.5f / sqrtf(s1); g2 *= 0.5f / sqrtf(s2); break;
                    default: break;
                    }
                    S1 = cf{g1 * X1.re, g1 * X1.im};
                    S2 = cf{g2 * X2.re, g2 * X2.im};
                }
                if (part_i == 0) {
                    // k = 0 pairs with 256: both real-valued bins carry the full (not half) weight
                    const float e0 = complex_out ? cot_edge : 2.f;
                    const float s0r = lane == 0 ? e0 * S1.re : S1.re, s0i = lane == 0 ? 0.f : S1.im;
                    const float s6r = lane == 0 ? e0 * S2.re : S2.re, s6i = lane == 0 ? 0.f : S2.im;
                    S1 = cf{s0r, s0i};
                    S2 = cf{s6r, s6i};
                }
                // Zin[k] = (a + b) + i Q, Zin[256-k] = conj(a + b) + i conj(Q), a = S1, b = conj(S2),
                // Q = conj(W) (a - b)
                const cf ab = {S1.re + S2.re, S1.im - S2.im};
                const cf amb = {S1.re - S2.re, S1.im + S2.im};
                const cf Q = cmul(cf{W.re, -W.im}, amb);
                if (part_i == 2) {
                    if (lane == 0) z[128] = cf{2.f * S1.re, -2.f * S1.im};  // 2 conj(S[128])
                } else {
                    z[k] = cf{ab.re - Q.im, ab.im + Q.re};
                    if (!(part_i == 0 && lane == 0)) z[256 - k] = cf{ab.re + Q.im, -ab.im + Q.re};
                }
            }
        }
        DSA_WAVE_SYNC();
        // ---- inverse FFT-256 (unnormalised, conjugated twiddles), same data movement ----
#pragma unroll
        for (int m1 = 0; m1 < 16; ++m1) v[m1] = zf[j + 16 * m1];
        DSA_WAVE_SYNC();
        fft16<true>(v);
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1) {
            const cf t = t256[k1 * 16 + j];
            zf[k1 * 16 + (j ^ k1)] = cmul(v[FFT16_OUT(k1)], cf{t.re, -t.im});
        }
        DSA_WAVE_SYNC();
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = zf[j * 16 + (i ^ j)];
        DSA_WAVE_SYNC();
        fft16<true>(v);
        // lane j now holds time points m = j + 16 k0: samples l = 2m, 2m+1 -- the forward's own
        // register <-> sample map, so the window (and zmean adjoint) reuse wreg / the 16-lane sum
        {
            float gsum = 0.f;
#pragma unroll
            for (int k0 = 0; k0 < 16; ++k0) {
                cf o = v[FFT16_OUT(k0)];
                o = cf{o.re * wreg[2 * k0], o.im * wreg[2 * k0 + 1]};
                v[FFT16_OUT(k0)] = o;
                if (ZMEAN) gsum += o.re + o.im;
            }
            float gm = 0.f;
            if (ZMEAN) {
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o, 16);
                gm = gsum * inv_L;
            }
#pragma unroll
            for (int k0 = 0; k0 < 16; ++k0) {
                cf o = v[FFT16_OUT(k0)];
                if (ZMEAN) {
                    o.re = 32 * k0 < lim ? o.re - gm : 0.f;
                    o.im = 32 * k0 + 1 < lim ? o.im - gm : 0.f;
                }
                zf[j + 16 * k0] = o;  // gframe[l] as floats: l = 2 (j + 16 k0) + {0, 1}
            }
        }
        DSA_WAVE_SYNC();
        // ---- overlap-add of the pass's frames; one contiguous partial span per pass ----
        float* dst = part + c * (long)span;
        for (int sidx = lane; sidx < span; sidx += 64) {
            float acc = 0.f;
#pragma unroll
            for (int f = 0; f < kFPW; ++f) {
                const int l = sidx - f * P;
                if (f < nvalid && l >= 0 && l < L) acc += reinterpret_cast<const float*>(zbuf + f * 256)[l];
            }
            dst[sidx] = acc;
        }
    }
}

// gx[b][t] = sum over the passes whose span covers t (adjoint of the on-the-fly padding: positions
// outside [0, T) are dropped for constant padding -- other modes use the generic backward).
// div != nullptr (inverse STFT): the sum is divided by div[t] + div_eps, the overlap-added squared window
// (unframe.py:203-205), so Unframe's division costs no pass of its own.
__global__ void stft_span_gather_kernel(const float* __restrict__ part, long B, long Tlen, int P, int left, int span,
                                        int chunks_per_utt, float* __restrict__ gx, const float* __restrict__ div,
                                        float div_eps)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Tlen) return;
    const long p = t + left;          // position in the padded signal
    const long stride = (long)kFPW * P;  // pass c starts at padded position c * stride
    long c_hi = p / stride;
    if (c_hi > chunks_per_utt - 1) c_hi = chunks_per_utt - 1;
    long c_lo = p - span + 1 <= 0 ? 0 : (p - span + stride) / stride;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {   // grid.y is capped at 65535 utterances
        float acc = 0.f;
        for (long c = c_lo; c <= c_hi; ++c) acc += part[(b * chunks_per_utt + c) * (long)span + (p - c * stride)];
        gx[b * Tlen + t] = div ? acc / (div[t] + div_eps) : acc;
    }
}

static int stft512_lds_bytes(int L, int P, int* io_floats)
{
    // the input stretch and the staged output tile both live inside the 4 x 256 complex tile
    int span = (kFPW - 1) * P + L;
    *io_floats = (span + 3) & ~3;
    if (*io_floats > kFPW * 512) return 1 << 30;  // stretch does not fit: use the generic kernel
    return kFPW * kZS * 8 + 256 * 8 + 16;   // (the backward kernel keeps stride 256 inside the same allocation)
}

static int stft512_lds_bytes2() { return 2 * kFPW * kZS * 8 + 256 * 8 + 2 * kFPW * 4; }   // two waves + the shared table

}  // namespace dsa

using namespace dsa;

// =========================================================================== C-ABI

static void stft512_launch(bool zmean, dim3 grid, hipStream_t st, const float* x, long T, long N, int L, int P, int left, int mode,
                           const float* w, const float* tw, float eps, int use_floor, float floor_lin, int fmt, float* y,
                           long total_chunks, int chunks_per_utt, int io_floats)
{
    // `grid` counts waves; they are paired into 128-thread workgroups that share the twiddle table
    const bool plain = !use_floor && fmt == DSA_SPEC_POWER && mode == DSA_PAD_CONSTANT;
    const dim3 g2((grid.x + 1) / 2);
    const int lds2 = stft512_lds_bytes2();
    // the packed-float32 kernel with register-direct stores (stft_pk.h) where it applies -- round 6: every pad mode (the mode only
    // changes what the passes that reach over an utterance's end read) and, as an instantiation of its own, zmean and the relative floor
    if (fmt == DSA_SPEC_POWER && L == 400 && (P & 1) == 0 && 3 * P + 512 <= kFPW * kZS * 2) {
        if (zmean || use_floor)
            hipLaunchKernelGGL((stft512_fwd_pk_kernel<400, 0, true>), g2, dim3(128), lds2, st, x, T, N, L, P, left, w, tw, eps, y,
                               total_chunks, chunks_per_utt, (const float*)nullptr, 0.f, 0.f, 0, mode, (int)zmean, use_floor ? floor_lin : -1.f);
        else
            hipLaunchKernelGGL((stft512_fwd_pk_kernel<400>), g2, dim3(128), lds2, st, x, T, N, L, P, left, w, tw, eps, y,
                               total_chunks, chunks_per_utt, (const float*)nullptr, 0.f, 0.f, 0, mode);
        return;
    }
#define DSA_STFT_FWD_LAUNCH(ZM, PL, LCV)                                                                                 \
    hipLaunchKernelGGL((stft512_fwd_kernel<ZM, PL, LCV>), g2, dim3(128), lds2, st, x, T, N, L, P, left, mode, w, tw,      \
                       eps, use_floor, floor_lin, fmt, y, total_chunks, chunks_per_utt, io_floats)
    if (zmean) DSA_STFT_FWD_LAUNCH(true, false, 0);
    else if (plain && L == 400) DSA_STFT_FWD_LAUNCH(false, true, 400);
    else if (plain) DSA_STFT_FWD_LAUNCH(false, true, 0);
    else DSA_STFT_FWD_LAUNCH(false, false, 0);
#undef DSA_STFT_FWD_LAUNCH
}

DSA_EXPORT int dsa_stft_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft,
                            const void* w, const void* twiddle, int32_t center, int32_t zmean,
                            int32_t pad_mode, double eps, int32_t use_floor, double relative_floor_db,
                            int32_t out_format, int32_t dtype, int32_t algo, void* y, void* stream)
{
    DSA_REQUIRE(L > 0 && P > 0 && T > 0 && B >= 0, "stft: sizes must be positive");
    DSA_REQUIRE(nfft > 1 && nfft % 2 == 0, "stft: fft_length must be positive even");
    DSA_REQUIRE(pad_mode >= 0 && pad_mode <= 3, "stft: unknown pad mode");
    DSA_REQUIRE(out_format >= 0 && out_format <= 5, "stft: unknown out_format");
    // F.pad(mode="reflect") needs every pad amount below the signal length (frame.py:130-137: (L//2, (L-1)//2) when
    // centred, (0, L-1) otherwise) and rejects a one-sample signal
    DSA_REQUIRE(pad_mode != DSA_PAD_REFLECT || (center ? L / 2 : L - 1) < T || L == 1,
                "stft: reflect padding needs pad < input length");
    hipStream_t st = (hipStream_t)stream;
    int64_t N = dsa_num_frames(T, P);
    if (B * N == 0) return DSA_OK;
    int left = center ? L / 2 : 0;
    int in_floats = 0;
    int lds = stft512_lds_bytes(L, P, &in_floats);
    bool tuned_ok = dtype == DSA_F32 && nfft == 512 && L <= 512 && lds <= 64 * 1024;
    if (algo == DSA_ALGO_TUNED && !tuned_ok)
        return fail(DSA_ERR_UNSUPPORTED, "stft: tuned kernel needs float32, fft_length 512, frame_length <= 512%s");
    if (tuned_ok && algo != DSA_ALGO_GENERIC) {
        int chunks_per_utt = (int)((N + kFPW - 1) / kFPW);
        long total_chunks = (long)B * chunks_per_utt;
        // persistent waves, every one of them resident from the start: four per SIMD (two-wave workgroups, 19.5 KB of LDS each)
        long grid = 256L * 16;
        if (grid > total_chunks) grid = total_chunks;
        float floor_lin = use_floor ? (float)pow(10.0, relative_floor_db / 10.0) : 0.f;
        stft512_launch(zmean != 0, dim3((unsigned)grid), st, (const float*)x, (long)T, (long)N, L, P, left,
                       pad_mode, (const float*)w, (const float*)twiddle, (float)eps, use_floor, floor_lin,
                       out_format, (float*)y, total_chunks, chunks_per_utt, in_floats);
        return check_launch("stft512_fwd");
    }
    // fft_length 1024 / 2048 (the 44.1 / 48 kHz set-ups of utils/public.py:61-104), power format, constant padding, no zmean, no
    // relative floor: the packed kernel of stft_pk_big.h (round 6; DSA_STFT_BIG=0: the generic kernel, for A/B runs)
    const bool big_on = env_int("DSA_STFT_BIG", 1) != 0;
    if (big_on && dtype == DSA_F32 && algo != DSA_ALGO_GENERIC && (nfft == 1024 || nfft == 2048) && !zmean && !use_floor &&
        out_format == DSA_SPEC_POWER && pad_mode == DSA_PAD_CONSTANT && L <= nfft && (L & 1) == 0 && (P & 1) == 0 && (left & 1) == 0 &&
        (T & 1) == 0 && (((size_t)x) & 7) == 0 && B * N < (int64_t(1) << 31)) {
        const int S = nfft / 512, FPP = 4 / S;
        const int need = (L + 32 * S - 1) / (32 * S);   // sample pairs per lane
        const int chunks_per_utt = (int)((N + FPP - 1) / FPP);
        const long total_chunks = (long)B * chunks_per_utt;
        const int lds_big = 4 * 4 * kZS * 8 + 256 * 8;
        long wgs = (total_chunks + 3) / 4;
        if (wgs > 256L * 3) wgs = 256L * 3;   // persistent: three four-wave workgroups per CU (126 .. 167 registers: 3 .. 4 waves per SIMD)
#define DSA_BIG_LAUNCH(SV, NRV)                                                                                                   \
    hipLaunchKernelGGL((stft_big_fwd_pk_kernel<SV, NRV>), dim3((unsigned)wgs), dim3(256), lds_big, st, (const float*)x, (long)T, (long)N, \
                       L, P, left, (const float*)w, (const float*)twiddle, (float)eps, (float*)y, total_chunks, chunks_per_utt)
        if (S == 2) {
            if (need <= 10) DSA_BIG_LAUNCH(2, 10);
            else if (need <= 13) DSA_BIG_LAUNCH(2, 13);
            else DSA_BIG_LAUNCH(2, 16);
        } else {
            if (need <= 10) DSA_BIG_LAUNCH(4, 10);
            else if (need <= 13) DSA_BIG_LAUNCH(4, 13);
            else DSA_BIG_LAUNCH(4, 16);
        }
#undef DSA_BIG_LAUNCH
        return check_launch(S == 2 ? "stft1024_fwd" : "stft2048_fwd");
    }
    return stft_generic_fwd(dtype, x, B, T, N, L, P, left, pad_mode, zmean, w, nfft, twiddle, out_format, eps, use_floor,
                            relative_floor_db, y, st);
}

// --------------------------------------------------------------------------- fused STFT -> mel filter bank
// (the per-lane table `plan` is the one dsa_fbank_scan_plan of fbank.hip makes)
DSA_EXPORT int dsa_stft_fbank_fwd(const void* x, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft, const void* w,
                                  const void* twiddle, int32_t center, double eps, const void* plan, int32_t C, double floor,
                                  double gamma, int32_t use_power, int32_t dtype, void* y, void* stream)
{
    DSA_REQUIRE(L > 0 && P > 0 && T > 0 && B >= 0, "stft_fbank: sizes must be positive");
    DSA_REQUIRE(B == 0 || (x && w && twiddle && plan && y), "stft_fbank: null pointer");
    DSA_REQUIRE(floor > 0, "stft_fbank: floor must be positive");
    if (!(dtype == DSA_F32 && nfft == 512 && L == 400 && (P & 1) == 0 && 3 * P + 512 <= kFPW * kZS * 2 && C >= 1 && C <= 126))
        return fail(DSA_ERR_UNSUPPORTED,
                    "stft_fbank: the fused kernel needs float32, fft_length 512, frame_length 400, an even frame period and at most "
                    "126 channels (use dsa_stft_fwd + dsa_fbank_fwd)%s");
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = dsa_num_frames(T, P);
    if (B * N == 0) return DSA_OK;
    const int left = center ? L / 2 : 0;
    const int chunks_per_utt = (int)((N + kFPW - 1) / kFPW);
    const long total_chunks = (long)B * chunks_per_utt;
    long waves = 256L * 16;   // four waves per SIMD, four-wave workgroups
    if (waves > total_chunks) waves = total_chunks;
    const int lds = 4 * kFPW * kZS * 8 + 256 * 8 + 16 * 13 * 8 + 128 * 8;
#define DSA_FB_LAUNCH(MODE)                                                                                                  \
    hipLaunchKernelGGL((stft512_fwd_pk_kernel<400, MODE>), dim3((unsigned)((waves + 3) / 4)), dim3(256), lds, st,              \
                       (const float*)x, (long)T, (long)N, L, P, left, (const float*)w, (const float*)twiddle, (float)eps,      \
                       (float*)y, total_chunks, chunks_per_utt, (const float*)plan, (float)floor, (float)gamma, C, (int)DSA_PAD_CONSTANT)
    if (use_power) DSA_FB_LAUNCH(1);
    else DSA_FB_LAUNCH(2);
#undef DSA_FB_LAUNCH
    return check_launch("stft512_fbank_fwd");
}

// dsa_stft_bwd and dsa_istft_fwd: div / div_eps only with out_format DSA_SPEC_COMPLEX_INV (the result is divided by
// div[t] + div_eps); x may be NULL then (a complex cotangent needs no X; the generic kernels get zeros).
static int stft_bwd_impl(const void* gy, const void* x, int64_t B, int64_t T, int32_t L, int32_t P,
                         int32_t nfft, const void* w, const void* twiddle, int32_t center, int32_t zmean,
                         int32_t pad_mode, double eps, int32_t use_floor, double relative_floor_db,
                         int32_t out_format, int32_t dtype, int32_t algo, void* gx, void* gw, void* stream,
                         const void* div, double div_eps)
{
    DSA_REQUIRE(L > 0 && P > 0 && T > 0 && B >= 0, "stft_bwd: sizes must be positive");
    DSA_REQUIRE(nfft > 1 && nfft % 2 == 0, "stft_bwd: fft_length must be positive even");
    DSA_REQUIRE(pad_mode >= 0 && pad_mode <= 3, "stft_bwd: unknown pad mode");
    DSA_REQUIRE(out_format >= 0 && out_format <= 5, "stft_bwd: unknown out_format");
    if (B == 0) return DSA_OK;
    hipStream_t st = (hipStream_t)stream;
    {
        // fft_length 1024 / 2048 (the 44.1 / 48 kHz set-ups), power format, constant padding, no zmean, no relative floor, fixed window:
        // the packed kernel of stft_bwd_pk_big.h (round 6; DSA_STFT_BIG_BWD=0: the generic backward, for A/B runs)
        const bool bigb_on = env_int("DSA_STFT_BIG_BWD", 1) != 0;
        const int64_t Nb = dsa_num_frames(T, P);
        const int leftb = center ? L / 2 : 0;
        if (bigb_on && dtype == DSA_F32 && algo != DSA_ALGO_GENERIC && (nfft == 1024 || nfft == 2048) && !zmean && !use_floor && !gw && !div &&
            out_format == DSA_SPEC_POWER && pad_mode == DSA_PAD_CONSTANT && L <= nfft && (L & 1) == 0 && (P & 1) == 0 && (leftb & 1) == 0 &&
            (T & 1) == 0 && (((size_t)x) & 7) == 0 && (((size_t)gx) & 7) == 0 && B * Nb < (int64_t(1) << 31) && x && gy && gx) {
            const int S = nfft / 512, FPP = 4 / S;
            const int need = (L + 32 * S - 1) / (32 * S);   // sample pairs per lane
            const int ppu = (int)((Nb + FPP - 1) / FPP);    // passes per utterance
            const int warm = ((L + P - 1) / P - 1 + FPP - 1) / FPP;   // passes whose tails a run inherits
            const long waves = 256L * 2 * 4;                 // two four-wave workgroups per CU
            long want = (waves + B - 1) / B;                 // runs per utterance that fill the chip ...
            const long longest = ppu / (4 * (warm > 0 ? warm : 1)) > 0 ? ppu / (4 * (warm > 0 ? warm : 1)) : 1;   // ... but no run shorter than four warm-ups
            const int runs = (int)(want < longest ? want : longest);
            const long items = (long)B * runs;
            const long wv = items < waves ? items : waves;
            const dim3 g2((unsigned)((wv + 3) / 4));
            const int lds_bb = 4 * 4 * kZS * 8 + 256 * 8 + 4 * (2 * 256 * S) * 4;
            auto launch = [&](auto sv, auto nrv) {   // the kernel's S and its sample pairs per lane
                return launch_lds<stft_big_bwd_pk_kernel<decltype(sv)::value, decltype(nrv)::value>>(
                    lds_bb, "stft_bwd: cannot reserve LDS%s", g2, dim3(256), lds_bb, st, (const float*)x, (const float*)gy, (long)T, (long)Nb, L, P, leftb,
                    (const float*)w, (const float*)twiddle, (float*)gx, items, runs, ppu, warm);
            };
            auto by_need = [&](auto sv) {
                return need <= 10 ? launch(sv, int_c<10>{}) : need <= 13 ? launch(sv, int_c<13>{}) : launch(sv, int_c<16>{});
            };
            if (int rc = S == 2 ? by_need(int_c<2>{}) : by_need(int_c<4>{})) return rc;
            return check_launch(S == 2 ? "stft1024_bwd" : "stft2048_bwd");
        }
    }
    {
        int io_floats = 0;
        int lds = stft512_lds_bytes(L, P, &io_floats);
        bool tuned_ok = dtype == DSA_F32 && nfft == 512 && L <= 512 && lds <= 64 * 1024 && !use_floor && !gw &&
                        pad_mode == DSA_PAD_CONSTANT;
        if (algo == DSA_ALGO_TUNED && !tuned_ok)
            return fail(DSA_ERR_UNSUPPORTED,
                        "stft_bwd: tuned kernel needs float32, fft_length 512, constant padding, no floor, fixed window%s");
        if (tuned_ok && algo != DSA_ALGO_GENERIC) {
            int64_t N = dsa_num_frames(T, P);
            int chunks_per_utt = (int)((N + kFPW - 1) / kFPW);
            long total_chunks = (long)B * chunks_per_utt;
            int span = (kFPW - 1) * P + L;
            // the packed kernel with the overlap-add carried in registers (stft_bwd_pk.h): one launch, no workspace
            {
            const bool cplx = out_format == DSA_SPEC_COMPLEX || out_format == DSA_SPEC_COMPLEX_INV;
            const int left = center ? L / 2 : 0;
            if (!zmean && L == 400 && (P == 80 || P == 160) && (cplx || out_format == DSA_SPEC_POWER || out_format == DSA_SPEC_MAG)) {
                const int ppu = chunks_per_utt;                       // passes of four frames per utterance
                const long waves = 256L * 16;
                long want = (waves + B - 1) / B;                       // runs per utterance that fill the chip ...
                constexpr int min_run = 4;                             // shortest run of passes a wave takes (each run adds one warm-up pass)
                const long longest = ppu / min_run > 0 ? ppu / min_run : 1;
                const int runs = (int)(want < longest ? want : longest);
                const long items = (long)B * runs;
                const long wv = items < waves ? items : waves;
                const dim3 g2((unsigned)((wv + 3) / 4));             // four-wave workgroups share the twiddle and window tables
                const int lds2 = 4 * kFPW * kZS * 8 + 256 * 8 + 16 * 13 * 8;
                const float cs = out_format == DSA_SPEC_COMPLEX_INV ? 1.f / 512.f : 0.5f;
                const float ce = out_format == DSA_SPEC_COMPLEX_INV ? 1.f : 2.f;
                // frame periods of 5 ms and 10 ms at 16 kHz (the 25 ms window): one instantiation each
#define DSA_STFT_BWD_PK_LAUNCH(PC, CP, MG)                                                                                   \
    hipLaunchKernelGGL((stft512_bwd_pk_kernel<400, PC, CP, MG>), g2, dim3(256), lds2, st, (const float*)x, (const float*)gy, \
                       (long)T, (long)N, left, (const float*)w, (const float*)twiddle, cs, ce, (float*)gx, items, runs, ppu,   \
                       (const float*)div, (float)div_eps, (float)eps)
                if (P == 80) {
                    if (cplx) DSA_STFT_BWD_PK_LAUNCH(80, true, false);
                    else if (out_format == DSA_SPEC_MAG) DSA_STFT_BWD_PK_LAUNCH(80, false, true);
                    else DSA_STFT_BWD_PK_LAUNCH(80, false, false);
                } else {
                    if (cplx) DSA_STFT_BWD_PK_LAUNCH(160, true, false);
                    else if (out_format == DSA_SPEC_MAG) DSA_STFT_BWD_PK_LAUNCH(160, false, true);
                    else DSA_STFT_BWD_PK_LAUNCH(160, false, false);
                }
#undef DSA_STFT_BWD_PK_LAUNCH
                return check_launch("stft512_bwd_pk");
            }
            }
            float* part = nullptr;
            if (hipMallocAsync((void**)&part, sizeof(float) * (size_t)total_chunks * span, st) != hipSuccess)
                return fail(DSA_ERR_LAUNCH, "stft_bwd: workspace allocation failed%s");
            int waves_per_cu = 144 * 1024 / lds;
            if (waves_per_cu > 4 * DSA_STFT_BWD_WAVES) waves_per_cu = 4 * DSA_STFT_BWD_WAVES;
            long grid = 256L * waves_per_cu;
            if (grid > total_chunks) grid = total_chunks;
            int left = center ? L / 2 : 0;
            const bool cplx = out_format == DSA_SPEC_COMPLEX || out_format == DSA_SPEC_COMPLEX_INV;
#define DSA_STFT_BWD_LAUNCH(ZM, CP, PL)                                                                                   \
    hipLaunchKernelGGL((stft512_bwd_kernel<ZM, CP, PL>), dim3((unsigned)grid), dim3(64), lds, st, (const float*)x,        \
                       (const float*)gy, (long)T, (long)N, L, P, left, pad_mode, (const float*)w, (const float*)twiddle, \
                       (float)eps, out_format, part, total_chunks, chunks_per_utt, span)
            if (cplx) {
                long waves = 256L * 16;
                if (waves > total_chunks) waves = total_chunks;
                const int lds2 = 2 * kFPW * kZS * 8 + 256 * 8 + 16;
                const dim3 g2((unsigned)((waves + 1) / 2));
                if (zmean)
                    hipLaunchKernelGGL((stft512_bwd_kernel<true, true, false>), g2, dim3(128), lds2, st, (const float*)x,
                                       (const float*)gy, (long)T, (long)N, L, P, left, pad_mode, (const float*)w,
                                       (const float*)twiddle, (float)eps, out_format, part, total_chunks, chunks_per_utt, span);
                else
                    hipLaunchKernelGGL((stft512_bwd_kernel<false, true, false>), g2, dim3(128), lds2, st, (const float*)x,
                                       (const float*)gy, (long)T, (long)N, L, P, left, pad_mode, (const float*)w,
                                       (const float*)twiddle, (float)eps, out_format, part, total_chunks, chunks_per_utt, span);
            }
            else if (zmean) DSA_STFT_BWD_LAUNCH(true, false, false);
            else if (out_format == DSA_SPEC_POWER && pad_mode == DSA_PAD_CONSTANT) {
                // the plain instantiation: four waves per SIMD in two-wave workgroups (as the forward)
                long waves = 256L * 16;
                if (waves > total_chunks) waves = total_chunks;
                const int lds2 = 2 * kFPW * kZS * 8 + 256 * 8 + 16;
                hipLaunchKernelGGL((stft512_bwd_kernel<false, false, true>), dim3((unsigned)((waves + 1) / 2)), dim3(128), lds2,
                                   st, (const float*)x, (const float*)gy, (long)T, (long)N, L, P, left, pad_mode,
                                   (const float*)w, (const float*)twiddle, (float)eps, out_format, part, total_chunks,
                                   chunks_per_utt, span);
            }
            else DSA_STFT_BWD_LAUNCH(false, false, false);
#undef DSA_STFT_BWD_LAUNCH
            int rc = check_launch("stft512_bwd");
            if (rc == DSA_OK) {
                dim3 g2((unsigned)((T + 255) / 256), (unsigned)(B < 65535 ? B : 65535));
                hipLaunchKernelGGL(stft_span_gather_kernel, g2, dim3(256), 0, st, (const float*)part, (long)B, (long)T, P, left,
                                   span, chunks_per_utt, (float*)gx, (const float*)div, (float)div_eps);
                rc = check_launch("stft512_bwd");
            }
            (void)hipFreeAsync(part, st);
            return rc;
        }
    }
    return with_dtype(dtype, "stft_bwd", [&](auto tag) {   // (refused before the workspace is asked for)
        const size_t esz = sizeof(decltype(tag));
        void* x0 = nullptr;
        if (!x) {   // inverse transform through the generic kernels: they read a waveform, give them zeros
            if (hipMallocAsync(&x0, esz * (size_t)B * T, st) != hipSuccess || hipMemsetAsync(x0, 0, esz * (size_t)B * T, st) != hipSuccess)
                return fail(DSA_ERR_LAUNCH, "istft: workspace allocation failed%s");
            x = x0;
        }
        int rc = stft_generic_bwd(dtype, gy, x, B, T, L, P, nfft, w, twiddle, center, zmean, pad_mode, eps, use_floor, relative_floor_db,
                                  out_format, gx, gw, st);
        if (x0) (void)hipFreeAsync(x0, st);
        if (rc == DSA_OK && div) rc = dsa_div_rows(gx, B, T, div, div_eps, dtype, gx, stream);
        return rc;
    });
}

DSA_EXPORT int dsa_stft_bwd(const void* gy, const void* x, int64_t B, int64_t T, int32_t L, int32_t P,
                            int32_t nfft, const void* w, const void* twiddle, int32_t center, int32_t zmean,
                            int32_t pad_mode, double eps, int32_t use_floor, double relative_floor_db,
                            int32_t out_format, int32_t dtype, int32_t algo, void* gx, void* gw, void* stream)
{
    DSA_REQUIRE(B == 0 || T == 0 || x != nullptr, "stft_bwd: the waveform is required");
    return stft_bwd_impl(gy, x, B, T, L, P, nfft, w, twiddle, center, zmean, pad_mode, eps, use_floor, relative_floor_db,
                         out_format, dtype, algo, gx, gw, stream, nullptr, 0.0);
}

// InverseShortTimeFourierTransform._forward istft.py:186-193 in one call: y:(B,N,nfft/2+1) complex pairs ->
// out:(B,T) = overlap-add(window * irfft(y)[:L]) / (d + d_eps), d:(T) the overlap-added squared window.
DSA_EXPORT int dsa_istft_fwd(const void* y, int64_t B, int64_t T, int32_t L, int32_t P, int32_t nfft, const void* w,
                             const void* twiddle, int32_t center, const void* d, double d_eps, int32_t dtype, int32_t algo,
                             void* out, void* stream)
{
    DSA_REQUIRE(d != nullptr, "istft: the window-square sum is required");
    return stft_bwd_impl(y, nullptr, B, T, L, P, nfft, w, twiddle, center, 0, DSA_PAD_CONSTANT, 0.0, 0, 0.0,
                         DSA_SPEC_COMPLEX_INV, dtype, algo, out, nullptr, stream, d, d_eps);
}
