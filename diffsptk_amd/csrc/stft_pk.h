// Packed-float32 build of the fused STFT forward for the BASELINE configuration (included by stft.hip).
//
// stft512_fwd_kernel is vector-issue bound: 644 wave instructions per 4-frame pass, every complex add two
// v_add_f32, every complex multiply four.  gfx950 issues v_pk_{add,mul,fma}_f32 at the same rate as the scalar
// forms, and a complex value IS a register pair -- with the VOP3P operand modifiers (op_sel picks which half of
// a source feeds each half of the result, neg_lo / neg_hi negate per half) every step of a radix-4 butterfly,
// the multiplication by +-i and a complex multiply by a twiddle map onto packed instructions WITHOUT any
// register shuffling:
//     a + b, a - b                      1 instruction
//     a - i b, a + i b                  1 instruction (swap the halves of b, negate one)
//     a * t                             2 instructions (mul by t.re broadcast, fma by t.im broadcast on swapped a)
//     real-FFT split of a pair          8 instructions for TWO bins incl. |.|^2 + eps (was ~22 per bin pair)
// The compiler's own packed selection was measured slower on this code (it pairs registers with extra moves,
// DESIGN.md 3.1), so the arithmetic below is inline assembly on register pairs; loads, stores, addressing and
// the pass structure are the C++ of stft512_fwd_kernel.  Semantics: ShortTimeFourierTransform._forward,
// stft.py:237-241 (power format, eps, no relative floor, constant padding, no zmean -- the other options
// keep the all-options kernel).
#pragma once

#include "common.h"
#include "pk_math.h"
#include "stft_tile.h"

namespace dsa {

// The packed forward kernel.  Same pass structure, LDS carve-up, launch geometry and output as
// stft512_fwd_kernel<false, true, LC> (see there); P must be even (8-byte aligned sample pairs in LDS).
// (stft.hip is built with the compiler's packed-float32 selection switched off, which also makes the assembler
// reject v_pk_*_f32 in inline assembly: the target attribute switches the feature back on for this kernel only)
// (DSA_PK_TARGET: common.h)
// The power values leave the split's registers as 8-byte stores (a lane holds two neighbouring bins: every store instruction
// writes 512 consecutive bytes of one row) instead of being staged in LDS for 16-byte stores: the kernel is bound by LDS
// cycles, and a staged tile cost 18 four-byte LDS writes + 5 sixteen-byte reads per pass (a fifth of them).
//
// FB: the mel filter bank in the epilogue (SURVEY 8(f) row 1 without the spectrum's round trip through memory,
// fbank.py:306-321 on top of stft.py): `y` is then the (B N, C) filter-bank output glog(max(s H, floor)), s = the
// power values or their square roots.  H must have the two-adjacent-channels-per-bin structure of the mel filters;
// the host turns it into the per-lane plan `fbt` (dsa_fbank_scan_plan; tools/proto_fbank_scan.py is a lane-level
// model): with the register-direct split a lane holds the neighbouring bins (2l+1, 2l+2) and (255-2l, 254-2l) of a frame,
// so the bins between two channel centres are a RUN of lanes and the channel sums are segmented scans over lanes
// (v_fmac_f32_dpp with a 0/1 mask per lane and step: no transposition through LDS, no matrix operand images --
// neither would fit beside four waves per SIMD).  Four-wave workgroups: the window moves from registers to a
// shared LDS table to make room for the plan.
// The filter-bank epilogue's rare branches (a floor below 1e-30, gamma != 0) call the library's logf / powf.  Inlined into a
// kernel that carries DSA_PK_TARGET the compiler packs their polynomial code, with crossed forms (a low result half reading a
// high source half: the class no shipped kernel executes, common.h) -- so they stay calls to functions built without the feature.
__device__ __attribute__((noinline)) float fb_slow_log(float v) { return dsa_log(v); }
__device__ __attribute__((noinline)) float fb_slow_glog(float v, float gamma) { return (dsa_pow(v, gamma) - 1.f) / gamma; }

// OPTS (round 6): zmean (frame.py:139-140) and the relative floor (spec.py:174-176) -- an instantiation of its own, the plain kernel's
// code is untouched.  `opt_zmean`, `opt_floor` (< 0: none, else the linear factor 10^(dB / 10)) are its run-time switches.
// FBM: 0 spectrum out, 1 filter bank of the power values, 2 of the amplitudes.  Workgroups of two waves (four with FBM); they share the
// twiddle (and window) tables, nothing else.
template <int LC, int FBM = 0, bool OPTS = false>
__global__ __launch_bounds__(FBM ? 256 : 128, 4) DSA_PK_TARGET void stft512_fwd_pk_kernel(
    const float* __restrict__ x, long Tlen, long N, int L, int P, int left, const float* __restrict__ w,
    const float* __restrict__ twiddle, float eps, float* __restrict__ y, long total_chunks, int chunks_per_utt,
    const float* __restrict__ fbt, float fb_floor, float fb_gamma, int fbC, int pad_mode, int opt_zmean = 0, float opt_floor = -1.f)
{
    static_assert(!OPTS || (LC > 0 && !FBM), "zmean / relative floor build on the plain kernel");
    // pad_mode (round 6; frame.py:130-137): reflect / replicate / circular padding only changes which sample a position outside the
    // utterance reads -- the passes that reach over an end (stage_sync's element-wise path); interior passes never see it
    constexpr bool FB = FBM != 0;
    static_assert(!FB || LC > 0, "the filter-bank epilogue needs the frame length at compile time");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int WPB = FB ? 4 : 2;   // waves per workgroup (FB: window pairs from a shared LDS table instead of 26 registers per lane)
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    v2f* zbuf = reinterpret_cast<v2f*>(smem_raw) + wv * kFPW * kZS;
    float* io_buf = reinterpret_cast<float*>(zbuf);  // aliases zbuf: stretch -> tiles -> spectra -> filter-bank slots
    v2f* t256 = reinterpret_cast<v2f*>(smem_raw) + WPB * kFPW * kZS;
    v2f* wtab = t256 + 256;                          // FB: [16][NR] window pairs
    v2f* hend = wtab + 16 * (LC ? (LC + 31) / 32 : 16);   // FB: [128] (H[0][c], H[256][c])
    const long nw = (long)gridDim.x * WPB;
    const long wid = (long)blockIdx.x * WPB + wv;
    const int lane = threadIdx.x & 63;
    const int j = lane & 15;   // lane within the frame group
    const int fl = lane >> 4;  // frame slot within the pass (0..3)
    // pass k of wave `wid` is chunk wid + k nw: the passes in flight stay one compact window of the output
    const long c_first = wid;
    const long c_end = total_chunks;
    if (c_first >= c_end) return;
    constexpr int NR = LC ? (LC + 31) / 32 : 16;   // sample pairs a lane reads (the rest is zero padding)
    constexpr int K = 257;
    // (utterance, chunk) of a pass advance incrementally: one 64-bit division per wave
    // (32-bit: the wave count and the chunks of an utterance are far below 2^31; 64-bit divisions are ~150 instructions)
    const long b_step = (long)((unsigned long)nw / (unsigned)chunks_per_utt);
    const int ci_step = (int)(nw - b_step * chunks_per_utt);
    auto advance = [&](long& bb, int& cc, long& cq) __attribute__((always_inline)) {
        cq += nw;
        bb += b_step;
        cc += ci_step;
        if (cc >= chunks_per_utt) {
            cc -= chunks_per_utt;
            ++bb;
        }
    };
    // the stretch of samples the (up to) four frames of pass (bb, cc) share, straight from memory into the tile
    auto stage_sync = [&](long bb, int cc) __attribute__((always_inline)) {
        const long frame0 = (long)cc * kFPW;
        const int nvalid = (int)((N - frame0) < kFPW ? (N - frame0) : kFPW);
        const float* xb = x + bb * Tlen;
        const long g0 = frame0 * P - left;
        const int need = (nvalid - 1) * P + L;
        if (g0 >= 0 && g0 + need <= Tlen && (((size_t)(xb + g0)) & 15) == 0) {
            const float4* src4 = reinterpret_cast<const float4*>(xb + g0);
            float4* dst4 = reinterpret_cast<float4*>(io_buf);
            const int n4 = need >> 2;
            for (int s = lane; s < n4; s += 64) {
                dst4[s] = src4[s];
                // (a marker that keeps this loop's tail from being merged with the register-staged writes of the
                // pass loop: merged, those would inherit this loop's load waits -- and wait for the pass's stores)
                asm volatile("; stage_sync" : : "v"(s));
            }
            for (int s = (n4 << 2) + lane; s < need; s += 64) io_buf[s] = xb[g0 + s];
        } else {
            for (int s = lane; s < need; s += 64) io_buf[s] = load_padded(xb, g0 + s, Tlen, pad_mode);
        }
    };
    // Software pipeline over passes.  At the END of pass n the stretch of pass n+1 -- fetched into registers during
    // pass n -- goes into the (by then free) tile and the fetch for pass n+2 is issued, so every fetch has one whole
    // pass to arrive.  The wait for it sits BEFORE the output stores of the pass: vector-memory operations retire in
    // order, and a wait placed after the stores cannot tell them from the loads -- every pass would wait for its
    // own stores (measured: the pass period then follows the store latency).
    v4f pre0 = v4f{0.f, 0.f, 0.f, 0.f}, pre1 = pre0, pre2 = pre0;
    auto prefetch_into = [&](long bb, int cc, v4f& q0, v4f& q1, v4f& q2) __attribute__((always_inline)) -> bool {
        const long fr2 = (long)cc * kFPW;
        const int nv2 = (int)((N - fr2) < kFPW ? (N - fr2) : kFPW);
        const long g2 = fr2 * P - left;
        const int need2 = (nv2 - 1) * P + L;
        const float* xb2 = x + bb * Tlen;
        if (g2 >= 0 && g2 + need2 <= Tlen && (((size_t)(xb2 + g2)) & 15) == 0 && (need2 & 3) == 0 && need2 <= 768) {
            const v4f* src4 = reinterpret_cast<const v4f*>(xb2 + g2);
            const int n4 = need2 >> 2;
            q0 = src4[lane < n4 ? lane : n4 - 1];
            q1 = src4[lane + 64 < n4 ? lane + 64 : n4 - 1];
            q2 = src4[lane + 128 < n4 ? lane + 128 : n4 - 1];
            return true;
        }
        return false;
    };
    auto prefetch = [&](long bb, int cc) __attribute__((always_inline)) -> bool { return prefetch_into(bb, cc, pre0, pre1, pre2); };

    // The first pass's stretch is fetched like every other one -- issued first, so that its round trip to memory
    // overlaps the table loads below instead of following them.
    long b = (long)((unsigned)c_first / (unsigned)chunks_per_utt);
    int ci = (int)(c_first - b * chunks_per_utt);
    long c = c_first;
    bool pre_ok = prefetch(b, ci);

    v2f wreg[NR];
    v2f f_wd0, f_wu0, f_wd1, f_wu1, f_nb, f_mM;   // FB: the lane's plan (lower-half bin pair in .x, upper-half pair in .y)
    float f_mk[12];
    int f_addr[4], f_valid = 0;
    if (FB) {
        // every wave writes the whole (identical) tables, like the twiddle table below: no workgroup barrier needed
        v2f wt[4], he[2];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int i = lane + 64 * q4;
            const int l = 2 * (i / NR) + 32 * (i % NR);
            wt[q4] = v2f{(i < 16 * NR && l < L) ? w[l < L ? l : 0] : 0.f, (i < 16 * NR && l + 1 < L) ? w[l + 1 < L ? l + 1 : 0] : 0.f};
        }
        const float* fl_ = fbt + lane * 32;
        he[0] = v2f{fl_[26], fl_[27]};
        he[1] = v2f{fl_[28], fl_[29]};
        const v4f t0 = *reinterpret_cast<const v4f*>(fl_), t1 = *reinterpret_cast<const v4f*>(fl_ + 4);
        const v4f t2 = *reinterpret_cast<const v4f*>(fl_ + 8), t3 = *reinterpret_cast<const v4f*>(fl_ + 12);
        const v4f t4 = *reinterpret_cast<const v4f*>(fl_ + 16), t5 = *reinterpret_cast<const v4f*>(fl_ + 20);
        const int slots_w = __builtin_bit_cast(int, fl_[24]), flags_w = __builtin_bit_cast(int, fl_[25]);
        f_valid = __builtin_bit_cast(int, fl_[30]);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
            if (lane + 64 * q4 < 16 * NR) wtab[lane + 64 * q4] = wt[q4];
        hend[lane] = he[0];
        hend[lane + 64] = he[1];
        f_wd0 = v2f{t0.x, t0.y}, f_wu0 = v2f{t0.z, t0.w}, f_wd1 = v2f{t1.x, t1.y}, f_wu1 = v2f{t1.z, t1.w};
        f_nb = v2f{t2.x, t2.y};
        f_mk[0] = t2.z, f_mk[1] = t2.w, f_mk[2] = t3.x, f_mk[3] = t3.y, f_mk[4] = t3.z, f_mk[5] = t3.w;
        f_mk[6] = t4.x, f_mk[7] = t4.y, f_mk[8] = t4.z, f_mk[9] = t4.w, f_mk[10] = t5.x, f_mk[11] = t5.y;
        f_mM = v2f{t5.z, t5.w};
        // byte offsets of the lane's slot writes inside a [128]-float block; slot 127 is nobody's (C <= 126): "no write"
        f_addr[0] = 4 * ((flags_w & 1) ? (slots_w & 255) : 127);            // run total of the lower half  -> interval jE
        f_addr[1] = 4 * ((flags_w & 2) ? ((slots_w >> 8) & 255) : 127);     //              upper half
        f_addr[2] = 4 * ((flags_w & 4) ? ((slots_w >> 16) & 255) : 127);    // interval closed inside the lane, lower half
        f_addr[3] = 4 * ((flags_w & 8) ? ((slots_w >> 24) & 255) : 127);    //                                  upper half
    } else {
#pragma unroll
        for (int m1 = 0; m1 < NR; ++m1) {
            const int l = 2 * j + 32 * m1;
            wreg[m1] = v2f{l < L ? w[l] : 0.f, l + 1 < L ? w[l + 1] : 0.f};
        }
    }
    {
        // entry [k1 = i >> 4][j = i & 15]: W256^(j k1) = W512^(2 j k1), HALVED: the 1/2 of the real-FFT split (exact).
        // The four loads of a lane are issued together (as a loop they were four dependent round trips to memory
        // at the head of every wave).
        v2f t4[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int i = lane + 64 * q4;
            const int m = 2 * (i & 15) * (i >> 4);
            t4[q4] = *reinterpret_cast<const v2f*>(twiddle + 2 * m);
        }
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) t256[lane + 64 * q4] = t4[q4] * 0.5f;
    }
    // split twiddles W512^k of this lane's two pairs (k, 256 - k): k = 2 lane + 1, 2 lane + 2 (the lane's two bins are neighbours)
    const int kA = 2 * lane + 1, kB = 2 * lane + 2;
    v2f twA = v2f{twiddle[2 * kA], twiddle[2 * kA + 1]};
    v2f twB = v2f{twiddle[2 * kB], twiddle[2 * kB + 1]};
    const v2f eps2 = v2f{eps, eps};
    v2f* zf = zbuf + fl * kZS;
    // Every prologue load is consumed HERE: otherwise the wait for these loop-invariant registers lands at their
    // first use inside the pass loop, where it would also wait for whatever the pass has in flight.
    if (FB) {
        asm volatile("" : "+v"(f_wd0), "+v"(f_wu0), "+v"(f_wd1), "+v"(f_wu1), "+v"(f_nb), "+v"(f_mM));
#pragma unroll
        for (int i = 0; i < 12; ++i) asm volatile("" : "+v"(f_mk[i]));
        asm volatile("" : "+v"(f_addr[0]), "+v"(f_addr[1]), "+v"(f_addr[2]), "+v"(f_addr[3]), "+v"(f_valid));
    } else {
#pragma unroll
        for (int m1 = 0; m1 < NR; ++m1) asm volatile("" : "+v"(wreg[m1]));
    }
    asm volatile("" : "+v"(twA), "+v"(twB));
    if (pre_ok) {
        const long fr0 = (long)ci * kFPW;
        const int nv0 = (int)((N - fr0) < kFPW ? (N - fr0) : kFPW);
        const int n4 = ((nv0 - 1) * P + L) >> 2;
        asm volatile("" : "+v"(pre0), "+v"(pre1), "+v"(pre2) : : "memory");
        v4f* dst4 = reinterpret_cast<v4f*>(io_buf);
        if (lane < n4) dst4[lane] = pre0;
        if (lane + 64 < n4) dst4[lane + 64] = pre1;
        if (lane + 128 < n4) dst4[lane + 128] = pre2;
    } else {
        stage_sync(b, ci);
    }
    long b1 = b;
    int ci1 = ci;
    long c1 = c;
    advance(b1, ci1, c1);
    bool has1 = c1 < c_end;
    pre_ok = has1 ? prefetch(b1, ci1) : false;
    // One pass.  (q0, q1, q2, qok): the register set that holds the NEXT pass's stretch -- waited for before this pass's stores,
    // staged into the tile at the end of the pass, then re-used for the fetch one pass further on.
    auto run_pass = [&](v4f& q0, v4f& q1, v4f& q2, bool& qok) __attribute__((always_inline)) -> bool {
        const long frame0 = (long)ci * kFPW;
        const int nvalid = (int)((N - frame0) < kFPW ? (N - frame0) : kFPW);
        DSA_WAVE_SYNC();
        // ---- per frame: window (window.py:190), 256-point complex FFT (16 lanes x 16 points) ----
        v2f v[16];
        {
            const v2f* src = reinterpret_cast<const v2f*>(io_buf + fl * P + 2 * j);   // P even: 8-byte aligned
            v2f raw[NR];
#pragma unroll
            for (int m1 = 0; m1 < NR; ++m1) raw[m1] = src[16 * m1];   // reads past the frame stay inside the tile
            // samples past the frame are selected away, never multiplied: zero padding is exact and non-finite
            // neighbours stay out of frames that do not contain them
            if (LC && OPTS) {
                bool in0[NR], in1[NR];
#pragma unroll
                for (int m1 = 0; m1 < NR; ++m1) {
                    in0[m1] = 32 * m1 + 30 < LC || 32 * m1 + 2 * j < LC;
                    in1[m1] = 32 * m1 + 31 < LC || 32 * m1 + 1 + 2 * j < LC;
                    raw[m1] = v2f{in0[m1] ? raw[m1].x : 0.f, in1[m1] ? raw[m1].y : 0.f};
                }
                if (opt_zmean) pk_zero_mean<NR>(raw, in0, in1, LC);
#pragma unroll
                for (int m1 = 0; m1 < NR; ++m1) v[m1] = pk_mul(raw[m1], FB ? wtab[j * NR + m1] : wreg[m1]);
#pragma unroll
                for (int m1 = NR; m1 < 16; ++m1) v[m1] = v2f{0.f, 0.f};
            } else if (LC) {
#pragma unroll
                for (int m1 = 0; m1 < NR; ++m1) {
                    // element (m1, e) belongs to the frame iff 32 m1 + e + 2 j < LC; only the last pair can straddle
                    const bool in0 = 32 * m1 + 30 < LC || 32 * m1 + 2 * j < LC;
                    const bool in1 = 32 * m1 + 31 < LC || 32 * m1 + 1 + 2 * j < LC;
                    const v2f r = v2f{in0 ? raw[m1].x : 0.f, in1 ? raw[m1].y : 0.f};
                    v[m1] = pk_mul(r, FB ? wtab[j * NR + m1] : wreg[m1]);
                }
#pragma unroll
                for (int m1 = NR; m1 < 16; ++m1) v[m1] = v2f{0.f, 0.f};
            } else {
                int lim = L - 2 * j;
                asm volatile("" : "+v"(lim));   // per pass on purpose: hoisted, the select masks occupy 64 scalar registers
#pragma unroll
                for (int m1 = 0; m1 < 16; ++m1) {
                    const v2f r = v2f{32 * m1 < lim ? raw[m1].x : 0.f, 32 * m1 + 1 < lim ? raw[m1].y : 0.f};
                    v[m1] = pk_mul(r, wreg[m1]);
                }
            }
        }
        DSA_WAVE_SYNC();  // every lane has its samples: the stretch may be overwritten
        pk_fft16<(LC > 0 && NR <= 13)>(v);
#pragma unroll
        for (int k1 = 0; k1 < 16; ++k1)  // twiddle, then transposed store: (k1, j) -> k1*17 + j
            zf[k1 * 17 + j] = pk_cmul(v[FFT16_OUT(k1)], t256[k1 * 16 + j]);
        DSA_WAVE_SYNC();
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = zf[j * 17 + i];  // lane k1 = j reads A[i][k1]
        DSA_WAVE_SYNC();
        pk_fft16<false>(v);
#pragma unroll
        for (int k0 = 0; k0 < 16; ++k0) {
            // Z[k], k = j + 16 k0, at position k + 1 (k <= 128) or k + 2 (k >= 128; Z[128] at both 129 and 130):
            // the split below then reads its two neighbouring pairs (Z[2l+1], Z[2l+2]) and
            // (Z[254-2l], Z[255-2l]) as ONE 16-byte aligned access each (as 8-byte reads at a 16-byte lane
            // stride they were two-way bank conflicts: 15 % of the kernel's LDS cycles)
            zf[j + 16 * k0 + (k0 < 8 ? 1 : 2)] = v[FFT16_OUT(k0)];
            if (k0 == 8 && j == 0) zf[129] = v[FFT16_OUT(k0)];
        }
        DSA_WAVE_SYNC();
        // ---- real-FFT split, two bins (k, 256-k) per lane from one pair (a, b) = (Z[k], Z[256-k]) ----
        //   S = a + conj(b), Dd = a - conj(b), Pp = W^k Dd   (Z arrives halved, see t256):
        //   X[k] = (S.re + Pp.im, S.im - Pp.re),  X[256-k] = (S.re - Pp.im, -S.im - Pp.re)
        // computed as R = (Re X[k], Re X[256-k]) and I = (Im X[k], Im X[256-k]), so that
        // |X|^2 + eps of BOTH bins is two packed fused multiply-adds (spec.py:173).
        const long row0 = b * N + frame0;
        const long out0 = row0 * K;
        v2f pa[kFPW][2], pb[kFPW][2], z0[kFPW];
#pragma unroll
        for (int f = 0; f < kFPW; ++f) {
            const v2f* z = zbuf + f * kZS;
            const v4f a2 = *reinterpret_cast<const v4f*>(z + 2 * lane + 2);     // Z[2l+1], Z[2l+2]
            const v4f b2 = *reinterpret_cast<const v4f*>(z + 256 - 2 * lane);   // Z[254-2l], Z[255-2l]
            pa[f][0] = v2f{a2.x, a2.y};
            pa[f][1] = v2f{a2.z, a2.w};
            pb[f][1] = v2f{b2.x, b2.y};   // partner of kB = 2l+2: Z[254-2l]
            pb[f][0] = v2f{b2.z, b2.w};   // partner of kA = 2l+1: Z[255-2l]
            z0[f] = z[1];
        }
        DSA_WAVE_SYNC();   // all pairs are read before anything is written: the filter-bank slots reuse the same LDS
        // the fetch for the NEXT pass has had this whole pass to arrive; it is waited for here, before the stores
        // (unconditional: on a conditional path the compiler would still schedule its own wait at the register use below)
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2) : : "memory");
        v2f ends[kFPW];
#pragma unroll
        for (int f = 0; f < kFPW; ++f) {
            // the two real-valued end bins from Z[0] alone: X[0] = 2 (re + im), X[256] = 2 (re - im)
            v2f E;
            E = pk_lo_pm_hi(z0[f], z0[f]);
            const v2f E4 = pk_mul_s(E, v2f{4.f, 4.f});
            const v2f se = pk_fma_sc(E4, E, eps2);
            ends[f] = se;
            v2f sp[2];
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const v2f S = pk_add_conj(pa[f][part], pb[f][part]);
                const v2f Dd = pk_sub_conj(pa[f][part], pb[f][part]);
                const v2f Pp = pk_cmul(Dd, part == 0 ? twA : twB);
                v2f R, I, s;
                R = pk_lo_pm_hi(S, Pp);
                I = pk_hi_mp_lo(S, Pp);
                s = pk_fma_sc(R, R, eps2);
                s = pk_fma(I, I, s);
                sp[part] = s;
            }
            if (OPTS && opt_floor >= 0.f) {
                // spec.py:174-176: every bin of the frame at least (the frame's largest value) x 10^(dB / 10)
                float m = sp[0].x > sp[0].y ? sp[0].x : sp[0].y;
                m = sp[1].x > m ? sp[1].x : m;
                m = sp[1].y > m ? sp[1].y : m;
                m = se.x > m ? se.x : m;
                m = se.y > m ? se.y : m;
                const float flv = wave64_max(m) * opt_floor;
                sp[0] = v2f{sp[0].x > flv ? sp[0].x : flv, sp[0].y > flv ? sp[0].y : flv};
                sp[1] = v2f{sp[1].x > flv ? sp[1].x : flv, sp[1].y > flv ? sp[1].y : flv};
                ends[f] = v2f{se.x > flv ? se.x : flv, se.y > flv ? se.y : flv};
            }
            if (FB) {
                // ---- filter bank: the lane's four values of this frame, weighted, summed over the lanes of each interval ----
                v2f s0 = sp[0], s1 = sp[1];   // (bin 2l+1, bin 255-2l), (bin 2l+2, bin 254-2l)
                v2f en = se;
                if (FBM == 2) {               // fbank.py:315: amplitude domain
                    s0 = v2f{__builtin_amdgcn_sqrtf(s0.x), __builtin_amdgcn_sqrtf(s0.y)};
                    s1 = v2f{__builtin_amdgcn_sqrtf(s1.x), __builtin_amdgcn_sqrtf(s1.y)};
                    en = v2f{__builtin_amdgcn_sqrtf(en.x), __builtin_amdgcn_sqrtf(en.y)};
                    // (the square roots come from the transcendental unit: one idle issue slot before any hand-written
                    //  instruction may read them -- the compiler does not track hazards into inline assembly; the first
                    //  version of this epilogue summed them with v_pk_add_f32 and read stale registers)
                    asm volatile("s_nop 0" : "+v"(s0), "+v"(s1), "+v"(en));
                }
                ends[f] = en;
                // (a non-finite sample makes every bin of its frames non-finite, hence -- every channel has bins of non-zero
                //  weight -- every channel of those frames, and the scans never mix frames: no extra handling needed)
                // contributions of the lane's first (c*0) and second (c*1) bin of each half to the down / up sums
                const float cd0l = s0.x * f_wd0.x, cd0h = s0.y * f_wd0.y, cu0l = s0.x * f_wu0.x, cu0h = s0.y * f_wu0.y;
                float a0 = __builtin_fmaf(cd0l, f_nb.x, s1.x * f_wd1.x), a1 = __builtin_fmaf(cd0h, f_nb.y, s1.y * f_wd1.y);
                float a2 = __builtin_fmaf(cu0l, f_nb.x, s1.x * f_wu1.x), a3 = __builtin_fmaf(cu0h, f_nb.y, s1.y * f_wu1.y);
    // (a DPP operand must have been written at least two issue slots earlier: the leading s_nop covers the first
    //  step, afterwards three other instructions lie between a write and the next shifted read of a register)
#define DSA_FB_SCAN(NOP, CTRL, MLO, MHI)                                                 \
    asm volatile(NOP "v_fmac_f32_dpp %0, %0, %4 " CTRL "\n\t"                                 \
                 "v_fmac_f32_dpp %1, %1, %5 " CTRL "\n\t"                                 \
                 "v_fmac_f32_dpp %2, %2, %4 " CTRL "\n\t"                                 \
                 "v_fmac_f32_dpp %3, %3, %5 " CTRL                                        \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(MLO), "v"(MHI))
                DSA_FB_SCAN("s_nop 1\n\t", "row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1", f_mk[0], f_mk[6]);
                DSA_FB_SCAN("", "row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1", f_mk[1], f_mk[7]);
                DSA_FB_SCAN("", "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1", f_mk[2], f_mk[8]);
                DSA_FB_SCAN("", "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1", f_mk[3], f_mk[9]);
                DSA_FB_SCAN("", "row_bcast:15 row_mask:0xa bank_mask:0xf", f_mk[4], f_mk[10]);
                DSA_FB_SCAN("", "row_bcast:31 row_mask:0xc bank_mask:0xf", f_mk[5], f_mk[11]);
#undef DSA_FB_SCAN
                // intervals that end with the lane's FIRST bin: that bin + the run total of the previous lane
                float m0 = cd0l, m1 = cd0h, m2 = cu0l, m3 = cu0h;
                asm volatile("v_fmac_f32_dpp %0, %4, %8 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_fmac_f32_dpp %1, %5, %9 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_fmac_f32_dpp %2, %6, %8 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                             "v_fmac_f32_dpp %3, %7, %9 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                             : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3)
                             : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(f_mM.x), "v"(f_mM.y));
                // slots [f][down lower | down upper | up lower | up upper][128]: the down and the up sum of an interval are
                // 1024 bytes apart -- one ds_write2st64_b32 with immediate offsets for every frame
                char* sl = reinterpret_cast<char*>(zbuf) + f * 2048;
                *reinterpret_cast<float*>(sl + f_addr[0]) = a0;
                *reinterpret_cast<float*>(sl + 1024 + f_addr[0]) = a2;
                *reinterpret_cast<float*>(sl + 512 + f_addr[1]) = a1;
                *reinterpret_cast<float*>(sl + 1536 + f_addr[1]) = a3;
                *reinterpret_cast<float*>(sl + f_addr[2]) = m0;
                *reinterpret_cast<float*>(sl + 1024 + f_addr[2]) = m2;
                *reinterpret_cast<float*>(sl + 512 + f_addr[3]) = m1;
                *reinterpret_cast<float*>(sl + 1536 + f_addr[3]) = m3;
            } else if (f < nvalid) {
                // bins (2 lane + 1, 2 lane + 2) and (254 - 2 lane, 255 - 2 lane): two 8-byte stores, 512 consecutive
                // bytes of the row per instruction (lane 63 writes bin 128 twice, the same pair either way)
                float* yr = y + out0 + f * K;
                *reinterpret_cast<v2f_u4*>(yr + kA) = v2f{sp[0].x, sp[1].x};
                *reinterpret_cast<v2f_u4*>(yr + 256 - kB) = v2f{sp[1].y, sp[0].y};
            }
        }
        if (FB) {
            // ---- channel c = up-slope sum of interval c + down-slope sum of interval c + 1 (both halves) + the end bins ----
            DSA_WAVE_SYNC();
            const float* slf = reinterpret_cast<const float*>(zbuf);
            for (int cb = 0; cb < fbC; cb += 64) {
                const int ch = cb + lane;
                const int cc = ch < 126 ? ch : 126;
                const int vb = cb ? (f_valid >> 4) : f_valid;
                const v2f he = hend[cc];
                const bool has_ends = (f_valid & 256) != 0;   // some channel weights bin 0 or bin 256 (wave-uniform)
                float sums[kFPW];
#pragma unroll
                for (int f = 0; f < kFPW; ++f) {
                    const float* q = slf + f * 512 + cc;
                    float u0 = q[256], u1 = q[384], d0 = q[1], d1 = q[129];
                    u0 = (vb & 1) ? u0 : 0.f;
                    u1 = (vb & 2) ? u1 : 0.f;
                    d0 = (vb & 4) ? d0 : 0.f;
                    d1 = (vb & 8) ? d1 : 0.f;
                    float sum = (u0 + u1) + (d0 + d1);
                    if (has_ends) sum += he.x * ends[f].x + he.y * ends[f].y;
                    sums[f] = sum < fb_floor ? fb_floor : sum;                               // fbank.py:317 (NaN stays NaN)
                }
                if (fb_gamma == 0.f && fb_floor >= 1e-30f) {                                 // fbank.py:318
                    // v_log_f32 (1 ulp, normal arguments: the sums are >= floor) times ln 2
#pragma unroll
                    for (int f = 0; f < kFPW; ++f) sums[f] = __builtin_amdgcn_logf(sums[f]) * 0.69314718055994531f;
                } else if (fb_gamma == 0.f) {
#pragma unroll 1
                    for (int f = 0; f < kFPW; ++f) {
                        float v = sums[0];
                        v = f == 1 ? sums[1] : v, v = f == 2 ? sums[2] : v, v = f == 3 ? sums[3] : v;
                        v = fb_slow_log(v);
                        sums[0] = f == 0 ? v : sums[0], sums[1] = f == 1 ? v : sums[1];
                        sums[2] = f == 2 ? v : sums[2], sums[3] = f == 3 ? v : sums[3];
                    }
                } else {
#pragma unroll 1
                    for (int f = 0; f < kFPW; ++f) {
                        float v = sums[0];
                        v = f == 1 ? sums[1] : v, v = f == 2 ? sums[2] : v, v = f == 3 ? sums[3] : v;
                        v = fb_slow_glog(v, fb_gamma);
                        sums[0] = f == 0 ? v : sums[0], sums[1] = f == 1 ? v : sums[1];
                        sums[2] = f == 2 ? v : sums[2], sums[3] = f == 3 ? v : sums[3];
                    }
                }
#pragma unroll
                for (int f = 0; f < kFPW; ++f)
                    if (ch < fbC && f < nvalid) y[(row0 + f) * fbC + ch] = sums[f];
            }
        } else {   // bins 0 and 256 of the (up to) four frames: lanes 0..7, one instruction
            const int fe = lane >> 1;
            v2f e = ends[0];
            e = fe == 1 ? ends[1] : e;
            e = fe == 2 ? ends[2] : e;
            e = fe == 3 ? ends[3] : e;
            if (fe < nvalid) y[out0 + fe * K + ((lane & 1) ? 256 : 0)] = (lane & 1) ? e.y : e.x;
        }
        DSA_WAVE_SYNC();
        if (!has1) return false;
        // ---- the next pass's stretch into the tile (LDS operations of a wave execute in order: the filter-bank slots
        // have been read), then the fetch for the pass after it ----
        DSA_WAVE_SYNC();
        if (qok) {
            const long fr1 = (long)ci1 * kFPW;
            const int nv1 = (int)((N - fr1) < kFPW ? (N - fr1) : kFPW);
            const int n4 = ((nv1 - 1) * P + L) >> 2;
            v4f* dst4 = reinterpret_cast<v4f*>(io_buf);
            if (lane < n4) dst4[lane] = q0;
            if (lane + 64 < n4) dst4[lane + 64] = q1;
            if (lane + 128 < n4) dst4[lane + 128] = q2;
        } else {
            stage_sync(b1, ci1);
        }
        c = c1;
        b = b1;
        ci = ci1;
        advance(b1, ci1, c1);
        has1 = c1 < c_end;
        qok = has1 ? prefetch_into(b1, ci1, q0, q1, q2) : false;
        return true;
    };
    while (run_pass(pre0, pre1, pre2, pre_ok)) {}
}

}  // namespace dsa
