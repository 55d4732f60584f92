// Excitation generation (include/diffsptk_amd.h, section a17):
//   excite  ExcitationGeneration._forward, excite.py:222-310   (there: about a dozen full-length element-wise passes, a float64 cumsum and
//           cummax over the whole signal and five boolean-mask gathers / scatters, each of which reads a count back to the host)
// pitch p:(B, N) in samples, 0 = unvoiced  ->  the voiced part of the excitation, (B, N P), zeros in unvoiced samples; ONE launch, no
// workspace, no host synchronisation.
//
// Per voiced frame n (p_n != 0), sample j < P:
//   target  b = p_{n+1}, or p_n when frame n + 1 is unvoiced or n is the last frame            (excite.py:236-239, linear_intpl.py:99)
//   pitch   a + w (b - a), w = j / P, in the data's dtype                                        (linear_intpl.py:100-105; zerodf.hip's lerp)
//   q       1 / pitch in the data's dtype, correctly rounded                                     (excite.py:262)
//   phase   the float64 sum of q from the first sample of the voiced run through this one, rounded to the data's dtype, plus the shift
//           (excite.py:263-265: cumsum(q.double()) - cummax(s * ~mask); s is constant over unvoiced frames, so the bias is the sum at
//           the run's start)
// and the shape of excite.py:28-114 on that phase; the two pulse shapes read the phase of the sample BEFORE (excite.py:281: the phase
// padded with a leading zero), which is the shift alone at the start of an utterance and after an unvoiced sample.
//
// The sum splits three ways: sum = carry_n (the frames of the run before n) + the samples of frame n up to j.  For float32 data every one
// of these float64 sums is EXACT (reciprocals of periods >= 1 are multiples of 2^-47 or so and the sums stay far below 2^5 times the
// sample count), so any partition gives the bits of the sequential cumsum; for float64 data the partition moves the last place of a
// float64 phase.
//
// One workgroup of four waves per utterance (a grid-stride loop when B exceeds the grid), 256 frames at a time:
//   A  thread t sums the P reciprocals of frame t (float64, sequential);
//   S  a segmented scan over the 256 frame totals -- an unvoiced frame resets the sum -- by wave shuffles and one pass over the four
//      wave totals, carried from chunk to chunk: carry_n;
//   B  each wave takes a quarter of the chunk's frames and walks their samples 64 at a time, lane = sample: the reciprocals again, a
//      wave scan that restarts at every frame's first sample (frames have one length, so a lane knows how far below it its frame
//      begins: no flags travel; the sum within the frame is carried from one group of 64 to the next while a frame lasts), carry_n
//      added, the shape evaluated, 64 consecutive values stored.
// The weights j / P come from LDS when P <= 512.  A single long utterance runs on one CU: N P samples through four waves.
#include "common.h"

namespace dsa {
namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_CHUNK = 256;        // frames per chunk: one per thread in phase A
constexpr int EX_WTAB = 512;         // the weights j / P are tabulated up to this frame period
constexpr int EX_MAX_PERIOD = 1 << 20;   // 256 frames of samples are indexed in 32 bits

// torch.fmod(v, 1): exact, the sign of v
template <typename T> __device__ __forceinline__ T ex_frac(T v) { return v - dsa_trunc(v); }

// inclusive segmented sum over the wave: an element with `head` starts a new segment with its own value.  On return `head` says
// whether a segment starts at or before this lane.
__device__ __forceinline__ void ex_wave_segscan(double& v, int& head, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double v2 = __shfl_up(v, o, 64);
        const int h2 = __shfl_up(head, o, 64);
        if (lane >= o) {
            if (!head) v += v2;
            head |= h2;
        }
    }
}

// inclusive sum over the wave within frames of equal length: lane's sample is the j-th of its frame, so the `o` lanes below it belong to
// the same frame exactly when o <= j.  A frame that began before lane 0 (j > lane) lacks what the lanes of the group before hold.
__device__ __forceinline__ void ex_wave_framescan(double& v, int j, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double v2 = __shfl_up(v, o, 64);
        if (o <= j && lane >= o) v += v2;
    }
}

// the shape on the phase (excite.py:28-114): `cur` the phase of this sample, `prev` of the sample before, both with the shift
template <typename T>
__device__ __forceinline__ T ex_shape(int type, bool bipolar, T pitch, T cur, T prev)
{
    const T tau = (T)kTau;
    switch (type) {
    case DSA_EXCITE_PULSE: {
        if (!(dsa_ceil(cur) - dsa_ceil(prev) >= (T)1)) return (T)0;
        const T e = dsa_sqrt(pitch);
        const bool twice = dsa_ceil((T)0.5 * cur) - dsa_ceil((T)0.5 * prev) >= (T)1;
        return bipolar && !twice ? -e : e;
    }
    case DSA_EXCITE_HARMONIC_PULSE: {
        const T nh = dsa_floor((T)0.5 * pitch);
        const T theta = tau * prev, half = (T)0.5 * theta, wide = (nh + (T)0.5) * theta;
        const T numer = bipolar ? dsa_cos(half) - dsa_cos(wide) : -dsa_sin(half) + dsa_sin(wide);
        const T denom = (T)2 * dsa_sin(half);
        const T e = dsa_abs(denom) < (T)1e-6 ? (bipolar ? (T)0 : nh) : numer / denom;
        return dsa_sqrt((T)2 / (nh < (T)1 ? (T)1 : nh)) * e;
    }
    case DSA_EXCITE_SINUSOIDAL: return bipolar ? dsa_sin(tau * cur) : (T)0.5 * ((T)1 - dsa_cos(tau * cur));
    case DSA_EXCITE_SAWTOOTH: {
        const T e = ex_frac(cur);
        return bipolar ? (T)2 * e - (T)1 : e;
    }
    case DSA_EXCITE_INVERTED_SAWTOOTH: {
        const T e = (T)1 - ex_frac(cur);
        return bipolar ? (T)2 * e - (T)1 : e;
    }
    case DSA_EXCITE_TRIANGLE:
        return bipolar ? (T)2 * dsa_abs((T)2 * ex_frac(cur + (T)0.75) - (T)1) - (T)1 : dsa_abs((T)2 * ex_frac(cur + (T)0.5) - (T)1);
    default: {   // DSA_EXCITE_SQUARE
        const T e = ex_frac(cur) <= (T)0.5 ? (T)1 : (T)0;
        return bipolar ? (T)2 * e - (T)1 : e;
    }
    }
}

template <typename T>
__global__ __launch_bounds__(EX_THREADS) void excite_kernel(const T* __restrict__ p, long B, long N, int P, int type, int bipolar, double shift0,
                                                            const T* __restrict__ shift, T* __restrict__ out)
{
    __shared__ T sp[EX_CHUNK + 1];          // the chunk's pitch values and the one after them (0 behind the last frame)
    __shared__ double scar[EX_CHUNK + 1];   // scar[f]: the run's sum before the chunk's frame f; scar[frames]: the next chunk's carry
    __shared__ T wt[EX_WTAB];               // j / P
    __shared__ double wave_v[EX_THREADS / 64];
    __shared__ int wave_h[EX_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool tab = P <= EX_WTAB;
    const T fP = (T)P;
    const double invP = 1.0 / (double)P;
    if (tab)
        for (int j = t; j < P; j += EX_THREADS) wt[j] = (T)j / fP;

    for (long u = blockIdx.x; u < B; u += gridDim.x) {
        const T* pu = p + u * N;
        T* ou = out + u * N * (long)P;
        const T sh = shift ? shift[u] : (T)shift0;
        double chunk_in = 0.0;   // the run's sum at the end of the chunk before this one

        for (long c0 = 0; c0 < N; c0 += EX_CHUNK) {
            const int frames = (int)(N - c0 < EX_CHUNK ? N - c0 : EX_CHUNK);
            __syncthreads();   // the chunk (or utterance) before this one has been read out of sp and scar; wt is written
            // ---- A: this thread's frame total
            double tot = 0.0;
            int head = 1;   // an unvoiced frame (and a thread beyond the chunk) resets the sum
            if (t < frames) {
                const T a = pu[c0 + t], nx = c0 + t + 1 < N ? pu[c0 + t + 1] : (T)0;
                sp[t] = a;
                if (t == frames - 1) sp[frames] = nx;
                if (a != (T)0) {
                    const T d = (nx != (T)0 ? nx : a) - a;
                    for (int j = 0; j < P; ++j) {
                        const T w = tab ? wt[j] : (T)j / fP;
                        tot += (double)((T)1 / (a + w * d));
                    }
                    head = 0;
                }
            }
            // ---- S: the segmented scan over the frame totals
            ex_wave_segscan(tot, head, lane);
            if (lane == 63) {
                wave_v[wave] = tot;
                wave_h[wave] = head;
            }
            __syncthreads();
            double before = chunk_in;   // the run's sum at the end of the wave before this one
            for (int w = 0; w < wave; ++w) before = wave_h[w] ? wave_v[w] : before + wave_v[w];
            if (t < frames) scar[t + 1] = head ? tot : before + tot;
            if (t == 0) scar[0] = chunk_in;
            __syncthreads();
            chunk_in = scar[frames];

            // ---- B: the samples of this wave's frames
            const int per = (frames + 3) >> 2;
            const int f0 = wave * per < frames ? wave * per : frames, f1 = f0 + per < frames ? f0 + per : frames;
            const unsigned s0 = (unsigned)f0 * (unsigned)P, s1 = (unsigned)f1 * (unsigned)P;
            T* oc = ou + c0 * (long)P;
            double run = 0.0;   // the sum within its frame of the last sample of the group before
            for (unsigned g = s0; g < s1; g += 64) {
                const unsigned i = g + lane;
                const bool live = i < s1;
                unsigned f = (unsigned)f0;
                if (live) {   // i / P: the float64 product can only fall short, and only where i is a multiple of P
                    f = (unsigned)((double)i * invP);
                    if ((f + 1) * (unsigned)P <= i) ++f;
                    if (f * (unsigned)P > i) --f;
                }
                const int j = live ? (int)(i - f * (unsigned)P) : 0;
                const T a = sp[f], nx = sp[f + 1];
                const bool voiced = live && a != (T)0;
                const T w = tab ? wt[j] : (T)j / fP;
                const T pitch = a + w * ((nx != (T)0 ? nx : a) - a);
                double v = voiced ? (double)((T)1 / pitch) : 0.0;
                ex_wave_framescan(v, j, lane);
                if (j > lane) v += run;   // the frame began in a group before this one
                const double up = __shfl_up(v, 1, 64);
                const double ex = j == 0 ? 0.0 : (lane == 0 ? run : up);   // the sum within the frame before this sample
                run = __shfl(v, 63, 64);
                if (live) {
                    const double base = scar[f];
                    const T cur = (T)(base + v) + sh, prev = (T)(base + ex) + sh;
                    oc[i] = voiced ? ex_shape<T>(type, bipolar != 0, pitch, cur, prev) : (T)0;
                }
            }
        }
    }
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_excite(const void* p, int64_t B, int64_t N, int32_t P, int32_t type, int32_t bipolar, double init_shift, const void* shift,
                          int32_t dtype, void* out, void* stream)
{
    if (!(B >= 0 && N >= 0 && P >= 1 && P <= EX_MAX_PERIOD)) return fail(DSA_ERR_INVALID_ARGUMENT, "excite: invalid sizes");
    if (N > 0 && B > INT64_MAX / N / P) return fail(DSA_ERR_INVALID_ARGUMENT, "excite: invalid sizes");   // B N P is an int64 offset
    if (type < DSA_EXCITE_PULSE || type > DSA_EXCITE_SQUARE) return fail(DSA_ERR_INVALID_ARGUMENT, "excite: unknown voiced type");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "excite: unknown dtype");
    if (B == 0 || N == 0) return DSA_OK;
    if (!(p && out)) return fail(DSA_ERR_INVALID_ARGUMENT, "excite: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B < (1 << 16) ? B : (1 << 16)));
    return with_dtype(dtype, "excite", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((excite_kernel<T>), grid, dim3(EX_THREADS), 0, st, (const T*)p, (long)B, (long)N, P, type, bipolar, init_shift,
                           (const T*)shift, (T*)out);
        return check_launch(dtype == DSA_F32 ? "excite_f32" : "excite_f64");
    });
}
