// Shared host/device helpers for the diffsptk_amd HIP library (gfx950 only).
#pragma once

// Translation units are built with the compiler's packed-float32 selection switched OFF (_lib.py: SOURCE_FLAGS): its own
// v_pk_*_f32 code pairs registers with extra moves, and it freely emits the forms with a set op_sel bit (a LOW result half
// reading a HIGH source half) -- the instruction class of every transient wrong result DESIGN.md 4 recorded, which no shipped
// kernel may execute (tests/test_host_cpu.py::test_no_crossed_packed_float32).  Switching the feature off also makes the
// assembler reject v_pk_*_f32 in inline assembly: a kernel that places packed instructions by hand carries this attribute,
// which switches the feature back on for that function only.
#if defined(__HIP_DEVICE_COMPILE__)
#define DSA_PK_TARGET __attribute__((target("packed-fp32-ops")))
#else
#define DSA_PK_TARGET
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <limits>
#include <type_traits>

#include "../../include/diffsptk_amd.h"
#include "env.h"          // env_int / env_text: every DSA_* route switch is read through them, at every call
#include "mcep_units.h"  // internal declarations of the mel-cepstral families, for the units that define and the units that call them

#define DSA_EXPORT extern "C" __attribute__((visibility("default")))

namespace dsa {

// ---- per-thread error / dispatch record -------------------------------------------------
inline char* err_buf()
{
    static thread_local char buf[512] = "";
    return buf;
}
inline const char*& kernel_name()
{
    static thread_local const char* name = "";
    return name;
}
inline int fail(int code, const char* fmt, const char* detail = "")
{
    snprintf(err_buf(), 512, fmt, detail);
    return code;
}
inline int check_launch(const char* name)
{
    kernel_name() = name;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(err_buf(), 512, "%s: launch failed: %s", name, hipGetErrorString(e));
        return DSA_ERR_LAUNCH;
    }
    return DSA_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, DEVICE): set once per device the process
// drives (`done` = bit mask of the devices that have it; a process may drive several GPUs).  launch_lds's own.
inline bool ensure_dynamic_lds(const void* kernel, int bytes, std::atomic<uint64_t>& done)
{
    int dev = 0;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    const uint64_t bit = known ? (uint64_t)1 << dev : 0;
    if (known && (done.load(std::memory_order_acquire) & bit)) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    if (known) done.fetch_or(bit, std::memory_order_release);
    return true;
}

// The launch of a kernel whose dynamic LDS may pass 48 KB.  reserve_bytes > 0: that much is reserved for Kernel first, once per
// device -- the record of the devices that have it is this instantiation's, so there is one per kernel by construction.  A site that
// needs the attribute only above a size passes `cond ? bytes : 0`.  lds_error is fail()'s FORMAT: a literal that ends in "%s", as
// every message of the library.  The caller names the route, in a check_launch of its own right behind.
template <auto Kernel, typename... Args>
inline int launch_lds(int reserve_bytes, const char* lds_error, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, Args... args)
{
    static std::atomic<uint64_t> devices{0};
    if (reserve_bytes > 0 && !ensure_dynamic_lds((const void*)Kernel, reserve_bytes, devices)) return fail(DSA_ERR_LAUNCH, lds_error);
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...);
    return DSA_OK;
}

// a compile-time integer as an argument: how a generic lambda takes an instantiation parameter (decltype(q)::value)
template <int V>
using int_c = std::integral_constant<int, V>;

// f(float{}) or f(double{}) by the dtype code of an entry; f is a generic lambda that says `using T = decltype(tag);` and holds the
// entry's argument list once.  Any other code is refused under the entry's name `what`.
template <typename F>
inline int with_dtype(int dtype, const char* what, F&& f)
{
    if (dtype == DSA_F32) return f(float{});
    if (dtype == DSA_F64) return f(double{});
    return fail(DSA_ERR_UNSUPPORTED, "%s: unsupported dtype", what);
}

// ---- functions one unit defines and another calls (those of the mel-cepstral families: mcep_units.h, included above) ----
// the generic route of the STFT (csrc/spec.hip), the fallback of dsa_stft_fwd / dsa_stft_bwd (csrc/stft.hip): float32 and float64
int stft_generic_fwd(int dtype, const void* x, int64_t B, int64_t Tlen, int64_t N, int L, int P, int left, int mode, int zmean,
                     const void* w, int nfft, const void* twiddle, int fmt, double eps, int use_floor, double floor_db, void* y,
                     hipStream_t st);
int stft_generic_bwd(int dtype, const void* gy, const void* x, int64_t B, int64_t Tlen, int L, int P, int nfft, const void* w,
                     const void* twiddle, int center, int zmean, int pad_mode, double eps, int use_floor, double floor_db, int fmt,
                     void* gx, void* gw, hipStream_t st);
// matrix-core "transform of the spectrum x (K x C) matrix" launcher of fbank.hip, shared with fftcep.hip
// (use_power: 0 sqrt x | 1 x | 2 log x;  post_mode 0: floor + glog, 1: scale with the first column halved,
//  3: first and last column halved;  needs float32, C <= 48, C < K <= 320)
int fbank_mfma_launch_ex(const void* x, int64_t F, int K, const void* H, int C, int ldh, double floor, double gamma,
                         int use_power, int post_mode, double post_scale, void* y, void* E, hipStream_t st, const char* name,
                         const void* W2 = nullptr, int Mo = 0, void* z = nullptr,   // optional second product z = y W2
                         int ldy = 0);   // row stride of y when it is a column slice of a wider matrix (0: C); post_mode 4: plain product

#define DSA_REQUIRE(cond, msg)                                              \
    do {                                                                    \
        if (!(cond)) return dsa::fail(DSA_ERR_INVALID_ARGUMENT, "%s", msg); \
    } while (0)

// ---- device helpers ------------------------------------------------------------------------
// F.pad index semantics of Frame (frame.py:134-137).  i indexes the UN-padded signal of
// length T; returns the source index, or -1 for a zero (constant mode).
__device__ __forceinline__ long pad_src_index(long i, long T, int mode)
{
    if (i >= 0 && i < T) return i;
    switch (mode) {
    case DSA_PAD_REFLECT: {
        if (T == 1) return 0;
        long period = 2 * (T - 1);
        long j = i % period;
        if (j < 0) j += period;
        return j < T ? j : period - j;
    }
    case DSA_PAD_REPLICATE: return i < 0 ? 0 : T - 1;
    case DSA_PAD_CIRCULAR: {
        long j = i % T;
        if (j < 0) j += T;
        return j;
    }
    default: return -1;
    }
}

template <typename T>
__device__ __forceinline__ T load_padded(const T* __restrict__ x, long i, long len, int mode)
{
    long j = pad_src_index(i, len, mode);
    return j < 0 ? T(0) : x[j];
}

// wave64 butterfly reductions
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        T u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// block reductions through LDS scratch of >= blockDim.x/64 elements; result broadcast to all
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* scratch)
{
    v = wave_sum(v);
    int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[w] = v;
    __syncthreads();
    T s = 0;
    for (int i = 0; i < nw; ++i) s += scratch[i];
    return s;
}
template <typename T>
__device__ __forceinline__ T block_max(T v, T* scratch)
{
    v = wave_max(v);
    int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[w] = v;
    __syncthreads();
    T s = scratch[0];
    for (int i = 1; i < nw; ++i) s = scratch[i] > s ? scratch[i] : s;
    return s;
}

// inclusive prefix sum over the wave; `lane`: the caller's lane index, in the form the caller already holds it
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
// The exclusive prefix of v over a team's threads (rank t of `team`, a multiple of 64; the team's waves are whole waves of the
// workgroup) and the team's total; red: team / 64 slots of the team's own.  Every thread of the workgroup calls it (two barriers).
template <typename V>
__device__ __forceinline__ V team_scan_excl(V v, V* red, int t, int team, V& total)
{
    const int lane = t & 63, w = t >> 6, nw = team >> 6;
    const V inc = wave_scan_incl(v, lane);
    __syncthreads();   // an earlier call's slots may still be read
    if (lane == 63) red[w] = inc;
    __syncthreads();
    V before = 0, all = 0;
    for (int i = 0; i < nw; ++i) {
        if (i < w) before += red[i];
        all += red[i];
    }
    total = all;
    return before + inc - v;
}

// one value of a wave-wide register, from the lane `src` (wave-uniform), as a scalar: v_readlane, no LDS crossbar round trip
template <typename T>
__device__ __forceinline__ T wave_readlane(T v, int src)
{
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
    } else {
        const long long b = __builtin_bit_cast(long long, v);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), src);
        return __builtin_bit_cast(T, (long long)(((unsigned long long)hi << 32) | lo));
    }
}

// a tile of `cnt` consecutive elements (rows of M1) between global memory and LDS rows of stride S, by one wave: coalesced on the
// global side, and with an odd S free of bank conflicts for the lane-per-row access that follows
template <typename T>
__device__ __forceinline__ void wave_tile_in(T* lds, const T* __restrict__ g, long base, int cnt, int M1, int S)
{
    int r = threadIdx.x / M1, c = threadIdx.x - r * M1;
    const int dq = 64 / M1, dr = 64 - dq * M1;
    for (int i = threadIdx.x; i < cnt; i += 64) {
        lds[r * S + c] = g[base + i];
        r += dq;
        c += dr;
        if (c >= M1) { c -= M1; ++r; }
    }
}
template <typename T>
__device__ __forceinline__ void wave_tile_out(const T* lds, T* __restrict__ g, long base, int cnt, int M1, int S)
{
    int r = threadIdx.x / M1, c = threadIdx.x - r * M1;
    const int dq = 64 / M1, dr = 64 - dq * M1;
    for (int i = threadIdx.x; i < cnt; i += 64) {
        g[base + i] = lds[r * S + c];
        r += dq;
        c += dr;
        if (c >= M1) { c -= M1; ++r; }
    }
}

// the lg low bits of k in reverse order, lg in 1 .. 32: where a radix-2 transform of 2^lg points that does not reorder leaves X[k]
__device__ __forceinline__ int fft_brev(int k, int lg) { return (int)(__brev((unsigned)k) >> (32 - lg)); }

constexpr double kPi = 3.14159265358979323846264338327950288;
constexpr double kTau = 6.283185307179586476925286766559;   // math.tau (utils/private.py)

// products, sums, differences and quotients that the compiler may not contract with their neighbours (the units are built with
// -ffp-contract=on, which fuses within one expression only; these are expressions of their own)
__device__ __forceinline__ float rn_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double rn_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float rn_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double rn_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float rn_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double rn_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float rn_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double rn_div(double a, double b) { return __ddiv_rn(a, b); }

__device__ __forceinline__ float dsa_log(float v) { return logf(v); }
__device__ __forceinline__ double dsa_log(double v) { return log(v); }
__device__ __forceinline__ float dsa_exp(float v) { return expf(v); }
__device__ __forceinline__ double dsa_exp(double v) { return exp(v); }
__device__ __forceinline__ float dsa_pow(float a, float b) { return powf(a, b); }
__device__ __forceinline__ double dsa_pow(double a, double b) { return pow(a, b); }
__device__ __forceinline__ float dsa_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double dsa_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float dsa_cos(float v) { return cosf(v); }
__device__ __forceinline__ double dsa_cos(double v) { return cos(v); }
__device__ __forceinline__ float dsa_sin(float v) { return sinf(v); }
__device__ __forceinline__ double dsa_sin(double v) { return sin(v); }
__device__ __forceinline__ float dsa_log10(float v) { return log10f(v); }
__device__ __forceinline__ double dsa_log10(double v) { return log10(v); }
__device__ __forceinline__ float dsa_abs(float v) { return fabsf(v); }
__device__ __forceinline__ double dsa_abs(double v) { return fabs(v); }
__device__ __forceinline__ float dsa_floor(float v) { return floorf(v); }
__device__ __forceinline__ double dsa_floor(double v) { return floor(v); }
__device__ __forceinline__ float dsa_ceil(float v) { return ceilf(v); }
__device__ __forceinline__ double dsa_ceil(double v) { return ceil(v); }
__device__ __forceinline__ float dsa_trunc(float v) { return truncf(v); }
__device__ __forceinline__ double dsa_trunc(double v) { return trunc(v); }
__device__ __forceinline__ float dsa_fmod(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double dsa_fmod(double a, double b) { return fmod(a, b); }
__device__ __forceinline__ bool dsa_isfinite(float v) { return isfinite(v); }
__device__ __forceinline__ bool dsa_isfinite(double v) { return isfinite(v); }
template <typename T> __device__ __forceinline__ T dsa_inf() { return std::numeric_limits<T>::infinity(); }

// spectrum formatter of spec.py:123-132 applied to s = |X|^2 + eps (already floored)
template <typename T>
__device__ __forceinline__ T spec_format(T s, int fmt)
{
    switch (fmt) {
    case DSA_SPEC_DB: return T(10) * dsa_log10(s);
    case DSA_SPEC_LOGMAG: return T(0.5) * dsa_log(s);
    case DSA_SPEC_MAG: return dsa_sqrt(s);
    default: return s;
    }
}

}  // namespace dsa
