// The binary16 machinery of every mel-cepstral kernel family: a float32 operand as two binary16 pieces, x = hi + lo, so that a
// product runs as three v_mfma_f32_16x16x32_f16 accumulated in float32 (csrc/mcep_mfma_f16.h explains the scheme).  Here: the vector
// and address-space typedefs, the streamed-image loads, the splits, and the image layouts that more than one unit reads -- the
// forward unit writes the images of the 512-point family (mh, mhb) that mcep_mfma_bwd.hip consumes, and the stage geometry of the
// 48 kHz family (mrh) is shared by mcep_resid.hip and mcep_big.hip.  Everything else stays beside its kernel.
#pragma once

#include "common.h"
#include "mcep_solve.h"   // f32x4, namespace mm

namespace dsa {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// explicit global address space: a pointer that went through an opaque asm statement is otherwise loaded from
// with FLAT instructions, which count on the LDS counter too and stall every LDS wait behind an L2 round trip
typedef const __attribute__((address_space(1))) f16x8* gf16x8_ptr;
// Streaming the operand images from L2: a buffer descriptor over the image block (wave-uniform) + a 32-bit lane offset +
// a constant -- buffer_load_dwordx4 takes all three without a vector instruction (as 64-bit per-lane pointers the steps
// beyond the 4 KB immediate cost two carry-chained vector additions per window: 94 vector instructions per tile and step)
typedef int i32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const _Float16* base, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f16x8 gload8(__amdgpu_buffer_rsrc_t rsrc, unsigned lane_bytes, int const_bytes)
{
    const i32x4v r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)lane_bytes, const_bytes, 0);
    return __builtin_bit_cast(f16x8, r);
}
typedef const __attribute__((address_space(1))) float* gf32_ptr;

// fft_length 512, cep_order 24: scales, operand images and the LDS regions of the images (forward and backward; the forward's other
// regions, its stopping rule and the fused prologue's tables continue this namespace in csrc/mcep_mfma_f16.h)
namespace mh {
using namespace mm;
constexpr float SD = 16.f;      // scale of the D^T image (|-2 log2(e) D| <= ~7)
constexpr float SM = 1024.f;    // scale of mc
constexpr float SE = 65536.f;   // scale of the E^T image (|E| <= ~0.01)
constexpr int SE_LOG2 = 16;
constexpr float SG = 4096.f;    // scale of the (ln 2) G^T image (|G| <= 0.13 for |alpha| <= 0.95)
constexpr float SL = 128.f;     // scale of log2 X (|log2 X| < 150 for any float32 input)
// operand images in global memory (binary16 elements), written by mcep_h_prep_kernel once per launch
constexpr int IMG_D = 16 * 64 * 8, IMG_E = 24 * 64 * 8, IMG_G = 16 * 64 * 8;
constexpr int IMG_DH = 0, IMG_DL = IMG_DH + IMG_D, IMG_EH = IMG_DL + IMG_D, IMG_EL = IMG_EH + IMG_E;
constexpr int IMG_GH = IMG_EL + IMG_E, IMG_GL = IMG_GH + IMG_G, IMG_HALVES = IMG_GL + IMG_G;
constexpr int IMG_BYTES = IMG_HALVES * 2 + 32 * 4;  // + the Nyquist row G[256][0..24] as float32
constexpr int EMAX_LOG2 = 15;   // largest scaled e is <= 2^15
// LDS carve-up (float units; same region sizes as namespace mm: the binary16 hi + lo images take
// exactly the room of one float32 image)
constexpr int DH_OFF = 0;                    // [16 mt][64 lane] f16x8
constexpr int DL_OFF = DH_OFF + 16 * 64 * 4;
constexpr int EH_OFF = DL_OFF + 16 * 64 * 4;  // [3 it][8 j][64 lane] f16x8
constexpr int EL_OFF = EH_OFF + 24 * 64 * 4;
}  // namespace mh

// (continued in csrc/mcep_mfma_bwd_f16.h: the backward's scales and LDS carve-up)
namespace mhb {
using namespace mh;
// backward images (binary16 elements) behind the forward ones in the per-launch workspace
constexpr int IMG_EB = 16 * 2 * 64 * 8, IMG_DB = 2 * 8 * 64 * 8, IMG_GB = 16 * 64 * 8;
constexpr int B_BASE = IMG_BYTES / 2;                 // halves: forward images + the Nyquist row of G
constexpr int IMG_EBH = B_BASE, IMG_EBL = IMG_EBH + IMG_EB;
constexpr int IMG_DBH = IMG_EBL + IMG_EB, IMG_DBL = IMG_DBH + IMG_DB;
constexpr int IMG_GBH = IMG_DBL + IMG_DB, IMG_GBL = IMG_GBH + IMG_GB;
constexpr int IMG_B_HALVES = IMG_GBL + IMG_GB;
constexpr int TAIL_B = 32 + 64 + 256;                 // float32: -2 D[c][256] | E[256][m] | E[bin][48]
constexpr int IMG_B_BYTES = IMG_B_HALVES * 2 + TAIL_B * 4;
}  // namespace mhb

// the 48 kHz family (csrc/mcep_resid_f16.h): bins in stages of 32, four waves per workgroup
namespace mrh {
constexpr int WAVES = 4;
constexpr int LOG2_SD = 9;     // scale of the -2 log2(e) D image (|D| <= ~20 for |alpha| <= 0.9)
constexpr int LOG2_SE = 16;    // scale of the E image (|E| <= ~0.03)
constexpr int EMAX_LOG2 = 13;  // scaled e is at most 2^13
constexpr int stage_halves(int ks1, int nt) { return (4 * ks1 + 2 * nt) * 512; }
}  // namespace mrh

__device__ __forceinline__ f32x4 mfma_h(f16x8 a, f16x8 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// x = hi + lo in binary16 (round to nearest): two values at a time
__device__ __forceinline__ void split2(float x0, float x1, f16x2& hi, f16x2& lo)
{
    hi = __builtin_convertvector(f32x2v{x0, x1}, f16x2);
    // lo = binary16(x - float(hi)), the difference exact in float32: ONE v_fma_mixlo_f16 / v_fma_mixhi_f16 per value (binary16
    // operand taken from its half register, float32 multiply-add, result rounded into the low / high half of the destination).
    // Round 2 used v_fma_mix_f32 + a packed conversion (three instructions per pair), the compiler's own form is five.
    const unsigned hb = __builtin_bit_cast(unsigned, hi);
    // (one statement: the compiler does not see a half-register write inside inline assembly, and gfx950 wants a wait state
    // between such a write and the next vector instruction touching the register -- the second half's read-modify-write)
    unsigned lb;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\ts_nop 0\n\t"
        "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\ts_nop 0"
        : "=&v"(lb) : "v"(hb), "v"(x0), "v"(x1));
    lo = __builtin_bit_cast(f16x2, lb);
}
// the hi piece alone (the one-term products of a coarse Newton step): the packed conversion of split2, no lo piece
__device__ __forceinline__ f16x2 split2_hi(float x0, float x1)
{
    return __builtin_convertvector(f32x2v{x0, x1}, f16x2);
}
// four values at a time: the two pairs' half-register writes interleaved, so that the wait state between the low-half write and
// the high half's read-modify-write of one destination is the other pair's instruction (3 of 4 s_nop fewer per four values)
__device__ __forceinline__ void split4(float x0, float x1, float x2, float x3, f16x2& hiA, f16x2& hiB, f16x2& loA, f16x2& loB)
{
    hiA = __builtin_convertvector(f32x2v{x0, x1}, f16x2);
    hiB = __builtin_convertvector(f32x2v{x2, x3}, f16x2);
    const unsigned ha = __builtin_bit_cast(unsigned, hiA), hb = __builtin_bit_cast(unsigned, hiB);
    unsigned la, lb;
    asm("v_fma_mixlo_f16 %0, %2, -1.0, %4 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixlo_f16 %1, %3, -1.0, %6 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %2, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %3, -1.0, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\ts_nop 0"
        : "=&v"(la), "=&v"(lb) : "v"(ha), "v"(hb), "v"(x0), "v"(x1), "v"(x2), "v"(x3));
    loA = __builtin_bit_cast(f16x2, la);
    loB = __builtin_bit_cast(f16x2, lb);
}
// c * s + b on both halves of a register pair: v_pk_fma_f32 (two flops per lane and issue slot)
#ifdef DSA_MCEP_NOPK
__device__ __forceinline__ f32x2v fma2(f32x2v c, float s, f32x2v b)
{
    float r0 = __builtin_fmaf(c[0], s, b[0]), r1 = __builtin_fmaf(c[1], s, b[1]);
    asm volatile("" : "+v"(r0));
    return f32x2v{r0, r1};
}
#else
__device__ __forceinline__ f32x2v fma2(f32x2v c, float s, f32x2v b) { return c * f32x2v{s, s} + b; }
#endif
__device__ __forceinline__ f32x2v lo2(f32x4 v) { return __builtin_shufflevector(v, v, 0, 1); }
__device__ __forceinline__ f32x2v hi2(f32x4 v) { return __builtin_shufflevector(v, v, 2, 3); }

__device__ __forceinline__ void split1(float x, _Float16& hi, _Float16& lo)
{
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// v = hi + lo (binary16), eight values of one MFMA operand
__device__ __forceinline__ void split8(const float (&v)[8], f16x8& hi, f16x8& lo)
{
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        f16x2 h, l;
        split2(v[i], v[i + 1], h, l);
        hi[i] = h[0]; hi[i + 1] = h[1];
        lo[i] = l[0]; lo[i + 1] = l[1];
    }
}

}  // namespace dsa
