// The Newton step of the mel-generalized cepstral analysis (gamma != 0, fft_length 512, cep_order 24, float32) in one launch, and
// the step's backward: the kernels are in mgcep_step_f16.h, this unit launches them (callers: mgc.hip).  With them, the step's solve
// as a launch of its own (thsolve_quad24_kernel; callers: thsolve.hip, mgc.hip).  That kernel stays in THIS unit and not in
// thsolve_quad.hip, whose size-templated form it is: compiled without it, mgcep_step_h_kernel comes out with another register
// allocation and schedule in its build of the system (profiles/mcep_split_isa.txt).
#include "mgcep_step_f16.h"

namespace dsa {

// ---------------------------------------------------------------------------------------------
// The quad-layout solve of the tuned mel-cepstral kernels (mcep_solve.h) for the Toeplitz-plus-Hankel systems of the
// mel-generalized cepstral analysis (mgcep.py:226-229:
// solve(symmetric_toeplitz(p) + hankel(q), r), n = 24 = the cepstral order): 16 systems per wave in the quad layout, no
// pivoting -- the matrix is the Hessian of a criterion that is convex for -1 <= gamma <= 0 (SPTK's theq() solves it
// without pivoting for the same reason).  The 24 x 24 system rides in the 25 x 25 machinery with row / column 24 as an
// identity pair: row 24 stores slot 6 only (diagonal 1 on lane 0, right-hand side 0 on lane 1) and column 24 of the other
// rows comes through the slot-6 pointers as zeros, so it never couples.  One system per wave with a pivot search
// (th_solve_reg, csrc/thsolve.hip) took 0.2 ms per 51 200 systems; this takes 0.02 ms.
// ---------------------------------------------------------------------------------------------
// `r` rows are r_stride floats apart and start r_off floats in (the Newton step of mgcep hands over its (F, 25) vector with
// the right-hand side in columns 1 .. 24); `add` (or NULL): g = add + solution (the step's update b <- b + solve(..)).
__global__ __launch_bounds__(256) DSA_PK_TARGET void thsolve_quad24_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                             const float* __restrict__ r, long F, float* g,
                                                             int r_stride, int r_off, const float* add)   // (g may be add)
{
    using namespace mm;
    __shared__ __attribute__((aligned(16))) float lds[4 * 16 * kTq + 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* wl = lds + wave * 16 * kTq;
    float* cst = lds + 4 * 16 * kTq;           // [0, 28): zeros | [32, 57): e_24
    if (threadIdx.x < 64) cst[threadIdx.x] = threadIdx.x == 32 + 24 ? 1.f : 0.f;
    __syncthreads();
    const int nq = lane >> 2, gs = lane & 3;
    const GroupMask gq = make_group_mask(gs);
    const long ntiles = (F + 15) / 16;
    for (long tile = (long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long)gridDim.x * 4) {
        __builtin_amdgcn_wave_barrier();
        // stage the 16 records (missing systems: the identity, right-hand side 0).  The tile's q, p and r rows are three
        // CONTIGUOUS runs of memory: each is copied by an unrolled loop of independent loads (as one loop over the record
        // layout with a guarded load per element, every element waited out its own round trip: 43 of the kernel's 59 us)
        const long fbase = tile * 16;
        const long nvalid = (F - fbase) < 16 ? (F - fbase) : 16;
        for (int e = lane; e < 16 * kTq; e += 64) wl[e] = 0.f;
        float vq[12], vp[6], vr[6];
#pragma unroll
        for (int it = 0; it < 12; ++it) {   // 16 x 47 = 752 values of q
            const int idx = lane + 64 * it;
            const bool ok = idx < 752 && idx < nvalid * 47;
            vq[it] = ok ? q[fbase * 47 + (ok ? idx : 0)] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < 6; ++it) {    // 16 x 24 = 384 values of p and of r
            const int idx = lane + 64 * it;
            const bool ok = idx < nvalid * 24;
            vp[it] = ok ? p[fbase * 24 + (ok ? idx : 0)] : ((idx % 24) == 0 ? 1.f : 0.f);   // missing system: p = e_0
            vr[it] = ok ? r[(fbase + (ok ? idx / 24 : 0)) * r_stride + r_off + (ok ? idx % 24 : 0)] : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 12; ++it) {
            const int idx = lane + 64 * it;
            if (idx < 752) wl[(idx / 47) * kTq + (idx % 47)] = vq[it];
        }
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int idx = lane + 64 * it, fr = idx / 24, k = idx - fr * 24;
            wl[fr * kTq + 52 + 27 + k] = vp[it];     // mirrored Toeplitz window: p[|d|] at 27 + d
            wl[fr * kTq + 52 + 27 - k] = vp[it];
            wl[fr * kTq + 104 + k] = vr[it];
        }
        __builtin_amdgcn_wave_barrier();
        const float* rt_q = wl + nq * kTq;
        const float* rr_q = rt_q + 52;
        float xq[KS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, keep_if(gq.m[1], -1.f)};
        bool bad = false;
        {
            f32x4 a[blk::NBLK];
            float ninvs[M1];
            int gsv = gs;
            asm volatile("" : "+v"(gsv));
            const float* zr = cst;
            const float* pa6 = gsv == 0 ? cst + 32 : (gsv == 1 ? rt_q + 104 : zr);   // column 24: e_24 | right-hand side | 0
            blk_build_rows<0>(a, rt_q, rr_q, pa6, zr, gs);
            blk_elim_all(a, gq, ninvs, std::make_integer_sequence<int, M1>{});
            blk_backsub_all(a, xq, gq, ninvs, std::make_integer_sequence<int, blk::NG>{});
            // No pivoting here: that is sound for the positive definite systems of the analysis (gamma in [-1, 0]), and nothing
            // guarantees it for an arbitrary caller.  A pivot that is not positive (ninv = -1 / pivot not negative, or not finite)
            // marks the system: it is solved again below, with row pivoting, by the whole wave (th_solve_reg.h) -- the answer the
            // reference's LAPACK call gives.  (Round 3 wrote NaN and re-solved in a second launch that every call paid for.)
#pragma unroll
            for (int k = 0; k < M1 - 1; ++k) bad |= !(ninvs[k] < 0.f && ninvs[k] > -3.0e38f);
        }
        const long f = tile * 16 + nq;
        if (f < F && !bad) {
#pragma unroll
            for (int c = 0; c < 6; ++c) g[f * 24 + gs + 4 * c] = add ? add[f * 24 + gs + 4 * c] + xq[c] : xq[c];
        }
        unsigned long long marked = __ballot(bad && gs == 0 && f < F);
        while (marked) {   // uniform; normally empty
            const int bl = __builtin_ctzll(marked);
            marked &= marked - 1;
            const int sy = bl >> 2;
            const float* qs2 = wl + sy * kTq;               // q window
            const float* ps2 = qs2 + 52 + 27;               // p[d] at the centre of the mirrored window
            const float rhs = lane < 24 ? qs2[104 + lane] : 0.f;
            int col;
            float sol;
            th_solve_reg<float, 24>(ps2, qs2, rhs, 24, lane, col, sol);
            const long fs = tile * 16 + sy;
            if (lane < 24) g[fs * 24 + col] = add ? add[fs * 24 + col] + sol : sol;
        }
    }
}

int thsolve_quad24_fwd(const void* p, const void* q, const void* r, int64_t F, void* g, hipStream_t st, int r_stride, int r_off,
                       const void* add)
{
    long blocks = ((F + 15) / 16 + 3) / 4;
    if (blocks > 256L * 4) blocks = 256L * 4;
    hipLaunchKernelGGL(thsolve_quad24_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)p, (const float*)q,
                       (const float*)r, (long)F, (float*)g, r_stride, r_off, (const float*)add);
    return check_launch("th_solve_quad_fwd");
}

int mgcep_step_bwd_h(const void* x, const void* b1, const void* gpt, const void* gqt, const void* gr, int64_t F, double gamma,
                     const void* images, const void* gx_in, void* gx, void* gb1, hipStream_t st)
{
    const int lds_bytes = 2 * mgh::BW_STAGE_HALVES * 2;
    const long ntiles = (long)((F + 15) / 16);
    long blocks = (ntiles + mgh::WAVES - 1) / mgh::WAVES;
    if (blocks > 256) blocks = 256;
    if (int rc = launch_lds<mgcep_step_bwd_h_kernel>(lds_bytes, "mgcep_step_bwd_h: cannot reserve the LDS stage buffers%s", dim3((unsigned)blocks),
                                                     dim3(mgh::WAVES * 64), lds_bytes, st, (const float*)x, (const float*)b1, (const float*)gpt,
                                                     (const float*)gqt, (const float*)gr, (long)F, (float)gamma, (const _Float16*)images,
                                                     (const float*)gx_in, (float*)gx, (float*)gb1))
        return rc;
    return check_launch("mgcep_step_bwd_h");
}

int mgcep_step_solve_fwd(const void* x, const void* b1, int64_t F, double gamma, const void* images, void* b1_out, void* r_out, hipStream_t st,
                         void* pt_out, void* qt_out, int n_steps, void* b1_prev_out)
{
    const int lds_bytes = mgh::LDS_FLOATS * 4;
    const long ntiles = (long)((F + 15) / 16);
    long blocks = (ntiles + mgh::WAVES - 1) / mgh::WAVES;
    if (blocks > 256) blocks = 256;
    if (int rc = launch_lds<mgcep_step_h_kernel>(lds_bytes, "mgcep_step_solve: cannot reserve the LDS stage buffers%s", dim3((unsigned)blocks),
                                                 dim3(mgh::WAVES * 64), lds_bytes, st, (const float*)x, (const float*)b1, (long)F, (float)gamma,
                                                 (const _Float16*)images, (float*)b1_out, (float*)r_out, (float*)pt_out, (float*)qt_out, n_steps,
                                                 (float*)b1_prev_out))
        return rc;
    return check_launch("mgcep_step_solve");
}

}  // namespace dsa
